"""cc_db_verify_batch (batched verification of caller-proposed candidates, hint lists generated on the device by cc_k_hints_expand) on
the MI355X: against the oracle's hint flow in the setting of test_gpu_hints.py, and 1 024 items in one call against the loop of
cc_db_check_hints over the same items (memcmp), on a common database and on a large-k one (nnk = 128)."""
import time

import numpy as np
import pytest

from test_emu_hints import INT_FIELDS, _demo_hints

pytestmark = pytest.mark.gpu

_world = {}


def _setting(cc):
    """130 full-size scans on a 100 m loop (test_gpu_hints.py::test_check_hints_matches_oracle), ingested once per session"""
    if not _world:
        w = cc.synth.World(loop_len=100.0)
        n = 130
        xyzi, poses, ts = cc.synth.make_sequence(n, world=w, device="cuda")
        offs = np.arange(n + 1, dtype=np.int64) * xyzi.shape[1]
        ctx = cc.Context(0, max_batch=128)
        desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
        _world["v"] = (ctx, desc, np.asarray(ts), np.arange(n, dtype=np.int32), cc.desc_to_numpy(desc).copy())
    return _world["v"]


def _assert_bound_is_not_marginal(L, hdesc, q, cands, bound=1000.0):
    for c in cands:
        k1 = hdesc["keys"][c][1:5].astype(np.float64).reshape(4, L.NPIV, 1, L.KEY_DIM)
        k2 = hdesc["keys"][q][1:5].astype(np.float64).reshape(4, 1, L.NPIV, L.KEY_DIM)
        d = ((k1 - k2) ** 2).sum(-1)
        assert not (np.abs(d - bound) <= 1e-4 * bound).any(), (q, c)


def test_verify_matches_oracle(cc, oracle):
    import torch
    L = cc.L
    ctx, desc, ts, seeds, hdesc = _setting(cc)
    n = len(hdesc)
    db = cc.Database(ctx, capacity=n)
    db.add_scans(desc, ts, seeds)
    n_full = n_res = 0
    for qi in (105, 112, 120, 129):
        cands = [qi - 100, qi - 101, qi - 99, (qi - 50) % n]
        _assert_bound_is_not_marginal(L, hdesc, qi, cands)
        otgt = oracle.Scan.from_desc(hdesc[qi], int_id=qi)
        oscans = [oracle.Scan.from_desc(hdesc[g], int_id=int(g)) for g in cands]
        hints = _demo_hints(L, hdesc, qi, cands)
        assert len(hints) > 50
        exp_h = np.zeros(len(hints), L.hint_dt)
        exp_h["cand_gidx"] = np.array(cands)[hints[:, 0]]
        exp_h["level"], exp_h["seq_src"], exp_h["seq_tgt"] = hints[:, 1], hints[:, 2], hints[:, 3]
        for mfo in (5, 1):
            eres, _ = oracle.check_hints(otgt, oscans, hints, max_fine_opt=mfo)
            res, hl = db.verify(desc[qi:qi + 1], [cands], max_fine_opt=mfo, want_hints=True)
            res = res[0]
            assert hl[0].tobytes() == exp_h.tobytes(), (qi, len(hl[0]), len(exp_h))
            for f in INT_FIELDS:
                exp = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[int(eres[f])]
                assert exp == res[f], (qi, f, exp, res[f])
            if eres["n_res"]:
                assert abs(eres["correlation"] - res["correlation"]) < 1e-4
                assert np.abs(eres["tf"] - res["tf"]).max() < 1e-4
            n_full += int(res["cand_aft_check3"] > 0 and res["n_res"] == 1)
            n_res += int(eres["n_res"])
    assert n_full > 0 and n_res >= 4
    torch.cuda.synchronize()
    db.close()


def _items_1024(n_scans, seed=5):
    """queries 100..129 cycled, 1 to 8 random distinct candidates each; the place a query revisits (100 scans earlier) or one of
    its two neighbours is among them for about half of the items, so that enough of them close a loop"""
    rng = np.random.default_rng(seed)
    qidx = np.arange(1024, dtype=np.int32) % 30
    tab = np.full((1024, 8), -1, np.int32)
    for i in range(1024):
        m = int(rng.integers(1, 9))
        c = [int(x) for x in rng.choice(n_scans, m, replace=False)]
        if rng.random() < 0.5:
            true = int(qidx[i]) + int(rng.integers(-1, 2))  # query 100 + qidx revisits scan qidx
            true = min(max(true, 0), n_scans - 1)
            if true not in c:
                c[int(rng.integers(0, m))] = true
        tab[i, :m] = c
    return qidx, tab


def _batch_against_loop(cc, nnk, timed):
    import torch
    L = cc.L
    ctx, desc, ts, seeds, hdesc = _setting(cc)
    n = len(hdesc)
    dcfg = L.default_db_cfg()
    dcfg.nnk = nnk
    db = cc.Database(ctx, dcfg, capacity=n)
    db.add_scans(desc, ts, seeds)
    qdesc = desc[100:130].contiguous()
    qidx, tab = _items_1024(n)
    before = db.query(qdesc, seeds[100:])
    res, hl = db.verify(qdesc, tab, qidx=qidx, max_fine_opt=5, want_hints=True)
    loop = np.zeros(1024, L.query_result_dt)
    for i in range(1024):
        loop[i], _ = db.check_hints(qdesc[qidx[i]], hl[i], max_fine_opt=5)
    bad = [i for i in range(1024) if res[i].tobytes() != loop[i].tobytes()]
    assert not bad, (len(bad), bad[:5], res[bad[0]], loop[bad[0]])
    assert (res["n_knn_hits"] == [len(h) for h in hl]).all()
    n_closed = int((res["n_res"] == 1).sum())
    print("nnk %d: %d of 1024 items close a loop, %d hints in all" % (nnk, n_closed, int(res["n_knn_hits"].sum())))
    assert n_closed >= 100, n_closed
    # the streamed form (two halves, one wait) gives the same bytes; so does the query path before and after
    a = db.verify_submit(qdesc, tab[:512], qidx=qidx[:512], max_fine_opt=5)
    b = db.verify_submit(qdesc, tab[512:], qidx=qidx[512:], max_fine_opt=5)
    db.query_wait()
    assert a.tobytes() + b.tobytes() == res.tobytes()
    after = db.query(qdesc, seeds[100:])
    assert before.tobytes() == after.tobytes()
    if timed:  # 5 warm-up and 20 timed repetitions each, median, same process
        def med(fn):
            t = []
            for r in range(25):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t.append(time.perf_counter() - t0)
            return float(np.median(t[5:]))

        def the_loop():
            for i in range(1024):
                db.check_hints(qdesc[qidx[i]], hl[i], max_fine_opt=5)

        t_batch = med(lambda: db.verify(qdesc, tab, qidx=qidx, max_fine_opt=5))
        t_loop = med(the_loop)
        print("1024 items: cc_db_verify_batch %.3f ms, loop of cc_db_check_hints %.1f ms, ratio %.1f" % (1e3 * t_batch, 1e3 * t_loop, t_loop / t_batch))
        assert t_batch < t_loop, (t_batch, t_loop)
    torch.cuda.synchronize()
    db.close()


def test_1024_items_equal_the_check_hints_loop_and_are_faster(cc):
    _batch_against_loop(cc, 50, timed=True)


def test_1024_items_on_a_large_k_database(cc):
    _batch_against_loop(cc, 128, timed=False)
