"""The ranked list of a query's refined candidates (the *_ranked entry points, cc_k_final_r / cc_k_final_rl) on the MI355X: parts
A, B and C of test_emu_ranked.py on the device (the 64-scan looping drive, the oracle's descriptors, the oracle peeled
candidate by candidate), an nnk = 100 database (the large-k instances) and the per-scan path on scan handles."""
import ctypes as C

import numpy as np
import pytest

import ranked_common as RC
from test_dyn_thres_oracle import INT_FIELDS

pytestmark = pytest.mark.gpu

_state = {}


def _tensor(cc, desc):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(desc).tobytes(), np.uint8).reshape(len(desc), cc.DESC_BYTES).copy()).cuda()


def ranked_setup(cc, oracle):
    """the drive's descriptors (the oracle's) in a device database; plain and ranked answers at every scan's own epoch, once"""
    if not _state:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        ctx = cc.Context(0, max_batch=16)
        d = _tensor(cc, desc)
        db = cc.Database(ctx, dcfg, capacity=len(desc))
        db.add_scans(d, ts, seeds)
        plain, knn, cnt = db.query(d, seeds, want_knn=True)
        res, knn2, cnt2, (cands, n) = db.query(d, seeds, want_knn=True, ranked=16)
        assert knn2.tobytes() == knn.tobytes() and np.array_equal(cnt, cnt2)
        _state.update(ctx=ctx, d=d, db=db, plain=plain, knn=knn, cnt=cnt, r16=(res, cands, n))
    s = _state
    return s["ctx"], s["d"], s["db"], s["plain"], s["knn"], s["cnt"], s["r16"]


def eligible(cc, oracle, ntidy, mfo, knn, cnt, key):
    out = {}
    for q in np.nonzero((ntidy >= 2) & (ntidy <= mfo))[0]:
        lst, _ = RC.peel_query(cc, oracle, int(q), knn[q], cnt[q], max_fine_opt=mfo, key=key)
        if lst is not None:
            out[int(q)] = lst
    return out


def _report(what, rows, lists):
    """largest deviation from the peeled oracle, printed before anything is asserted"""
    dc = dt = 0.0
    for row, lst in zip(rows, lists):
        for k, (g, corr, tf) in enumerate(lst):
            dc = max(dc, abs(float(row[k]["correlation"]) - corr))
            dt = max(dt, float(np.abs(row[k]["tf"] - tf).max()))
    print("%s: %d lists, %d entries, max |d correlation| %.3g, max |d pose| %.3g" % (what, len(lists), sum(len(x) for x in lists), dc, dt))


def test_query_lists_structure_and_peeled_oracle(cc, oracle):
    """Part A"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = cc.L
    ctx, d, db, plain, knn, cnt, (res, cands, n) = ranked_setup(cc, oracle)
    assert res.tobytes() == plain.tobytes(), "h_res of the ranked call differs from the plain call's"
    for f in INT_FIELDS:
        assert np.array_equal(res[f], ores[f]), f
    RC.check_structure(L, res, cands, n, 16, dcfg.max_fine_opt)
    assert int((n >= 2).sum()) >= 20
    r3, (c3, n3) = db.query(d, seeds, ranked=3)
    assert r3.tobytes() == plain.tobytes()
    RC.check_structure(L, r3, c3, n3, 3, dcfg.max_fine_opt)
    assert np.array_equal(n3, np.minimum(n, 3)) and c3.tobytes() == np.ascontiguousarray(cands[:, :3]).tobytes()
    el = eligible(cc, oracle, ores["n_cand_tidy"], dcfg.max_fine_opt, knn, cnt, "drive")
    _report("query path", [cands[q] for q in el], list(el.values()))
    for q, lst in el.items():
        RC.check_against_peeled(cands[q], int(n[q]), lst, ("query", q))
    assert len(el) >= 5 and sum(len(x) >= 4 for x in el.values()) >= 3, {q: len(x) for q, x in el.items()}


def test_hint_and_verify_flows(cc, oracle):
    """Part B"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = cc.L
    ctx, d, db, plain, knn, cnt, _ = ranked_setup(cc, oracle)
    el = eligible(cc, oracle, ores["n_cand_tidy"], dcfg.max_fine_opt, knn, cnt, "drive")
    rows, lists = [], []
    for q, lst in list(el.items())[:5]:
        hints = RC.to_hint_dt(L, RC.hints_of_knn(L, knn[q], cnt[q]))
        one, sc1 = db.check_hints(d[q], hints, max_fine_opt=dcfg.max_fine_opt)
        r, sc, (c, n) = db.check_hints(d[q], hints, max_fine_opt=dcfg.max_fine_opt, ranked=16)
        assert r.tobytes() == one.tobytes() and sc.tobytes() == sc1.tobytes()
        RC.check_structure(L, np.array([r]), c, n, 16, dcfg.max_fine_opt)
        rows.append(c[0])
        lists.append(lst)
    _report("hint flow", rows, lists)
    for row, lst in zip(rows, lists):
        RC.check_against_peeled(row, len(lst), lst, "hints")
    assert len(lists) >= 3
    qs = [38, 39, 40]
    qd = d[qs].contiguous()
    items = [[0, 1, 2, 3]] * 3 + [[]]
    res, hl, (c, n) = db.verify(qd, items, qidx=[0, 1, 2, 1], max_fine_opt=5, want_hints=True, ranked=16)
    ref = db.verify(qd, items, qidx=[0, 1, 2, 1], max_fine_opt=5)
    assert res.tobytes() == ref.tobytes()
    RC.check_structure(L, res, c, n, 16, 5)
    assert n[3] == 0 and res[3]["n_res"] == 0
    rows, lists = [], []
    for i, q in enumerate(qs):
        r1, _, (c1, n1) = db.check_hints(d[q], hl[i], max_fine_opt=5, ranked=16)
        assert r1.tobytes() == res[i].tobytes() and c1.tobytes() == c[i:i + 1].tobytes() and n1[0] == n[i]
        h = hl[i]
        hints = np.stack([h["cand_gidx"], h["level"], h["seq_src"], h["seq_tgt"]], 1).astype(np.int32)
        lst, first = RC.peel(oracle, desc, dcfg, q, hints, 5)
        assert int(first["n_cand_tidy"]) <= 5 and all(lst[k][1] - lst[k + 1][1] > RC.TIE_GAP for k in range(len(lst) - 1)), (q, lst)
        assert int(n[i]) == len(lst)
        rows.append(c[i])
        lists.append(lst)
    _report("verification", rows, lists)
    for row, lst in zip(rows, lists):
        RC.check_against_peeled(row, len(lst), lst, "verify")
    assert sum(len(x) >= 2 for x in lists) >= 2


def test_chunks_lanes_and_streaming(cc, oracle):
    """Part C"""
    import torch
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    ctx, d, db, plain, knn, cnt, (res, cands, n) = ranked_setup(cc, oracle)
    tail = np.array([36, 37, 38, 39, 40, 41, 48, 54], np.int32)
    qd = torch.cat([d[:1].repeat(64, 1), d[tail.tolist()]]).contiguous()
    ep = np.concatenate([np.zeros(64, np.int32), tail])
    db.set_lanes(2)
    # the synchronous host-descriptor call cuts 72 queries into chunks of 64 and 8: the lists are those of the chunk at b0 = 64
    L = cc.L
    lb, ub = L.default_thresholds()
    hq = np.ascontiguousarray(np.concatenate([desc[:1].repeat(64), desc[tail]]))
    rb = np.zeros(72, L.query_result_dt)
    cb, nb, ro = L.rank_buffers(72, 16)
    assert cc.lib().cc_db_query_batch_host_ranked(db.h, hq.ctypes.data, 72, ep.ctypes.data, C.addressof(lb), C.addressof(ub), rb.ctypes.data,
                                                  C.addressof(ro)) == 0, cc.lib().cc_last_error()
    assert not rb["n_res"][:64].any() and not nb[:64].any() and not cb[:64].tobytes().strip(b"\0")
    assert rb[64:].tobytes() == plain[tail].tobytes() and cb[64:].tobytes() == np.ascontiguousarray(cands[tail]).tobytes()
    assert np.array_equal(nb[64:], n[tail]) and nb[64:].min() >= 2
    r2, (c2, n2) = db.query(qd, ep, ranked=16)
    assert r2.tobytes() == rb.tobytes() and c2.tobytes() == cb.tobytes() and np.array_equal(n2, nb)
    # two halves with a plain batch between them, one wait
    t1, t2 = tail[:4].tolist(), tail[4:].tolist()
    a1, (ac1, an1) = db.query_submit(d[t1].contiguous(), tail[:4], ranked=16)
    aq = db.query_submit(d[58:], seeds[58:])
    a2, (ac2, an2) = db.query_submit(d[t2].contiguous(), tail[4:], ranked=5)
    db.query_wait()
    assert a1.tobytes() == plain[t1].tobytes() and a2.tobytes() == plain[t2].tobytes() and aq.tobytes() == plain[58:].tobytes()
    assert ac1.tobytes() == np.ascontiguousarray(cands[t1]).tobytes() and np.array_equal(an1, n[t1])
    assert ac2.tobytes() == np.ascontiguousarray(cands[t2][:, :5]).tobytes() and np.array_equal(an2, np.minimum(n[t2], 5))
    # a chunk larger than the zero-copy limit on each of four lanes
    db.set_lanes(4)
    big = np.arange(64, dtype=np.int32).repeat(5)
    rbig, (cbig, nbig) = db.query(d[big.tolist()].contiguous(), big, ranked=16)
    assert rbig.tobytes() == plain[big].tobytes() and cbig.tobytes() == np.ascontiguousarray(cands[big]).tobytes() and np.array_equal(nbig, n[big])
    db.set_lanes(2)


def test_large_nnk_instances(cc, oracle):
    """nnk = 100: cc_k_final_rl, peeled against the oracle (the hint flow does not depend on nnk; the oracle's replay of the
    driver loop with nnk = 100 fixes the integers)"""
    import torch
    desc, ts, seeds, dcfg0, _ = RC.drive(cc, oracle)
    L = cc.L
    dcfg = L.DbCfg.from_buffer_copy(bytes(dcfg0))
    dcfg.nnk = 100
    ctx, d = ranked_setup(cc, oracle)[:2]
    db = cc.Database(ctx, dcfg, capacity=len(desc))
    assert db.knn_stride == L.KNN_MAX_LARGE
    db.add_scans(d, ts, seeds)
    odb = oracle.DB(dcfg)
    ores = np.zeros(len(desc), L.query_result_dt)
    for i in range(len(desc)):
        s = oracle.Scan.from_desc(desc[i], int_id=i)
        ores[i] = odb.query(s)
        odb.add_scan(s, ts[i])
        odb.push_and_balance(int(seeds[i]), ts[i])
    plain = db.query(d, seeds)
    res, knn, cnt, (cands, n) = db.query(d, seeds, want_knn=True, ranked=16)
    assert res.tobytes() == plain.tobytes()
    for f in INT_FIELDS:
        assert np.array_equal(res[f], ores[f]), f
    RC.check_structure(L, res, cands, n, 16, dcfg.max_fine_opt)
    assert cnt.max() > L.KNN_MAX
    el = eligible(cc, oracle, res["n_cand_tidy"], dcfg.max_fine_opt, knn, cnt, "nnk100")
    _report("nnk = 100", [cands[q] for q in el], list(el.values()))
    for q, lst in el.items():
        RC.check_against_peeled(cands[q], int(n[q]), lst, ("nnk100", q))
    assert len(el) >= 3 and max(len(x) for x in el.values()) >= 4, {q: len(x) for q, x in el.items()}
    torch.cuda.synchronize()
    db.close()


def test_per_scan_path(cc, oracle):
    """cc_db_query_scan_batch_submit_ranked on scan handles, n = 1 and n = 8: the lists of the batch call on the same descriptors"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = cc.L
    lib = cc.lib()
    ctx, d, db = ranked_setup(cc, oracle)[:3]
    x, poses, ts2 = cc.synth.make_sequence(64, world=cc.synth.World(loop_len=40.0), beams=16, azim=450)
    qs = np.arange(36, 44, dtype=np.int32)
    hs = (C.c_void_p * 8)()
    for j, q in enumerate(qs):
        pts = np.ascontiguousarray(x[q].numpy().reshape(-1, 4), np.float32)
        h = C.c_void_p()
        assert lib.cc_scan_ingest(ctx.h, pts.ctypes.data, len(pts), 0, C.byref(h)) == 0, lib.cc_last_error()
        hs[j] = h
    hd = np.zeros(8, L.scan_desc_dt)
    for j in range(8):
        p = C.c_void_p()
        assert lib.cc_scan_desc(hs[j], C.byref(p)) == 0, lib.cc_last_error()
        C.memmove(hd[j:].ctypes.data, p, L.scan_desc_dt.itemsize)
    ref, (rc_, rn_) = db.query(_tensor(cc, hd), qs, ranked=16)
    assert int((rn_ >= 2).sum()) >= 4, rn_
    lb, ub = L.default_thresholds()
    # refusals on VALID handles: the rank argument, and thresholds that fail lb.strictSmaller(ub) -- before the handles are gathered
    r8 = np.zeros(8, L.query_result_dt)
    c8, n8, ro8 = L.rank_buffers(8, 16)
    fn = lib.cc_db_query_scan_batch_submit_ranked
    for bad in (None, L.RankOut(None, n8.ctypes.data, 16, 0), L.RankOut(c8.ctypes.data, None, 16, 0), L.RankOut(c8.ctypes.data, n8.ctypes.data, 0, 0),
                L.RankOut(c8.ctypes.data, n8.ctypes.data, 17, 0)):
        assert fn(db.h, hs, 8, qs.ctypes.data, C.addressof(lb), C.addressof(ub), r8.ctypes.data, C.addressof(bad) if bad is not None else None) == -1
    bad_ub = L.Score.from_buffer_copy(bytes(ub))
    bad_ub.i_ovlp_sum = lb.i_ovlp_sum
    assert fn(db.h, hs, 8, qs.ctypes.data, C.addressof(lb), C.addressof(bad_ub), r8.ctypes.data, C.addressof(ro8)) == -1
    assert b"cc_db_query_scan_batch_submit_ranked" in lib.cc_last_error()
    assert fn(db.h, hs, 8, np.full(8, 65, np.int32).ctypes.data, C.addressof(lb), C.addressof(ub), r8.ctypes.data, C.addressof(ro8)) == -1
    assert lib.cc_db_query_wait(db.h) == 0 and not r8.tobytes().strip(b"\0") and not n8.any() and not c8.tobytes().strip(b"\0")
    # n = 8: one chain
    assert lib.cc_db_query_scan_batch_submit_ranked(db.h, hs, 8, qs.ctypes.data, C.addressof(lb), C.addressof(ub), r8.ctypes.data, C.addressof(ro8)) == 0, \
        lib.cc_last_error()
    assert lib.cc_db_query_collect(db.h, r8.ctypes.data, 8) == 0, lib.cc_last_error()
    assert r8.tobytes() == ref.tobytes() and c8.tobytes() == rc_.tobytes() and np.array_equal(n8, rn_)
    # n = 1: the per-scan loop's query, several in flight, each collected by its own result
    r1 = np.zeros(8, L.query_result_dt)
    c1, n1, _ = L.rank_buffers(8, 16)
    keep = []
    for j in range(8):
        ro = L.RankOut(c1[j:].ctypes.data, n1[j:].ctypes.data, 16, 0)
        one = (C.c_void_p * 1)(hs[j])
        keep.append((ro, one))
        assert lib.cc_db_query_scan_batch_submit_ranked(db.h, one, 1, qs[j:].ctypes.data, C.addressof(lb), C.addressof(ub), r1[j:].ctypes.data,
                                                        C.addressof(ro)) == 0, lib.cc_last_error()
    for j in range(8):
        assert lib.cc_db_query_collect(db.h, r1[j:].ctypes.data, 1) == 0, lib.cc_last_error()
    assert r1.tobytes() == ref.tobytes() and c1.tobytes() == rc_.tobytes() and np.array_equal(n1, rn_)
    for j in range(8):
        lib.cc_scan_release(hs[j])
