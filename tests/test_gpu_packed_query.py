"""Packed records and stored scans as the query of Database.query / verify / score_poses on the MI355X (cc_db_*_submit_packed,
cc_k_prep_packed in the place of cc_k_pack_hot + cc_k_gmm_prep).  The yardstick is the descriptor form of the same call: every
output is compared by tobytes().  The drive is the 64-scan looping world of test_dyn_thres_oracle.py (31 loop closures on the
CPU harness), ingested on the device."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy",
              "n_knn_hits"]
N = 64
_world = {}


def world(cc):
    """the drive on the device: context, descriptors, stamps, seeds, config, a two-lane database holding it, its packed records"""
    if not _world:
        L = cc.L
        dcfg = L.default_db_cfg()
        dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
        x, poses, ts = cc.synth.make_sequence(N, world=cc.synth.World(loop_len=40.0), beams=16, azim=450)
        offs = np.arange(N + 1, dtype=np.int64) * x.shape[1]
        ctx = cc.Context(0, max_batch=N)
        desc = ctx.ingest(x.reshape(-1, 4).cuda().contiguous(), offs)
        ts, seeds = np.asarray(ts), np.arange(N, dtype=np.int32)
        db = cc.Database(ctx, dcfg, capacity=N)
        db.set_lanes(2)
        db.add_scans(desc, ts, seeds)
        hot, feat = ctx.pack(desc)
        _world["v"] = (ctx, desc, ts, seeds, dcfg, db, (hot, feat), x.numpy().reshape(-1, 4), offs)
    return _world["v"]


def flat(out):
    """the numpy arrays of a call's return value, in order"""
    if isinstance(out, np.ndarray):
        return [out]
    if out is None:
        return []
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in flat(o)]
    raise TypeError(type(out))


def same_bytes(a, b):
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb)
    for k, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), ("output", k)


def not_empty(res, n_hit=4, counts=None):
    """equality of empty answers must not pass a comparing test: asserted on the descriptor path's outputs"""
    assert (res["n_res"] > 0).sum() >= n_hit, res["n_res"]
    if counts is not None:
        assert (counts >= 2).sum() >= 2, counts


def cycled(n):
    return (np.arange(n) % N).astype(np.int32)


def gather(desc, rec):
    import torch
    return desc[torch.as_tensor(np.asarray(rec, np.int64), device=desc.device)].contiguous()


# ---- 1 ----
def test_replay_from_the_database(cc, oracle):
    ctx, desc, ts, seeds, dcfg, db, packed, xh, offs = world(cc)
    ep = np.arange(N, dtype=np.int32)
    a = db.query(desc, ep)
    not_empty(a, 20)
    b = db.query(db.stored(range(N)), ep)
    same_bytes(a, b)
    ores, _, _odesc = oracle.run_sequence(xh, offs, ts, seeds, dcfg=dcfg, want_desc=True)
    for f in INT_FIELDS:
        assert np.array_equal(ores[f], b[f]), f
    m = ores["n_res"] > 0
    assert m.sum() >= 20
    assert np.abs(ores["correlation"][m] - b["correlation"][m]).max() < 1e-4
    assert np.abs(ores["tf"][m] - b["tf"][m]).max() < 1e-4


# ---- 2 ----
def test_caller_arrays(cc):
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    ep = np.arange(N, dtype=np.int32)
    a = db.query(desc, ep)
    not_empty(a)
    same_bytes(a, db.query(cc.Packed(hot, feat), ep))
    rng = np.random.RandomState(5)
    idx = np.concatenate([[0, 1, 63, 1, 63, 0], rng.permutation(N), rng.randint(0, N, 20)]).astype(np.int32)
    a = db.query(gather(desc, idx), idx)
    not_empty(a)
    same_bytes(a, db.query(cc.Packed(hot, feat, idx), idx))
    late = np.full(len(idx), N, np.int32)
    a = db.query(gather(desc, idx), late)
    not_empty(a)
    same_bytes(a, db.query(cc.Packed(hot, feat, idx), late))
    # a source of one record
    g = int(np.nonzero(a["n_res"] > 0)[0][0])
    g = int(idx[g])
    h1, f1 = ctx.pack(desc[g:g + 1])
    ep3 = np.array([g, N, N], np.int32)
    a = db.query(gather(desc, [g, g, g]), ep3)
    assert (a["n_res"] > 0).any()
    same_bytes(a, db.query(cc.Packed(h1, f1, [0, 0, 0]), ep3))


# ---- 3 ----
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_chunk_shapes(cc, n):
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    full = db.query(desc, np.arange(N, dtype=np.int32))
    rec = cycled(n) if n > 1 else np.nonzero(full["n_res"] > 0)[0][:1].astype(np.int32)
    a = db.query_submit(gather(desc, rec), rec)
    db.query_wait()
    not_empty(a, 4 if n > 1 else 1)
    b = db.query_submit(cc.Packed(hot, feat, rec), rec)
    c = db.query_submit(db.stored(rec), rec)
    db.query_wait()
    same_bytes(a, b)
    same_bytes(a, c)


@pytest.mark.parametrize("n", [1024 + 65, 1024 + 3])
def test_streamed_full_chunk_and_remainder(cc, n):
    """a full chunk of 1 024 on one lane and the remainder on the next: 65 items (with the copies) or 3 (a zero-copy chunk)"""
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    rec = cycled(n)
    a = db.query_submit(gather(desc, rec), rec)
    db.query_wait()
    not_empty(a)
    b = db.query_submit(db.stored(rec), rec)
    c = db.query_submit(cc.Packed(hot, feat, rec), rec)
    db.query_wait()
    same_bytes(a, b)
    same_bytes(a, c)


@pytest.mark.parametrize("n", [40, 130])
def test_packed_and_descriptor_chunks_alternate_on_a_lane(cc, n):
    """Each lane takes a descriptor chunk with loop closures, then a packed chunk, then a descriptor chunk again: the list heads
    and pass counters the previous chunk left behind are cleared by whichever prep kernel runs next."""
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    rec = cycled(n)
    quiet = np.zeros(n, np.int32)
    qd = gather(desc, rec)
    ref = db.query_submit(qd, rec)
    ref0 = db.query_submit(qd, quiet)
    db.query_wait()
    not_empty(ref)
    assert not ref0["n_res"].any()
    outs = []
    for k in range(2):
        outs.append((ref, db.query_submit(qd, rec)))
    for k in range(2):
        outs.append((ref0, db.query_submit(cc.Packed(hot, feat, rec), quiet)))
    for k in range(2):
        outs.append((ref, db.query_submit(db.stored(rec), rec)))
    for k in range(2):
        outs.append((ref0, db.query_submit(qd, quiet)))
    for k in range(2):
        outs.append((ref, db.query_submit(cc.Packed(hot, feat, rec), rec)))
    db.query_wait()
    for want, got in outs:
        same_bytes(want, got)


# ---- 4 ----
def test_ranked_detail_and_knn(cc):
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    rec = cycled(70)
    qd = gather(desc, rec)
    a = db.query(qd, rec, ranked=16, detail=True, want_knn=True)
    not_empty(a[0], 4, a[3][1])
    assert a[2].any()
    same_bytes(a, db.query(cc.Packed(hot, feat, rec), rec, ranked=16, detail=True, want_knn=True))
    same_bytes(a, db.query(db.stored(rec), rec, ranked=16, detail=True, want_knn=True))
    a = db.query_submit(qd, rec, ranked=16, detail=True)
    b = db.query_submit(db.stored(rec), rec, ranked=16, detail=True)
    db.query_wait()
    same_bytes(a, b)
    a = db.query(qd, rec, want_knn=True)
    same_bytes(a, db.query(db.stored(rec), rec, want_knn=True))


def _other_db(cc, dyn=False, nnk=None):
    ctx, desc, ts, seeds, dcfg0, db0, packed, xh, offs = world(cc)
    dcfg = cc.L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = dcfg0.max_elapse, dcfg0.min_elapse
    if nnk:
        dcfg.nnk = nnk
    db = cc.Database(ctx, dcfg, capacity=N)
    db.set_lanes(2)
    if dyn:
        db.set_dynamic_thres(True)
    db.add_scans(desc, ts, seeds)
    return db


def test_dynamic_thresholds(cc):
    ctx, desc, ts, seeds, dcfg, db0, (hot, feat), xh, offs = world(cc)
    db = _other_db(cc, dyn=True)
    ep = np.arange(N, dtype=np.int32)
    a = db.query(desc, ep, ranked=16, detail=True)
    not_empty(a[0], 4, a[1][1])
    same_bytes(a, db.query(db.stored(ep), ep, ranked=16, detail=True))
    same_bytes(a, db.query(cc.Packed(hot, feat), ep, ranked=16, detail=True))
    db.close()


def test_large_k_database(cc):
    ctx, desc, ts, seeds, dcfg, db0, (hot, feat), xh, offs = world(cc)
    db = _other_db(cc, nnk=128)
    assert db.knn_stride == cc.L.KNN_MAX_LARGE
    rec = cycled(70)
    a = db.query(gather(desc, rec), rec, want_knn=True)
    not_empty(a[0])
    same_bytes(a, db.query(db.stored(rec), rec, want_knn=True))
    same_bytes(a, db.query(cc.Packed(hot, feat, rec), rec, want_knn=True))
    db.close()


# ---- 5 ----
def test_verify(cc):
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    full = db.query(desc, np.arange(N, dtype=np.int32))
    qidx, cands = [], []
    for q in np.nonzero(full["n_res"] > 0)[0][:12]:
        c = int(full["cand_gidx"][q])
        lst = []
        for g in (int(q), c, c + 1, c - 1, int(q) - 1, c + 2, 3, c - 2):   # q is among its own candidates
            if 0 <= g < N and g not in lst:
                lst.append(g)
        qidx.append(int(q))
        cands.append(lst)
    assert len(qidx) >= 8 and max(len(c) for c in cands) == 8
    a = db.verify(desc, cands, qidx=qidx, want_hints=True)
    not_empty(a[0])
    assert sum(len(h) > 0 for h in a[1]) >= 4
    same_bytes(a, db.verify(db.stored(), cands, qidx=qidx, want_hints=True))
    same_bytes(a, db.verify(db.stored(qidx), cands, want_hints=True))
    same_bytes(a, db.verify(cc.Packed(hot, feat), cands, qidx=qidx, want_hints=True))
    a = db.verify(desc, cands, qidx=qidx, want_hints=True, ranked=8, detail=True)
    not_empty(a[0], 4, a[2][1])
    same_bytes(a, db.verify(db.stored(qidx), cands, want_hints=True, ranked=8, detail=True))
    a = db.verify_submit(desc, cands, qidx=qidx, ranked=8)
    b = db.verify_submit(cc.Packed(hot, feat, qidx), cands, ranked=8)
    c = db.verify_submit(db.stored(), cands, qidx=qidx)
    db.query_wait()
    same_bytes(a, b)
    same_bytes(a[0], c)


# ---- 6 ----
def test_pose(cc):
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    full = db.query(desc, np.arange(N, dtype=np.int32))
    hit = np.nonzero(full["n_res"] > 0)[0][:10]
    q = np.concatenate([hit, hit[:3], [7]]).astype(np.int32)
    g = np.concatenate([full["cand_gidx"][hit], full["cand_gidx"][hit[:3]], [7]]).astype(np.int32)
    tf = np.concatenate([full["tf"][hit] + np.array([0.4, -0.3, 0.01]), full["tf"][hit[:3]], np.zeros((1, 3))])
    tries = tf[:, None, :] + np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0.01]], np.float64)[None]
    kw = dict(tries=tries, curvature=True, min_corr=float("-inf"))
    a = db.score_poses(desc, q, g, tf, **kw)
    assert (a[0]["n_pairs"] > 0).sum() >= 4 and (a[0]["flags"] & cc.L.PF_REFINED).sum() >= 4
    assert a[0]["n_pairs"][-1] > 0, "a scan against itself at tf = 0"
    same_bytes(a, db.score_poses(db.stored(), q, g, tf, **kw))
    same_bytes(a, db.score_poses(cc.Packed(hot, feat), q, g, tf, **kw))
    big = cycled(70) % len(q)
    a = db.score_poses_submit(desc, q[big], g[big], tf[big], tries=tries[big])
    db.query_wait()
    b = db.score_poses_submit(db.stored(), q[big], g[big], tf[big], tries=tries[big])
    db.query_wait()
    same_bytes(a, b)


# ---- 7 ----
def test_stored_queries_in_flight_across_an_append(cc):
    ctx, desc, ts, seeds, dcfg0, db0, packed, xh, offs = world(cc)
    dcfg = cc.L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = dcfg0.max_elapse, dcfg0.min_elapse
    db = cc.Database(ctx, dcfg, capacity=N)
    db.set_lanes(2)
    db.add_scans(desc[:40], ts[:40], seeds[:40])
    ep = np.arange(40, dtype=np.int32)
    fly = db.query_submit(db.stored(ep), ep, ranked=4)
    db.add_scans_prepare(desc[40:])
    db.add_scans(desc[40:], ts[40:], seeds[40:])
    db.query_wait()
    assert len(db) == N
    after = db.query(db.stored(ep), ep, ranked=4)
    not_empty(after[0], 4, after[1][1])
    same_bytes(after, fly)
    same_bytes(after, db.query(desc[:40], ep, ranked=4))
    db.close()


# ---- 8 (the first three; the CPU harness runs them all) ----
def test_refusals(cc):
    ctx, desc, ts, seeds, dcfg, db, (hot, feat), xh, offs = world(cc)
    L = cc.L
    lib = cc.lib()
    ep = np.arange(N, dtype=np.int32)
    ref = db.query(desc, ep)
    fly = db.query_submit(db.stored(ep), ep)   # a chunk submitted before the refusals still delivers
    lb, ub = L.default_thresholds()
    one = np.zeros(1, np.int32)
    res = np.zeros(1, L.query_result_dt)
    tail = (one.ctypes.data, 1, one.ctypes.data, C.addressof(lb), C.addressof(ub), res.ctypes.data, None, None, None, None, None)
    assert lib.cc_db_query_submit_packed(db.h, None, *tail) == -1 and lib.cc_last_error()
    for s in (L.PackedSrc(hot.data_ptr(), None, N, 0), L.PackedSrc(None, feat.data_ptr(), N, 0), L.PackedSrc(hot.data_ptr(), feat.data_ptr(), 0, 0)):
        assert lib.cc_db_query_submit_packed(db.h, C.addressof(s), *tail) == -1 and lib.cc_last_error()
    assert not res.tobytes().strip(b"\0")
    db.query_wait()
    same_bytes(ref, fly)
    same_bytes(ref, db.query(cc.Packed(hot, feat), ep))


# ---- 9: the class mirror ----
def test_mirror_stored_methods(cc, tmp_path):
    """ContourDB::queryStored(i, i) hands out what queryRangedKNN answered for scan i during the drive; verifyStored and
    scorePosesStored what verifyCandidates and scorePoses do on the scan's ContourManager (tests/stored_mirror_check.cpp)"""
    import os
    import subprocess

    from test_emu_packed_query import mirror_outcome
    from test_mirror_read_ahead import _build, _lists
    exe = _build(tmp_path, "stored_mirror_check.cpp", "stored_mirror_check", gpu=True)
    lst, pos = _lists(cc, tmp_path, 64, 16, 450, 1.0)
    r = subprocess.run([exe, str(pos), str(lst)], env=dict(os.environ, CC_DB_READ_AHEAD="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    o = mirror_outcome(r.stdout)
    assert o["n"] == 64 and o["closed"] >= 4 and o["lists"] >= 2 and o["verified"] == 4 and o["posed"] >= 2, o
    assert o["bad"] == [0, 0, 0, 0], o
