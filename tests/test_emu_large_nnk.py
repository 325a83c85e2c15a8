"""Large-k databases (CC_KNN_MAX < nnk <= CC_KNN_MAX_LARGE) on the CPU harness: cc_db_create's bounds, the d_knn stride, and
the whole query chain's large-k instances (cc_k_knn_l ... cc_k_final_l) against the oracle's replay of the reference loop."""
import ctypes as C

import numpy as np
import pytest

import emu_api

INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy",
              "n_knn_hits"]


def _db_cfg(L, nnk, qlv=(1, 2, 3)):
    d = L.default_db_cfg()
    d.max_elapse, d.min_elapse = 2.5, 1.5
    d.nnk, d.n_q_levels = nnk, len(qlv)
    for i, v in enumerate(qlv):
        d.q_levels[i] = v
    return d


def _query(api, db, qdesc, epochs, stride, lb=None, ub=None):
    """cc_db_query_batch with hit buffers of the database's stride (emu_api.db_query sizes them for CC_KNN_MAX)."""
    L = api.L
    if lb is None:
        lb, ub = L.default_thresholds()
    qdesc = np.ascontiguousarray(qdesc)
    epochs = np.ascontiguousarray(epochs, np.int32)
    nq = len(epochs)
    res = np.zeros(nq, L.query_result_dt)
    knn = np.zeros((nq, L.NQLEV, L.NPIV, stride), L.knn_hit_dt)
    cnt = np.zeros((nq, L.NQLEV, L.NPIV), np.int32)
    api.chk(api.lib.cc_db_query_batch(db, C.c_void_p(qdesc.ctypes.data), nq, C.c_void_p(epochs.ctypes.data), C.byref(lb),
                                      C.byref(ub), C.c_void_p(res.ctypes.data), C.c_void_p(knn.ctypes.data),
                                      C.c_void_p(cnt.ctypes.data), None), "cc_db_query_batch")
    return res, knn, cnt


def test_layouts_export_the_large_bound(oracle):
    assert oracle.L.KNN_MAX == 64 and oracle.L.KNN_MAX_LARGE == 256


def test_create_accepts_nnk_up_to_256(oracle):
    L = oracle.L
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=8)
    for nnk, stride in ((1, 64), (50, 64), (64, 64), (65, 256), (128, 256), (200, 256), (256, 256)):
        db = api.db_create(ctx, _db_cfg(L, nnk), cap=16)
        assert api.lib.cc_db_knn_stride(db) == stride, nnk
        api.lib.cc_db_destroy(db)
    for nnk in (0, 257, 1000):
        h = C.c_void_p()
        rc = api.lib.cc_db_create(ctx, C.byref(_db_cfg(L, nnk)), 16, C.byref(h))
        assert rc == -1, nnk
        assert b"256" in api.lib.cc_last_error(), api.lib.cc_last_error()
    assert api.lib.cc_db_knn_stride(None) == 0


def _sequence(cc, oracle, d, lb=None, ub=None):
    w = cc.synth.World(loop_len=40.0)
    n = 64
    x, poses, ts = cc.synth.make_sequence(n, world=w, beams=16, azim=450)
    xs = x.numpy().reshape(-1, 4)
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(xs, offs, ts, seeds, dcfg=d, lb=lb, ub=ub, want_desc=True)
    return n, ts, seeds, ores, odesc


@pytest.mark.parametrize("qlv", [(1, 2, 3), (2, 3, 4)])
@pytest.mark.parametrize("nnk", [65, 128, 256])
def test_large_nnk_loop_sequence_matches_oracle(cc, oracle, nnk, qlv):
    """Every integer field equals the oracle's, correlation and pose within 1e-6; the hit counts per search are the
    oracle's min(visible keys within dist_ub, nnk) (n_knn_hits) and the lists are sorted by (distance, key order).
    (A large-k database always walks: the tiled search has no large-k instance, whatever CC_KNN_MODE says.)"""
    L = oracle.L
    d = _db_cfg(L, nnk, qlv)
    n, ts, seeds, ores, odesc = _sequence(cc, oracle, d)
    hit = np.nonzero(ores["n_res"] > 0)[0]
    assert len(hit) >= 3
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=8)
    db = api.db_create(ctx, d, cap=n)
    assert api.lib.cc_db_knn_stride(db) == 256
    api.db_add(db, odesc, ts, seeds)
    qs = np.unique(np.concatenate([hit[:3], [20, n - 1]])).astype(np.int32)
    res, knn, cnt = _query(api, db, odesc[qs], qs, 256)
    for k, qi in enumerate(qs):
        for f in INT_FIELDS:
            assert ores[f][qi] == res[f][k], (qi, f, ores[f][qi], res[f][k])
        if ores["n_res"][qi]:
            assert abs(ores["correlation"][qi] - res["correlation"][k]) < 1e-6
            assert np.abs(ores["tf"][qi] - res["tf"][k]).max() < 1e-6
    assert cnt.max() <= nnk and (cnt.sum(axis=(1, 2)) == res["n_knn_hits"]).all()
    for q in range(len(qs)):
        for ll in range(L.NQLEV):
            for s in range(L.NPIV):
                c = cnt[q, ll, s]
                dd = knn["dist_sq"][q, ll, s, :c]
                assert (np.diff(dd) >= 0).all()
                assert (knn["level"][q, ll, s, :c] == qlv[ll]).all() if ll < len(qlv) else c == 0
    api.lib.cc_db_destroy(db)


def test_large_nnk_first_64_hits_equal_the_common_instance(cc, oracle):
    """The first min(cnt, 64) hits of an nnk = 128 search are an nnk = 64 search's hits when the 64-th distance is the
    radius of both (no crowd of equal distances at it): the two instances agree on what they share."""
    L = oracle.L
    d64, d128 = _db_cfg(L, 64), _db_cfg(L, 128)
    n, ts, seeds, ores, odesc = _sequence(cc, oracle, d64)
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=8)
    out = []
    for d, stride in ((d64, 64), (d128, 256)):
        db = api.db_create(ctx, d, cap=n)
        api.db_add(db, odesc, ts, seeds)
        qs = np.arange(40, n, 4, dtype=np.int32)
        out.append(_query(api, db, odesc[qs], qs, stride))
        api.lib.cc_db_destroy(db)
    (_, k64, c64), (_, k128, c128) = out
    assert (np.minimum(c128, 64) == c64).all()
    for f in ("gidx", "level", "seq", "dist_sq"):
        a, b = k64[f], k128[f][..., :64]
        m = np.arange(64)[None, None, None, :] < c64[..., None]
        assert (a[m] == b[m]).all(), f


def test_large_nnk_dynamic_thresholds_match_the_oracle(cc, oracle):
    """cc_db_set_dynamic_thres on an nnk = 128 database: the replay kernels' large-k instances against tests/dyn_oracle.py."""
    import dyn_oracle
    L = oracle.L
    d = _db_cfg(L, 128)
    lb, ub = L.default_thresholds()
    w = cc.synth.World(loop_len=40.0)
    n = 64
    x, poses, ts = cc.synth.make_sequence(n, world=w, beams=16, azim=450)
    xs = x.numpy().reshape(-1, 4)
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    _, _, odesc = oracle.run_sequence(xs, offs, ts, seeds, dcfg=d, lb=lb, ub=ub, want_desc=True)
    ores = dyn_oracle.run_sequence(odesc, ts, seeds, d, lb=lb, ub=ub, dyn=1)
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=8)
    db = api.db_create(ctx, d, cap=n)
    api.chk(api.lib.cc_db_set_dynamic_thres(db, 1), "cc_db_set_dynamic_thres")
    api.db_add(db, odesc, ts, seeds)
    qs = np.arange(20, n, 3, dtype=np.int32)
    res, _, _ = _query(api, db, odesc[qs], qs, 256, lb, ub)
    for k, qi in enumerate(qs):
        for f in INT_FIELDS:
            assert ores[f][qi] == res[f][k], (qi, f, ores[f][qi], res[f][k])
        if ores["n_res"][qi]:
            assert abs(ores["correlation"][qi] - res["correlation"][k]) < 1e-6
            assert np.abs(ores["tf"][qi] - res["tf"][k]).max() < 1e-6
    api.lib.cc_db_destroy(db)


def _fake_desc(L, rng, n):
    from test_hostdb_bookkeeping import _fake_desc as f
    return f(L, rng, n)


@pytest.mark.parametrize("nnk", [65, 200, 256])
def test_knn_crowded_layer_large_nnk_matches_oracle(oracle, nnk):
    """The capacity case of the large-k walk: thousands of near-identical keys, so every 64-key step passes the radius
    test and the pending list reaches 2 nnk - 1 + 64 entries (575 at nnk = 256, sorted in the 1 024-entry network) before
    it is tightened.  Every search is full, and every hit list equals the oracle's whole list (tests/knn_full_oracle.cpp:
    QueryDebug::knn, all nnk entries), so a radius that tightened too early would show."""
    import knn_oracle
    L = oracle.L
    rng = np.random.default_rng(21)
    n = 450
    desc = _fake_desc(L, rng, n)
    base = rng.uniform(8.0, 12.0, L.KEY_DIM).astype(np.float32)
    desc["keys"] = (base[None, None, None, :] + rng.normal(0, 0.05, (n, L.NLEV, L.NPIV, L.KEY_DIM))).astype(np.float32)
    ts = np.arange(n) * 0.1
    seeds = np.arange(n, dtype=np.int32)
    dcfg = L.default_db_cfg()
    dcfg.nnk = nnk
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=4)
    db = api.db_create(ctx, dcfg, cap=n)
    api.db_add(db, desc, ts, seeds)
    odb = knn_oracle.DB(dcfg)
    for i in range(n):
        odb.add(desc[i], ts[i], i)
    q = desc[[3, 420]].copy()
    q["keys"] += np.float32(0.01)
    res, knn, cnt = _query(api, db, q, np.full(2, n, np.int32), 256)
    for kq in range(2):
        oknn, ocnt = odb.query_knn(q[kq], 10000 + kq)
        assert np.array_equal(ocnt, cnt[kq]) and ocnt.min() == nnk
        for f in ("gidx", "level", "seq", "dist_sq"):
            assert np.array_equal(oknn[f][..., :nnk], knn[kq][f][..., :nnk]), f
    odb.close()
    api.lib.cc_db_destroy(db)
