"""Large-k databases (64 < nnk <= 256) on the GPU: the query chain's large-k instances against the oracle's replay of the
reference driver loop, full searches against brute force, chunking over lanes, the host-descriptor and per-scan entry
points, dynamic thresholds, and the hint flow on a large-k database.  (A large-k database always runs the walk search.)"""
import numpy as np
import pytest

from test_gpu_query import INT_FIELDS, _seq_vs_oracle, loop_sequence  # noqa: F401  (loop_sequence: the module fixture)

pytestmark = pytest.mark.gpu


def _dcfg(L, nnk):
    d = L.default_db_cfg()
    d.nnk = nnk
    return d


def test_sequence_large_nnk(cc, oracle, loop_sequence):  # noqa: F811
    """nnk = 200 on the 420-scan loop: every integer of every query result equals the oracle's, correlation and pose
    within 1e-4; the searches hold more hits than the common instance could."""
    xyzi, poses, ts = loop_sequence
    ores, res = _seq_vs_oracle(cc, oracle, xyzi, ts, dcfg=_dcfg(cc.L, 200))
    _, r50 = _seq_vs_oracle(cc, oracle, xyzi, ts)
    print("loop, per query: n_knn_hits %.0f (nnk 50: %.0f), checks %.0f (%.0f)"
          % (res["n_knn_hits"].mean(), r50["n_knn_hits"].mean(), res["cand_aft_check1"].mean(), r50["cand_aft_check1"].mean()))
    assert res["n_knn_hits"].sum() > r50["n_knn_hits"].sum()


@pytest.fixture(scope="module")
def kitti_cut(cc):
    w = cc.synth.World(kitti=True)
    idx = np.concatenate([np.arange(1484, 1684), np.arange(2667, 2837)])
    xyzi, poses, ts = cc.synth.make_sequence(0, world=w, device="cuda", indices=idx)
    return xyzi, poses, ts


def test_sequence_kitti_shaped_large_nnk(cc, oracle, kitti_cut):
    xyzi, poses, ts = kitti_cut
    ores, res = _seq_vs_oracle(cc, oracle, xyzi, ts, dcfg=_dcfg(cc.L, 200), min_hits=40)
    print("kitti-shaped nnk 200, per query: %.0f kNN hits, %.0f checks" % (res["n_knn_hits"].mean(), res["cand_aft_check1"].mean()))


def test_submit_wait_over_lanes_equals_one_query(cc, kitti_cut):
    """370 queries on an nnk = 200 database go out in chunks of <= 256: query_submit / query_wait on two and four lanes
    give what one query() call gives, hits included."""
    import torch
    xyzi, poses, ts = kitti_cut
    n, P = xyzi.shape[0], xyzi.shape[1]
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=128)
    desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
    db = cc.Database(ctx, cfg=_dcfg(cc.L, 200), capacity=n)
    assert db.knn_stride == 256
    db.add_scans(desc, ts, seeds)
    ref, knn, cnt = db.query(desc, seeds, want_knn=True)
    assert knn.shape == (n, 3, 6, 256) and cnt.max() > 64
    for lanes in (2, 4):
        db.set_lanes(lanes)
        a = db.query_submit(desc[:300], seeds[:300])
        b = db.query_submit(desc[300:], seeds[300:])
        db.query_wait()
        assert a.tobytes() == ref[:300].tobytes() and b.tobytes() == ref[300:].tobytes(), lanes
        assert db.query(desc, seeds).tobytes() == ref.tobytes()
    torch.cuda.synchronize()
    db.close()
    ctx.close()


def test_knn_near_ties_full_searches_nnk_256(cc):
    """Around every query key hundreds of DB keys whose distances differ by a few ulps, and exact duplicates: at nnk = 256
    every search is full, and every list passes knn_bruteforce_check -- sorted, unique, the f32 distances of the reference's
    accumulation order, and no visible key of a settled scan closer than the 256-th hit."""
    import torch
    from test_gpu_properties import knn_bruteforce_check
    L = cc.L
    w = cc.synth.World(loop_len=100.0)
    n = 600
    xyzi, _, _ = cc.synth.make_sequence(64, world=w, device="cuda", beams=32, azim=900)
    ctx = cc.Context(0, max_batch=64)
    P = xyzi.shape[1]
    desc0 = ctx.ingest(xyzi.reshape(-1, 4), np.arange(65, dtype=np.int64) * P)
    d0 = cc.desc_to_numpy(desc0)
    d = np.concatenate([d0] * (n // 64 + 1))[:n].copy()
    rng = np.random.default_rng(11)
    keys = d["keys"].reshape(n, 6, 6, 10)
    base = rng.uniform(150.0, 420.0, (6, 6, 10)).astype(np.float32)
    for i in range(n):
        u = rng.normal(size=(6, 6, 10))
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        r0 = 3.0 * (1.0 + rng.integers(0, 6, (6, 6, 1)) * 2.0 ** -21)
        keys[i] = (base + (u * r0).astype(np.float32)).astype(np.float32)
    keys[::7] = keys[1::7][:len(keys[::7])]
    d["keys"] = keys.reshape(d["keys"].shape)
    q = d[:48].copy()
    qk = q["keys"].reshape(48, 6, 6, 10)
    qk[:] = base[None] + rng.normal(0, 0.02, qk.shape).astype(np.float32)
    q["keys"] = qk.reshape(q["keys"].shape)
    dd = torch.from_numpy(np.frombuffer(d.tobytes(), np.uint8).reshape(n, cc.DESC_BYTES).copy()).cuda()
    dq = torch.from_numpy(np.frombuffer(q.tobytes(), np.uint8).reshape(48, cc.DESC_BYTES).copy()).cuda()
    db = cc.Database(ctx, cfg=_dcfg(L, 256), capacity=n + 8)
    db.add_scans(dd, np.arange(n) / 10.0, np.arange(n, dtype=np.int32))
    r1, knn1, cnt1 = db.query(dq, np.full(48, n, np.int32), want_knn=True, allow_flagged=True)
    assert cnt1.min() == 256, (cnt1.min(), cnt1.max())
    _, ranges = db.bucket_state()
    knn_bruteforce_check([d["keys"][:, lev].reshape(-1, 10).astype(np.float32) for lev in (1, 2, 3)], q, knn1, cnt1, ranges, n,
                         range(0, 48, 5), nnk=256, settle=300)
    db.close()
    ctx.close()


def test_host_and_per_scan_entry_points_large_nnk(cc):
    """cc_db_query_host, cc_db_query_batch_host, cc_db_query_scan and cc_db_query_scan_submit / cc_db_query_collect on an
    nnk = 200 database answer what the batched device call answers."""
    import ctypes as C
    import torch
    L = cc.L
    lib = cc.lib()
    w = cc.synth.World(loop_len=100.0)
    n = 130
    xyzi, poses, ts = cc.synth.make_sequence(n, world=w, device="cuda")
    P = xyzi.shape[1]
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=128)
    desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
    d = _dcfg(L, 200)
    d.max_elapse, d.min_elapse = 2.5, 1.5  # short DB delays: the revisits of lap 1 are searchable
    db = cc.Database(ctx, cfg=d, capacity=n + 8)
    db.add_scans(desc[:120], ts[:120], seeds[:120])
    qs = np.arange(100, 130, dtype=np.int32)
    ep = np.full(len(qs), 120, np.int32)
    ref = db.query(desc[100:130].contiguous(), ep)
    assert ref["n_knn_hits"].min() > 0
    lb, ub = L.default_thresholds()
    hdesc = np.ascontiguousarray(np.frombuffer(desc.cpu().numpy().tobytes(), dtype=L.scan_desc_dt))
    got = np.zeros(len(qs), L.query_result_dt)
    assert lib.cc_db_query_batch_host(db.h, C.c_void_p(hdesc[100:].ctypes.data), len(qs), C.c_void_p(ep.ctypes.data), C.byref(lb),
                                      C.byref(ub), C.c_void_p(got.ctypes.data)) == 0
    assert got.tobytes() == ref.tobytes()
    one = np.zeros(1, L.query_result_dt)
    for k in (0, 7, 25):
        assert lib.cc_db_query_host(db.h, C.c_void_p(hdesc[100 + k:].ctypes.data), C.byref(lb), C.byref(ub), C.c_void_p(one.ctypes.data)) == 0
        assert one.tobytes() == ref[k:k + 1].tobytes(), k
    xh = np.ascontiguousarray(xyzi.cpu().numpy().astype(np.float32))
    sub = np.zeros(3, L.query_result_dt)
    scans = []
    for j, k in enumerate((3, 11, 19)):
        h = C.c_void_p()
        assert lib.cc_scan_ingest(ctx.h, C.c_void_p(xh[100 + k].ctypes.data), C.c_int64(P), 0, C.byref(h)) == 0, lib.cc_last_error()
        scans.append(h)
        assert lib.cc_db_query_scan(db.h, h, C.byref(lb), C.byref(ub), C.c_void_p(one.ctypes.data)) == 0, lib.cc_last_error()
        assert one.tobytes() == ref[k:k + 1].tobytes(), k
        assert lib.cc_db_query_scan_submit(db.h, h, 120, C.byref(lb), C.byref(ub), C.c_void_p(sub[j:].ctypes.data)) == 0
    assert lib.cc_db_query_collect(db.h, C.c_void_p(sub.ctypes.data), 3) == 0, lib.cc_last_error()
    assert sub.tobytes() == ref[[3, 11, 19]].tobytes()
    for h in scans:
        lib.cc_scan_release(h)
    torch.cuda.synchronize()
    db.close()
    ctx.close()


def test_dynamic_thresholds_large_nnk(cc, oracle):
    """test_gpu_dynamic_thres._drive on an nnk = 128 database: both modes against tests/dyn_oracle.py."""
    from test_gpu_dynamic_thres import _drive
    w = cc.synth.World(loop_len=40.0)
    xyzi, poses, ts = cc.synth.make_sequence(120, world=w, device="cuda", beams=32, azim=900)
    d = cc.L.default_db_cfg()
    d.nnk = 128
    d.max_elapse, d.min_elapse = 2.5, 1.5
    _drive(cc, oracle, xyzi, ts, dcfg=d, min_diff=0)


def test_hints_on_a_large_nnk_database(cc):
    """The hint flow keeps the 64-stride kernels on any database: an nnk = 200 database gives the scores and the result
    an nnk = 50 one gives."""
    from test_emu_hints import _demo_hints
    import torch
    L = cc.L
    w = cc.synth.World(loop_len=100.0)
    n = 130
    xyzi, poses, ts = cc.synth.make_sequence(n, world=w, device="cuda")
    P = xyzi.shape[1]
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=128)
    desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
    hdesc = np.frombuffer(desc.cpu().numpy().tobytes(), dtype=L.scan_desc_dt)
    dbs = []
    for nnk in (50, 200):
        db = cc.Database(ctx, cfg=_dcfg(L, nnk), capacity=n)
        db.add_scans(desc, ts, seeds)
        dbs.append(db)
    n_pass = 0
    for qi in (105, 120, 129):
        cands = [qi - 100, qi - 101, qi - 99, (qi - 50) % n]
        hints = _demo_hints(L, hdesc, qi, cands)
        h = np.zeros(len(hints), L.hint_dt)
        h["cand_gidx"] = np.array(cands)[hints[:, 0]]
        h["level"], h["seq_src"], h["seq_tgt"] = hints[:, 1], hints[:, 2], hints[:, 3]
        (ra, sa), (rb, sb) = [db.check_hints(desc[qi], h, max_fine_opt=5) for db in dbs]
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes(), qi
        n_pass += int(sa["passed"].sum())
    assert n_pass > 10
    torch.cuda.synchronize()
    for db in dbs:
        db.close()
    ctx.close()
