"""Pose curvature and refinement detail per ranked candidate (the *_ranked_detail entry points: cc_k_gmm_hess, cc_k_final_rd /
cc_k_final_rdl) on the MI355X, through the Python interface: the checks of test_emu_ranked_detail.py on the device against the
CPU oracle (ranked_detail_common.py) -- the verify flow on the hand-picked pairs that cover the code-list shapes, the 64-scan
drive through the query, hint and scan-handle flows, chunks above the zero-copy limit, an nnk = 100 database, dynamic
thresholds and the refusals."""
import ctypes as C

import numpy as np
import pytest

import ranked_common as RC
import ranked_detail_common as RD
from test_emu_ranked_detail import check_pairs_answer, pair_scans

pytestmark = pytest.mark.gpu

_state = {}


def _tensor(cc, desc):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(desc).tobytes(), np.uint8).reshape(len(desc), cc.DESC_BYTES).copy()).cuda()


def setup(cc, oracle):
    """the drive's descriptors (the oracle's) in a device database; ranked and detail answers at every scan's own epoch, once"""
    if not _state:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        ctx = cc.Context(0, max_batch=16)
        d = _tensor(cc, desc)
        db = cc.Database(ctx, dcfg, capacity=len(desc))
        db.add_scans(d, ts, seeds)
        r0, (c0, n0) = db.query(d, seeds, ranked=16)
        res, (c, n), det = db.query(d, seeds, ranked=16, detail=True)
        _state.update(ctx=ctx, d=d, db=db, plain=(r0, c0, n0), det=(res, c, n, det))
    s = _state
    return s["ctx"], s["d"], s["db"], s["plain"], s["det"]


def test_verify_flow_covers_the_code_list_shapes(cc, oracle):
    """Part (a)"""
    import torch
    L = cc.L
    all_desc, items, qidx = pair_scans(cc, oracle)
    n = len(all_desc)
    ctx = setup(cc, oracle)[0]
    d = _tensor(cc, all_desc)
    db = cc.Database(ctx, L.default_db_cfg(), capacity=n)
    db.add_scans(d, np.arange(n) * 100.0, np.arange(n, dtype=np.int32))
    r0, (c0, n0) = db.verify(d, items, qidx=qidx, ranked=8)
    res, (c, cnt), det = db.verify(d, items, qidx=qidx, ranked=8, detail=True)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(cnt, n0)
    check_pairs_answer(L, oracle, all_desc, qidx, res, c, cnt, det)
    # the streamed form
    rs, (cs, ns), ds = db.verify_submit(d, items, qidx=qidx, ranked=8, detail=True)
    db.query_wait()
    assert rs.tobytes() == res.tobytes() and cs.tobytes() == c.tobytes() and np.array_equal(ns, cnt) and ds.tobytes() == det.tobytes()
    torch.cuda.synchronize()
    db.close()


def test_drive_query_hint_and_scan_handle_flows(cc, oracle):
    """Part (b)"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = cc.L
    lib = cc.lib()
    ctx, d, db, (r0, c0, n0), (res, c, n, det) = setup(cc, oracle)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(n, n0), "detail changed h_res or h_cands"
    RD.check_structure(L, c, n, det, 16)
    assert int(n.sum()) >= 100
    st = RD.new_stats()
    try:
        RD.check_rows(oracle, desc, "drive", seeds, c, n, det, "query", st)
    finally:
        RD.report(st, "part (b), query flow")
    # chunks above the zero-copy limit on two lanes (the rows are copied out behind the ranked rows), and the streamed form
    big = np.arange(64, dtype=np.int32).repeat(3)
    db.set_lanes(2)
    rb, (cb, nb), dbig = db.query(d[big.tolist()].contiguous(), big, ranked=16, detail=True)
    assert rb.tobytes() == r0[big].tobytes() and cb.tobytes() == np.ascontiguousarray(c0[big]).tobytes()
    assert dbig.tobytes() == np.ascontiguousarray(det[big]).tobytes()
    sub = np.nonzero(n >= 2)[0][:12]
    r3, (c3, n3), d3 = db.query_submit(d[sub.tolist()].contiguous(), seeds[sub], ranked=3, detail=True)
    db.query_wait()
    assert d3.tobytes() == np.ascontiguousarray(det[sub][:, :3]).tobytes() and c3.tobytes() == np.ascontiguousarray(c[sub][:, :3]).tobytes()
    # the hint flow of one query, on its own kNN hits
    _, knn, kcnt = db.query(d, seeds, want_knn=True)
    q = int(np.nonzero(n >= 3)[0][0])
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, knn[q], kcnt[q]))
    r1, sc1, (c1, n1) = db.check_hints(d[q], hints, max_fine_opt=dcfg.max_fine_opt, ranked=16)
    rh, sch, (ch, nh), dh = db.check_hints(d[q], hints, max_fine_opt=dcfg.max_fine_opt, ranked=16, detail=True)
    assert rh.tobytes() == r1.tobytes() and sch.tobytes() == sc1.tobytes() and ch.tobytes() == c1.tobytes() and nh[0] == n1[0] >= 3
    RD.check_structure(L, ch, nh, dh, 16)
    RD.check_rows(oracle, desc, "drive", [q], ch, nh, dh, "hints", RD.new_stats())
    # scan handles: the rows of the batch call on the handles' descriptors; the reference on the device's descriptor of the query
    x, _, _ = cc.synth.make_sequence(64, world=cc.synth.World(loop_len=40.0), beams=16, azim=450)
    qs = np.arange(36, 40, dtype=np.int32)
    hs = (C.c_void_p * 4)()
    hd = np.zeros(4, L.scan_desc_dt)
    for j, qq in enumerate(qs):
        pts = np.ascontiguousarray(x[qq].numpy().reshape(-1, 4), np.float32)
        h = C.c_void_p()
        assert lib.cc_scan_ingest(ctx.h, pts.ctypes.data, len(pts), 0, C.byref(h)) == 0, lib.cc_last_error()
        hs[j] = h
        p = C.c_void_p()
        assert lib.cc_scan_desc(h, C.byref(p)) == 0, lib.cc_last_error()
        C.memmove(hd[j:].ctypes.data, p, L.scan_desc_dt.itemsize)
    ref, (rc_, rn_), rd_ = db.query(_tensor(cc, hd), qs, ranked=16, detail=True)
    lb, ub = L.default_thresholds()
    r4 = np.zeros(4, L.query_result_dt)
    c4, n4, ro4 = L.rank_buffers(4, 16)
    d4 = L.rank_detail_buffer(4, 16)
    assert lib.cc_db_query_scan_batch_submit_ranked_detail(db.h, hs, 4, qs.ctypes.data, C.addressof(lb), C.addressof(ub), r4.ctypes.data,
                                                           C.addressof(ro4), d4.ctypes.data) == 0, lib.cc_last_error()
    assert lib.cc_db_query_collect(db.h, r4.ctypes.data, 4) == 0, lib.cc_last_error()
    assert r4.tobytes() == ref.tobytes() and c4.tobytes() == rc_.tobytes() and np.array_equal(n4, rn_) and d4.tobytes() == rd_.tobytes()
    assert n4.sum() >= 4
    st = RD.new_stats()
    for j in range(4):
        tgt = oracle.Scan.from_desc(hd[j], int_id=int(qs[j]))
        for k in range(int(n4[j])):
            RD.check_entry(oracle, RD.scan_of(oracle, desc, c4[j][k]["cand_gidx"], "drive"), tgt, c4[j][k], d4[j][k], ("handles", j, k), st)
    RD.report(st, "part (b), scan handles")
    for j in range(4):
        lib.cc_scan_release(hs[j])


def test_large_k_database(cc, oracle):
    """Part (c): nnk = 100 (cc_k_final_rdl)"""
    import torch
    desc, ts, seeds, dcfg0, _ = RC.drive(cc, oracle)
    L = cc.L
    dcfg = L.DbCfg.from_buffer_copy(bytes(dcfg0))
    dcfg.nnk = 100
    ctx, d = setup(cc, oracle)[:2]
    db = cc.Database(ctx, dcfg, capacity=len(desc))
    assert db.knn_stride == L.KNN_MAX_LARGE
    db.add_scans(d, ts, seeds)
    qs = np.array([38, 40, 47], np.int32)
    qd = d[qs.tolist()].contiguous()
    r0, (c0, n0) = db.query(qd, qs, ranked=16)
    res, (c, n), det = db.query(qd, qs, ranked=16, detail=True)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(n, n0)
    RD.check_structure(L, c, n, det, 16)
    assert n[0] >= 2
    st = RD.new_stats()
    RD.check_rows(oracle, desc, "drive", qs, c, n, det, "large-k", st, rows=[0])
    RD.report(st, "part (c)")
    torch.cuda.synchronize()
    db.close()


def test_dynamic_thresholds(cc, oracle):
    """Part (d)"""
    import torch
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = cc.L
    ctx, d = setup(cc, oracle)[:2]
    db = cc.Database(ctx, dcfg, capacity=len(desc))
    db.add_scans(d, ts, seeds)
    db.set_dynamic_thres(1)
    qs = np.arange(34, 58, dtype=np.int32)
    qd = d[qs.tolist()].contiguous()
    r0, (c0, n0) = db.query(qd, qs, ranked=16)
    res, (c, n), det = db.query(qd, qs, ranked=16, detail=True)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(n, n0)
    RC.check_structure(L, res, c, n, 16, dcfg.max_fine_opt)
    RD.check_structure(L, c, n, det, 16)
    assert int((n >= 2).sum()) >= 5
    st = RD.new_stats()
    try:
        RD.check_rows(oracle, desc, "drive", qs, c, n, det, "dyn", st)
    finally:
        RD.report(st, "part (d)")
    torch.cuda.synchronize()
    db.close()


def test_refusals(cc, oracle):
    """Part (e): h_detail NULL and detail=True without ranked queue nothing; the size and a following plain query are unaffected"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = cc.L
    lib = cc.lib()
    ctx, d, db, (r0, c0, n0), _ = setup(cc, oracle)
    lb, ub = L.default_thresholds()
    q = np.array([38, 40], np.int32)
    qd = d[q.tolist()].contiguous()
    hq = np.ascontiguousarray(desc[q])
    res = np.zeros(2, L.query_result_dt)
    cands, cnt, ro = L.rank_buffers(2, 16)
    size = len(db)
    a = C.addressof
    tab = np.array([[0, 1, -1, -1, -1, -1, -1, -1], [2, -1, -1, -1, -1, -1, -1, -1]], np.int32)
    cfg = L.VerifyCfg(0, 5, 1000.0, 0)
    hints = np.zeros(1, L.hint_dt)
    hints["level"] = 1
    rcs = {
        "submit": lib.cc_db_query_submit_ranked_detail(db.h, qd.data_ptr(), 2, q.ctypes.data, a(lb), a(ub), res.ctypes.data, None, None, None, a(ro), None),
        "batch_host": lib.cc_db_query_batch_host_ranked_detail(db.h, hq.ctypes.data, 2, q.ctypes.data, a(lb), a(ub), res.ctypes.data, a(ro), None),
        "verify": lib.cc_db_verify_submit_ranked_detail(db.h, qd.data_ptr(), 2, None, tab.ctypes.data, 2, a(cfg), a(lb), a(ub), res.ctypes.data,
                                                        None, None, None, a(ro), None),
        "hints": lib.cc_db_check_hints_ranked_detail(db.h, qd.data_ptr(), hints.ctypes.data, 1, a(lb), a(ub), 5, res.ctypes.data, None, None, a(ro), None),
    }
    assert all(rc == -1 for rc in rcs.values()), rcs
    assert b"h_detail" in lib.cc_last_error()
    with pytest.raises(ValueError):
        db.query(qd, q, detail=True)
    with pytest.raises(ValueError):
        db.verify(qd, [[0, 1], [2]], detail=True)
    with pytest.raises(ValueError):
        db.check_hints(qd[0], hints, detail=True)
    assert lib.cc_db_query_wait(db.h) == 0
    assert not res.tobytes().strip(b"\0") and not cands.tobytes().strip(b"\0") and not cnt.any(), "a refused call wrote an answer"
    assert len(db) == size
    assert db.query(qd, q).tobytes() == r0[q].tobytes()
