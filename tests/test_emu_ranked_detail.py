"""Pose curvature and refinement detail per ranked candidate (the *_ranked_detail entry points: cc_k_gmm_hess, cc_k_final_rd /
cc_k_final_rdl) on the CPU harness, against the CPU oracle (ranked_detail_common.py): the verify flow on hand-picked pairs that
cover the code-list shapes, the 64-scan drive through the query and hint flows, a large-k database, dynamic thresholds, the
refusals, the ABI layout and cc_est_sens_info.

Observed on the harness (all entries of parts a-d): gradient within 9.2e-15 sqrt(H_kk), the reference's two step sizes within
4.4e-11 of each other, the Hessian within 7.5e-12 of the half-step reference (scaled metric)."""
import ctypes as C
import os

import numpy as np

import ranked_common as RC
import ranked_detail_common as RD
from test_emu_large_nnk import _db_cfg
from emu_api import calls
from test_emu_ranked import Ranked

EINVAL = -1
HERE = os.path.dirname(os.path.abspath(__file__))
_state = {}
RANKED = ("cc_db_query_submit_ranked", "cc_db_query_batch_host_ranked", "cc_db_query_scan_batch_submit_ranked", "cc_db_verify_submit_ranked",
          "cc_db_verify_batch_host_ranked", "cc_db_check_hints_ranked", "cc_db_check_hints_host_ranked")


class RankedDetail(Ranked):
    """ctypes helper for the *_ranked_detail entry points on the harness ("device" pointers are host pointers there)"""

    def query_d(self, qdesc, epochs, k, submit=False):
        """-> (results, cands [n, k], counts [n], detail [n, k])"""
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        if submit:
            self.keep.append(qdesc)
            r = calls.query(self.lib, self.db, epochs, qdesc=qdesc.ctypes.data, ranked=k, detail=True, wait=False, keep=self.keep)
            return (r.res,) + r.rank + (r.detail,)
        lb, ub = L.default_thresholds()
        epochs = np.ascontiguousarray(epochs, np.int32)
        res = np.zeros(len(qdesc), L.query_result_dt)
        cands, cnt, ro = L.rank_buffers(len(qdesc), k)
        det = L.rank_detail_buffer(len(qdesc), k)
        rc = self.lib.cc_db_query_batch_host_ranked_detail(self.db, self.p(qdesc), len(qdesc), self.p(epochs), self.b(lb), self.b(ub),
                                                           self.p(res), self.b(ro), self.p(det))
        self.api.chk(rc, "ranked detail query")
        return res, cands, cnt, det

    def hints_d(self, qdesc, hints, k, mfo=10, host=False):
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        if not host:
            r = calls.check_hints(self.lib, self.db, qdesc.ctypes.data, hints, max_fine_opt=mfo, ranked=k, detail=True)
            return (r.res[0],) + r.rank + (r.detail,)
        lb, ub = L.default_thresholds()
        hints = np.ascontiguousarray(hints, L.hint_dt)
        res = np.zeros(1, L.query_result_dt)
        cands, cnt, ro = L.rank_buffers(1, k)
        det = L.rank_detail_buffer(1, k)
        rc = self.lib.cc_db_check_hints_host_ranked_detail(self.db, self.p(qdesc), self.p(hints), len(hints), self.b(lb), self.b(ub), int(mfo),
                                                           self.p(res), None, self.b(ro), self.p(det))
        self.api.chk(rc, "cc_db_check_hints_ranked_detail")
        return res[0], cands, cnt, det

    def verify_d(self, qdesc, cand_lists, k, qidx=None, mfo=10, bound=1000.0, host=False):
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        if not host:  # the submit followed by the wait
            r = calls.verify(self.lib, self.db, cand_lists, qdesc=qdesc.ctypes.data, n_desc=len(qdesc), qidx=qidx, levels=None, max_fine_opt=mfo,
                             max_key_dist_sq=bound, ranked=k, detail=True)
            return (r.res,) + r.rank + (r.detail,)
        lb, ub = L.default_thresholds()
        tab = self.table(cand_lists)
        n = len(tab)
        qi = None if qidx is None else np.ascontiguousarray(qidx, np.int32)
        cfg = L.VerifyCfg(0, mfo, bound, 0)
        res = np.zeros(n, L.query_result_dt)
        cands, cnt, ro = L.rank_buffers(n, k)
        det = L.rank_detail_buffer(n, k)
        rc = self.lib.cc_db_verify_batch_host_ranked_detail(self.db, self.p(qdesc), len(qdesc), self.p(qi), self.p(tab), n, self.b(cfg),
                                                            self.b(lb), self.b(ub), self.p(res), self.b(ro), self.p(det))
        self.api.chk(rc, "cc_db_verify_batch_host_ranked_detail")
        return res, cands, cnt, det


def pair_scans(cc, oracle):
    """The scans of part (a): the seven recorded descriptors with long pair lists (tests/golden/make_ranked_detail_fixture.py: a
    KITTI-shaped scan and two small moves of it, two dense-world scans and two moves) followed by six scans of the sparse
    looping drive (0, 1, 16, 17, 37, 38), and the items verified on them."""
    L = oracle.L
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    fx = np.load(os.path.join(HERE, "golden", "ranked_detail_scans.npz"))["desc"]
    fx = np.frombuffer(fx.tobytes(), L.scan_desc_dt)
    all_desc = np.concatenate([fx, desc[[0, 1, 16, 17, 37, 38]]])
    items = [[1, 2, 3, 4, 5, 6, 7, 8],   # the KITTI-shaped scan against its two moves (> 1 280 pairs) and six others: eight candidates
             [4, 5, 6],                  # the dense scan against its moves and its neighbour (257 .. 1 280)
             [7, 8, 9, 10, 11],          # drive scan 38 against 0, 1, 16, 17, 37 (<= 64)
             [0, 2]]
    qidx = [0, 3, 12, 1]
    return all_desc, items, qidx


def check_pairs_answer(L, oracle, all_desc, qidx, res, c, n, det):
    RC.check_structure(L, res, c, n, 8, 10)
    RD.check_structure(L, c, n, det, 8)
    npairs = np.concatenate([det[i]["n_pairs"][:n[i]] for i in range(len(n))])
    print("part (a): entries per item", n.tolist(), "n_pairs", sorted(npairs.tolist()))
    assert (npairs <= 64).any() and ((npairs >= 257) & (npairs <= 1280)).any() and (npairs > 1280).any(), sorted(npairs.tolist())
    assert n[0] >= 2 and n[2] >= 3, "several candidates of one item should survive"
    st = RD.new_stats()
    try:
        RD.check_rows(oracle, all_desc, "pairs", qidx, c, n, det, "verify", st)
    finally:
        RD.report(st, "part (a)")


def setup(cc, oracle):
    if not _state:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        v = RankedDetail(oracle.L, desc, ts, seeds, dcfg)
        _state.update(v=v, plain=v.query(desc, seeds, 16), det=v.query_d(desc, seeds, 16))
    return _state["v"], _state["plain"], _state["det"]


def test_abi_layout(cc):
    """sizeof(cc_ranked_detail_t) == 120 and the numpy record has the C struct's offsets"""
    import subprocess
    import tempfile
    L = cc.L
    root = os.path.dirname(HERE)
    names = ("hess", "grad", "tf_init", "corr_init", "iterations", "termination", "n_pairs", "flags")
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "cont2_amd.h"\nint main(void) { printf("%zu' + " %zu" * len(names) + '\\n", '
           'sizeof(cc_ranked_detail_t), ' + ", ".join("offsetof(cc_ranked_detail_t, %s)" % f for f in names) + "); return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(td, "t")]).split()]
    dt = L.ranked_detail_dt
    assert got == [120] + [dt.fields[f][1] for f in names], got
    assert dt.itemsize == 120 and got[1:] == [0, 48, 72, 96, 104, 108, 112, 116]
    assert L.rank_detail_buffer(3, 5).shape == (3, 5)


def test_verify_flow_covers_the_code_list_shapes(cc, oracle):
    """Part (a)"""
    L = oracle.L
    all_desc, items, qidx = pair_scans(cc, oracle)
    n = len(all_desc)
    v = RankedDetail(L, all_desc, np.arange(n) * 100.0, np.arange(n, dtype=np.int32), L.default_db_cfg())
    res, c, cnt, det = v.verify_d(all_desc, items, 8, qidx=qidx)
    r0, c0, n0, _ = v.verify(all_desc, items, 8, qidx=qidx)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(cnt, n0)
    check_pairs_answer(L, oracle, all_desc, qidx, res, c, cnt, det)
    # the synchronous host form gives the same bytes
    rh, ch, nh, dh = v.verify_d(all_desc, items, 8, qidx=qidx, host=True)
    assert rh.tobytes() == res.tobytes() and ch.tobytes() == c.tobytes() and np.array_equal(nh, cnt) and dh.tobytes() == det.tobytes()


def test_drive_query_and_hint_flows(cc, oracle):
    """Part (b)"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, (r0, c0, n0), (res, c, n, det) = setup(cc, oracle)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(n, n0), "detail changed h_res or h_cands"
    RD.check_structure(L, c, n, det, 16)
    assert int(n.sum()) >= 100
    st = RD.new_stats()
    try:
        RD.check_rows(oracle, desc, "drive", seeds, c, n, det, "query", st)
    finally:
        RD.report(st, "part (b), query flow")
    # a shorter list is the prefix; the streamed form gives the same rows
    sub = np.nonzero(n >= 2)[0][:12]
    r3, c3, n3, d3 = v.query_d(desc[sub], seeds[sub], 3, submit=True)
    v.api.db_query_wait(v.db)
    assert d3.tobytes() == np.ascontiguousarray(det[sub][:, :3]).tobytes() and c3.tobytes() == np.ascontiguousarray(c[sub][:, :3]).tobytes()
    # the hint flow of one query, on its own kNN hits
    _, knn, kcnt = v.api.db_query(v.db, desc, seeds, want_knn=True)
    q = int(np.nonzero(n >= 3)[0][0])
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, knn[q], kcnt[q]))
    r1, c1, n1 = v.hints(desc[q:q + 1], hints, 16, mfo=dcfg.max_fine_opt)
    for host in (False, True):
        rh, ch, nh, dh = v.hints_d(desc[q:q + 1], hints, 16, mfo=dcfg.max_fine_opt, host=host)
        assert rh.tobytes() == r1.tobytes() and ch.tobytes() == c1.tobytes() and nh[0] == n1[0] >= 3
        RD.check_structure(L, ch, nh, dh, 16)
        st = RD.new_stats()
        RD.check_rows(oracle, desc, "drive", [q], ch, nh, dh, "hints", st)


def test_large_k_database(cc, oracle):
    """Part (c): nnk = 100 (cc_k_final_rdl)"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v = RankedDetail(L, desc, ts, seeds, _db_cfg(L, 100))
    qs = np.array([38, 40, 47], np.int32)
    r0, c0, n0 = v.query(desc[qs], qs, 16)
    res, c, n, det = v.query_d(desc[qs], qs, 16)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(n, n0)
    RD.check_structure(L, c, n, det, 16)
    assert n[0] >= 2
    st = RD.new_stats()
    RD.check_rows(oracle, desc, "drive", qs, c, n, det, "large-k", st, rows=[0])
    RD.report(st, "part (c)")


def test_dynamic_thresholds(cc, oracle):
    """Part (d)"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v = RankedDetail(L, desc, ts, seeds, dcfg)
    assert v.lib.cc_db_set_dynamic_thres(v.db, 1) == 0
    qs = np.arange(34, 58, dtype=np.int32)
    r0, c0, n0 = v.query(desc[qs], qs, 16)
    res, c, n, det = v.query_d(desc[qs], qs, 16)
    assert res.tobytes() == r0.tobytes() and c.tobytes() == c0.tobytes() and np.array_equal(n, n0)
    RC.check_structure(L, res, c, n, 16, dcfg.max_fine_opt)
    RD.check_structure(L, c, n, det, 16)
    assert int((n >= 2).sum()) >= 5
    st = RD.new_stats()
    try:
        RD.check_rows(oracle, desc, "drive", qs, c, n, det, "dyn", st)
    finally:
        RD.report(st, "part (d)")


def test_refusals(cc, oracle):
    """Part (e): h_detail NULL (and what the ranked call refuses) queues nothing; the handle stays usable"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, (r0, c0, n0), _ = setup(cc, oracle)
    lb, ub = L.default_thresholds()
    q = np.array([38, 40], np.int32)
    qd = np.ascontiguousarray(desc[q])
    res = np.zeros(2, L.query_result_dt)
    cands, cnt, ro = L.rank_buffers(2, 16)
    det = L.rank_detail_buffer(2, 16)
    _, knn, kcnt = v.api.db_query(v.db, desc[38:39], seeds[38:39], want_knn=True)
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, knn[0], kcnt[0]))
    tab = v.table([[0, 1], [2]])
    cfg = L.VerifyCfg(0, 5, 1000.0, 0)
    p, b = v.p, v.b
    size = v.lib.cc_db_size(v.db)

    def calls(r, d):
        lib = v.lib
        yield "submit", lib.cc_db_query_submit_ranked_detail(v.db, p(qd), 2, p(q), b(lb), b(ub), p(res), None, None, None, r, d)
        yield "batch_host", lib.cc_db_query_batch_host_ranked_detail(v.db, p(qd), 2, p(q), b(lb), b(ub), p(res), r, d)
        yield "scan_batch", lib.cc_db_query_scan_batch_submit_ranked_detail(v.db, None, 1, p(q), b(lb), b(ub), p(res), r, d)
        yield "verify", lib.cc_db_verify_submit_ranked_detail(v.db, p(qd), 2, None, p(tab), 2, b(cfg), b(lb), b(ub), p(res), None, None, None, r, d)
        yield "verify_host", lib.cc_db_verify_batch_host_ranked_detail(v.db, p(qd), 2, None, p(tab), 2, b(cfg), b(lb), b(ub), p(res), r, d)
        yield "hints", lib.cc_db_check_hints_ranked_detail(v.db, p(qd), p(hints), len(hints), b(lb), b(ub), 5, p(res), None, None, r, d)
        yield "hints_host", lib.cc_db_check_hints_host_ranked_detail(v.db, p(qd), p(hints), len(hints), b(lb), b(ub), 5, p(res), None, r, d)

    pend = v.query_d(qd, q, 16, submit=True)  # a detail chunk in flight while every refusal is made
    for fn, rc in calls(b(ro), None):
        assert rc == EINVAL, ("h_detail NULL", fn, rc)
        assert b"h_detail" in v.lib.cc_last_error(), v.lib.cc_last_error()
    for what, bad in (("rank NULL", None), ("max_ret 17", L.RankOut(cands.ctypes.data, cnt.ctypes.data, 17, 0)),
                      ("h_n NULL", L.RankOut(cands.ctypes.data, None, 16, 0))):
        for fn, rc in calls(b(bad), p(det)):
            assert rc == EINVAL, (what, fn, rc)
    bad_ub = L.Score.from_buffer_copy(bytes(ub))
    bad_ub.i_ovlp_sum = lb.i_ovlp_sum
    assert v.lib.cc_db_query_submit_ranked_detail(v.db, p(qd), 2, p(q), b(lb), b(bad_ub), p(res), None, None, None, b(ro), p(det)) == EINVAL
    assert not res.tobytes().strip(b"\0") and not cands.tobytes().strip(b"\0") and not cnt.any() and not det.tobytes().strip(b"\0"), \
        "a refused call wrote an answer"
    assert v.lib.cc_db_size(v.db) == size
    v.api.db_query_wait(v.db)
    assert pend[0].tobytes() == r0[q].tobytes() and pend[1].tobytes() == np.ascontiguousarray(c0[q]).tobytes()
    assert pend[3].tobytes() == np.ascontiguousarray(_state["det"][3][q]).tobytes()
    after = v.api.db_query(v.db, desc[q], q)
    assert after.tobytes() == r0[q].tobytes()


def test_python_detail_needs_ranked(cc):
    """detail=True without ranked is a ValueError, raised before the library is called (Database._detail_args)"""
    import pytest
    with pytest.raises(ValueError):
        cc.Database._detail_args(4, None, True)
    assert cc.Database._detail_args(4, None, False) is None and cc.Database._detail_args(4, 3, True).shape == (4, 3)


def test_est_sens_info(cc, oracle):
    """Part (f): J^-T H J^-1 with J from central differences of cc_est_sens_tf (affine in the translation; the theta column by a
    five-point difference, whose error at h = 1e-3 is h^4 / 30 of the lever arm's fifth derivative: ~3e-12 relative)"""
    import emu_api
    lib = emu_api.abi.bind(C.CDLL(emu_api.build()))
    rng = np.random.default_rng(5)

    def sens(tf, nr, nc):
        tf = np.ascontiguousarray(tf, np.float64)
        out = np.zeros(3)
        lib.cc_est_sens_tf(tf.ctypes.data, nr, nc, out.ctypes.data)
        return out

    for nr, nc in ((150, 150), (120, 200)):
        for _ in range(8):
            A = rng.normal(size=(3, 3))
            H = A @ A.T + 0.1 * np.eye(3)
            h6 = np.ascontiguousarray(H[np.triu_indices(3)])
            tf = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-3, 3)])
            out = np.zeros(6)
            lib.cc_est_sens_info(h6.ctypes.data, tf.ctypes.data, nr, nc, out.ctypes.data)
            J = np.zeros((3, 3))
            for k, h in enumerate((0.5, 0.5, 1e-3)):
                e = np.zeros(3)
                e[k] = h
                J[:, k] = (-sens(tf + 2 * e, nr, nc) + 8 * sens(tf + e, nr, nc) - 8 * sens(tf - e, nr, nc) + sens(tf - 2 * e, nr, nc)) / (12 * h)
            Ji = np.linalg.inv(J)
            ref = Ji.T @ H @ Ji
            got = RD.mat(out)
            assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), (got, ref)
