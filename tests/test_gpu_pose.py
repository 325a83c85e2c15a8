"""Caller-given relative poses (Database.score_poses / score_poses_submit: cc_db_pose_batch / cc_db_pose_submit) on the MI355X,
device descriptors: tests 1-4 and 6 of test_emu_pose.py with the same bars (pose_common.py; the observed maxima are printed),
the gating checks, chunking over the lanes (1 100 items in two chunks, 300 items on an nnk = 100 database with 256-item lanes)
and the 64-scan looping drive, every ranked entry of which is re-scored from its detail row's tf_init in one pose call."""
import ctypes as C

import numpy as np
import pytest

import pose_common as PC
import ranked_common as RC

pytestmark = pytest.mark.gpu

_state = {}


def _tensor(cc, desc):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(desc).tobytes(), np.uint8).reshape(len(desc), cc.DESC_BYTES).copy()).cuda()


class GpuBack(PC.Back):
    def __init__(self, cc, dcfg=None):
        L = self.L = cc.L
        self.cc = cc
        self.desc = PC.fixture_desc(L)
        n = len(self.desc)
        self.ctx = _state.setdefault("ctx", None) or cc.Context(0, max_batch=16)
        _state["ctx"] = self.ctx
        self.d = _tensor(cc, self.desc)
        self.db = cc.Database(self.ctx, dcfg or L.default_db_cfg(), capacity=n)
        self.db.add_scans(self.d, np.arange(n) * 100.0, np.arange(n, dtype=np.int32))
        self.lib = cc.lib()
        self.keep = []

    def verify_d(self, lists, qidx, k):
        res, (c, n), det = self.db.verify(self.d, lists, qidx=qidx, ranked=k, detail=True)
        return res, c, n, det

    def pose(self, items, refine=1, min_corr=PC.NINF, tries=None, curv=False, submit=False):
        fn = self.db.score_poses_submit if submit else self.db.score_poses
        out = fn(self.d, items["q"], items["gidx"], items["tf"], refine=refine, min_corr=min_corr, tries=tries, curvature=curv)
        if submit is True:
            self.wait()
        return out

    def query(self, qs):
        return self.db.query(self.d[qs.tolist()].contiguous(), np.full(len(qs), len(self.desc), np.int32))

    def query_submit(self, qs):
        qd = self.d[qs.tolist()].contiguous()
        self.keep.append(qd)
        return self.db.query_submit(qd, np.full(len(qs), len(self.desc), np.int32))

    def wait(self):
        self.db.query_wait()

    def last_error(self):
        return self.lib.cc_last_error()

    def raw(self, fn, db, qdesc, items, n, cfg, tries, res, tc):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        r = np.zeros(2, self.L.pose_result_dt)
        t = np.zeros((2, self.L.POSE_TRY_MAX + 1))
        host = fn.endswith("_host")
        qd = (self.desc.ctypes.data if host else self.d.data_ptr()) if qdesc else None
        a = [self.db.h if db else None, qd, len(self.desc), p(items), n, C.addressof(cfg) if cfg is not None else None, p(tries),
             p(r) if res else None, p(t) if tc else None, None]
        rc = getattr(self.lib, fn)(*(a if host else a + [None]))
        return rc, r, t


def back(cc):
    if "B" not in _state:
        _state["B"] = GpuBack(cc)
    return _state["B"]


def test_against_the_oracle_over_the_pair_count_classes(cc, oracle):
    """Test 1"""
    PC.check_against_oracle(back(cc), oracle)


def test_try_poses(cc, oracle):
    """Test 2"""
    PC.check_tries(back(cc), oracle)


def test_curvature(cc, oracle):
    """Test 3"""
    PC.check_curvature(back(cc), oracle)


def test_agreement_with_the_verify_flow(cc, oracle):
    """Test 4"""
    PC.check_agreement(back(cc), oracle)


def test_gating_and_bookkeeping(cc, oracle):
    """Test 5"""
    PC.check_gating(back(cc), oracle)


def test_refusals(cc, oracle):
    """Test 6; the Python layer's own shape checks"""
    B = back(cc)
    PC.check_refusals(B, ("cc_db_pose_submit", "cc_db_pose_batch", "cc_db_pose_batch_host"))
    items, _ = PC.start_items(B)
    with pytest.raises(ValueError):
        B.db.score_poses(B.d, items["q"][:2], items["gidx"][:3], items["tf"][:2])
    with pytest.raises(ValueError):
        B.db.score_poses(B.d, items["q"][:2], items["gidx"][:2], items["tf"][:2], tries=np.zeros((2, 3)))
    with pytest.raises(cc.CCError) as e:
        B.db.score_poses(B.d, items["q"][:2], items["gidx"][:2], items["tf"][:2], tries=np.zeros((2, 9, 3)))
    assert e.value.rc == PC.EINVAL


def _chunking(B, n_big):
    """n_big items cycling over the test-1 item set, and the same content as 40 items: row i equals its template's row"""
    items, _ = PC.start_items(B)
    resA, _, cvA = PC.refined_run(B)
    tries = PC.try_poses(B)[:, :2]
    _, tA, _ = B.pose(items, refine=1, min_corr=PC.NINF, tries=np.ascontiguousarray(tries))
    for n in (n_big, 40):
        idx = np.arange(n) % len(items)
        for submit in (True, False):   # streamed: chunks of qb_max; synchronous: one chunk per lane
            r, t, cv = B.pose(items[idx], refine=1, min_corr=PC.NINF, tries=np.ascontiguousarray(tries[idx]), curv=True, submit=submit)
            PC.rows_close(r, resA[idx], ("chunking", n, submit))
            assert np.abs(t - tA[idx]).max() <= PC.SAME_BAR, (n, submit)
            for f in ("hess", "grad"):
                assert np.allclose(cv[f], cvA[f][idx], rtol=1e-9, atol=1e-12), (n, submit, f)


def test_chunking_over_the_lanes(cc, oracle):
    """1 100 items: two chunks (1 024 + 76 streamed, 576 + 524 synchronous)"""
    _chunking(back(cc), 1100)


def test_chunking_large_k_database(cc, oracle):
    """nnk = 100: lanes of 256 items; 300 items"""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.nnk = 100
    B = GpuBack(cc, dcfg)
    assert B.db.knn_stride == L.KNN_MAX_LARGE
    _chunking(B, 300)
    torch.cuda.synchronize()
    B.db.close()


def test_drive_entries_rescored(cc, oracle):
    """every ranked entry of the 64-scan drive (ranked = 16, detail), re-scored as a pose item from its tf_init: one pose call"""
    import torch
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    B = back(cc)
    d = _tensor(cc, desc)
    db = cc.Database(B.ctx, dcfg, capacity=len(desc))
    db.add_scans(d, ts, seeds)
    res, (c, n), det = db.query(d, seeds, ranked=16, detail=True)
    ents = [(q, c[q][k], det[q][k]) for q in range(len(desc)) for k in range(int(n[q]))]
    assert len(ents) >= 100
    r, _, cv = db.score_poses(d, [q for q, _, _ in ents], [int(e["cand_gidx"]) for _, e, _ in ents], [x["tf_init"] for _, _, x in ents],
                              refine=True, min_corr=PC.NINF, curvature=True)
    mx = {"corr": 0.0, "tf": 0.0, "corr_init": 0.0, "hess": 0.0}
    for i, (q, e, x) in enumerate(ents):
        PC.agree(B, q, e, x, r[i], cv[i], ("drive entry", i, q, int(e["cand_gidx"])), mx)
    print("drive: %d entries; max |corr| %.2e (beyond the f32 rounding of the entry) |tf| %.2e |corr_init| %.2e hess %.2e (scaled)"
          % (len(ents), mx["corr"], mx["tf"], mx["corr_init"], mx["hess"]))
    torch.cuda.synchronize()
    db.close()
