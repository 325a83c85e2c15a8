"""Caller-given relative poses (cc_db_pose_submit / cc_db_pose_batch / cc_db_pose_batch_host: cc_k_pose_problems, cc_k_pose_select,
cc_k_pose_eval, cc_k_pose_final around the unchanged cc_k_gmm_init / cc_k_gmm_refine) on the CPU harness, against the CPU oracle
(pose_common.py): a database of the seven recorded descriptors, host descriptors, a few dozen items per call.

1 start poses from the verify flow, shifted, and pushed away until the pair count has fallen through its five classes: corr_init,
  correlation, pose, iterations and termination against oracle.gmm;  2 try poses (1, 3, 8 per item) against oracle.gmm_eval;
3 curvature with ranked_detail_common's bars, refined and unrefined;  4 agreement with the verify flow's ranked + detail rows;
5 gating and bookkeeping;  6 refusals.

Observed on the harness: 19 items with 0, 78, 235-236, 275-1 242 and 1 306-1 323 pairs (the five classes), none from which the
oracle's line search fails; corr_init / correlation / pose within 2.6e-15 / 1.4e-15 / 2.9e-13 of the oracle, try values within
3.3e-15, gradient within 1.0e-15 sqrt(H_kk), Hessian within 3.0e-12 of the half-step reference; the verify flow's six entries
reproduced exactly.  Every part prints its figures (pytest -s)."""
import numpy as np

import pose_common as PC
from emu_api import calls
from test_emu_ranked_detail import RankedDetail

_state = {}
POSE_FNS = ("cc_db_pose_submit", "cc_db_pose_batch", "cc_db_pose_batch_host")


class EmuBack(PC.Back):
    def __init__(self, cc, oracle):
        L = self.L = oracle.L
        self.desc = PC.fixture_desc(L)
        n = len(self.desc)
        self.v = RankedDetail(L, self.desc, np.arange(n) * 100.0, np.arange(n, dtype=np.int32), L.default_db_cfg())
        self.lib, self.db, self.api = self.v.lib, self.v.db, self.v.api
        self.keep = []

    def verify_d(self, lists, qidx, k):
        return self.v.verify_d(self.desc, lists, k, qidx=qidx)

    def pose(self, items, refine=1, min_corr=PC.NINF, tries=None, curv=False, submit=False):
        """synchronous: cc_db_pose_batch_host; submit=True: cc_db_pose_submit + wait; submit="no-wait": the caller waits"""
        L, p, b = self.L, self.v.p, self.v.b
        items = np.ascontiguousarray(items)
        if submit:
            r = calls.pose(self.lib, self.db, items["q"], items["gidx"], items["tf"], qdesc=self.desc.ctypes.data, n_desc=len(self.desc), refine=refine,
                           min_corr=min_corr, tries=tries, curvature=curv, wait=False, keep=self.keep)
            if submit is True:
                self.wait()
            return r.res, (r.try_corr if r.try_corr is not None and r.try_corr.shape[1] else None), r.curv
        n = len(items)
        nt = 0 if tries is None else tries.shape[1]
        tr = None if tries is None else np.ascontiguousarray(tries, np.float64)
        cfg = L.PoseCfg(int(refine), float(min_corr), nt, 0)
        res = np.zeros(n, L.pose_result_dt)
        tc = np.zeros((n, nt)) if nt else None
        cv = np.zeros(n, L.pose_curv_dt) if curv else None
        self.api.chk(self.lib.cc_db_pose_batch_host(self.db, p(self.desc), len(self.desc), p(items), n, b(cfg), p(tr), p(res), p(tc), p(cv)),
                     "cc_db_pose_batch_host")
        return res, tc, cv

    def query(self, qs):
        return self.api.db_query(self.db, self.desc[qs], np.full(len(qs), len(self.desc), np.int32))

    def query_submit(self, qs):
        res, keep = self.api.db_query_submit(self.db, self.desc[qs], np.full(len(qs), len(self.desc), np.int32))
        self.keep.append(keep)
        return res

    def wait(self):
        self.api.db_query_wait(self.db)

    def last_error(self):
        return self.lib.cc_last_error()

    def raw(self, fn, db, qdesc, items, n, cfg, tries, res, tc):
        p, b = self.v.p, self.v.b
        r = np.zeros(2, self.L.pose_result_dt)
        t = np.zeros((2, self.L.POSE_TRY_MAX + 1))
        a = [self.db if db else None, p(self.desc) if qdesc else None, len(self.desc), p(items), n, b(cfg), p(tries), p(r) if res else None,
             p(t) if tc else None, None]
        rc = getattr(self.lib, fn)(*(a if fn.endswith("_host") else a + [None]))
        return rc, r, t


def back(cc, oracle):
    if "B" not in _state:
        _state["B"] = EmuBack(cc, oracle)
    return _state["B"]


def test_abi_layout(cc):
    PC.check_abi(cc)


def test_against_the_oracle_over_the_pair_count_classes(cc, oracle):
    """Test 1"""
    PC.check_against_oracle(back(cc, oracle), oracle)


def test_try_poses(cc, oracle):
    """Test 2"""
    PC.check_tries(back(cc, oracle), oracle)


def test_curvature(cc, oracle):
    """Test 3"""
    PC.check_curvature(back(cc, oracle), oracle)


def test_agreement_with_the_verify_flow(cc, oracle):
    """Test 4"""
    PC.check_agreement(back(cc, oracle), oracle)


def test_gating_and_bookkeeping(cc, oracle):
    """Test 5"""
    PC.check_gating(back(cc, oracle), oracle)


def test_refusals(cc, oracle):
    """Test 6"""
    PC.check_refusals(back(cc, oracle), POSE_FNS)


def test_python_argument_checks(cc):
    """Database.score_poses refuses malformed shapes before the library is called"""
    import pytest
    L = cc.L
    it = L.pose_items([0, 1], [2, 3], np.zeros((2, 3)))
    assert it.dtype == L.pose_item_dt and it["gidx"].tolist() == [2, 3]
    with pytest.raises(ValueError):
        L.pose_items([0, 1], [2, 3], np.zeros((3, 3)))
