"""K3 (csrc/k_knn.h) on built keys, on the MI355X through the Python package (knn_cases.py): every search of every query of
every case, walk (cc_k_knn, cc_k_knn_l) and tiled (cc_k_knn_order + cc_k_knn_tile; cc_db_debug_knn_chunks says which ran), is held
to the oracle (R1) -- hit_cnt, gidx, level, seq and the bits of dist_sq -- after the numpy restatement (R2) has agreed with R1 on
the list and shown that the case sits on the edge its name states.  Every part prints its cases (pytest -s)."""
import numpy as np
import pytest

import knn_cases as K

pytestmark = pytest.mark.gpu

_state = {}


class GpuBack:
    name = "MI355X"

    def __init__(self, cc):
        import torch
        self.cc, self.L, self.torch = cc, cc.L, torch
        self.ctx = cc.Context(0, max_batch=4)

    def _tensor(self, desc):
        desc = np.ascontiguousarray(desc).reshape(-1)
        return self.torch.from_numpy(np.frombuffer(desc.tobytes(), np.uint8).reshape(len(desc), self.cc.DESC_BYTES).copy()).cuda()

    def _chunks(self, db):
        out = np.zeros(3, np.int64)
        assert self.cc.lib().cc_db_debug_knn_chunks(db.h, out.ctypes.data) == 0
        return out

    def run(self, case, mode):
        import os
        L = self.L
        old = os.environ.get("CC_KNN_MODE")
        os.environ["CC_KNN_MODE"] = str(mode)   # read when the database is created
        try:
            db = self.cc.Database(self.ctx, case.dcfg(L), capacity=case.n + 1)
        finally:
            if old is None:
                os.environ.pop("CC_KNN_MODE", None)
            else:
                os.environ["CC_KNN_MODE"] = old
        db.add_scans(self._tensor(case.desc(L, case.keys)), case.ts, case.seeds)
        if case.lanes1:
            db.set_lanes(1)
        if case.prelude:
            _, _, c0 = db.query(self._tensor(case.desc(L, K.prelude_queries())), np.full(4, case.n, np.int32), want_knn=True,
                                allow_flagged=True)
            assert c0[:, 0].min() == case.nnk
        before = self._chunks(db)
        _, knn, cnt = db.query(self._tensor(case.desc(L, case.q)), case.epochs, want_knn=True, allow_flagged=True)
        ran = self._chunks(db) - before
        db.close()
        return knn, cnt, ran


    def pieces(self, case, pieces):
        """the database built append by append: per piece (the three layers' views, the queries of that epoch, their lists and counts)"""
        L = self.L
        db = self.cc.Database(self.ctx, case.dcfg(L), capacity=case.n + 1)
        desc, out, p0 = self._tensor(case.desc(L, case.keys)), [], 0
        for p in pieces:
            db.add_scans(desc[p0:p], case.ts[p0:p], case.seeds[p0:p])
            views = [db.debug_key_view(ll) for ll in range(3)]
            sel = np.nonzero(case.epochs == p)[0]
            knn = cnt = None
            if len(sel):
                _, knn, cnt = db.query(self._tensor(case.desc(L, case.q[sel])), case.epochs[sel], want_knn=True, allow_flagged=True)
            out.append((views, sel, knn, cnt))
            p0 = p
        db.close()
        return out


def back(cc):
    if "B" not in _state:
        _state["B"] = GpuBack(cc)
    return _state["B"]


@pytest.mark.parametrize("part", K.PARTS)
def test_cases(cc, oracle, part):
    log = []
    sel = K.part(part)
    assert sel
    for case in sel:
        K.check(back(cc), case, oracle, log)
    print("\n".join(log))


def test_views(cc, oracle):
    """D: the sorted key view after every append, and a database built in pieces against one built in a single append"""
    log = []
    for case in K.view_cases():
        K.check_views(back(cc), case, oracle, log)
    print("\n".join(log))
