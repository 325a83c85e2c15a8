"""K3 (csrc/k_knn.h) on built keys, on the CPU harness (knn_cases.py): every search of every query of every case, walk
(cc_k_knn, cc_k_knn_l) and tiled (cc_k_knn_order + cc_k_knn_tile), is held to the oracle (R1) -- hit_cnt, gidx, level, seq and the
bits of dist_sq -- after the numpy restatement (R2) has agreed with R1 on the list and shown that the case sits on the edge its
name states.  Every part prints its cases (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_api
import knn_cases as K


class EmuBack:
    name = "harness"

    def __init__(self, oracle, so=None):
        self.L, self.so = oracle.L, so

    def run(self, case, mode):
        L = self.L
        old = os.environ.get("CC_KNN_MODE")
        os.environ["CC_KNN_MODE"] = str(mode)
        try:
            api = emu_api.EmuApi(L, self.so)
            ctx = api.create(max_batch=4)
            db = api.db_create(ctx, case.dcfg(L), cap=case.n + 1)
        finally:
            if old is None:
                os.environ.pop("CC_KNN_MODE", None)
            else:
                os.environ["CC_KNN_MODE"] = old
        api.db_add(db, case.desc(L, case.keys), case.ts, case.seeds)
        stride = api.lib.cc_db_knn_stride(db)
        if case.lanes1:
            api.chk(api.lib.cc_db_set_lanes(db, 1), "cc_db_set_lanes")
        if case.prelude:
            _, c0 = self._query(api, db, case.desc(L, K.prelude_queries()), np.full(4, case.n, np.int32), stride)
            assert c0[:, 0].min() == case.nnk
        before = self._chunks(api, db)
        knn, cnt = self._query(api, db, case.desc(L, case.q), case.epochs, stride)
        ran = self._chunks(api, db) - before
        api.lib.cc_db_destroy(db)
        api.lib.cc_destroy(ctx)
        return knn, cnt, ran

    def pieces(self, case, pieces):
        """the database built append by append: per piece (the three layers' views, the queries of that epoch, their lists and counts)"""
        L = self.L
        api = emu_api.EmuApi(L, self.so)
        ctx = api.create(max_batch=4)
        db = api.db_create(ctx, case.dcfg(L), cap=case.n + 1)
        desc, out, p0 = case.desc(L, case.keys), [], 0
        for p in pieces:
            api.db_add(db, desc[p0:p], case.ts[p0:p], case.seeds[p0:p])
            views = [K.raw_view(api.lib, db, ll) for ll in range(3)]
            sel = np.nonzero(case.epochs == p)[0]
            knn, cnt = self._query(api, db, case.desc(L, case.q[sel]), case.epochs[sel], L.KNN_MAX) if len(sel) else (None, None)
            out.append((views, sel, knn, cnt))
            p0 = p
        api.lib.cc_db_destroy(db)
        api.lib.cc_destroy(ctx)
        return out

    def _chunks(self, api, db):
        out = np.zeros(3, np.int64)
        api.chk(api.lib.cc_db_debug_knn_chunks(db, C.c_void_p(out.ctypes.data)), "cc_db_debug_knn_chunks")
        return out

    def _query(self, api, db, qd, epochs, stride):
        L = self.L
        nq = len(qd)
        knn = np.zeros((nq, L.NQLEV, L.NPIV, stride), L.knn_hit_dt)
        cnt = np.full((nq, L.NQLEV, L.NPIV), -7, np.int32)
        emu_api.calls.query(api.lib, db, epochs, qdesc=qd.ctypes.data, knn=knn.ctypes.data, knn_cnt=cnt.ctypes.data)
        return knn, cnt


_state = {}


def back(oracle):
    if "B" not in _state:
        _state["B"] = EmuBack(oracle)
    return _state["B"]


@pytest.mark.parametrize("part", K.PARTS)
def test_cases(cc, oracle, part):
    log = []
    sel = K.part(part)
    assert sel
    for case in sel:
        K.check(back(oracle), case, oracle, log)
    print("\n".join(log))


def test_views(cc, oracle):
    """D: the sorted key view after every append, and a database built in pieces against one built in a single append"""
    log = []
    for case in K.view_cases():
        K.check_views(back(oracle), case, oracle, log)
    print("\n".join(log))
