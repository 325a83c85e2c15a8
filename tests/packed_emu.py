"""TEST INFRASTRUCTURE: ctypes driver of the *_submit_packed entry points and of their descriptor twins on the CPU harness
(tests/emu/libcc_emu.so; "device" pointers are host pointers there).  Every call returns a dict of numpy arrays whose
tobytes() are compared between the two paths."""
import ctypes as C

import numpy as np

import emu_api
from emu_api import calls

CMAX = 8  # CC_VERIFY_CANDS_MAX
CC_EINVAL = -1


def aligned(shape, dtype, align=16, off=0):
    """a zeroed C-contiguous array whose base is `off` bytes past an `align`-byte boundary"""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    raw = np.zeros(n + 2 * align, np.uint8)
    s = (-raw.ctypes.data) % align + off
    return raw[s:s + n].view(dt).reshape(shape)


def _p(a):
    return None if a is None else a.ctypes.data


def _b(s):
    return None if s is None else C.cast(C.byref(s), C.c_void_p)


class PackedEmu:
    def __init__(self, L, dcfg, cap=64, lanes=None, dyn=False, so=None):
        self.L = L
        self.api = emu_api.EmuApi(L, so)
        lib = self.lib = self.api.lib
        self.ctx = self.api.create(max_batch=8)
        self.db = self.api.db_create(self.ctx, dcfg, cap=cap)
        if lanes is not None:
            self.api.chk(lib.cc_db_set_lanes(self.db, lanes), "cc_db_set_lanes")
        if dyn:
            self.api.chk(lib.cc_db_set_dynamic_thres(self.db, 1), "cc_db_set_dynamic_thres")
        self.keep = []

    def close(self):
        self.lib.cc_db_destroy(self.db)
        self.lib.cc_destroy(self.ctx)

    def add(self, desc, ts, seeds):
        self.api.db_add(self.db, desc, ts, seeds)

    def pack(self, desc, off=0):
        """cc_pack_scans into 16-byte aligned arrays (off: bytes both bases lie past the boundary)"""
        hb, fb = self.api.packed_sizes()
        desc = np.ascontiguousarray(desc)
        hot, feat = aligned((len(desc), hb), np.uint8, off=off), aligned((len(desc), fb), np.uint8, off=off)
        self.api.chk(self.lib.cc_pack_scans(self.ctx, _p(desc), len(desc), _p(hot), _p(feat), None), "cc_pack_scans")
        return hot, feat

    def src(self, packed=None):
        """cc_packed_src_t: of (hot, feat) arrays, or of the database's own records"""
        if packed is None:
            return self.L.PackedSrc(None, None, 0, 0)
        self.keep.append(packed)  # (the struct holds bare pointers)
        return self.L.PackedSrc(packed[0].ctypes.data, packed[1].ctypes.data, len(packed[0]), 0)

    def wait(self, tolerate=()):
        rc = self.lib.cc_db_query_wait(self.db)
        if rc not in tolerate:
            self.api.chk(rc, "cc_db_query_wait")
        return rc

    def _modes(self, n, ranked, detail):
        L = self.L
        ro = rc_ = rn_ = det = None
        if ranked is not None:
            rc_, rn_, ro = L.rank_buffers(n, ranked)
        if detail:
            det = L.rank_detail_buffer(n, ranked)
        return ro, rc_, rn_, det

    @staticmethod
    def _out(res, rc_, rn_, det, **more):
        o = {"res": res}
        if rc_ is not None:
            o["rank"], o["rank_n"] = rc_, rn_
        if det is not None:
            o["detail"] = det
        o.update({k: v for k, v in more.items() if v is not None})
        return o

    def _run(self, flow, wait, raw_rc, source, *args, **kw):
        """A flow of `calls` as its submit form on `source`: a descriptor array or a cc_packed_src_t.  -> (Out, its rank pair), or
        with raw_rc (None, the submit's return code); the wait is this driver's.  raw_rc reaches the library's own validation only
        with inputs that pass the checks calls.py makes first (the lengths of idx and qidx, the shape of tries, at most
        VERIFY_CANDS_MAX candidates): those raise ValueError here; a refusal test of such an input calls self.lib directly."""
        if isinstance(source, self.L.PackedSrc):
            kw["src"] = source
        else:
            qd = np.ascontiguousarray(source)
            self.keep.append(qd)
            kw["qdesc"] = qd.ctypes.data
            if flow is not calls.query:
                kw["n_desc"] = len(qd)
        try:
            r = flow(self.lib, self.db, *args, wait=False, keep=self.keep, **kw)
        except calls.CCError as e:
            if raw_rc:
                return None, e.rc
            raise
        if raw_rc:
            return None, 0
        if wait:
            self.wait()
        rk = r.rank if getattr(r, "rank", None) is not None else (None, None)
        return r, rk

    # ---- query ----
    def query(self, source, rec, epochs, ranked=None, detail=False, want_knn=False, wait=True, lb=None, ub=None, raw_rc=False):
        """source: a descriptor array (the descriptor path on desc[rec]) or a cc_packed_src_t (the packed path on records rec;
        rec None: record i).  Returns the outputs (valid after wait()); raw_rc: the submit's return code instead."""
        L = self.L
        nq = len(np.asarray(epochs).reshape(-1))
        ks = self.lib.cc_db_knn_stride(self.db)
        knn = np.zeros((nq, 3, L.NPIV, ks), L.knn_hit_dt) if want_knn else None
        cnt = np.zeros((nq, 3, L.NPIV), np.int32) if want_knn else None
        self.keep.append((knn, cnt))
        kw = {}
        if isinstance(source, L.PackedSrc):
            kw["idx"] = rec
        elif rec is not None:
            source = source[np.asarray(rec)]
        r, rk = self._run(calls.query, wait, raw_rc, source, epochs, lb=lb, ub=ub, knn=_p(knn), knn_cnt=_p(cnt), ranked=ranked, detail=detail, **kw)
        return rk if r is None else self._out(r.res, rk[0], rk[1], r.detail, knn=knn, knn_cnt=cnt)

    # ---- verify ----
    table = staticmethod(calls.cand_table)

    def verify(self, source, qidx, cands, ranked=None, detail=False, mask=0, mfo=10, bound=1000.0, wait=True, raw_rc=False):
        n = len(cands)
        hints = np.zeros((max(n, 1), self.L.HINT_MAX), self.L.hint_dt)
        hcnt = np.zeros(max(n, 1), np.int32)
        self.keep.append((hints, hcnt))
        r, rk = self._run(calls.verify, wait, raw_rc, source, cands, qidx=qidx, levels=emu_api.levels_of(mask), max_fine_opt=mfo, max_key_dist_sq=bound,
                          hints=_p(hints), n_hints=_p(hcnt), ranked=ranked, detail=detail)
        return rk if r is None else self._out(r.res, rk[0], rk[1], r.detail, hints=hints, hint_cnt=hcnt)

    # ---- pose ----
    def pose(self, source, q, gidx, tf, tries=None, curvature=False, refine=1, min_corr=0.3, wait=True, raw_rc=False):
        r, rk = self._run(calls.pose, wait, raw_rc, source, q, gidx, tf, tries=tries, curvature=curvature, refine=refine, min_corr=min_corr)
        return rk if r is None else self._out(r.res, None, None, None, try_corr=r.try_corr, curv=r.curv)


def same_bytes(a, b):
    """every output of two calls, byte for byte"""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
