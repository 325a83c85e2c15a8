"""TEST INFRASTRUCTURE: ctypes driver of the *_submit_packed entry points and of their descriptor twins on the CPU harness
(tests/emu/libcc_emu.so; "device" pointers are host pointers there).  Every call returns a dict of numpy arrays whose
tobytes() are compared between the two paths."""
import ctypes as C

import numpy as np

import emu_api

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
    return None if a is None else C.c_void_p(a.ctypes.data)


def _b(s):
    return None if s is None else C.cast(C.byref(s), C.c_void_p)


class PackedEmu:
    def __init__(self, L, dcfg, cap=64, lanes=None, dyn=False, so=None):
        self.L = L
        self.api = emu_api.EmuApi(L, so)
        lib = self.lib = self.api.lib
        for f in ("cc_db_query_submit_packed", "cc_db_verify_submit_packed", "cc_db_pose_submit_packed", "cc_db_query_submit_ranked",
                  "cc_db_query_submit_ranked_detail", "cc_db_verify_submit", "cc_db_verify_submit_ranked", "cc_db_verify_submit_ranked_detail",
                  "cc_db_pose_submit", "cc_db_set_lanes", "cc_db_set_dynamic_thres", "cc_db_knn_stride"):
            getattr(lib, f).restype = C.c_int
        V = C.c_void_p
        lib.cc_db_query_submit_packed.argtypes = [V, V, V, C.c_int] + [V] * 9
        lib.cc_db_verify_submit_packed.argtypes = [V, V, V, V, C.c_int] + [V] * 9
        lib.cc_db_pose_submit_packed.argtypes = [V, V, V, C.c_int] + [V] * 6
        lib.cc_db_query_submit.argtypes = [V, V, C.c_int] + [V] * 7
        lib.cc_db_query_submit_ranked.argtypes = [V, V, C.c_int] + [V] * 8
        lib.cc_db_query_submit_ranked_detail.argtypes = [V, V, C.c_int] + [V] * 9
        lib.cc_db_verify_submit.argtypes = [V, V, C.c_int, V, V, C.c_int] + [V] * 7
        lib.cc_db_verify_submit_ranked.argtypes = [V, V, C.c_int, V, V, C.c_int] + [V] * 8
        lib.cc_db_verify_submit_ranked_detail.argtypes = [V, V, C.c_int, V, V, C.c_int] + [V] * 9
        lib.cc_db_pose_submit.argtypes = [V, V, C.c_int, V, C.c_int] + [V] * 6
        lib.cc_db_set_lanes.argtypes = [V, C.c_int]
        lib.cc_db_set_dynamic_thres.argtypes = [V, C.c_int]
        lib.cc_db_knn_stride.argtypes = [V]
        lib.cc_db_query_wait.argtypes = [V]
        lib.cc_db_size.argtypes = [V]
        self.ctx = self.api.create(max_batch=8)
        self.db = self.api.db_create(self.ctx, dcfg, cap=cap)
        if lanes is not None:
            self.api.chk(lib.cc_db_set_lanes(self.db, lanes), "cc_db_set_lanes")
        if dyn:
            self.api.chk(lib.cc_db_set_dynamic_thres(self.db, 1), "cc_db_set_dynamic_thres")
        self.keep = []

    def close(self):
        self.lib.cc_db_destroy.argtypes = [C.c_void_p]
        self.lib.cc_db_destroy(self.db)
        self.lib.cc_destroy.argtypes = [C.c_void_p]
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

    # ---- query ----
    def query(self, source, rec, epochs, ranked=None, detail=False, want_knn=False, wait=True, lb=None, ub=None, raw_rc=False):
        """source: a descriptor array (the descriptor path on desc[rec]) or a cc_packed_src_t (the packed path on records rec;
        rec None: record i).  Returns the outputs (valid after wait()); raw_rc: the submit's return code instead."""
        L = self.L
        if lb is None:
            lb, ub = L.default_thresholds()
        epochs = np.ascontiguousarray(epochs, np.int32)
        nq = len(epochs)
        res = np.zeros(nq, L.query_result_dt)
        ro, rc_, rn_, det = self._modes(nq, ranked, detail)
        ks = self.lib.cc_db_knn_stride(self.db)
        knn = np.zeros((nq, 3, L.NPIV, ks), L.knn_hit_dt) if want_knn else None
        cnt = np.zeros((nq, 3, L.NPIV), np.int32) if want_knn else None
        if isinstance(source, L.PackedSrc):
            r = None if rec is None else np.ascontiguousarray(rec, np.int32)
            self.keep.append((source, r, epochs, res, ro, rc_, rn_, det, knn, cnt))
            rc = self.lib.cc_db_query_submit_packed(self.db, _b(source), _p(r), nq, _p(epochs), _b(lb), _b(ub), _p(res), _p(knn), _p(cnt), None,
                                                    _b(ro), _p(det))
        else:
            qd = np.ascontiguousarray(source if rec is None else source[np.asarray(rec)])
            self.keep.append((qd, epochs, res, ro, rc_, rn_, det, knn, cnt))
            head = (self.db, _p(qd), nq, _p(epochs), _b(lb), _b(ub), _p(res), _p(knn), _p(cnt), None)
            if det is not None:
                rc = self.lib.cc_db_query_submit_ranked_detail(*head, _b(ro), _p(det))
            elif ro is not None:
                rc = self.lib.cc_db_query_submit_ranked(*head, _b(ro))
            else:
                rc = self.lib.cc_db_query_submit(*head)
        if raw_rc:
            return rc
        self.api.chk(rc, "query submit")
        if wait:
            self.wait()
        return self._out(res, rc_, rn_, det, knn=knn, knn_cnt=cnt)

    # ---- verify ----
    @staticmethod
    def table(cands):
        tab = np.full((len(cands), CMAX), -1, np.int32)
        for i, c in enumerate(cands):
            tab[i, :len(c)] = c
        return tab

    def verify(self, source, qidx, cands, ranked=None, detail=False, mask=0, mfo=10, bound=1000.0, wait=True, raw_rc=False):
        L = self.L
        lb, ub = L.default_thresholds()
        tab = self.table(cands)
        n = len(tab)
        qi = None if qidx is None else np.ascontiguousarray(qidx, np.int32)
        cfg = L.VerifyCfg(mask, mfo, bound, 0)
        res = np.zeros(n, L.query_result_dt)
        hints = np.zeros((max(n, 1), L.HINT_MAX), L.hint_dt)
        hcnt = np.zeros(max(n, 1), np.int32)
        ro, rc_, rn_, det = self._modes(n, ranked, detail)
        self.keep.append((source, tab, qi, cfg, res, hints, hcnt, ro, rc_, rn_, det))
        if isinstance(source, L.PackedSrc):
            rc = self.lib.cc_db_verify_submit_packed(self.db, _b(source), _p(qi), _p(tab), n, _b(cfg), _b(lb), _b(ub), _p(res), _p(hints), _p(hcnt), None,
                                                     _b(ro), _p(det))
        else:
            qd = np.ascontiguousarray(source)
            self.keep.append(qd)
            head = (self.db, _p(qd), len(qd), _p(qi), _p(tab), n, _b(cfg), _b(lb), _b(ub), _p(res), _p(hints), _p(hcnt), None)
            if det is not None:
                rc = self.lib.cc_db_verify_submit_ranked_detail(*head, _b(ro), _p(det))
            elif ro is not None:
                rc = self.lib.cc_db_verify_submit_ranked(*head, _b(ro))
            else:
                rc = self.lib.cc_db_verify_submit(*head)
        if raw_rc:
            return rc
        self.api.chk(rc, "verify submit")
        if wait:
            self.wait()
        return self._out(res, rc_, rn_, det, hints=hints, hint_cnt=hcnt)

    # ---- pose ----
    def pose(self, source, q, gidx, tf, tries=None, curvature=False, refine=1, min_corr=0.3, wait=True, raw_rc=False):
        L = self.L
        items = L.pose_items(q, gidx, tf)
        n = len(items)
        tr = tc = None
        nt = 0
        if tries is not None:
            tr = np.ascontiguousarray(tries, np.float64)
            nt = tr.shape[1]
            tc = np.zeros((n, nt), np.float64)
        cfg = L.PoseCfg(int(refine), float(min_corr), nt, 0)
        res = np.zeros(n, L.pose_result_dt)
        cv = np.zeros(n, L.pose_curv_dt) if curvature else None
        self.keep.append((source, items, tr, tc, cfg, res, cv))
        if isinstance(source, L.PackedSrc):
            rc = self.lib.cc_db_pose_submit_packed(self.db, _b(source), _p(items), n, _b(cfg), _p(tr), _p(res), _p(tc), _p(cv), None)
        else:
            qd = np.ascontiguousarray(source)
            self.keep.append(qd)
            rc = self.lib.cc_db_pose_submit(self.db, _p(qd), len(qd), _p(items), n, _b(cfg), _p(tr), _p(res), _p(tc), _p(cv), None)
        if raw_rc:
            return rc
        self.api.chk(rc, "pose submit")
        if wait:
            self.wait()
        return self._out(res, None, None, None, try_corr=tc, curv=cv)


def same_bytes(a, b):
    """every output of two calls, byte for byte"""
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
