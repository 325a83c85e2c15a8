"""TEST INFRASTRUCTURE: numpy-pointer driver of the cc_* C-ABI for the CPU-emulated build
(tests/emu/libcc_emu.so).  "Device" pointers are host pointers there."""
import ctypes as C
import os
import subprocess

import numpy as np

import cc_amd

abi, calls = cc_amd.load().abi, cc_amd.load().calls
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "emu", "libcc_emu.so")


def build(variant=None, flags=()):
    """the harness library; variant: a second library tests/emu/libcc_emu_<variant>.so compiled with the extra `flags`"""
    so = SO if variant is None else os.path.join(HERE, "emu", "libcc_emu_%s.so" % variant)
    srcs = [os.path.join(HERE, "emu", "emu_main.cpp"), os.path.join(HERE, "emu", "hip", "hip_runtime.h")]
    csrc = os.path.join(HERE, "..", "contour-context_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc)]
    srcs.append(os.path.join(HERE, "..", "include", "cont2_amd.h"))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["sh", os.path.join(HERE, "emu", "build.sh")] + ([] if variant is None else [os.path.basename(so)] + list(flags)))
    return so


# one OS thread per HIP thread: keep the grids of the list-driven kernels small on the harness (read at cc_db_create).
# Tests that run a program of their own on the harness pass this to the subprocess; it must never reach the GPU library.
SMALL_GRIDS = {"CC_B1_GRID": "6", "CC_B2_GRID": "6", "CC_GMM_GRID": "6"}


def levels_of(mask):
    """a cc_verify_cfg_t.level_mask -> the levels= of calls.verify (0, the library's "all four", is None)"""
    return [lv for lv in (1, 2, 3, 4) if mask >> (lv - 1) & 1] or None


class EmuApi:
    def __init__(self, L, so=None):
        self.L = L
        self.lib = abi.bind(C.CDLL(so or build()))
        self.keep = []  # what the submits in flight read and write, until db_query_wait

    def chk(self, rc, what):
        calls.chk(self.lib, rc, what)

    def create(self, cfg=None, max_batch=8):
        cfg = cfg or self.L.default_manager_cfg()
        h = C.c_void_p()
        self.chk(self.lib.cc_create(0, C.byref(cfg), max_batch, C.byref(h)), "cc_create")
        self._cfg = cfg
        return h

    def ingest(self, ctx, xyzi, offsets, debug=False):
        L = self.L
        xyzi = np.ascontiguousarray(xyzi, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, L.scan_desc_dt)
        ncell = self._cfg.n_row * self._cfg.n_col
        dbg = None
        dbg_p = None
        if debug:
            dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32),
                   "labels": np.zeros((n, L.NLEV, ncell), np.int16)}
            st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
            dbg_p = C.cast(st, C.c_void_p)
        self.chk(self.lib.cc_ingest_batch(ctx, C.c_void_p(xyzi.ctypes.data), C.c_void_p(offsets.ctypes.data), n,
                                          C.c_void_p(desc.ctypes.data), dbg_p, None), "cc_ingest_batch")
        return (desc, dbg) if debug else desc

    def ingest_host(self, ctx, xyzi, offsets):
        xyzi = np.ascontiguousarray(xyzi, np.float32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        self.chk(self.lib.cc_ingest_host(ctx, C.c_void_p(xyzi.ctypes.data), C.c_void_p(offsets.ctypes.data), n,
                                         C.c_void_p(desc.ctypes.data)), "cc_ingest_host")
        return desc

    def db_create(self, ctx, cfg=None, cap=1024):
        for k, v in SMALL_GRIDS.items():
            os.environ.setdefault(k, v)
        cfg = cfg or self.L.default_db_cfg()
        h = C.c_void_p()
        self.chk(self.lib.cc_db_create(ctx, C.byref(cfg), cap, C.byref(h)), "cc_db_create")
        return h

    def db_add(self, db, desc, ts, seeds):
        desc = np.ascontiguousarray(desc)
        ts = np.ascontiguousarray(ts, np.float64)
        seeds = np.ascontiguousarray(seeds, np.int32)
        self.chk(self.lib.cc_db_add_scans(db, C.c_void_p(desc.ctypes.data), len(desc), C.c_void_p(ts.ctypes.data),
                                          C.c_void_p(seeds.ctypes.data), None), "cc_db_add_scans")

    def db_add_prepared(self, db, desc, ts, seeds):
        """cc_db_add_scans_prepare + cc_db_add_scans on the same (pointer, n): the streamed form of db_add."""
        desc = np.ascontiguousarray(desc)
        ts = np.ascontiguousarray(ts, np.float64)
        seeds = np.ascontiguousarray(seeds, np.int32)
        self.chk(self.lib.cc_db_add_scans_prepare(db, C.c_void_p(desc.ctypes.data), len(desc), None), "cc_db_add_scans_prepare")
        self.chk(self.lib.cc_db_add_scans(db, C.c_void_p(desc.ctypes.data), len(desc), C.c_void_p(ts.ctypes.data),
                                          C.c_void_p(seeds.ctypes.data), None), "cc_db_add_scans")

    def packed_sizes(self):
        hb, fb = C.c_size_t(), C.c_size_t()
        self.lib.cc_packed_sizes(C.byref(hb), C.byref(fb))
        return int(hb.value), int(fb.value)

    def pack(self, ctx, desc):
        """full descriptors -> (hot, feat) uint8 arrays [n, HOT_BYTES] / [n, FEAT_BYTES] (cc_pack_scans)"""
        desc = np.ascontiguousarray(desc)
        hb, fb = self.packed_sizes()
        hot = np.zeros((len(desc), hb), np.uint8)
        feat = np.zeros((len(desc), fb), np.uint8)
        self.chk(self.lib.cc_pack_scans(ctx, C.c_void_p(desc.ctypes.data), len(desc), C.c_void_p(hot.ctypes.data),
                                        C.c_void_p(feat.ctypes.data), None), "cc_pack_scans")
        return hot, feat

    def db_add_packed(self, db, hot, feat, ts, seeds):
        hot, feat = np.ascontiguousarray(hot), np.ascontiguousarray(feat)
        ts = np.ascontiguousarray(ts, np.float64)
        seeds = np.ascontiguousarray(seeds, np.int32)
        self.chk(self.lib.cc_db_add_packed(db, C.c_void_p(hot.ctypes.data), C.c_void_p(feat.ctypes.data), len(hot),
                                           C.c_void_p(ts.ctypes.data), C.c_void_p(seeds.ctypes.data), None), "cc_db_add_packed")

    def db_query(self, db, qdesc, epochs, lb=None, ub=None, want_knn=False):
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        nq = len(qdesc)
        knn = np.zeros((nq, 3, L.NPIV, L.KNN_MAX), L.knn_hit_dt) if want_knn else None
        cnt = np.zeros((nq, 3, L.NPIV), np.int32) if want_knn else None
        res = calls.query(self.lib, db, epochs, qdesc=qdesc.ctypes.data, lb=lb, ub=ub, knn=knn.ctypes.data if want_knn else None,
                          knn_cnt=cnt.ctypes.data if want_knn else None).res
        return (res, knn, cnt) if want_knn else res

    def db_query_submit(self, db, qdesc, epochs):
        """cc_db_query_submit: returns (result array, keep-alive tuple); valid after db_query_wait."""
        qdesc = np.ascontiguousarray(qdesc)
        self.keep.append(qdesc)
        r = calls.query(self.lib, db, epochs, qdesc=qdesc.ctypes.data, wait=False, keep=self.keep)
        return r.res, (qdesc, r.keep)

    def db_query_wait(self, db):
        self.chk(self.lib.cc_db_query_wait(db), "cc_db_query_wait")
        self.keep = []

    def check_hints(self, db, qdesc, hints, lb=None, ub=None, max_fine_opt=10):
        qdesc = np.ascontiguousarray(qdesc)
        r = calls.check_hints(self.lib, db, qdesc.ctypes.data, hints, lb, ub, max_fine_opt)
        return r.res[0], r.scores

    def bucket_state(self, db):
        sizes = np.zeros((3, 6), np.int32)
        ranges = np.zeros((3, 7), np.float32)
        self.chk(self.lib.cc_db_bucket_state(db, C.c_void_p(sizes.ctypes.data), C.c_void_p(ranges.ctypes.data)), "bucket_state")
        return sizes, ranges
