"""TEST INFRASTRUCTURE: ctypes driver of tests/knn_masked_oracle.cpp -- the oracle's query with the trees filtered to a
row of allowed scans, built here with the oracle's flags on first use (the exact-scan backend, the oracle's default)."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "emu", "liborcmask.so")
_lib = None


def build():
    src = os.path.join(HERE, "knn_masked_oracle.cpp")
    deps = [src] + [os.path.join(ROOT, "oracle", f) for f in os.listdir(os.path.join(ROOT, "oracle")) if f.endswith((".cpp", ".h"))]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = SO + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "oracle"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", tmp])
        os.replace(tmp, SO)
    return SO


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        V = C.c_void_p
        _lib.orcm_db_query.argtypes = [V, V, V, V, V, C.c_int, V, C.c_int, V, V]
        _lib.orcm_db_query.restype = None
        for f in ("orc_db_create", "orc_scan_from_desc"):
            getattr(_lib, f).restype = V
        _lib.orc_scan_from_desc.argtypes = [V, V, C.c_int]
        _lib.orc_db_create.argtypes = [V]
        _lib.orc_db_add_scan.argtypes = [V, V, C.c_double]
        _lib.orc_db_push_and_balance.argtypes = [V, C.c_int, C.c_double]
        _lib.orc_db_free.argtypes = [V]
        _lib.orc_scan_free.argtypes = [V]
        _lib.orc_knn_backend_active.restype = C.c_int
        assert _lib.orc_knn_backend_active() == 0  # the exact scan
    return _lib


class DB:
    """The oracle's ContourDB with a query that sees only the scans of a row."""

    def __init__(self, dcfg):
        self.cfg = dcfg
        self.h = lib().orc_db_create(C.addressof(dcfg))
        self._scans = []  # the DB keeps pointers to the scans' managers

    def _scan(self, d, int_id):
        L = O.L
        d = np.ascontiguousarray(np.asarray(d).reshape(1).astype(L.scan_desc_dt))
        mcfg = L.default_manager_cfg()
        h = lib().orc_scan_from_desc(C.c_void_p(d.ctypes.data), C.addressof(mcfg), int(int_id))
        self._scans.append((d, mcfg, h))
        return h

    def add(self, d, ts, seed):
        lib().orc_db_add_scan(self.h, self._scan(d, seed), float(ts))
        lib().orc_db_push_and_balance(self.h, int(seed), float(ts))

    def query(self, d, int_id, row=None, stride=256, lb=None, ub=None):
        """row: uint32 [row_words] or None (no restriction) -> (result record, hits [NQLEV, NPIV, stride], counts [NQLEV, NPIV])"""
        L = O.L
        if lb is None:
            lb, ub = L.default_thresholds()
        res = np.zeros(1, L.query_result_dt)
        knn = np.zeros((L.NQLEV, L.NPIV, stride), L.knn_hit_dt)
        cnt = np.zeros((L.NQLEV, L.NPIV), np.int32)
        r = None if row is None else np.ascontiguousarray(row, np.uint32)
        lib().orcm_db_query(self.h, self._scan(d, int_id), C.addressof(lb), C.addressof(ub), None if r is None else C.c_void_p(r.ctypes.data),
                            0 if r is None else len(r), C.c_void_p(res.ctypes.data), stride, C.c_void_p(knn.ctypes.data),
                            C.c_void_p(cnt.ctypes.data))
        return res[0], knn, cnt

    def close(self):
        if self.h:
            lib().orc_db_free(self.h)
            self.h = None
        for _, _, h in self._scans:
            lib().orc_scan_free(h)
        self._scans = []
