"""TEST INFRASTRUCTURE: ctypes driver of tests/knn_full_oracle.cpp -- the oracle's whole kNN hit lists (up to nnk = 256),
built here with the oracle's flags on first use."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "emu", "liborcknn.so")
_lib = None


def build():
    src = os.path.join(HERE, "knn_full_oracle.cpp")
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
        _lib.orcknn_db_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for f in ("orc_db_create", "orc_scan_from_desc"):
            getattr(_lib, f).restype = C.c_void_p
        _lib.orc_scan_from_desc.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.orc_db_create.argtypes = [C.c_void_p]
        _lib.orc_db_add_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
        _lib.orc_db_push_and_balance.argtypes = [C.c_void_p, C.c_int, C.c_double]
        _lib.orc_db_free.argtypes = [C.c_void_p]
        _lib.orc_scan_free.argtypes = [C.c_void_p]
    return _lib


class DB:
    """The oracle's ContourDB with a query that returns every hit of every search."""

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

    def query_knn(self, d, int_id, stride=256):
        L = O.L
        lb, ub = L.default_thresholds()
        knn = np.zeros((L.NQLEV, L.NPIV, stride), L.knn_hit_dt)
        cnt = np.zeros((L.NQLEV, L.NPIV), np.int32)
        lib().orcknn_db_query(self.h, self._scan(d, int_id), C.addressof(lb), C.addressof(ub), stride,
                              C.c_void_p(knn.ctypes.data), C.c_void_p(cnt.ctypes.data))
        return knn, cnt

    def close(self):
        if self.h:
            lib().orc_db_free(self.h)
            self.h = None
        for _, _, h in self._scans:
            lib().orc_scan_free(h)
        self._scans = []
