"""TEST INFRASTRUCTURE: ctypes driver of tests/dyn_thres_oracle.cpp, the CPU oracle of the reference's DYNAMIC_THRES=1
build (built here with the oracle's flags on first use)."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "emu", "liborcdyn.so")
_lib = None


def build():
    src = os.path.join(HERE, "dyn_thres_oracle.cpp")
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
        O.lib()  # the scan / DB handles come from the oracle's own library (the same code, compiled once more here)
        _lib = C.CDLL(build())
        _lib.orcdyn_db_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.orcdyn_check_hints.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        for f in ("orc_db_create", "orc_scan_from_desc"):
            getattr(_lib, f).restype = C.c_void_p
        _lib.orc_scan_from_desc.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.orc_db_create.argtypes = [C.c_void_p]
        _lib.orc_db_add_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_double]
        _lib.orc_db_push_and_balance.argtypes = [C.c_void_p, C.c_int, C.c_double]
        _lib.orc_db_free.argtypes = [C.c_void_p]
        _lib.orc_scan_free.argtypes = [C.c_void_p]
    return _lib


class _Scan:
    def __init__(self, d, int_id):
        L = O.L
        self.d = np.ascontiguousarray(np.asarray(d).reshape(1).astype(L.scan_desc_dt))
        self.cfg = L.default_manager_cfg()
        self.h = lib().orc_scan_from_desc(C.c_void_p(self.d.ctypes.data), C.addressof(self.cfg), int(int_id))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.orc_scan_free(self.h)


def run_sequence(desc, ts, seeds, dcfg, lb=None, ub=None, dyn=1):
    """The reference driver loop from descriptors (query at epoch i, then addScan + pushAndBalance), every query answered
    by orcdyn_db_query with the given mode.  Returns a query_result_dt array."""
    L = O.L
    if lb is None:
        lb, ub = L.default_thresholds()
    n = len(desc)
    d = lib().orc_db_create(C.addressof(dcfg))
    res = np.zeros(n, L.query_result_dt)
    keep = []
    try:
        for i in range(n):
            s = _Scan(desc[i], i)
            keep.append(s)
            lib().orcdyn_db_query(d, s.h, C.addressof(lb), C.addressof(ub), int(dyn), C.c_void_p(res[i:i + 1].ctypes.data))
            lib().orc_db_add_scan(d, s.h, float(ts[i]))
            lib().orc_db_push_and_balance(d, int(seeds[i]), float(ts[i]))
    finally:
        lib().orc_db_free(d)
    return res


def check_hints(desc, q, cands, hints, sim, lb=None, ub=None, max_fine_opt=10, dyn=1):
    """orcdyn_check_hints: hints [n][4] = (index into cands, level, seq_src, seq_tgt) -> (result with cand_gidx = index into
    cands, scores [n][6] = ovlp_sum, max_one, in_ang_rng, indiv_sim, orie_sim, passed)"""
    L = O.L
    if lb is None:
        lb, ub = L.default_thresholds()
    hints = np.ascontiguousarray(hints, np.int32).reshape(-1, 4)
    cs = [_Scan(desc[g], int(g)) for g in cands]
    t = _Scan(desc[q], int(q))
    hs = (C.c_void_p * len(cs))(*[c.h for c in cs])
    res = np.zeros(1, L.query_result_dt)
    sc = np.zeros((len(hints), 6), np.int32)
    lib().orcdyn_check_hints(t.h, hs, len(cs), C.c_void_p(hints.ctypes.data), len(hints), C.addressof(sim), C.addressof(lb),
                             C.addressof(ub), int(max_fine_opt), int(dyn), C.c_void_p(res.ctypes.data), C.c_void_p(sc.ctypes.data))
    return res[0], sc
