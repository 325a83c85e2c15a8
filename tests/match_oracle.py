"""TEST INFRASTRUCTURE: ctypes driver of tests/match_oracle.cpp -- the oracle's hint flow with the selected proposal's
constellation exported per candidate, built here with the oracle's flags on first use."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(HERE, "emu", "liborcmatch.so")
KEY_CAP = 400   # a constellation is a set of (level 1..4, seq_src 0..9, seq_tgt 0..9)
_lib = None

MATCH_DT = np.dtype([("cand", "<i4"), ("n_props", "<i4"), ("idx_sel", "<i4"), ("survived", "<i4"), ("vote_cnt", "<i4"), ("n_pairs", "<i4"),
                     ("area_perc", "<f4"), ("area_perc_tidy", "<f4")])


def build():
    src = os.path.join(HERE, "match_oracle.cpp")
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
        _lib.orcx_check_hints_matches.argtypes = [V, V, C.c_int, V, C.c_int, V, V, V, C.c_int, C.c_int, V, V, V]
        _lib.orcx_check_hints_matches.restype = C.c_int
        for f in ("orc_scan_from_desc",):
            getattr(_lib, f).restype = V
        _lib.orc_scan_from_desc.argtypes = [V, V, C.c_int]
        _lib.orc_scan_free.argtypes = [V]
    return _lib


class Scan:
    """A ContourManager of THIS library (its handles are not oracle_py's: two copies of the oracle's code are loaded)."""

    def __init__(self, d, int_id=0):
        L = O.L
        self.d = np.ascontiguousarray(np.asarray(d).reshape(1).astype(L.scan_desc_dt))
        self.mcfg = L.default_manager_cfg()
        self.h = lib().orc_scan_from_desc(C.c_void_p(self.d.ctypes.data), C.addressof(self.mcfg), int(int_id))

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.orc_scan_free(self.h)
            self.h = None


def check_hints_matches(tgt, cands, hints, sim=None, lb=None, ub=None):
    """tgt / cands: Scan objects of this module; hints: int [n][4] of (index into cands, level, seq_src, seq_tgt).
    -> (array of MATCH_DT in candidates_ order, list of int8 [n_pairs, 3] key arrays in the map's order)"""
    L = O.L
    sim = sim or L.default_db_cfg().cont_sim
    if lb is None:
        lb, ub = L.default_thresholds()
    hints = np.ascontiguousarray(hints, np.int32).reshape(-1, 4)
    hs = (C.c_void_p * max(len(cands), 1))(*[c.h for c in cands])
    cap = max(len(cands), 1)
    ci, cf = np.zeros((cap, 6), np.int32), np.zeros((cap, 2), np.float32)
    keys = np.zeros((cap, KEY_CAP, 3), np.int8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    n = lib().orcx_check_hints_matches(tgt.h, hs, len(cands), p(hints), len(hints), C.addressof(sim), C.addressof(lb), C.addressof(ub), cap, KEY_CAP,
                                       p(ci), p(cf), p(keys))
    assert n <= cap
    out = np.zeros(n, MATCH_DT)
    for j, f in enumerate(("cand", "n_props", "idx_sel", "survived", "vote_cnt", "n_pairs")):
        out[f] = ci[:n, j]
    out["area_perc"], out["area_perc_tidy"] = cf[:n, 0], cf[:n, 1]
    assert (out["n_pairs"] <= KEY_CAP).all()
    return out, [keys[k, :out["n_pairs"][k]].copy() for k in range(n)]
