"""K4 (csrc/k_check.h) on built scans, on the CPU harness (constell_cases.py): every scene is one cc_db_check_hints call whose
per-hint scores, pass records and result record are held against the oracle (R1) and, up to the individual similarity, against
the numpy restatement (R2); the merge scenes (E) are held, candidate by candidate, against the oracle's export through
cc_db_debug_cands.  The harness leaves nothing out.  Every part prints its figures (pytest -s)."""
import numpy as np
import pytest

import constell_cases as K
import emu_api

_state = {}


class EmuBack:
    name = "harness"

    def __init__(self, oracle, so=None):
        self.L = oracle.L
        self.api = emu_api.EmuApi(self.L, so)
        self.ctx = self.api.create(max_batch=2)
        descs = K.database(self.L)
        self.db = self.api.db_create(self.ctx, self.L.default_db_cfg(), cap=len(descs))
        self.api.db_add(self.db, descs, np.arange(len(descs)) * 100.0, np.arange(len(descs), dtype=np.int32))

    def hints(self, sc, h, lb, ub):
        q = np.ascontiguousarray(sc.tgt.reshape(1))
        return K.raw_hints(self.api.lib, self.db, q.ctypes.data, h, lb, ub, self.L)

    def cands(self):
        return K.raw_cands(self.api.lib, self.db, self.L)

    def raw(self, sc):
        self.q = np.ascontiguousarray(sc.tgt.reshape(1))
        return self.api.lib, self.db, self.q.ctypes.data, None

    def sync(self):
        pass

    def dynamic(self, on):
        self.api.chk(self.api.lib.cc_db_set_dynamic_thres(self.db, 1 if on else 0), "cc_db_set_dynamic_thres")

    def verify(self, qdesc, qidx, cands):
        L = self.L
        n = len(cands)
        hints, cnt = np.zeros((n, L.HINT_MAX), L.hint_dt), np.zeros(n, np.int32)
        r = emu_api.calls.verify(self.api.lib, self.db, cands, qdesc=qdesc.ctypes.data, n_desc=len(qdesc), qidx=qidx, max_key_dist_sq=float("inf"),
                                 hints=hints.ctypes.data, n_hints=cnt.ctypes.data, tolerate=(K.CC_ECAPACITY,))
        return r.res, [hints[i, :cnt[i]].copy() for i in range(n)]


def back(oracle):
    if "B" not in _state:
        _state["B"] = EmuBack(oracle)
    return _state["B"]


def _names(prefix):
    return lambda L: [sc for sc in K.scenes(L) if sc.name.startswith(prefix)]


def test_builder_and_references(cc, oracle):
    """every built descriptor is what the oracle holds, R2 agrees with R1 on every hint, every case reaches its edge"""
    lines = K.scene_facts(oracle.L, oracle)
    print("\n".join(lines))
    assert len(K.database(oracle.L)) <= 100   # "about 80 built scans": the scan pairs of the A-D scenes and 70 candidates of the merge scenes


@pytest.mark.parametrize("part", ["A gate", "A rings", "A classes", "A shapes", "B deep", "B sort/", "B sort, capped", "C window", "C cap", "D b2", "D acos", "D nrm"])
def test_scenes(cc, oracle, part):
    log = []
    sel = _names(part)(oracle.L)
    assert sel
    for sc in sel:
        K.check_scene(back(oracle), oracle.L, oracle, sc, log)
    print("\n".join(log))


def test_merge(cc, oracle):
    """E: every candidate's merged proposal through cc_db_debug_cands against the oracle's export"""
    log = []
    for sc in K.merge_scenes(oracle.L):
        K.check_merge(back(oracle), oracle.L, oracle, sc, log)
    print("\n".join(log))


def test_getter_against_ranked_detail(cc, oracle):
    sel = [sc for sc in K.merge_scenes(oracle.L) if sc.name in ("E proposals", "E 65 candidates")]
    assert [K.check_ranked_entries(back(oracle), oracle.L, oracle, sc) for sc in sel] == [10, 16]


def test_batch(cc, oracle):
    """F, on 30 items (the harness runs a thread per check slot): every A-D scan pair and 17 candidates of the merge scenes"""
    log = []
    K.check_batch(back(oracle), oracle.L, oracle, 30, log)
    print("\n".join(log))


def test_table_under_dynamic_thresholds(cc, oracle):
    log = []
    assert K.check_dynamic(back(oracle), oracle.L, oracle, log) >= 25
    print("\n".join(log))
