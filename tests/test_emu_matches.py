"""The matched contour pairs behind each ranked entry (include/cont2_amd_matches.h: cc_k_merge_m / cc_k_merge_lm, cc_k_match_emit /
cc_k_match_emit_l) on the CPU harness: the cases of match_cases.py -- the built merge scenes, the bit edges, the 64-scan drive
at nnk 50 and 128, the residuals and the three inlier bars, what must not move, the forms, the lanes and every refusal."""
import ctypes as C

import numpy as np
import pytest

import constell_cases as K
import emu_api
import match_cases as M
import ranked_common as RC
from test_emu_large_nnk import _db_cfg

_state = {}


class EmuBack:
    """a database on the harness ("device" pointers are host pointers there)"""
    stream = None

    def __init__(self, L, desc, ts, seeds, dcfg, lanes=None, dyn=False):
        self.L = L
        self.api = emu_api.EmuApi(L)
        self.lib = self.api.lib
        self.ctx = self.api.create(max_batch=2)
        self.db = self.api.db_create(self.ctx, dcfg, cap=len(desc))
        if lanes is not None:
            self.api.chk(self.lib.cc_db_set_lanes(self.db, lanes), "cc_db_set_lanes")
        self.api.db_add(self.db, desc, ts, seeds)
        if dyn:
            self.api.chk(self.lib.cc_db_set_dynamic_thres(self.db, 1), "cc_db_set_dynamic_thres")
        self.keep = []

    def dev(self, a):
        self.keep.append(a)
        return a.ctypes.data

    dev_out = dev

    @staticmethod
    def fetch(a):
        return a

    def sync(self):
        pass


def scenes_back(oracle):
    if "E" not in _state:
        L = oracle.L
        d = K.database(L)
        _state["E"] = EmuBack(L, d, np.arange(len(d)) * 100.0, np.arange(len(d), dtype=np.int32), L.default_db_cfg())
    return _state["E"]


def drive_back(cc, oracle, key="nnk 50", **kw):
    if key not in _state:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        cfg = _db_cfg(oracle.L, 128) if key == "nnk 128" else dcfg
        _state[key] = EmuBack(oracle.L, desc, ts, seeds, cfg, **kw)
    return _state[key]


def test_merge_scenes(cc, oracle):
    """case 1"""
    log = []
    st = M.check_merge_scenes(scenes_back(oracle), oracle.L, oracle, log)
    print("\n".join(log))
    assert st["merged"] >= 1 and st["multi"] >= 5


def test_bit_edges(cc, oracle):
    """case 2: bits 63, 64 and 399, and cc_match_pairs"""
    M.check_bit_edges(scenes_back(oracle), oracle.L, oracle)


@pytest.mark.parametrize("key", ["nnk 50", "nnk 128"])
def test_drive(cc, oracle, key):
    """case 3 (nnk 128: the large-k merge and emit instances), with case 4's residual tolerance on every entry"""
    B = drive_back(cc, oracle, key)
    assert B.lib.cc_db_knn_stride(B.db) == (256 if key == "nnk 128" else 64)
    M.check_drive(B, cc, oracle, key)


def test_inlier_bars(cc, oracle):
    """case 4"""
    M.check_bars(scenes_back(oracle), oracle.L, oracle)


def test_nothing_else_moves(cc, oracle):
    """case 5"""
    M.check_nothing_else_moves(drive_back(cc, oracle), cc, oracle, "nnk 50")


def test_forms(cc, oracle):
    """case 6: stored, packed, masked and host forms"""
    B = drive_back(cc, oracle)
    desc = RC.drive(cc, oracle)[0]
    hot, feat = B.api.pack(B.ctx, desc)
    B.keep.append((hot, feat))
    M.check_forms(B, cc, oracle, "nnk 50", (hot.ctypes.data, feat.ctypes.data, len(hot)))


def test_verify(cc, oracle):
    """case 6: one item of eight candidates"""
    M.check_verify(scenes_back(oracle), oracle.L, oracle)


def test_four_lanes(cc, oracle):
    """case 6: 130 queries over four lanes, max_ret 1, 4 and 16"""
    B = drive_back(cc, oracle)
    _, ref = M.drive_reference(B, cc, oracle, "nnk 50")
    M.check_lanes(drive_back(cc, oracle, "four lanes", lanes=4), cc, oracle, ref)


def test_refusals(cc, oracle):
    """case 7"""
    M.check_refusals(drive_back(cc, oracle), cc, oracle, drive_back(cc, oracle, "dynamic", dyn=True))


def test_python_matches_need_ranked(cc):
    with pytest.raises(ValueError):
        cc.calls._match(4, None, 1.0)
    rows, mo = cc.calls._match(4, 3, 1.5)
    assert rows.shape == (4, 3) and rows.dtype == cc.L.ranked_match_dt and mo.inlier_px == 1.5 and cc.calls._match(4, 3, None) == (None, None)
    row = np.zeros((), cc.L.ranked_match_dt)
    row["pairs"][0], row["pairs"][1], row["pairs"][6] = np.uint64(1 << 63), np.uint64(1), np.uint64(1 << 15)
    assert cc.match_pairs(row).tolist() == [[1, 6, 3], [1, 6, 4], [4, 9, 9]] and cc.match_pairs(row).dtype == np.int8
