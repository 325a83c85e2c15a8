"""K5 on synthetic ellipse tables, on the CPU harness (gmm_cases.py): A cc_gmm_feat of cc_pack_scans against the restatement and
the derived ac bound; B the pair pre-selection of cc_k_gmm_init through cc_db_pose_submit with refine = 0, on both init instances
(the harness launches cc_k_gmm_init on CC_GMM_GRID = 6 workgroups: calls of at most 6 items take the wave-per-problem instance, a
call whose chunks hold 64 items the 16-lane one); C the list-length edges through cc_k_gmm_refine, and once more on a second
harness library compiled with CC_GMM_PACK_MIN_PROBLEMS = 8, in which the call of all 21 items sends the lists of 97..256 pairs to
the packed 16-lane instance (four problems to a wave, 32 records each in LDS, the rest in the pair pool).

The harness leaves nothing out.  Every part prints its figures (pytest -s)."""
import os

import numpy as np

import emu_api
import gmm_cases as G
import pose_common as PC
from packed_emu import PackedEmu

_state = {}
PACK_MIN = 8


class EmuBack:
    def __init__(self, oracle, name="harness", so=None):
        self.L, self.name, self.so = oracle.L, name, so
        self.p = self.db = None

    def _emu(self):
        if self.p is None:
            self.p = PackedEmu(self.L, self.L.default_db_cfg(), cap=64, so=self.so)
        return self.p

    def pack(self, desc):
        return np.array(self._emu().pack(desc)[1])

    def open(self, desc, small_grid):
        """one database of the descriptors serves both runs: the harness's grid is small already"""
        if self.db is None:
            self._emu().add(desc, np.arange(len(desc)) * 100.0, np.arange(len(desc), dtype=np.int32))
            self.db = np.ascontiguousarray(desc)
        return self.db

    def switch(self, h):
        return int(os.environ["CC_GMM_GRID"])   # read by cc_db_create (emu_api.SMALL_GRIDS)

    def pose(self, h, items, refine, tries):
        o = self._emu().pose(h, items["q"], items["gidx"], items["tf"], tries=tries, refine=refine, min_corr=G.NINF)
        return o["res"], o.get("try_corr")


def back(oracle):
    if "B" not in _state:
        _state["B"] = EmuBack(oracle)
    return _state["B"]


def test_feat_records(cc, oracle):
    """A"""
    worst, worst_o = G.check_feat(back(oracle), oracle)
    print("A harness: largest ac error / bound %.3f (the oracle's own sum %.3f)" % (worst, worst_o))


def test_pair_selection(cc, oracle):
    """B"""
    G.check_selection(back(oracle), oracle)


def test_list_length_edges(cc, oracle):
    """C"""
    _state["C"] = G.check_lists(back(oracle), oracle)


def test_list_length_edges_packed(cc, oracle):
    """C on the library whose in-between lists are packed four to a wave from 8 selected problems on: against oracle.gmm in full,
    the packed run (21 problems) against the unpacked one (4 problems) and against the shipped threshold's rows within SAME_BAR"""
    assert 4 < PACK_MIN <= len(G.C_COUNTS)
    so = emu_api.build("pack%d" % PACK_MIN, ["-DCC_GMM_PACK_MIN_PROBLEMS=%d" % PACK_MIN])
    res = G.check_lists(EmuBack(oracle, "harness, packed from %d problems" % PACK_MIN, so), oracle)
    std = _state["C"] if "C" in _state else G.check_lists(back(oracle), oracle)
    PC.rows_close(res, std, "the packed library against the shipped threshold")
    mid = [k for k, n in enumerate(G.C_COUNTS) if 97 <= n <= 256]
    d = np.abs(res["correlation"][mid] - std["correlation"][mid]).max()
    print("C packed against shipped, the 97..256 items: max |corr| %.2e" % d)
