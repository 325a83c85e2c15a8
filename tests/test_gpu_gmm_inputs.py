"""K5 on synthetic ellipse tables, on the MI355X through the Python package (gmm_cases.py): A cc_gmm_feat of Context.pack against
the restatement and the derived ac bound; B the pair pre-selection of cc_k_gmm_init through Database.score_poses with refine = 0,
on both init instances; C the list-length edges through cc_k_gmm_refine.

The init instances.  cc_k_gmm_init takes a wave per problem while a chunk's problem count is at most its grid (`n_prob <=
gridDim.x`): the first run makes calls of ONE item, which hold whatever the grid is.  The package's default grid (tune.gmm of
cc_db_api.inc, 4 096) is above a pose chunk's 1 024 items, so the default never reaches the 16-lane instance through a pose call:
the second run uses a database made while CC_GMM_GRID = 64 is in the environment (the library's own launch-geometry variable,
read once per handle), in a call of 256 items -- two chunks of 128.
Which instance ran is vouched for by that host condition alone; nothing the kernel returns names it."""
import os

import numpy as np
import pytest

import gmm_cases as G

pytestmark = pytest.mark.gpu

_state = {}
SMALL_GRID = 64


class GpuBack:
    name = "MI355X"

    def __init__(self, cc):
        self.cc, self.L = cc, cc.L
        self.ctx = cc.Context(0, max_batch=16)
        self.dbs = {}

    def _tensor(self, desc):
        import torch
        return torch.from_numpy(np.frombuffer(np.ascontiguousarray(desc).tobytes(), np.uint8).reshape(len(desc), self.cc.DESC_BYTES).copy()).cuda()

    def pack(self, desc):
        import torch
        _, feat = self.ctx.pack(self._tensor(desc))
        torch.cuda.synchronize()
        return feat.cpu().numpy()

    def open(self, desc, small_grid):
        key = bool(small_grid)
        if key not in self.dbs:
            assert "CC_GMM_GRID" not in os.environ, "the test sets the launch geometry itself"
            if small_grid:
                os.environ["CC_GMM_GRID"] = str(SMALL_GRID)
            try:
                db = self.cc.Database(self.ctx, self.L.default_db_cfg(), capacity=len(desc))
            finally:
                os.environ.pop("CC_GMM_GRID", None)
            d = self._tensor(desc)
            db.add_scans(d, np.arange(len(desc)) * 100.0, np.arange(len(desc), dtype=np.int32))
            self.dbs[key] = (db, d, SMALL_GRID if small_grid else 1)
        return self.dbs[key]

    def switch(self, h):
        return h[2]

    def pose(self, h, items, refine, tries):
        res, tc, _ = h[0].score_poses(h[1], items["q"], items["gidx"], items["tf"], refine=bool(refine), min_corr=G.NINF, tries=tries)
        return res, tc


def back(cc):
    if "B" not in _state:
        _state["B"] = GpuBack(cc)
    return _state["B"]


def test_feat_records(cc, oracle):
    """A"""
    worst, worst_o = G.check_feat(back(cc), oracle)
    print("A MI355X: largest ac error / bound %.3f (the oracle's own sum %.3f)" % (worst, worst_o))


def test_pair_selection(cc, oracle):
    """B"""
    G.check_selection(back(cc), oracle)


def test_list_length_edges(cc, oracle):
    """C"""
    G.check_lists(back(cc), oracle)
