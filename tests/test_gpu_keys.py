"""The retrieval keys of the ingest path on the MI355X, held to the bit against tests/key_reference.py on the oracle's inputs, at the
edges of the key phase (tests/key_cases.py): the quad's tail lanes and the order of its four additions (DPP broadcasts), the
ballot-ordered lists, the second anchor group in reused LDS and the clamp exist in this form on hardware only.  The same inputs took
the list, mid and big paths on the CPU harness (test_emu_keys.py asserts that); here the counters of cc_ingest_path_counts say which
body took a call's scans, and the cases assert it."""
import numpy as np
import pytest

import key_cases

pytestmark = pytest.mark.gpu


class GpuBackEnd:
    def __init__(self, cc):
        self.cc = cc
        self._counts = None

    def ingest(self, scans, cfg, debug=False):
        import torch
        ctx = self.cc.Context(0, cfg, max_batch=len(scans))
        offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans, 0), np.float32)).cuda()
        zeroed = torch.zeros((len(scans), self.cc.DESC_BYTES), dtype=torch.uint8, device="cuda")   # rows past n_stored are not written
        out = ctx.ingest(x, offs, out=zeroed, debug=debug)
        torch.cuda.synchronize()
        d = self.cc.desc_to_numpy(out[0] if debug else out).copy()
        pc = ctx.path_counts()                # a context of this call alone: its counters are the call's
        self._counts = {"list": len(scans) - pc["mid"], "mid": pc["mid"] - pc["big"], "big": pc["big"]}
        assert sum(pc["why"]) == pc["mid"], pc
        ctx.close()
        return d

    def paths(self):
        """per scan only where the counts decide it: all of the call's scans on one body"""
        n = sum(self._counts.values())
        return next(({kk: set(range(n)) if kk == k else set() for kk in self._counts} for k, v in self._counts.items() if v == n), None)

    def path_counts(self):
        return self._counts


def test_quad_tails_and_empty_list(cc, oracle):
    key_cases.case_quad_tails_and_empty_list(GpuBackEnd(cc), oracle)


def test_anchor_groups(cc, oracle):
    key_cases.case_anchor_groups(GpuBackEnd(cc), oracle)


def test_clipping_and_seams(cc, oracle):
    key_cases.case_clipping_and_seams(GpuBackEnd(cc), oracle)


def test_long_stretches_and_cap(cc, oracle):
    key_cases.case_long_stretches_and_cap(GpuBackEnd(cc), oracle)


def test_radii_and_piv_firsts(cc, oracle):
    key_cases.case_radii_and_piv_firsts(GpuBackEnd(cc), oracle)


def test_three_paths_both_launch_shapes_and_debug(cc, oracle):
    key_cases.case_three_paths_both_launch_shapes_and_debug(GpuBackEnd(cc), oracle)
