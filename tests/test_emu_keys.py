"""The retrieval keys of the ingest path on the CPU harness, against tests/key_reference.py on the oracle's inputs, at the edges of
the key phase (tests/key_cases.py).  The harness build prints which K2 path took each scan (CC_EMU_TRACE_K2); the cases assert it."""
import ctypes as C

import numpy as np

import emu_api
import key_cases


class EmuBackEnd:
    def __init__(self, oracle, capfd):
        self.api = emu_api.EmuApi(oracle.L)
        self.capfd = capfd
        self._paths = self._counts = None

    def ingest(self, scans, cfg, debug=False):
        ctx = self.api.create(cfg=cfg, max_batch=len(scans))
        offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
        self.capfd.readouterr()
        out = self.api.ingest(ctx, np.concatenate(scans, 0), offs, debug=debug)
        err = self.capfd.readouterr().err.splitlines()
        seen = {int(l.split("scan")[1].split(":")[0]) for l in err if l.startswith("[k2 list] scan") and "active cells" in l}
        handed = {int(l.split("scan")[1].split()[0]) for l in err if "handed to the mid path" in l}
        big = {int(l.split("scan")[1]) for l in err if l.startswith("[k2 big] scan")}
        every = set(range(len(scans)))   # (a scan the list kernel turns away at its door is handed on before it is counted)
        assert big <= handed <= every and seen | handed == every, (seen, handed, big)
        self._paths = {"list": every - handed, "mid": handed - big, "big": big}
        pc = (C.c_int32 * 6)()                # a context of this call alone: its counters are the call's
        self.api.chk(self.api.lib.cc_ingest_path_counts(ctx, pc), "cc_ingest_path_counts")
        self._counts = {"list": len(scans) - pc[0], "mid": pc[0] - pc[5], "big": pc[5]}
        assert self._counts == {k: len(v) for k, v in self._paths.items()} and sum(pc[1:5]) == pc[0], (self._counts, self._paths, pc[:])
        self.api.lib.cc_destroy(ctx)
        return out[0] if debug else out

    def paths(self):
        return self._paths

    def path_counts(self):
        return self._counts


def _be(oracle, capfd, monkeypatch):
    monkeypatch.setenv("CC_EMU_TRACE_K2", "1")
    return EmuBackEnd(oracle, capfd)


def test_quad_tails_and_empty_list(oracle, capfd, monkeypatch):
    key_cases.case_quad_tails_and_empty_list(_be(oracle, capfd, monkeypatch), oracle)


def test_anchor_groups(oracle, capfd, monkeypatch):
    key_cases.case_anchor_groups(_be(oracle, capfd, monkeypatch), oracle)


def test_clipping_and_seams(oracle, capfd, monkeypatch):
    key_cases.case_clipping_and_seams(_be(oracle, capfd, monkeypatch), oracle)


def test_long_stretches_and_cap(oracle, capfd, monkeypatch):
    key_cases.case_long_stretches_and_cap(_be(oracle, capfd, monkeypatch), oracle)


def test_radii_and_piv_firsts(oracle, capfd, monkeypatch):
    key_cases.case_radii_and_piv_firsts(_be(oracle, capfd, monkeypatch), oracle)


def test_three_paths_both_launch_shapes_and_debug(oracle, capfd, monkeypatch):
    key_cases.case_three_paths_both_launch_shapes_and_debug(_be(oracle, capfd, monkeypatch), oracle)
