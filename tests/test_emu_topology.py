"""K2's labelling, member lists, statistics walks and hand-offs on built images (tests/topology_cases.py) on the CPU harness: every
designed scene on the body it was designed for, then with filler (mid body) and with blobs (big body), and random images for the
three bodies.  The harness prints which body took each scan (CC_EMU_TRACE_K2); the back end holds cc_ingest_path_counts to those
lines, and the cases hold both to the path predicted from the oracle.  The harness runs a workgroup's threads one after the other:
what it shows is the outcome of one order of the unions (tests/test_gpu_topology.py runs the same cases on the device)."""
import pytest

import topology_cases as TC
from test_emu_height_images import EmuBack


def _be(oracle, capfd, monkeypatch):
    monkeypatch.setenv("CC_EMU_TRACE_K2", "1")
    return EmuBack(oracle, capfd)


@pytest.mark.parametrize("group", sorted(TC.GROUPS))
def test_designed(oracle, capfd, monkeypatch, group):
    TC.run_group(_be(oracle, capfd, monkeypatch), oracle, TC.GROUPS[group], twice=False)


def test_every_designed_scene_is_in_a_group():
    assert sorted(n for g in TC.GROUPS.values() for n in g) == sorted(TC.cases("base"))


@pytest.mark.parametrize("which", ["mid", "big"])
@pytest.mark.parametrize("part", range(4))
def test_designed_on_the_other_bodies(oracle, capfd, monkeypatch, which, part):
    TC.run_group(_be(oracle, capfd, monkeypatch), oracle, TC.variant_names(which, part, 4), which, twice=False, singly=False)


@pytest.mark.parametrize("first", range(0, 256, 64))
def test_random_images_list(oracle, capfd, monkeypatch, first):
    TC.run_fuzz(_be(oracle, capfd, monkeypatch), oracle, "list", range(first, first + 64), 64, False)


@pytest.mark.parametrize("recipe", ["mid", "big"])
def test_random_images_other_bodies(oracle, capfd, monkeypatch, recipe):
    TC.run_fuzz(_be(oracle, capfd, monkeypatch), oracle, recipe, range(32), 32, False)
