"""K2's labelling, member lists, statistics walks and hand-offs on built images (tests/topology_cases.py) on the MI355X.  The list
kernel's union-find links runs with a 32-bit CAS while other threads halve paths with 16-bit stores, all six level sets in one
slot space and one LDS work list; the CPU harness runs those threads one after the other, so only here do they meet.  Every call
is made twice, the second time with its images in reversed order (the same scan in another workgroup, beside other neighbours on its
CU): equal bytes.  The designed scenes also go one image per call, the other launch shape, which attributes the body to the scan.
Which body took a call's scans comes from cc_ingest_path_counts and is held to the path predicted from the oracle.  These runs
are evidence of outcomes, not of which interleavings occurred."""
import pytest

import topology_cases as TC
from test_gpu_height_images import GpuBack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", sorted(TC.GROUPS))
def test_designed(cc, oracle, group):
    TC.run_group(GpuBack(cc), oracle, TC.GROUPS[group])


@pytest.mark.parametrize("which", ["mid", "big"])
@pytest.mark.parametrize("part", range(4))
def test_designed_on_the_other_bodies(cc, oracle, which, part):
    TC.run_group(GpuBack(cc), oracle, TC.variant_names(which, part, 4), which)


@pytest.mark.parametrize("first", range(0, 1024, 128))
def test_random_images_list(cc, oracle, first):
    TC.run_fuzz(GpuBack(cc), oracle, "list", range(first, first + 128), 128, True)


@pytest.mark.parametrize("recipe", ["mid", "big"])
def test_random_images_other_bodies(cc, oracle, recipe):
    TC.run_fuzz(GpuBack(cc), oracle, recipe, range(128), 128, True)
