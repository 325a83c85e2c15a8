"""The wave / row primitives, math routines and bit-for-bit carriers of csrc/ one by one on the CPU harness: the cases and
references of tests/primitive_cases.py, which tests/test_gpu_primitives.py runs on the device.  The harness compiles the
CC_EMU forms of csrc/cc_group.h (width-16 shuffles) and seeds cc_rsqrt with 1 / sqrt(x); everything else is the code the
device runs."""
import pytest

import dev_probe
import primitive_cases as pc


@pytest.fixture(scope="module")
def P():
    return dev_probe.EmuProbe()


@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("name", sorted(pc.GROUP_OPS))
def test_row_collective_under_divergence(P, name, block):
    """every non-empty set of rows active and rows in the two branches of an if / else: only the caller's row is involved"""
    assert pc.check_group(P, pc.GROUP_OPS[name], block) == 17


@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("name", sorted(pc.WAVE_OPS))
def test_whole_wave_collective(P, name, block):
    pc.check_group(P, pc.WAVE_OPS[name], block)


def test_wave_id_and_uniform_values(P):
    pc.check_uniform(P)


def test_pk_fma_is_fused(P):
    pc.check_pk_fma(P)


def test_load3f_from_4_byte_aligned_bases(P):
    pc.check_load3f(P)


def test_exp_nonpos_within_derived_bound(P):
    pc.check_exp_nonpos(P)


def test_rsqrt_within_derived_bound(P):
    pc.check_rsqrt(P)


def test_sqrt_f64_correctly_rounded(P):
    pc.check_sqrt(P)


def test_gmm_term_value_and_gradient(P):
    pc.check_gmm_term(P)


def test_eigen2f_matches_oracle_restatement(P, oracle):
    pc.check_eigen2f(P)


def test_std_sort_one_lane(P, oracle):
    pc.check_sort_desc(P, oracle, wave=False)
    pc.check_sort_asc_f(P, oracle)
