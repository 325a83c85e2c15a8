"""The wave / row primitives, math routines and bit-for-bit carriers of csrc/ one by one ON THE DEVICE: probe kernels
(tests/devprobe) compiled with the library's own flags call the product's functions -- the DPP controls, readlanes, the
mbcnt pair, inverse_ballot, v_rsq_f64, the device's f32 division and sqrtf -- on the cases of tests/primitive_cases.py,
the same ones tests/test_emu_primitives.py runs on the CPU harness.  Where both sides are IEEE operation for operation the
device must give the harness' bits."""
import pytest

import dev_probe
import primitive_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    return dev_probe.GpuProbe()


@pytest.fixture(scope="module")
def H():
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


def test_exp_nonpos_within_derived_bound_and_harness_bits(P, H):
    pc.check_exp_nonpos(P, other=H)


def test_rsqrt_within_derived_bound(P, H):
    pc.check_rsqrt(P, other=H)


def test_sqrt_f64_correctly_rounded(P):
    pc.check_sqrt(P)


def test_gmm_term_value_and_gradient(P):
    pc.check_gmm_term(P)


def test_atan2f_replica_bits(P, H):
    pc.check_atan2f(P, other=H)


def test_acosf_replica_bits(P, H):
    pc.check_acosf(P, other=H)


def test_eigen2f_bits(P, H, oracle):
    pc.check_eigen2f(P, other=H)


def test_std_sort_one_lane(P, oracle):
    pc.check_sort_desc(P, oracle, wave=False)
    pc.check_sort_asc_f(P, oracle)


def test_std_sort_wave(P, oracle):
    pc.check_sort_desc(P, oracle, wave=True)


def test_block_bitonic_and_scans(P):
    pc.check_block_sort_and_scans(P)
