"""cc_atan2f_fdlibm (csrc/cc_stats.h): the device's restatement of glibc's atan2f, used for BCI::RelativePoint::theta
(contour_mng.h:860).  Compiled for the CPU by the test harness and compared BIT FOR BIT with std::atan2(float, float) of this libm (through
the oracle library; numpy's float32 arctan2 is a SIMD routine of its own): differences of BEV coordinates, random bit
patterns, the special cases."""
import ctypes as C

import numpy as np

import emu_api
import primitive_cases as pc


def _mine(y, x):
    lib = C.CDLL(emu_api.build())
    y = np.ascontiguousarray(y, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(y)
    lib.emu_atan2f(C.c_void_p(y.ctypes.data), C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), C.c_long(len(y)))
    return out


def test_bit_identical_to_libm():
    # differences of contour centres inside the 150 x 150 BEV, random bit patterns, the special cases (primitive_cases.py:
    # the device runs a cut of the same sets, tests/test_gpu_primitives.py)
    y, x = pc.atan2f_args(4_000_000)
    want = pc.libm_atan2f(y, x)
    got = _mine(y, x)
    bad = np.nonzero(want.view(np.uint32) != got.view(np.uint32))[0]
    assert len(bad) == 0, [(float(y[i]), float(x[i]), float(want[i]), float(got[i])) for i in bad[:5]]


def test_acosf_bit_identical_to_libm():
    """cc_acosf_fdlibm (csrc/cc_stats.h): the orientation filter of checkConstellCorrespSim (contour_mng.h:1195-1210) compares
    acos values with pi / 6; the device library's acosf is off by an ulp now and then (round 6, fuzz drive 131409)."""
    x = pc.acosf_args(6_000_000)   # dot products of unit vectors, some beyond +-1 (NaN), random bit patterns, special cases
    want = pc.libm_acosf(x)
    lib = C.CDLL(emu_api.build())
    got = np.zeros_like(x)
    lib.emu_acosf(C.c_void_p(x.ctypes.data), C.c_void_p(got.ctypes.data), C.c_long(len(x)))
    same = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
    bad = np.nonzero(~same)[0]
    assert len(bad) == 0, (len(bad), x[bad[:5]], want[bad[:5]], got[bad[:5]])
