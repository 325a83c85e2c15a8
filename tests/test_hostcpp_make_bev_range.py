"""The class mirror's makeBEV with a RangeImage (hostcpp/cont2/contour_mng.h, mirror-only) against its single-cloud makeBEV of the
cloud computed on the host by the header's formula -- tests/make_bev_range_check.cpp, on the CPU harness here and on the GPU through
libcont2_amd.so."""
import os
import subprocess

import numpy as np
import pytest

import emu_api
from point_motion import random_knots
from range_images import procedural_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_range_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, H, W, env=None):
    K = 8
    images, _ = procedural_ranges(H, W, 1, seed=6)   # u16, 2 mm, row-major, 5 % no-return
    path = tmp_path / "ranges.bin"
    images[0].tofile(path)
    knots = random_knots(1, K, seed=3, max_shift=3.0)[0]
    args = [str(H), str(W), str(K)] + [repr(float(v)) for v in knots.reshape(-1)]
    r = subprocess.run([exe, str(path)] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, pix, nc = r.stdout.split()[-3:]
    assert tag == "ok" and int(pix) == H * W and int(nc) > 10, r.stdout[-300:]


def test_make_bev_of_a_range_image_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_range_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, 16, 601, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_of_a_range_image_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_range_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path, 64, 1875)
