"""The class mirror's makeBEV with a per-point time and knot matrices (hostcpp/cont2/contour_mng.h, mirror-only) against its
single-cloud makeBEV of the host-moved cloud -- tests/make_bev_motion_check.cpp, on the CPU harness here and on the GPU through
libcont2_amd.so."""
import os
import subprocess

import numpy as np
import pytest

import emu_api
from parity import terrain_scan
from point_motion import random_knots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_motion_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, n, env=None):
    K = 8
    s = terrain_scan(6, n=n, scale=1.4)
    s[:, 3] = np.random.default_rng(4).uniform(0.5, 0.6, n).astype(np.float32)   # the time rides in the fourth float: t_begin 0.5, 0.1 long
    s[:5, 3] = np.float32([np.nan, -1.0, 9.0, np.inf, -np.inf])                     # ... and a few that are clamped
    path = tmp_path / "scan.bin"
    s.tofile(path)
    knots = random_knots(1, K, seed=3)[0]
    args = [repr(0.5), repr(float(np.float32(K) / np.float32(0.1))), str(K)] + [repr(float(v)) for v in knots.reshape(-1)]
    r = subprocess.run([exe, str(path)] + args, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, pts, nc = r.stdout.split()[-3:]
    assert tag == "ok" and int(pts) == n and int(nc) > 10, r.stdout[-300:]


def test_make_bev_with_motion_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_motion_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, 8001, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_with_motion_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_motion_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path, 60001)
