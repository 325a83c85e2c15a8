"""The class mirror's makeBEV from several clouds with their own transforms (hostcpp/cont2/contour_mng.h, mirror-only) against the
single-cloud makeBEV of the transformed and concatenated cloud -- tests/make_bev_segments_check.cpp, on the CPU harness here and on
the GPU through libcont2_amd.so."""
import os
import subprocess

import numpy as np
import pytest

import emu_api
from parity import terrain_scan
from point_layouts import rigid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_segments_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, n, env=None):
    s = terrain_scan(6, n=n, scale=1.4)
    s[:, 3] = np.float32(np.nan)   # the fourth float of a record is not the rasteriser's to read
    path = tmp_path / "scan.bin"
    s.tofile(path)
    T = [rigid(0.7, np.deg2rad(2.0), np.deg2rad(-3.0), (1.5, -2.0, 0.3), np.float32).reshape(12),
         rigid(-2.1, np.deg2rad(-1.0), np.deg2rad(1.5), (-0.8, 2.5, -0.2), np.float32).reshape(12)]
    r = subprocess.run([exe, str(path)] + [repr(float(v)) for m in T for v in m], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, pts, nc = r.stdout.split()[-3:]
    assert tag == "ok" and int(pts) == n and int(nc) > 10, r.stdout[-300:]


def test_make_bev_from_segments_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_segments_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, 8001, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_from_segments_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_segments_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path, 60001)
