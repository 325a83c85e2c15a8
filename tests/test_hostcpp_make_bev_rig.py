"""The class mirror's makeBEV from a rig's clouds -- each de-skewed by its time words on its slice of the knots or moved by its matrix,
each filtered by its own label word -- (hostcpp/cont2/contour_mng.h, mirror-only) against the single-cloud makeBEV of the moved, kept
points built on the host: tests/make_bev_rig_check.cpp, on the CPU harness here and on the GPU through libcont2_amd.so."""
import os
import subprocess

import numpy as np
import pytest

import emu_api
from parity import terrain_scan
from point_filter import kitti_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_rig_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, n, env=None):
    s = terrain_scan(8, n=n, scale=1.4)
    lab = kitti_labels(np.random.default_rng(9), s)
    s[:, 3] = lab.view(np.float32)
    path = tmp_path / "scan.bin"
    s.tofile(path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, pts, kept, nc = r.stdout.split()[-4:]
    assert tag == "ok" and int(pts) == n and 10 < int(kept) < n and int(nc) > 10, r.stdout[-300:]


def test_make_bev_from_a_rig_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_rig_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, 8001, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_from_a_rig_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_rig_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path, 60001)
