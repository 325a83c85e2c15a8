"""The class mirror's makeBEV with a BevCoords (hostcpp/cont2/contour_mng.h, mirror-only) against its plain makeBEV of the cloud
converted on the host by the header's three steps -- tests/make_bev_coords_check.cpp, on the CPU harness here and on the GPU through
libcont2_amd.so.  The program's input buffers hold exactly the spanned bytes in front of an inaccessible page: an over-read faults."""
import os
import subprocess

import numpy as np
import pytest

import emu_api
import point_coords as PC
from parity import terrain_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_coords_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, n, env=None):
    q = PC.quantised(terrain_scan(9, n=n, scale=1.4))
    O = PC.geo_origins(1, seed=44)[0]
    path = tmp_path / "scan.bin"
    np.ascontiguousarray(q + O).tofile(path)
    r = subprocess.run([exe, str(path)] + [repr(float(v)) for v in O], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, pts, nc = r.stdout.split()[-3:]
    assert tag == "ok" and int(pts) == n and int(nc) > 10, r.stdout[-300:]


def test_make_bev_with_coords_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_coords_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, 8001, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_with_coords_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_coords_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path, 12001)
