"""The class mirror's makeBEV with a HeightImage (hostcpp/cont2/contour_mng.h, mirror-only): a manager made from a cloud and one made
from the first's getBevImage(), pillar positions and minimum compare equal -- tests/make_bev_image_check.cpp, on the CPU harness here and
on the GPU through libcont2_amd.so."""
import os
import subprocess

import pytest

import emu_api
from parity import terrain_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_image_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, env=None):
    path = tmp_path / "cloud.bin"
    terrain_scan(7, n=8000).tofile(path)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, occ, nc = r.stdout.split()[-3:]
    assert tag == "ok" and int(occ) > 3000 and int(nc) > 10, r.stdout[-300:]


def test_make_bev_of_a_height_image_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_image_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_of_a_height_image_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_image_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path)
