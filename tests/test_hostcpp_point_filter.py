"""The class mirror's makeBEV with a BevFilter (hostcpp/cont2/contour_mng.h, mirror-only) against its plain makeBEV of the cloud
compacted on the host -- tests/make_bev_filter_check.cpp, on the CPU harness here and on the GPU through libcont2_amd.so."""
import os
import subprocess

import numpy as np
import pytest

import emu_api
from parity import terrain_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "make_bev_filter_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(exe, tmp_path, n, env=None):
    rng = np.random.default_rng(12)
    s = terrain_scan(9, n=n, scale=1.4)
    # the label word: class in the low 16 bits -- a tenth of the records moving (252 .. 259), biased to the high points so that dropped
    # records own cells -- and in the high 16 an "instance id" that makes the word, read as an f32, 1.x, 2.x, 3.x or 4.x
    cls = rng.integers(0, 100, n).astype(np.uint32)
    moving = (rng.random(n) < 0.05) | ((s[:, 2] > np.quantile(s[:, 2], 0.8)) & (rng.random(n) < 0.3))
    cls[moving] = rng.integers(252, 260, int(moving.sum())).astype(np.uint32)
    inst = rng.choice(np.array([0x3F80, 0x4000, 0x4040, 0x4080], np.uint32), n)
    s[:, 3] = ((inst << np.uint32(16)) | cls).view(np.float32)
    path = tmp_path / "scan.bin"
    s.tofile(path)
    r = subprocess.run([exe, str(path), "1.5", "3.5"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, pts, kept_c, kept_r, nc = r.stdout.split()[-5:]
    assert tag == "ok" and int(pts) == n and int(kept_c) == n - int(moving.sum()) and int(nc) > 10, r.stdout[-300:]
    assert int(kept_r) == int(((inst == 0x4000) | (inst == 0x4040)).sum())


def test_make_bev_with_a_filter_on_the_cpu_harness(tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "make_bev_filter_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(exe, tmp_path, 8001, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_make_bev_with_a_filter_on_the_gpu(tmp_path):
    exe = str(tmp_path / "make_bev_filter_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(exe, tmp_path, 12001)
