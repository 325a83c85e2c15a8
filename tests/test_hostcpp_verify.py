"""The class mirror's ContourDB::verifyCandidates (hostcpp/cont2/contour_db.h, mirror-only) against the mirror's own CandidateManager
demo loop on the same candidates -- tests/verify_candidates_check.cpp, on the CPU harness here and on the GPU through
libcont2_amd.so."""
import os
import subprocess

import pytest

import emu_api
from test_hostcpp_pair_flow import _pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "contour-context_amd")
SRC = os.path.join(ROOT, "tests", "verify_candidates_check.cpp")
COMMON = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-I", os.path.join(PKG, "hostcpp"), "-I", os.path.join(ROOT, "include")]


def _run(cc, oracle, exe, tmp_path, device=None, env=None):
    import numpy as np
    xs, odesc, qi, c, dcfg = _pair(cc, oracle, device)
    files = []
    for k, g in enumerate((3, c, c + 1)):   # database scans 0, 1, 2: a far scan, the revisited place, its neighbour
        files.append(str(tmp_path / ("cand%d.bin" % k)))
        xs[g].astype(np.float32).tofile(files[-1])
    files.append(str(tmp_path / "query.bin"))
    xs[qi].astype(np.float32).tofile(files[-1])
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    tag, n_res, which, corr, n_hints = r.stdout.split()[-5:]
    assert tag == "ok" and int(n_res) == 1 and int(which) in (1, 2) and float(corr) > 0.3 and int(n_hints) > 30, r.stdout[-300:]


def test_verify_candidates_on_the_cpu_harness(cc, oracle, tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "verify_candidates_check")
    subprocess.check_call(COMMON + ["-L", os.path.dirname(emu_so), "-lcc_emu", "-Wl,-rpath," + os.path.dirname(emu_so), "-o", exe])
    _run(cc, oracle, exe, tmp_path, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_verify_candidates_on_the_gpu(cc, oracle, tmp_path):
    exe = str(tmp_path / "verify_candidates_check")
    subprocess.check_call(COMMON + ["-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    _run(cc, oracle, exe, tmp_path, device="cuda")
