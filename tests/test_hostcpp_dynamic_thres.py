"""The class mirror (hostcpp/cont2/contour_db.h) built with the reference's DYNAMIC_THRES=1 (it used to stop with #error):
it compiles, and its single-pair flow (hostcpp/examples/pair_demo.cpp) gives the dynamic CPU oracle's per-hint scores and
result (tests/dyn_thres_oracle.cpp).  CPU variant on the execution harness of the product TU; the GPU variant links the
product library (and tests/test_gpu_dynamic_thres.py runs the offline driver batch_bin_test.cpp built the same way)."""
import os
import subprocess

import numpy as np
import pytest

import dyn_oracle
import emu_api
from test_emu_hints import _demo_hints
from test_hostcpp_pair_flow import _pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCPP = os.path.join(ROOT, "contour-context_amd", "hostcpp")
PKG = os.path.join(ROOT, "contour-context_amd")

TU = r"""
#include "cont2/contour_db.h"
SequentialTimeProfiler stp;
static_assert(CC_MIRROR_DYNAMIC_THRES == DYN_EXPECT, "the macro selects the mode");
int use(const std::shared_ptr<const ContourManager> &q, const std::shared_ptr<const ContourManager> &c) {
  CandidateScoreEnsemble lb, ub;
  CandidateManager m(q, lb, ub);
  m.checkCandWithHint(c, ConstellationPair(1, 0, 0));
  return m.cand_aft_check3;
}
"""


def _compile(tmp_path, defs):
    src = tmp_path / "tu.cpp"
    src.write_text(TU)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", *defs, "-I", HOSTCPP, "-I", os.path.join(ROOT, "include"), str(src)])


def test_mirror_compiles_with_dynamic_thres(tmp_path):
    _compile(tmp_path, ["-DDYNAMIC_THRES=1", "-DDYN_EXPECT=1"])


def test_mirror_default_stays_static(tmp_path):
    _compile(tmp_path, ["-DDYN_EXPECT=0"])
    _compile(tmp_path, ["-DDYNAMIC_THRES=0", "-DDYN_EXPECT=0"])


def pair_demo_vs_dyn_oracle(cc, oracle, exe, tmp_path, device=None, env=None):
    """run pair_demo (built with -DDYNAMIC_THRES=1) on the pair of the short loop drive; compare with orcdyn_check_hints"""
    L = oracle.L
    xs, odesc, qi, c, dcfg = _pair(cc, oracle, device)
    old, new = tmp_path / "old.bin", tmp_path / "new.bin"
    xs[c].astype(np.float32).tofile(old)
    xs[qi].astype(np.float32).tofile(new)
    out = subprocess.check_output([exe, str(old), str(new), "5", str(tmp_path / "img")], text=True, env=env)
    hl = [[int(v) for v in l.split()[1:]] for l in out.split("\n") if l.startswith("H ")]
    rl = [l.split()[1:] for l in out.split("\n") if l.startswith("R ")]
    hints = _demo_hints(L, odesc, qi, [c])
    eres, esc = dyn_oracle.check_hints(odesc, qi, [c], hints, dcfg.cont_sim, max_fine_opt=5, dyn=1)
    _, ssc = dyn_oracle.check_hints(odesc, qi, [c], hints, dcfg.cont_sim, max_fine_opt=5, dyn=0)
    assert len(hl) == len(hints) and len(rl) == 1
    for got, h, s in zip(hl, hints, esc):
        assert got[:3] == list(h[1:]) and got[3:] == list(s[:5]), (got, h, s)
    r = rl[0]
    assert int(r[0]) == eres["n_res"]
    if eres["n_res"]:
        assert abs(float(r[1]) - eres["correlation"]) < 1e-6
        assert np.abs(np.array([float(v) for v in r[2:5]]) - eres["tf"]).max() < 1e-5
    n_changed = int((esc[:, :5] != ssc[:, :5]).any(1).sum())
    assert n_changed > 0, "the raised bars changed no returned score: the drive would not tell the modes apart"
    return n_changed


def test_pair_demo_dynamic_on_cpu_harness(cc, oracle, tmp_path):
    emu_so = emu_api.build()
    exe = str(tmp_path / "pair_demo_dyn_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-DDYNAMIC_THRES=1", os.path.join(PKG, "hostcpp", "examples", "pair_demo.cpp"),
                           "-I", os.path.join(PKG, "hostcpp"), "-L", os.path.dirname(emu_so), "-lcc_emu",
                           "-Wl,-rpath," + os.path.dirname(emu_so), "-pthread", "-o", exe])
    pair_demo_vs_dyn_oracle(cc, oracle, exe, tmp_path, env=dict(os.environ, **emu_api.SMALL_GRIDS))


@pytest.mark.gpu
def test_pair_demo_dynamic_on_gpu(cc, oracle, tmp_path):
    exe = str(tmp_path / "pair_demo_dyn")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-DDYNAMIC_THRES=1", os.path.join(PKG, "hostcpp", "examples", "pair_demo.cpp"),
                           "-I", os.path.join(PKG, "hostcpp"), "-L", PKG, "-lcont2_amd", "-Wl,-rpath," + PKG,
                           "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    pair_demo_vs_dyn_oracle(cc, oracle, exe, tmp_path, device="cuda")
