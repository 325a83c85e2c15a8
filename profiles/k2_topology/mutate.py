"""Does tests/test_emu_topology.py bite?  Each edit below is made on a scratch copy of csrc/ (never in the tree), the CPU harness
is built from the copy, and the topology tests run on that library.  One line per edit on stdout: the tests that fail.
usage: python profiles/k2_topology/mutate.py [edit names ...]     (from the repository root; results in a temporary directory)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIST, BODY = "k_contours_list.h", "k_contours.h"
UNION = "      if (cc_lds_vread16(LAB + a_) != cc_lds_vread16(LAB + b_)) cc_uf_union_h(LAB, a_, b_);           \\\n"
EDITS = {   # name -> (file, old, new, occurrences)
    "1_m_n": (LIST, "unsigned m_n = b_n & ~(b_w & b_nw);", "unsigned m_n = b_n & ~b_w;", 1),
    "2_m_w": (LIST, "unsigned m_w = ((i & 63) == 0) ? b_w : 0u;", "unsigned m_w = 0u;", 1),
    "3_col0": (LIST, "if (cc == 0) f3 &= 6u;", "", 1),
    "4_col_last": (LIST, "if (cc == n_col - 1) f3 &= 3u;", "", 1),
    "5_bit62": (LIST, "if (bit > 61) raw |=", "if (bit > 62) raw |=", 1),
    "6_overflow_union": (LIST, UNION, "      (void)a_; (void)b_; \\\n", 1),
    "7_padding": (LIST, "const int a4 = (a + 1) & ~1;", "const int a4 = a;", 1),
    "8_lane_tail": (LIST, "mk[u] = (unsigned)-(int)(u < nv);  // all ones for a member", "mk[u] = (unsigned)-(int)(u <= nv);  // all ones for a member", 1),
    "9_big_at_65": (LIST, "a >= CC_K2L_BIG ? 7", "a > CC_K2L_BIG ? 7", 2),
    "10a_cB_always": (BODY, "if (ra == rmin && cp.cB < cm) cm = cp.cB;", "if (ra == rmin) cm = cp.cB;", 1),
    "10b_cB_never": (BODY, "if (ra == rmin && cp.cB < cm) cm = cp.cB;", "", 1),
}
RUN = """
import sys
sys.path[:0] = [%(root)r, %(root)r + "/oracle", %(root)r + "/tests"]
import emu_api
emu_api.build = lambda *a, **k: %(so)r
emu_api.SO = %(so)r
import pytest
sys.exit(pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu", "--tb=line", %(root)r + "/tests/test_emu_topology.py"]))
"""


def one(name, tmp):
    f, old, new, n = EDITS[name]
    d = os.path.join(tmp, name)
    shutil.copytree(os.path.join(ROOT, "contour-context_amd", "csrc"), os.path.join(d, "contour-context_amd", "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
    os.makedirs(os.path.join(d, "tests"))
    for sub in ("emu", "devprobe"):
        shutil.copytree(os.path.join(ROOT, "tests", sub), os.path.join(d, "tests", sub), ignore=shutil.ignore_patterns("*.so", "__pycache__"))
    p = os.path.join(d, "contour-context_amd", "csrc", f)
    s = open(p).read()
    assert s.count(old) == n, (name, s.count(old))
    open(p, "w").write(s.replace(old, new))
    so = os.path.join(d, "tests", "emu", "libcc_emu.so")
    subprocess.check_call(["sh", os.path.join(d, "tests", "emu", "build.sh")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, "-c", RUN % {"root": ROOT, "so": so}], capture_output=True, text=True, cwd=d)
    failed = re.findall(r"^FAILED \S+::(\S+)", r.stdout, flags=re.M)
    scenes = sorted({n for m in re.findall(r"SCENES THAT FAIL: ([^'\"]*)", r.stdout) for n in m.split() if not n.startswith("fuzz_")})
    open(os.path.join(tmp, name + ".log"), "w").write(r.stdout + r.stderr)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "(no output)"
    if r.returncode < 0:
        last = "the harness process ended on signal %d" % -r.returncode
    return "%-18s %s\n%-18s   tests:  %s\n%-18s   scenes: %s" % (name, last, "", " ".join(failed) if failed else "nothing fails", "", " ".join(scenes) or "-")


if __name__ == "__main__":
    names = sys.argv[1:] or list(EDITS)
    tmp = tempfile.mkdtemp(prefix="k2_mutants_")
    print("logs in", tmp)
    with ThreadPoolExecutor(4) as ex:
        for line in ex.map(lambda n: one(n, tmp), names):
            print(line, flush=True)
