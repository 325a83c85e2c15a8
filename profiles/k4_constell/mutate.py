"""Does tests/test_emu_constell.py bite?  Each edit below is made on a scratch copy of csrc/ (never in the tree), the CPU harness
is built from the copy, and the constellation tests run on that library.  No edit makes a kernel write out of bounds, and no
mutated build is for the GPU.  One block per edit on stdout: the tests and the cases that fail.
usage: python profiles/k4_constell/mutate.py [edit names ...]     (from the repository root; results in a temporary directory)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHK, MRG = "k_check.h", "k_merge.h"
EDITS = {   # name -> (file, old, new, occurrences)
    "a1_shl_carry": (CHK, "(S[w] << 1) | (w > 0 ? (S[w - 1] >> 63) : 0ull)", "(S[w] << 1)", 1),
    "a2_shr_carry": (CHK, "(S[w] >> 1) | (w < 3 ? (S[w + 1] << 63) : 0ull)", "(S[w] >> 1)", 1),
    "a3_eig_switch": (CHK, "if ((ea < eb ? eb : ea) > 2.0f) {", "if ((ea < eb ? eb : ea) >= 2.0f) {", 2),
    "a4_cell_switch": (CHK, "a.cell_cnt) > 15 &&", "a.cell_cnt) > 16 &&", 1),
    # (with `>` a segment without a left stopper has no cut: the guard, made in the scratch copy only, keeps it inside the segment)
    "b1_partition_ge": (CHK, ["ls = k >= piv;", "      if (K > 0 && (int)rasc[nR - K] < cut) cut = rasc[nR - K];\n"],
                        ["ls = k > piv;", "      if (K > 0 && (int)rasc[nR - K] < cut) cut = rasc[nR - K];\n      if (cut > last) cut = last;\n      if (cut <= first) cut = first + 1;\n"], 1),
    "b0_deep_no_regeneration": (CHK, "    cc_group_sync();\n    cc_b1_gen_pairs<PPM>(L, ntp, sl);\n    cc_group_sync();\n    if (sl == 0)\n      ccsort::std_sort",
                                "    cc_group_sync();\n    if (sl == 0)\n      ccsort::std_sort", 1),
    "b0_deep_never": (CHK, "      if (depth == 0) {\n        deep = true;\n        break;\n      }\n      depth--;", "      depth--;", 1),
    "b2_rank_position_16": (CHK, "const unsigned long long me = ((unsigned long long)kme << 32) | (unsigned)sl;",
                            "const unsigned long long me = ((unsigned long long)kme << 32) | (unsigned)(npp - 1 - sl);", 1),
    "b3_rank_position_64": (CHK, "me[u] = ((unsigned long long)kv[u] << 32) | (unsigned)p;", "me[u] = ((unsigned long long)kv[u] << 32) | (unsigned)(npp - 1 - p);", 1),
    "b4_rank_position_bins": (CHK, "(f2 == f && o2 < o)", "(f2 == f && o2 > o)", 1),
    "b5_counting_start": (CHK, "const int start = bn ? L.hist[bn - 1] : 0, end = L.hist[bn];",
                          "const int start = bn > 1 ? L.hist[bn - 2] : 0, end = L.hist[bn];", 1),
    "b6_clamp_ge": (CHK, "(xw >= 2 * 3.14159265358979323846 ? 1.0 : 0.0)", "(xw > 2 * 3.14159265358979323846 ? 1.0 : 0.0)", 1),
    "b7_pair_hi": (CHK, ".bit_pos <= tb + 1;", ".bit_pos < tb + 1;", 1),
    "c1_wrap_t_up": (CHK, "#define CC_B1_WRAP_T (-0x1.858eb6p+2f)", "#define CC_B1_WRAP_T (-0x1.858eb4p+2f)", 1),
    "c2_wrap_t_down": (CHK, "#define CC_B1_WRAP_T (-0x1.858eb6p+2f)", "#define CC_B1_WRAP_T (-0x1.858eb8p+2f)", 1),
    "c3_range_ge": (CHK, "d >= CC_B1_WRAP_T : d > angular_range;", "d >= CC_B1_WRAP_T : d >= angular_range;", 1),
    "c4_tie_rule": (CHK, "if (len > bestL || (len == bestL && p1 < bestP)) {", "if (len >= bestL) {", 1),
    "c5_anchor_clause": (CHK, "if (e < longest && e < n_in - 1) {", "if (e < longest) {", 1),
    "d1_lim_9": (CHK, "const int lim = ncs < 10 ? ncs : 10;", "const int lim = ncs < 9 ? ncs : 9;", 1),
    "d2_sure_1_5": (CHK, "1.001f", "1.5f", 2),
    "d2b_sure_0_5": (CHK, "1.001f", "0.5f", 2),
    "d3_acos_band_0": (CHK, "if (fabsf(da - pi6) < 1e-5f || fabsf(db - pi6) < 1e-5f) {", "if (false) {", 1),
    "d4_nrm_branch": (CHK, "if (nrm < 1e-6) {  // (group-uniform)", "if (false) {", 1),
    "d5_stable_filter": (CHK, "L.keepf[k] = L.keepf[num_sim - 1];  // std::swap",
                         "for (int z_ = k; z_ < num_sim - 1; z_++) L.keepf[z_] = L.keepf[z_ + 1];  // std::swap", 1),
    "e1_nprops_2": (MRG, "} else if (nprops <= 3) {", "} else if (nprops <= 2) {", 1),
    "e2_w1_before_vote": (MRG, "        p->vote_cnt += np;\n        const int w1 = p->vote_cnt, w2 = np;", "        const int w1 = p->vote_cnt, w2 = np;\n        p->vote_cnt += np;", 1),
    "e3_before_late": (MRG, "      else if (before >= 0)\n        L.next[before] = (short)i;", "      else if (k >= 0)\n        L.next[L.clast[k]] = (short)i;", 1),
    # (the cg slots behind the last candidate are inside the array, STR + 4 entries: stale values are read, nothing is written out of bounds)
    "e4_sentinels": (MRG, "    if (lane < 4) L.cg[nc + lane] = -1;\n    __syncthreads();  // the next round", "    __syncthreads();  // the next round", 1),
    # (one trip of the candidate loop only; the candidates it leaves out get a record of their own and no correlation problem, so
    # nothing downstream reads what was never written)
    "e5_stride": (MRG, "  for (int k = tid; k < nc; k += CC_MERGE_BLOCK) {\n    int i = L.firstrec[k];",
                  "  for (int k = tid; k < nc; k += CC_MERGE_BLOCK) {\n    if (k >= CC_MERGE_BLOCK) {\n      cc_cand_out o_;\n      o_.gidx = L.gid[L.firstrec[k]];\n      o_.nprops = 0;\n"
                  "      o_.gmm_idx = -1;\n      o_.pad = 0;\n      cands_all[(size_t)q * CC_CHK_STRIDE_K(KM) + k] = o_;\n      L.want[k] = 0;\n      continue;\n    }\n    int i = L.firstrec[k];", 1),
    # the second arms of the 2.0 px and 0.3 rad bars: what decides inside the 1e-9 bands
    "e6_band_t_always": (MRG, '        if (!near_t && n2 <= 4.0 * (1.0 + 1e-9)) near_t = sqrt(n2) < 2.0;', '        if (!near_t && n2 <= 4.0 * (1.0 + 1e-9)) near_t = true;', 1),
    "e7_band_t_never": (MRG, '        if (!near_t && n2 <= 4.0 * (1.0 + 1e-9)) near_t = sqrt(n2) < 2.0;', "", 1),
    "e8_band_r_always": (MRG, '          if (!near_r && d00 > 0.0 && ay <= lim * (1.0 + 1e-9)) near_r = fabs(atan2(d10, d00)) < 0.3;', '          if (!near_r && d00 > 0.0 && ay <= lim * (1.0 + 1e-9)) near_r = true;', 1),
    "e9_band_r_never": (MRG, '          if (!near_r && d00 > 0.0 && ay <= lim * (1.0 + 1e-9)) near_r = fabs(atan2(d10, d00)) < 0.3;', "", 1),
    # the bar of the sequential branch of the umeyama
    "d6_nrm_bar_1e_5": (CHK, "if (nrm < 1e-6) {  // (group-uniform)", "if (nrm < 1e-5) {  // (group-uniform)", 1),
    "d7_nrm_bar_1e_9": (CHK, "if (nrm < 1e-6) {  // (group-uniform)", "if (nrm < 1e-9) {  // (group-uniform)", 1),
}
PARTS = "not shapes"   # the 1 152-hint calls take most of the harness's time and add no case of their own to these edits
RUN = """
import sys
sys.path[:0] = [%(root)r, %(root)r + "/oracle", %(root)r + "/tests"]
import emu_api
emu_api.build = lambda *a, **k: %(so)r
emu_api.SO = %(so)r
import pytest
sys.exit(pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu", "--tb=line", "-k", %(parts)r, %(root)r + "/tests/test_emu_constell.py"]))
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
    olds, news = (old, new) if isinstance(old, list) else ([old], [new])
    for o_, n_ in zip(olds, news):
        assert s.count(o_) == n, (name, o_, s.count(o_))
        s = s.replace(o_, n_)
    open(p, "w").write(s)
    old, new = olds[0], news[0]
    so = os.path.join(d, "tests", "emu", "libcc_emu.so")
    subprocess.check_call(["sh", os.path.join(d, "tests", "emu", "build.sh")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        r = subprocess.run([sys.executable, "-c", RUN % {"root": ROOT, "so": so, "parts": PARTS}], capture_output=True, text=True, cwd=d, timeout=400)
        out, rc = r.stdout, r.returncode
    except subprocess.TimeoutExpired as e:
        out, rc = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), None
    failed = re.findall(r"^FAILED \S+::(\S+)", out, flags=re.M)
    cases = ["%s: %s" % m for m in re.findall(r"AssertionError: \(\('([^']+)', '?([^',)]+)", out)]
    open(os.path.join(tmp, name + ".log"), "w").write(out)
    last = out.strip().splitlines()[-1] if out.strip() else "(no output)"
    if rc is None:
        last = "the harness process did not end within 400 s"
    elif rc < 0:
        last = "the harness process ended on signal %d" % -rc
    return "%-22s %s -> %s\n%-22s   %s\n%-22s   tests: %s\n%-22s   first failing case per test: %s" % (
        name, old.splitlines()[0].strip()[:70], new.splitlines()[0].strip()[:70] if new else "(removed)", "", last, "",
        " ".join(failed) if failed else "nothing fails", "", "; ".join(cases) or "-")


if __name__ == "__main__":
    names = sys.argv[1:] or list(EDITS)
    tmp = tempfile.mkdtemp(prefix="k4_mutants_")
    print("logs in", tmp)
    with ThreadPoolExecutor(6) as ex:
        for line in ex.map(lambda n: one(n, tmp), names):
            print(line, flush=True)
