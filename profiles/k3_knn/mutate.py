"""Does tests/test_emu_knn.py bite?  Each edit below is made on a scratch copy of csrc/ (never in the tree), the CPU harness is
built from the copy, and the K3 cases run on that library.  No edit makes a kernel write out of bounds, and no mutated build is
for the GPU.  One block per edit on stdout: the parts that fail and the first failing case of each.
usage: python profiles/k3_knn/mutate.py [edit names ...]     (from the repository root; results in a temporary directory)"""
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KNN = "k_knn.h"
BUCKET = "if (!found && rg[i] <= k[0] && rg[i + 1] > k[0]) {"
PRE_POST_W = "(tightened ? (r <= ub) : (r < ub))"
PRE_POST_T = "(L.st[js].tight ? (r_ <= ub) : (r_ < ub))"
EDITS = {   # name -> [(old, new, occurrences[, file]), ...]; the file is k_knn.h unless named
    # A1: the bucket rule (the walk and the tiled search carry a copy each)
    "a1_bucket_lo_lt": [(BUCKET, "if (!found && rg[i] < k[0] && rg[i + 1] > k[0]) {", 2)],
    "a1_bucket_hi_ge": [(BUCKET, "if (!found && rg[i] <= k[0] && rg[i + 1] >= k[0]) {", 2)],
    "a1_s2_at_2mid": [("if (i == 2 * mid + 1) t_s2 = rg[i];", "if (i == 2 * mid) t_s2 = rg[i];", 2)],
    "a1_e1_at_mid": [("if (i == mid + 1) t_e1 = rg[i];", "if (i == mid + 2) t_e1 = rg[i];", 2)],
    # A2: the 9-ary searches of the walk, the binary searches of the tiled search
    "a2_walk_lb_le": [("(K[(unsigned)(p < 0 ? 0 : p)] < tg)", "(K[(unsigned)(p < 0 ? 0 : p)] <= tg)", 1)],
    "a2_walk_clamp": [("      p = p < hi - 1 ? p : hi - 1;\n", "      p = p < hi - 2 ? p : hi - 2;\n", 1)],
    "a2_tile_lb_le": [("      if (K[m_] < tg)\n", "      if (K[m_] <= tg)\n", 1)],
    # A3: the virtual positions of the walk (index E1 is read, inside the layer whenever the second range holds a key)
    "a3_splice_up": [("(v_ < ua_len ? ua0 + v_ : ub0 + (v_ - ua_len))", "(v_ <= ua_len ? ua0 + v_ : ub0 + (v_ - ua_len))", 1)],
    "a3_splice_down": [("(v_ < db_len ? db_top - v_ : da_top - (v_ - db_len))", "(v_ <= db_len ? db_top - v_ : da_top - (v_ - db_len))", 1)],
    # A4: the radius
    "a4_walk_pre_le": [(PRE_POST_W, "(tightened ? (r <= ub) : (r <= ub))", 1)],
    "a4_walk_post_lt": [(PRE_POST_W, "(tightened ? (r < ub) : (r < ub))", 1)],
    "a4_walk_open_post_lt": [("(tightened ? (far2[dir] <= ub) : (far2[dir] < ub))", "(tightened ? (far2[dir] < ub) : (far2[dir] < ub))", 1)],
    "a4_tile_pre_le": [(PRE_POST_T, "(L.st[js].tight ? (r_ <= ub) : (r_ <= ub))", 1)],
    "a4_tile_post_lt": [(PRE_POST_T, "(L.st[js].tight ? (r_ < ub) : (r_ < ub))", 1)],
    "a4_tile_out_ge": [("(tightj ? (e * e > ubj) : (e * e >= ubj))", "(tightj ? (e * e >= ubj) : (e * e >= ubj))", 1)],
    "a4_tie_break_reversed": [("| (unsigned)kcur[dir];", "| (unsigned)(0x7fffffff - kcur[dir]);", 1), ("| (unsigned)kid;", "| (unsigned)(0x7fffffff - kid);", 1),
                              ("const unsigned id = (unsigned)(first & 0xFFFFFFFFu);", "const unsigned id = 0x7fffffffu - (unsigned)(first & 0xFFFFFFFFu);", 2),
                              ("const unsigned id = (unsigned)(v[a] & 0xFFFFFFFFu);", "const unsigned id = 0x7fffffffu - (unsigned)(v[a] & 0xFFFFFFFFu);", 1)],
    "a4_walk_reduce_width": [("ub = cnt <= 128 ? cc_knn_reduce<2>(buf, cnt, nnk, lane, first) : cc_knn_reduce<4>(buf, cnt, nnk, lane, first);",
                              "ub = cnt <= 192 ? cc_knn_reduce<2>(buf, cnt, nnk, lane, first) : cc_knn_reduce<4>(buf, cnt, nnk, lane, first);", 1)],
    # A5: epochs
    "a5_walk_epoch_lt": [("act[dir] <= epoch &&", "act[dir] < epoch &&", 1)],
    "a5_tile_epoch_lt": [("if (act <= L.qb[js][4] &&", "if (act < L.qb[js][4] &&", 1)],
    # A6: the counts of the searches that do not run
    "a6_order_no_zero": [("        hit_cnt[q * (CC_NQLEV * CC_NPIV) + ll * CC_NPIV + seq] = 0;\n", "        ;\n", 1)],
    "a6_order_unqueried_layers": [("      hit_cnt[q * (CC_NQLEV * CC_NPIV) + P.n_q_levels * CC_NPIV + r] = 0;\n", "      ;\n", 1)],
    "a6_sum_test": [("if (!(sum != 0.f) || n <= 0) {", "if (!(k[0] != 0.f) || n <= 0) {", 1)],
    # B1/B2: order and groups
    "b1_drop_last_of_group": [("const bool valid = j < ns;", "const bool valid = j < ns - (ns == CC_KNN_TQ ? 1 : 0);", 1)],
    "b1_no_clamped_log": [("log2f(q0 > 1e-3f ? q0 : 1e-3f)", "log2f(q0 > 1e-3f ? q0 : 1.f)", 1)],
    "b2_sort_width_1024": [("  if (ns <= 1024) {\n", "  if (ns <= 1026) {\n", 1)],
    "b2_sort_width_4096": [("  } else if (ns <= 4096) {\n", "  } else if (ns <= 4098) {\n", 1)],
    # B3: the common walk
    "b3_idx_lt_n": [("vis |= (idx >= 0 && idx < n && (", "vis |= (idx >= 0 && (", 1)],
    "b3_vis_e1": [("((idx >= L0 && idx < E1) || (idx >= S2 && idx < E2))) ? (1u << (4 * t + r)) : 0u;", "((idx >= L0 && idx <= E1) || (idx >= S2 && idx < E2))) ? (1u << (4 * t + r)) : 0u;", 1)],
    "b3_kk_plus_one": [("const int kk = (tgt - 63 + CC_KNN_TSTRIDE - 1) / CC_KNN_TSTRIDE;", "const int kk = (tgt - 63 + CC_KNN_TSTRIDE - 1) / CC_KNN_TSTRIDE + 1;", 1)],
    "b3_down_jump_too_far": [("(s1 > L0 ? (s1 > E1 ? s1 - E1 : 0) : 0x7fffffff)", "(s1 > L0 ? (s1 > E1 ? s1 - E1 + 128 : 0) : 0x7fffffff)", 1)],
    # B4: queues and cut-backs (the crowds of the cases stay below CC_KNN_TTRIG, so the buffer bound holds without the branch)
    "b4_no_kept_branch": [("  if (kept > 64) {  // a crowd", "  if (false) {  // a crowd", 1)],
    "b4_select_keep_lt": [("const bool keep = d[a] <= hi;", "const bool keep = d[a] < hi;", 1)],
    "b4_final_cut_256": [("    if (cnt > 128) {  // what is within", "    if (cnt > 256) {  // what is within", 1)],
    "b4_left_over_dropped": [("      m_left = m;\n      sb_left = sb_cur;\n", "      m_left = 0u;\n      sb_left = sb_cur;\n", 1)],
    # C: the sorting networks of the large-k walk
    "c_width_128": [("  if (cnt <= 128)\n    f(std::integral_constant<int, 2>());", "  if (cnt <= 192)\n    f(std::integral_constant<int, 2>());", 1)],
    "c_width_256": [("  else if (cnt <= 256)\n    f(std::integral_constant<int, 4>());", "  else if (cnt <= 320)\n    f(std::integral_constant<int, 4>());", 1)],
    # D: the sorted view
    "d_old_before_new_reversed": [("      if (s_old0[mid] <= c)\n", "      if (s_old0[mid] < c)\n", 1), ("    if (s_old0[mid] <= c)\n", "    if (s_old0[mid] < c)\n", 1),
                                  ("      if (new_sorted0[mid] < c)\n", "      if (new_sorted0[mid] <= c)\n", 1)],
    "d_zero_fold_removed": [("const float c = keys[n_old + i] + 0.f;  // -0 -> +0", "const float c = keys[n_old + i];", 1)],
    "d_bulk_arrival_order": [("(ci == c && t0 + i < j)", "(ci == c && t0 + i > j)", 1)],
    # (both paths rank the new keys the same way: at m = 4 096 the counting kernel gives what the LDS sort gives -- EQUIVALENT by construction)
    "d_lds_threshold_ge": [("if (m <= 0 || m > CC_KSORT_LDS) return;", "if (m <= 0 || m >= CC_KSORT_LDS) return;", 1),
                           ("any_bulk = any_bulk || nn > CC_KSORT_LDS;", "any_bulk = any_bulk || nn >= CC_KSORT_LDS;", 1, "cc_db_api.inc"),
                           ("      if (SP.m[l] > CC_KSORT_LDS)\n", "      if (SP.m[l] >= CC_KSORT_LDS)\n", 1, "cc_db_api.inc")],
    "d_norm_row": [("      nrm += v * v;\n", "      nrm += v * v * 1.000002f;\n", 1)],
    "d_sact_of_moved_key": [("P.sact_new[l][dst] = P.act[l][P.sid_old[l][i]];", "P.sact_new[l][dst] = P.act[l][i];", 1)],
    "d_sact_refresh": [("P.sact_new[l][i] = P.act[l][P.sid_old[l][i]];", "P.sact_new[l][i] = P.act[l][i];", 1)],
    "c_width_512": [("  else if (cnt <= 512)\n    f(std::integral_constant<int, 8>());", "  else if (cnt <= 576)\n    f(std::integral_constant<int, 8>());", 1)],
}
RUN = """
import sys
sys.path[:0] = [%(root)r, %(root)r + "/oracle", %(root)r + "/tests"]
import emu_api
emu_api.build = lambda *a, **k: %(so)r
emu_api.SO = %(so)r
import pytest
sys.exit(pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu", "--tb=line", %(root)r + "/tests/test_emu_knn.py"]))
"""


def one(name, tmp):
    d = os.path.join(tmp, name)
    shutil.copytree(os.path.join(ROOT, "contour-context_amd", "csrc"), os.path.join(d, "contour-context_amd", "csrc"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
    os.makedirs(os.path.join(d, "tests"))
    for sub in ("emu", "devprobe"):
        shutil.copytree(os.path.join(ROOT, "tests", sub), os.path.join(d, "tests", sub), ignore=shutil.ignore_patterns("*.so", "__pycache__"))
    for e in EDITS[name]:
        old, new, n = e[:3]
        p = os.path.join(d, "contour-context_amd", "csrc", e[3] if len(e) > 3 else KNN)
        s = open(p).read()
        assert s.count(old) == n, (name, old, s.count(old))
        open(p, "w").write(s.replace(old, new))
    old, new = EDITS[name][0][:2]
    so = os.path.join(d, "tests", "emu", "libcc_emu.so")
    subprocess.check_call(["sh", os.path.join(d, "tests", "emu", "build.sh")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        r = subprocess.run([sys.executable, "-c", RUN % {"root": ROOT, "so": so}], capture_output=True, text=True, cwd=d, timeout=600)
        out, rc = r.stdout, r.returncode
    except subprocess.TimeoutExpired as e:
        out, rc = (e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""), None
    failed = re.findall(r"^FAILED \S+::(?:test_cases\[(.+?)\]|(test_views))", out, flags=re.M)
    failed = [a or b for a, b in failed]
    cases = sorted(set(re.findall(r"AssertionError: ((?:dev against R1, |D ).*?): ", out)))
    open(os.path.join(tmp, name + ".log"), "w").write(out)
    last = out.strip().splitlines()[-1] if out.strip() else "(no output)"
    if rc is None:
        last = "the harness process did not end within 600 s"
    elif rc < 0:
        last = "the harness process ended on signal %d" % -rc
    return "%-26s %s -> %s\n%-26s   %s\n%-26s   parts: %s\n%s" % (
        name, old.splitlines()[0].strip()[:70], new.splitlines()[0].strip()[:70] if new.strip() else "(removed)", "", last, "",
        " ".join(p.strip() for p in failed) if failed else "nothing fails", "\n".join("%-26s   %s" % ("", c) for c in cases) or "%-26s   -" % "")


if __name__ == "__main__":
    names = sys.argv[1:] or list(EDITS)
    tmp = tempfile.mkdtemp(prefix="k3_mutants_")
    print("logs in", tmp)
    with ThreadPoolExecutor(4) as ex:
        for line in ex.map(lambda n: one(n, tmp), names):
            print(line, flush=True)
