"""The class mirror's ranked answers (hostcpp/cont2/contour_db.h: ContourDB::setMaxReturn, the verifyCandidates overload,
CandidateManager::fineOptimize's max_ret) in the reference driver's loop on the 64-scan drive -- tests/ranked_mirror_check.cpp on
the CPU harness: with setMaxReturn(5) the vectors hold the lists the C-ABI gives (test_emu_ranked.py, part A), over the direct
path and over the database's read-ahead; without it the driver gets what it always got: the unchanged offline driver
(hostcpp/examples/batch_bin_test.cpp) writes, byte for byte, the outcome file it wrote before the mirror knew ranked answers
(tests/golden/outcome-short-loop-drive-harness.txt, recorded from that commit by tests/golden/make_driver_outcome_golden.py)."""
import os
import subprocess

import numpy as np

import emu_api
import ranked_common as RC
from test_emu_ranked import ranked_setup
from test_mirror_read_ahead import _build, _lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "outcome-short-loop-drive-harness.txt")
_out = {}


def driver_outcome(cc, work, root, read_ahead):
    """The offline driver of the checkout at `root` (hostcpp/examples/batch_bin_test.cpp against that checkout's class mirror and
    its CPU harness build) on the 64-scan drive, 0.4 s per scan, DB delays 10 / 6 s -> the bytes of its outcome file."""
    pkg = os.path.join(root, "contour-context_amd")
    emu_dir = os.path.join(root, "tests", "emu")
    if root == ROOT:
        emu_api.build()
    assert os.path.exists(os.path.join(emu_dir, "libcc_emu.so")), "build the harness of %s first (sh tests/emu/build.sh)" % root
    exe = str(work / "batch_bin_test_emu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(pkg, "hostcpp", "examples", "batch_bin_test.cpp"),
                               "-I", os.path.join(pkg, "hostcpp"), "-I", os.path.join(root, "include"), "-L", emu_dir, "-lcc_emu",
                               "-Wl,-rpath," + emu_dir, "-o", exe])
    if not os.path.exists(work / "scans.txt"):  # (the outcome file repeats the scans' paths: relative ones, and the driver runs in `work`)
        lst, pos = _lists(cc, work, 64, 16, 450, 4.0)
        lst.write_text(lst.read_text().replace(str(work) + os.sep, ""))
    out = work / "outcome.txt"
    cfg = open(os.path.join(pkg, "hostcpp", "examples", "batch_bin_test_config.yaml")).read()
    cfg = cfg.replace("/path/to/ts-sens_pose-kitti08.txt", str(work / "poses.txt")).replace("/path/to/ts-lidar_bins-kitti08.txt", str(work / "scans.txt"))
    cfg = cfg.replace("/path/to/outcome-kitti08.txt", str(out))
    cfg = cfg.replace("max_elapse_: 25.0", "max_elapse_: 10.0").replace("min_elapse_: 15.0", "min_elapse_: 6.0")
    (work / "cfg.yaml").write_text(cfg)
    env = dict(os.environ, **emu_api.SMALL_GRIDS)
    if not read_ahead:
        env.update(CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1")
    if out.exists():
        out.unlink()
    r = subprocess.run([exe, str(work / "cfg.yaml")], env=env, cwd=str(work), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    return open(out, "rb").read()


def _parse(stdout):
    out = {}
    for l in stdout.splitlines():
        t = l.split()
        if not t or t[0] not in ("q", "v", "f"):
            continue
        n = int(t[2])
        v = [float(x) for x in t[3:]]
        assert len(v) == 5 * n, l
        out.setdefault(t[0], {})[int(t[1])] = [(int(v[5 * k]), v[5 * k + 1], np.array(v[5 * k + 2:5 * k + 5])) for k in range(n)]
    return out


def _run(cc, tmp_path, max_ret, read_ahead):
    key = (max_ret, read_ahead)
    if key not in _out:
        if "exe" not in _out:
            _out["exe"] = _build(tmp_path, "ranked_mirror_check.cpp", "ranked_mirror_check", gpu=False)
            _out["lists"] = _lists(cc, tmp_path, 64, 16, 450, 1.0)
        lst, pos = _out["lists"]
        env = dict(os.environ, CC_EVAL_TIMERS="1", **emu_api.SMALL_GRIDS)
        if not read_ahead:
            env.update(CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1")
        r = subprocess.run([_out["exe"], str(pos), str(lst), str(max_ret)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "done 64" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
        _out[key] = (_parse(r.stdout), r.stdout, r.stderr)
    return _out[key]


def _same_entry(g, corr, tf, rec, what):
    """scan, correlation and translation bit for bit (the program prints %.17g); the angle went through Isometry2d -- rotate(theta),
    then atan2(T10, T00) -- so it may be a few ulp off"""
    assert g == rec["cand_gidx"] and corr == rec["correlation"] and tf[0] == rec["tf"][0] and tf[1] == rec["tf"][1], (what, g, corr, tf, rec)
    assert abs(tf[2] - rec["tf"][2]) <= 4 * np.spacing(max(abs(rec["tf"][2]), 1.0)), (what, tf[2], rec["tf"][2])


def _same(got, row, n, what):
    assert len(got) == n, (what, len(got), n)
    for k, (g, corr, tf) in enumerate(got):
        _same_entry(g, corr, tf, row[k], (what, k))


def test_set_max_return_gives_the_lists(cc, oracle, tmp_path):
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    v, plain, knn, cnt, (res, cands, n) = ranked_setup(cc, oracle)
    direct, direct_txt, _ = _run(cc, tmp_path, 5, read_ahead=False)
    for q in range(64):
        _same(direct["q"][q], cands[q], min(int(n[q]), 5), ("query", q))
    assert sum(len(x) >= 2 for x in direct["q"].values()) >= 20
    # verifyCandidates' list and fineOptimize's over the same candidates: the C-ABI's verify lists, and each other's bytes
    qs = [38, 39, 40]
    vres, vc, vn, _ = v.verify(desc[qs], [[0, 1, 2, 3]] * 3, 5, mfo=dcfg.max_fine_opt)
    for i, q in enumerate(qs):
        _same(direct["v"][q], vc[i], int(vn[i]), ("verify", q))
        assert len(direct["v"][q]) >= 2
    assert [l for l in direct_txt.splitlines() if l.startswith("f ")] == [("f" + l[1:]) for l in direct_txt.splitlines() if l.startswith("v ")]
    # the read-ahead path (answers queued through the ranked scan-batch call) hands out the same lines
    ahead, ahead_txt, err = _run(cc, tmp_path, 5, read_ahead=True)
    assert ahead_txt == direct_txt
    ra = [l for l in err.splitlines() if l.startswith("[ContourDB read-ahead]")]
    assert ra and int(ra[-1].split("queued queries")[1].split(",")[0]) > 0, ra


def test_default_is_the_single_answer(cc, oracle, tmp_path):
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    v, plain, knn, cnt, _ = ranked_setup(cc, oracle)
    for read_ahead in (False, True):
        got, txt, _ = _run(cc, tmp_path, 0, read_ahead)
        for q in range(64):
            r = plain[q]
            assert len(got["q"][q]) == int(r["n_res"]) <= 1, q
            if r["n_res"]:
                _same_entry(*got["q"][q][0], r, ("default", q))
        assert all(len(x) <= 1 for x in got["v"].values()) and all(len(x) <= 1 for x in got["f"].values())


def test_unchanged_driver_writes_the_outcome_file_it_wrote_before(cc, tmp_path):
    gold = open(GOLD, "rb").read()
    rows = [l.split(b"\t") for l in gold.splitlines()]
    assert len(rows) == 64 and sum(not r[1].endswith(b"-x") for r in rows) >= 5, "the recorded drive should close loops"
    for read_ahead in (False, True):
        assert driver_outcome(cc, tmp_path, ROOT, read_ahead) == gold, "outcome file differs (read-ahead %s)" % read_ahead
