"""The class mirror's ContourDB::scorePoses (hostcpp/cont2/contour_db.h) in the reference driver's loop on the 64-scan drive --
tests/pose_mirror_check.cpp on the CPU harness: its rows are the C-ABI's (cc_db_pose_batch_host with the same items in the same
chunk composition: one call per scorePoses call, one descriptor) bit for bit, T_best's angle within a few ulp (it passes through
an Isometry2d); a query with fewer try poses than the call's longest list gets its own count back; and with default-constructed
drivers nothing changes: the unchanged offline driver writes the outcome file it always wrote."""
import os
import subprocess

import numpy as np

import emu_api
import pose_common as PC
import ranked_common as RC
from test_emu_ranked_detail import setup
from test_hostcpp_ranked import GOLD, ROOT, driver_outcome
from test_mirror_read_ahead import _build, _lists


def _rows(stdout):
    out = {}
    for l in stdout.splitlines():
        t = l.split()
        if not t or t[0] != "p":
            continue
        seq, mode, k, cand = (int(x) for x in t[1:5])
        f = [float.fromhex(x) for x in t[5:8]]
        nt = int(t[8])
        p = 9
        tries = [[float.fromhex(x) for x in t[p + 3 * j:p + 3 * j + 3]] for j in range(nt)]
        p += 3 * nt
        vals = [float.fromhex(x) for x in t[p:p + 5]]
        ints = [int(x) for x in t[p + 5:p + 9]]
        rest = [float.fromhex(x) for x in t[p + 9:]]
        assert len(rest) == nt + 9, l
        out.setdefault((seq, mode), []).append(dict(k=k, cand=cand, tf=f, tries=tries, vals=vals, ints=ints, tc=rest[:nt], hess=rest[nt:nt + 6], grad=rest[nt + 6:]))
    return out


def test_score_poses_rows_are_the_c_abi_rows(cc, oracle, tmp_path):
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v = setup(cc, oracle)[0]
    lib = v.lib
    exe = _build(tmp_path, "pose_mirror_check.cpp", "pose_mirror_check", gpu=False)
    lst, pos = _lists(cc, tmp_path, 64, 16, 450, 1.0)
    env = dict(os.environ, CC_EVAL_TIMERS="1", CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1", **emu_api.SMALL_GRIDS)
    r = subprocess.run([exe, str(pos), str(lst)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "done 64" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    groups = _rows(r.stdout)
    assert len(groups) >= 4 and sum(len(g) for g in groups.values()) >= 8, sorted(groups)
    n_rows = 0
    for (seq, mode), g in sorted(groups.items()):
        n = len(g)
        nt = max(len(x["tries"]) for x in g)
        assert [x["k"] for x in g] == list(range(n)) and len(g[0]["tries"]) == 0 and (n == 1 or nt == 2)
        items = L.pose_items([0] * n, [x["cand"] for x in g], [x["tf"] for x in g])
        tries = np.array([[(x["tries"][t] if t < len(x["tries"]) else x["tf"]) for t in range(nt)] for x in g], np.float64).reshape(n, nt, 3)
        cfg = L.PoseCfg(mode, PC.NINF if mode else np.float32(0.3), nt, 0)
        res = np.zeros(n, L.pose_result_dt)
        tc = np.zeros((n, nt))
        cv = np.zeros(n, L.pose_curv_dt)
        qd = np.ascontiguousarray(desc[seq:seq + 1])
        rc = lib.cc_db_pose_batch_host(v.db, v.p(qd), 1, v.p(items), n, v.b(cfg), v.p(tries) if nt else None, v.p(res), v.p(tc) if nt else None, v.p(cv))
        v.api.chk(rc, "cc_db_pose_batch_host")
        for i, x in enumerate(g):
            what = (seq, mode, i, x["cand"])
            assert x["vals"][:4] == [res[i]["corr_init"], res[i]["correlation"], res[i]["tf"][0], res[i]["tf"][1]], (what, x["vals"], res[i])
            assert abs(x["vals"][4] - res[i]["tf"][2]) <= 4 * np.spacing(abs(res[i]["tf"][2])), (what, x["vals"][4], res[i]["tf"][2])
            assert x["ints"] == [int(res[i][f]) for f in ("n_pairs", "iterations", "termination", "flags")], (what, x["ints"], res[i])
            assert x["tc"] == tc[i, :len(x["tries"])].tolist(), (what, x["tc"], tc[i])
            assert x["hess"] == cv[i]["hess"].tolist() and x["grad"] == cv[i]["grad"].tolist(), what
            assert bool(res[i]["flags"] & L.PF_REFINED) == (mode == 1 and res[i]["n_pairs"] > 0), what
            if x["tries"]:   # the first try pose of a query is its T_init
                assert abs(x["tc"][0] - res[i]["corr_init"]) < PC.INIT_BAR, what
            n_rows += 1
    assert n_rows >= 8


def test_default_drivers_unchanged_offline_driver_writes_the_recorded_outcome(cc, tmp_path):
    gold = open(GOLD, "rb").read()
    for read_ahead in (False, True):
        assert driver_outcome(cc, tmp_path, ROOT, read_ahead) == gold, "outcome file differs (read-ahead %s)" % read_ahead
