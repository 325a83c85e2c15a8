"""The class mirror's ContourDB::queryAmong (hostcpp/cont2/contour_db.h) in the reference driver's loop on the 64-scan drive --
tests/listed_mirror_check.cpp on the CPU harness: with a restricted list it returns the filtered oracle's scan and pose for queries
37 and 57 and, to the bit, what queryAllowed returns for the same list (ranked entries, detail rows and match rows included); with
an all-scans list what queryRangedKNN returns."""
import os
import subprocess

import numpy as np

import emu_api
import masked_cases as M
from test_hostcpp_masked import _rows
from test_mirror_read_ahead import _build, _lists


def test_query_among_on_the_loop_drive(cc, oracle, tmp_path):
    ref = M.loop_reference(cc, oracle, 50)
    exe = _build(tmp_path, "listed_mirror_check.cpp", "listed_mirror_check", gpu=False)
    lst, pos = _lists(cc, tmp_path, 64, 16, 450, 1.0)
    env = dict(os.environ, CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1", **emu_api.SMALL_GRIDS)
    r = subprocess.run([exe, str(pos), str(lst)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "done 64" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])  # (3..5: the rows of queryAllowed differ)
    rows = _rows(r.stdout)
    for seq, kind, want in ((37, "not_best", 17), (57, "high", 32)):
        u, a, m, w, rk, rs = (rows[(seq, k)] for k in "uamwrs")
        assert len(u) == 1 and a == u, (seq, u, a)  # every scan listed: queryRangedKNN's answer, to the bit
        o = ref["ores"][M._pick(ref, seq, kind)]
        assert o["n_res"] == 1 and o["cand_gidx"] == want
        assert len(m) == 1 and m[0][0] == want, (seq, m)
        assert abs(m[0][1] - o["correlation"]) < 1e-6 and np.abs(np.array(m[0][2:]) - o["tf"]).max() < 1e-6, (seq, m, o)
        assert m == w and rk == rs, (seq, m, w, rk, rs)  # queryAllowed's answers, to the bit
        assert rk[0] == m[0] and 1 <= len(rk) <= 4
        allowed = [g for g in range(seq) if (g != u[0][0] if seq == 37 else g >= 32)]
        assert all(e[0] in allowed for e in rk), (seq, rk)
