"""The class mirror's detail rows (hostcpp/cont2/contour_db.h: ContourDB::setWantDetail / lastDetails, the same pair on
CandidateManager) in the reference driver's loop on the 64-scan drive -- tests/ranked_detail_mirror_check.cpp on the CPU
harness: with setWantDetail(true) and setMaxReturn(5), lastDetails() holds the C-ABI's cc_ranked_detail_t rows byte for byte
(test_emu_ranked_detail.py, part b), one per returned candidate, over the direct path (against C-ABI calls of the same chunk
composition: one query each) and over the database's read-ahead (every field byte for byte but corr_init: the initial
correlation's last bits depend on how many problems share a chunk, as every correlation of the library's does); with the default
(off) the unchanged offline driver writes the outcome file it always wrote."""
import os
import subprocess

import numpy as np

import emu_api
import ranked_common as RC
from test_emu_ranked_detail import setup
from test_hostcpp_ranked import GOLD, ROOT, driver_outcome
from test_mirror_read_ahead import _build, _lists

_out = {}


def _parse(stdout, itemsize):
    out = {}
    for l in stdout.splitlines():
        t = l.split()
        if not t or t[0] not in ("q", "v", "f"):
            continue
        nc, nd = int(t[2]), int(t[3])
        assert len(t) == 4 + nc + nd and all(len(x) == 2 * itemsize for x in t[4 + nc:]), l
        out.setdefault(t[0], {})[int(t[1])] = ([int(x) for x in t[4:4 + nc]], [bytes.fromhex(x) for x in t[4 + nc:]])
    return out


def _run(cc, tmp_path, read_ahead):
    if read_ahead not in _out:
        if "exe" not in _out:
            _out["exe"] = _build(tmp_path, "ranked_detail_mirror_check.cpp", "ranked_detail_mirror_check", gpu=False)
            _out["lists"] = _lists(cc, tmp_path, 64, 16, 450, 1.0)
        lst, pos = _out["lists"]
        env = dict(os.environ, CC_EVAL_TIMERS="1", **emu_api.SMALL_GRIDS)
        if not read_ahead:
            env.update(CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1")
        r = subprocess.run([_out["exe"], str(pos), str(lst), "5"], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "done 64" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
        _out[read_ahead] = (r.stdout, r.stderr)
    return _out[read_ahead]


def test_last_details_are_the_c_abi_rows(cc, oracle, tmp_path):
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, _, (res, c, n, det) = setup(cc, oracle)
    size = L.ranked_detail_dt.itemsize
    txt, _ = _run(cc, tmp_path, read_ahead=False)
    direct = _parse(txt, size)
    # The mirror asks one query at a time; so does the C-ABI call it is compared with.  (cc_k_gmm_init sums a problem's terms over
    # 16 or 64 lanes depending on how many problems its chunk holds, so corr_init -- like every correlation of the library -- is
    # reproducible bit for bit for the same chunk, and to the last ulp or two across chunk compositions; every other field of the
    # row does not depend on the chunk and is compared with the 64-query batch's rows as well.)
    for q in range(64):
        ids, rows = direct["q"][q]
        k = min(int(n[q]), 5)
        assert len(ids) == len(rows) == k, (q, len(ids), len(rows), k)
        assert ids == c[q]["cand_gidx"][:k].tolist(), q
        if k:
            _, c1, n1, d1 = v.query_d(desc[q:q + 1], seeds[q:q + 1], 5)
            assert n1[0] == k
        for j in range(k):
            assert rows[j] == d1[0][j].tobytes(), (q, j, np.frombuffer(rows[j], L.ranked_detail_dt), d1[0][j])
            got = np.frombuffer(rows[j], L.ranked_detail_dt)[0]
            for f in L.ranked_detail_dt.names:
                if f != "corr_init":
                    assert got[f].tobytes() == det[q][j][f].tobytes(), (q, j, f)
            assert abs(got["corr_init"] - det[q][j]["corr_init"]) <= 4 * np.spacing(1.0), (q, j)
    assert sum(len(x[1]) >= 2 for x in direct["q"].values()) >= 20
    # verifyCandidates and fineOptimize over the same candidates: the C-ABI's verify rows, and each other's bytes
    qs = [38, 39, 40]
    for q in qs:
        vres, vc, vn, vd = v.verify_d(desc[q:q + 1], [[0, 1, 2, 3]], 5, mfo=dcfg.max_fine_opt)  # (one item per call, as the mirror asks)
        i = 0
        ids, rows = direct["v"][q]
        assert ids == vc[i]["cand_gidx"][:vn[i]].tolist() and len(rows) == int(vn[i]) >= 2, (q, ids, vn[i])
        assert rows == [vd[i][j].tobytes() for j in range(int(vn[i]))], q
        assert direct["f"][q] == direct["v"][q], q
    # the read-ahead path (answers queued through the detail scan-batch call; the block travels with the ranked block)
    # hands out the same candidates and the same rows: every field byte for byte but corr_init, which the read-ahead's chunks
    # (several scans each) sum in another grouping than a chunk of one query -- within 4 ulp of 1
    ahead_txt, err = _run(cc, tmp_path, read_ahead=True)
    ahead = _parse(ahead_txt, size)
    n_rows = 0
    for kind in ("q", "v", "f"):
        assert ahead[kind].keys() == direct[kind].keys()
        for q, (ids, rows) in direct[kind].items():
            ids2, rows2 = ahead[kind][q]
            assert ids2 == ids and len(rows2) == len(rows), (kind, q)
            for r1, r2 in zip(rows, rows2):
                g1, g2 = np.frombuffer(r1, L.ranked_detail_dt)[0], np.frombuffer(r2, L.ranked_detail_dt)[0]
                for f in L.ranked_detail_dt.names:
                    if f != "corr_init":
                        assert g1[f].tobytes() == g2[f].tobytes(), (kind, q, f)
                assert abs(g1["corr_init"] - g2["corr_init"]) <= 4 * np.spacing(1.0), (kind, q)
                n_rows += 1
    assert n_rows >= 100
    ra = [l for l in err.splitlines() if l.startswith("[ContourDB read-ahead]")]
    assert ra and int(ra[-1].split("queued queries")[1].split(",")[0]) > 0, ra


def test_default_off_unchanged_driver_writes_the_recorded_outcome(cc, tmp_path):
    gold = open(GOLD, "rb").read()
    for read_ahead in (False, True):
        assert driver_outcome(cc, tmp_path, ROOT, read_ahead) == gold, "outcome file differs (read-ahead %s)" % read_ahead
