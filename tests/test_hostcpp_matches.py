"""The class mirror's match rows (hostcpp/cont2/contour_db.h: ContourDB::setWantMatches / lastMatches) in the reference driver's
loop on the 64-scan drive -- tests/match_mirror_check.cpp on the CPU harness: with setWantMatches(2.0) and setMaxReturn(5),
lastMatches() holds the C-ABI's cc_ranked_match_t rows byte for byte, one per returned candidate, through queryRangedKNN with the
database's read-ahead off (against C-ABI calls of the same chunk composition: one query each) and on (the same bytes again), and
through verifyCandidates; cc_match_pairs lists a row's pairs; switched off, nothing is collected."""
import os
import subprocess

import numpy as np

import emu_api
import match_cases as M
import ranked_common as RC
from test_emu_matches import drive_back
from test_mirror_read_ahead import _build, _lists

PX = 2.0
_out = {}


def _parse(stdout, itemsize):
    out = {}
    for l in stdout.splitlines():
        t = l.split()
        if not t or t[0] not in ("q", "v", "o"):
            continue
        nc, nd = int(t[2]), int(t[3])
        assert len(t) == 4 + nc + nd and all(len(x) == 2 * itemsize for x in t[4 + nc:]), l
        out.setdefault(t[0], {})[int(t[1])] = ([int(x) for x in t[4:4 + nc]], [bytes.fromhex(x) for x in t[4 + nc:]])
    return out


def _run(cc, tmp_path, read_ahead):
    if read_ahead not in _out:
        if "exe" not in _out:
            _out["exe"] = _build(tmp_path, "match_mirror_check.cpp", "match_mirror_check", gpu=False)
            _out["lists"] = _lists(cc, tmp_path, 64, 16, 450, 1.0)
        lst, pos = _out["lists"]
        env = dict(os.environ, CC_EVAL_TIMERS="1", **emu_api.SMALL_GRIDS)
        if not read_ahead:
            env.update(CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1")
        r = subprocess.run([_out["exe"], str(pos), str(lst), "5", repr(PX)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "done 64" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
        _out[read_ahead] = (r.stdout, r.stderr)
    return _out[read_ahead]


def test_last_matches_are_the_c_abi_rows(cc, oracle, tmp_path):
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    B = drive_back(cc, oracle)
    size = L.ranked_match_dt.itemsize
    txt, _ = _run(cc, tmp_path, read_ahead=False)
    direct = _parse(txt, size)
    n_rows = 0
    for q in range(64):
        ids, rows = direct["q"][q]
        r = M.run_query(B, desc[q:q + 1], seeds[q:q + 1], ranked=5, matches=PX)   # one query per call, as the mirror asks
        k = int(r.rank[1][0])
        assert len(ids) == len(rows) == k, (q, len(ids), len(rows), k)
        assert ids == r.rank[0][0]["cand_gidx"][:k].tolist(), q
        for j in range(k):
            assert rows[j] == r.match[0][j].tobytes(), (q, j, np.frombuffer(rows[j], L.ranked_match_dt), r.match[0][j])
            n_rows += 1
    assert n_rows >= 60 and sum(len(x[1]) >= 2 for x in direct["q"].values()) >= 20
    # the pair list of the first row handed out
    line = [l.split() for l in txt.splitlines() if l.startswith("p ")]
    assert len(line) == 1
    q0 = int(line[0][1])
    first = np.frombuffer(direct["q"][q0][1][0], L.ranked_match_dt)[0]
    assert int(line[0][2]) == first["n_pairs"] == len(line[0]) - 3
    assert [[int(v) for v in t.split(":")] for t in line[0][3:]] == L.match_pairs(first).tolist()
    # verifyCandidates over four candidates: the C-ABI's verify rows (the mirror's bound on the key distance and its max_fine_opt)
    for q in (38, 39, 40):
        v = M.calls.verify(B.lib, B.db, [[0, 1, 2, 3]], qdesc=B.dev(np.ascontiguousarray(desc[q:q + 1])), n_desc=1, levels=None,
                           max_fine_opt=int(dcfg.max_fine_opt), max_key_dist_sq=1000.0, ranked=5, matches=PX)
        ids, rows = direct["v"][q]
        k = int(v.rank[1][0])
        assert ids == v.rank[0][0]["cand_gidx"][:k].tolist() and len(rows) == k >= 2, (q, ids, k)
        assert rows == [v.match[0][j].tobytes() for j in range(k)], q
    # switched off: the same candidates, no rows
    assert direct["o"][40][0] == direct["q"][40][0] and direct["o"][40][1] == []
    # the read-ahead (answers queued through the matched scan-batch call; the block travels with the ranked block): the same rows
    ahead_txt, err = _run(cc, tmp_path, read_ahead=True)
    ahead = _parse(ahead_txt, size)
    for kind in ("q", "v", "o"):
        assert ahead[kind].keys() == direct[kind].keys()
        for q, (ids, rows) in direct[kind].items():
            assert ahead[kind][q] == (ids, rows), (kind, q)
    ra = [l for l in err.splitlines() if l.startswith("[ContourDB read-ahead]")]
    assert ra and int(ra[-1].split("queued queries")[1].split(",")[0]) > 0, ra


def test_pair_demo_prints_the_winning_candidates_pairs(cc, oracle, tmp_path):
    """hostcpp/examples/pair_demo.cpp on the harness: its M and P lines are the match oracle's record of the hints it printed"""
    from test_hostcpp_pair_flow import PKG, _pair
    import match_oracle as MO
    emu_so = emu_api.build()
    exe = str(tmp_path / "pair_demo_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(PKG, "hostcpp", "examples", "pair_demo.cpp"),
                           "-I", os.path.join(PKG, "hostcpp"), "-L", os.path.dirname(emu_so), "-lcc_emu",
                           "-Wl,-rpath," + os.path.dirname(emu_so), "-pthread", "-o", exe])
    xs, odesc, qi, c, dcfg = _pair(cc, oracle)
    old, new = tmp_path / "old.bin", tmp_path / "new.bin"
    xs[c].astype(np.float32).tofile(old)
    xs[qi].astype(np.float32).tofile(new)
    out = subprocess.check_output([exe, str(old), str(new), "5"], text=True, env=dict(os.environ, **emu_api.SMALL_GRIDS))
    hints = np.array([[0] + [int(v) for v in l.split()[1:4]] for l in out.split("\n") if l.startswith("H ")], np.int32)
    ml = [l.split()[1:] for l in out.split("\n") if l.startswith("M ")]
    pl = [[int(v) for v in l.split()[1:]] for l in out.split("\n") if l.startswith("P ")]
    assert len(ml) == 1 and len(hints) > 0
    ref, keys = MO.check_hints_matches(MO.Scan(odesc[qi], 1), [MO.Scan(odesc[c], 0)], hints, sim=dcfg.cont_sim)
    assert len(ref) == 1 and ref["survived"][0] == 1
    m = ml[0]
    assert [int(m[0]), int(m[1]), int(m[2])] == [int(ref["n_pairs"][0]), int(ref["vote_cnt"][0]), int(ref["n_props"][0])], (m, ref)
    assert np.float32(float(m[3])) == ref["area_perc"][0]   # (%.9g round-trips an f32)
    assert pl == keys[0].tolist() and len(pl) == int(m[0]) >= 3
    assert 0.0 <= float(m[4]) <= float(m[5]) and 0 <= int(m[6]) <= int(m[0])
