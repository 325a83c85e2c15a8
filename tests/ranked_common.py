"""TEST INFRASTRUCTURE shared by test_emu_ranked.py / test_gpu_ranked.py / test_hostcpp_ranked.py: the 64-scan looping drive,
the reference list of a query obtained by PEELING the oracle (which returns one candidate per call), and the structural
properties every ranked list has.

Peeling: the query's kNN hits, in [layer][anchor][k] order, are a hint list (gidx, level, hit.seq, anchor); the oracle's hint
flow on it returns the best candidate; every hint of that candidate is dropped and the flow runs again, until nothing is
returned.  Under static thresholds the checks of different candidates do not see each other and a candidate's refined
correlation does not depend on the others, so while n_cand_tidy <= max_fine_opt (every survivor is refined) the k-th run's
winner is entry k of the list.  Queries with more survivors than that are not peeled (fineOptimize refines a prefix that changes
when a candidate leaves), and neither are queries whose neighbouring oracle correlations lie within TIE_GAP of each other."""
import numpy as np

from test_dyn_thres_oracle import short_loop_drive

K = 16           # CC_RANK_MAX
TIE_GAP = 1e-5   # oracle correlations of neighbouring entries closer than this: the order is not the test's to decide
TOL = 1e-6       # correlation and pose against the oracle: the tolerance of the hint and verify tests
_cache = {}


def drive(cc, oracle):
    if "drive" not in _cache:
        _cache["drive"] = short_loop_drive(cc, oracle)
    return _cache["drive"]


def hints_of_knn(L, knn_q, cnt_q, n_levels=3):
    """the hits of one query [NQLEV][NPIV][stride] / [NQLEV][NPIV] -> int array [n][4] of (gidx, level, seq_src, seq_tgt)"""
    out = []
    for l in range(n_levels):
        for a in range(L.NPIV):
            for k in range(int(cnt_q[l, a])):
                h = knn_q[l, a, k]
                out.append((int(h["gidx"]), int(h["level"]) & 0xFF, int(h["seq"]), a))
    return np.array(out, np.int32).reshape(-1, 4)


def to_hint_dt(L, hints):
    h = np.zeros(len(hints), L.hint_dt)
    if len(hints):
        h["cand_gidx"], h["level"], h["seq_src"], h["seq_tgt"] = hints[:, 0], hints[:, 1], hints[:, 2], hints[:, 3]
    return h


def peel(oracle, desc, dcfg, q, hints, max_fine_opt):
    """-> (list of (gidx, correlation, tf) in peeling order, the first run's record).  hints: [n][4] with DB indices."""
    hints = np.asarray(hints, np.int32).reshape(-1, 4)
    tgt = oracle.Scan.from_desc(desc[q], int_id=int(q))
    out, first = [], None
    while len(hints):
        gs = sorted(set(int(g) for g in hints[:, 0]))
        loc = {g: i for i, g in enumerate(gs)}
        scans = [oracle.Scan.from_desc(desc[g], int_id=int(g)) for g in gs]
        h = hints.copy()
        h[:, 0] = [loc[int(g)] for g in hints[:, 0]]
        r, _ = oracle.check_hints(tgt, scans, h, sim=dcfg.cont_sim, max_fine_opt=max_fine_opt)
        if first is None:
            first = r.copy()
        if r["n_res"] == 0:
            break
        g = gs[int(r["cand_gidx"])]
        out.append((g, float(r["correlation"]), np.array(r["tf"], np.float64)))
        hints = hints[hints[:, 0] != g]
    if first is None:
        first = np.zeros(1, oracle.L.query_result_dt)[0]
    return out, first


def peel_query(cc, oracle, q, knn, cnt, max_fine_opt=None, key=None):
    """the peeled list of drive query q (its hits knn[q], cnt[q]), or None where peeling is not valid for it; cached"""
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    mfo = int(dcfg.max_fine_opt if max_fine_opt is None else max_fine_opt)
    ck = ("peel", key, int(q), mfo)
    if ck not in _cache:
        hints = hints_of_knn(oracle.L, knn, cnt)
        lst, first = peel(oracle, desc, dcfg, q, hints, mfo)
        ok = len(lst) > 0 and int(first["n_cand_tidy"]) <= mfo and len(lst) == int(first["n_cand_tidy"])
        ok = ok and all(lst[i][1] - lst[i + 1][1] > TIE_GAP for i in range(len(lst) - 1))
        _cache[ck] = (lst if ok else None, hints)
    return _cache[ck]


def check_structure(L, res, cands, cnt, max_ret, max_fine_opt):
    """what holds for every ranked answer, whatever the thresholds: counts, entry 0, order, distinct scans, zeroed rest"""
    n = len(res)
    assert cands.shape == (n, max_ret) and cnt.shape == (n,)
    zero = np.zeros(1, L.ranked_cand_dt).tobytes()
    for i in range(n):
        r = res[i]
        exp = min(max_ret, max_fine_opt, int(r["n_cand_tidy"])) if r["n_res"] > 0 else 0
        assert cnt[i] == exp, (i, cnt[i], exp)
        row = cands[i]
        if exp:
            assert row[0]["cand_gidx"] == r["cand_gidx"] and row[0]["correlation"].tobytes() == r["correlation"].tobytes() and \
                row[0]["tf"].tobytes() == r["tf"].tobytes(), (i, row[0], r)
            c = row["correlation"][:exp]
            assert (c[:-1] >= c[1:]).all(), (i, c)
            assert len(set(row["cand_gidx"][:exp].tolist())) == exp, (i, row["cand_gidx"][:exp])
            assert (row["flags"][:exp] & ~(r["flags"] & 6) == 0).all(), (i, row["flags"][:exp], r["flags"])
        for k in range(exp, max_ret):
            assert row[k].tobytes() == zero, (i, k, row[k])


def check_against_peeled(row, n, lst, what):
    assert n == len(lst), (what, n, len(lst))
    for k, (g, corr, tf) in enumerate(lst):
        assert row[k]["cand_gidx"] == g, (what, k, row[k]["cand_gidx"], g)
        assert abs(row[k]["correlation"] - corr) < TOL, (what, k, row[k]["correlation"], corr)
        assert np.abs(row[k]["tf"] - tf).max() < TOL, (what, k, row[k]["tf"], tf)
