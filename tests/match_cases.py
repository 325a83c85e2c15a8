"""TEST INFRASTRUCTURE shared by test_emu_matches.py / test_gpu_matches.py: the matched contour pairs behind each ranked entry
(include/cont2_amd_matches.h: the _m instances of cc_k_merge, cc_k_match_emit) held against the oracle's hint flow with the selected
proposal's constellation exported (match_oracle.py).

A back end B is a database on the CPU harness or on the device, driven through the marshalling layer (calls.py) both share:
  B.L, B.lib (the bound library), B.db (the cc_db handle), B.stream (None: the null stream)
  B.dev(array) -> the address of a device copy of a numpy array, kept alive by B (the harness: the array itself)
  B.sync()        everything queued on the device has run (the harness: nothing to do)

Held for equality, no tolerance: the pair set in key order, n_pairs, vote_cnt, n_props, flags, and area_perc bit for bit (the
device sums a proposal's pairs in ascending bit order, which is the order of the reference's std::map).  res_rms / res_max: within
RES_TOL = 1e-10 px of a numpy f64 evaluation from the two descriptors and the returned tf.  That figure is derived, not measured:
coordinates and translations stay below about 600 px, a component is two products, two sums, a difference (each within 2^-53
relative: ~7e-14 px) and a sincos of a few ulps (~1e-13 px on a 600 px lever); the square root and the mean keep the relative
error: ~1e-12 px in all, two orders below the bar.  n_inlier is exact; the tests choose bars no residual lies within 1e-9 of."""
import ctypes as C
import math

import numpy as np

import constell_cases as K
import match_oracle as MO
import ranked_common as RC
from cc_amd import load

calls = load().calls
RES_TOL = 1e-10
BAR_GAP = 1e-9
EINVAL = -1
_scans = {}
_cache = {}


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _b(s):
    return None if s is None else C.cast(C.byref(s), C.c_void_p)


def oscan(key, d, int_id):
    if key not in _scans:
        _scans[key] = MO.Scan(d, int_id)
    return _scans[key]


def expected(tgt, tgt_key, db_desc, db_key, hints, sim=None, lb=None, ub=None):
    """the oracle's candidates for a hint list [n][4] of (DB index, level, seq_src, seq_tgt)
    -> ({DB index: (MATCH_DT record, keys int8 [n_pairs, 3])}, the records in candidates_ order with `cand` a DB index)"""
    hints = np.asarray(hints, np.int32).reshape(-1, 4)
    gs = sorted(set(int(g) for g in hints[:, 0]))
    loc = {g: i for i, g in enumerate(gs)}
    scans = [oscan((db_key, g), db_desc[g], 100 + g) for g in gs]   # candidates are told apart by their int id
    h = hints.copy()
    h[:, 0] = [loc[int(g)] for g in hints[:, 0]]
    ref, keys = MO.check_hints_matches(oscan(tgt_key, tgt, 1000000), scans, h, sim=sim, lb=lb, ub=ub)
    ref = ref.copy()
    ref["cand"] = [gs[int(c)] for c in ref["cand"]]
    return {int(r["cand"]): (r, keys[k]) for k, r in enumerate(ref)}, ref


def residuals(tgt, src, keys, tf):
    """|T p_src - p_tgt| per pair in f64, T = [c -s x; s c y] of the returned tf (source: the database scan, target: the query)"""
    c, s = math.cos(float(tf[2])), math.sin(float(tf[2]))
    out = np.zeros(len(keys))
    for i, (lev, a, b) in enumerate(np.asarray(keys, np.int64).tolist()):
        ps = np.float64(src["cont"][lev][a]["pos_mean"])
        pt = np.float64(tgt["cont"][lev][b]["pos_mean"])
        out[i] = math.hypot(c * ps[0] - s * ps[1] + float(tf[0]) - pt[0], s * ps[0] + c * ps[1] + float(tf[1]) - pt[1])
    return out


def new_stats():
    return dict(entries=0, pairs=0, multi=0, merged=0, rms=0.0, mx=0.0, res=[])


def report(st, what):
    print("%s: %d entries, %d pairs, %d entries of multi-proposal candidates, %d with merged checks (vote_cnt > n_pairs); "
          "largest |res_rms - numpy| %.3g, |res_max - numpy| %.3g px" % (what, st["entries"], st["pairs"], st["multi"], st["merged"], st["rms"], st["mx"]))


def check_entry(L, row, cand, exp, tgt, src, inlier_px, what, st):
    """one ranked entry's match row against the oracle's record of its candidate and the numpy residuals"""
    r, keys = exp
    assert r["survived"] == 1, (what, "the entry's candidate does not survive on the oracle", r)
    got = L.match_pairs(row)
    assert got.tolist() == keys.tolist(), (what, "pair set", got.tolist(), keys.tolist())
    assert row["n_pairs"] == len(keys) == r["n_pairs"], (what, row["n_pairs"], len(keys))
    assert row["vote_cnt"] == r["vote_cnt"] and row["n_props"] == r["n_props"], (what, row["vote_cnt"], row["n_props"], r)
    assert r["area_perc"].tobytes() == r["area_perc_tidy"].tobytes(), (what, "the oracle's two area figures", r)
    assert row["area_perc"].tobytes() == r["area_perc"].tobytes(), (what, "area_perc", float(row["area_perc"]).hex(), float(r["area_perc"]).hex())
    assert row["flags"] == cand["flags"], (what, row["flags"], cand["flags"])
    res = residuals(tgt, src, keys, cand["tf"])
    rms, mx = math.sqrt(float((res * res).sum()) / len(res)), float(res.max())
    st["entries"] += 1
    st["pairs"] += len(keys)
    st["multi"] += int(r["n_props"] > 1)
    st["merged"] += int(r["vote_cnt"] > r["n_pairs"])
    st["rms"], st["mx"] = max(st["rms"], abs(float(row["res_rms"]) - rms)), max(st["mx"], abs(float(row["res_max"]) - mx))
    st["res"].append(res)
    assert abs(float(row["res_rms"]) - rms) <= RES_TOL and abs(float(row["res_max"]) - mx) <= RES_TOL, (what, row["res_rms"], rms, row["res_max"], mx)
    assert (np.abs(res - inlier_px) > BAR_GAP).all(), (what, "a residual lies on the bar: the test must choose another", inlier_px)
    assert row["n_inlier"] == int((res <= inlier_px).sum()), (what, row["n_inlier"], res.tolist(), inlier_px)


def check_rows(L, tgt, tgt_key, db_desc, db_key, hints, cands, n, rows, inlier_px, what, st, sim=None, lb=None, ub=None):
    """every entry of one query's list; -> the oracle's records"""
    exp, ref = expected(tgt, tgt_key, db_desc, db_key, hints, sim=sim, lb=lb, ub=ub)
    zero = np.zeros(1, L.ranked_match_dt).tobytes()
    for k in range(int(n)):
        g = int(cands[k]["cand_gidx"])
        assert g in exp, (what, k, "the entry's scan is no candidate of the oracle", g)
        check_entry(L, rows[k], cands[k], exp[g], tgt, db_desc[g], inlier_px, what + (k, g), st)
    for k in range(int(n), len(rows)):
        assert rows[k].tobytes() == zero, (what, k, "a row beyond the list is not zero")
    return ref


def pick_bar(res_all):
    """a bar between the residuals: the middle of the widest gap of the sorted values (at least 2 * BAR_GAP wide)"""
    v = np.unique(np.concatenate([np.asarray(r).reshape(-1) for r in res_all]))
    assert len(v) >= 2
    gaps = np.diff(v)
    order = np.argsort(-gaps)
    for i in order:   # the widest gap that leaves residuals on both sides
        bar = 0.5 * (v[i] + v[i + 1])
        if gaps[i] > 4 * BAR_GAP and (np.abs(v - bar) > BAR_GAP).all():
            return float(bar)
    raise AssertionError("no bar between the residuals")


# ---- the flows on a back end ------------------------------------------------------------------------------------------------
def run_hints(B, q1, hints, lb=None, ub=None, mfo=10, ranked=16, matches=None, detail=False):
    q = B.dev(np.ascontiguousarray(np.asarray(q1).reshape(1)))
    r = calls.check_hints(B.lib, B.db, q, hints, lb, ub, mfo, B.stream, ranked=ranked, detail=detail, matches=matches)
    B.sync()
    return r


def run_query(B, qdesc, epochs, want_knn=False, **kw):
    """calls.query on descriptors (qdesc an array) or a source (qdesc None, src= / idx= given); -> its record, with knn / kcnt"""
    L = B.L
    nq = len(np.asarray(epochs).reshape(-1))
    if qdesc is not None:
        kw["qdesc"] = B.dev(np.ascontiguousarray(qdesc))
    knn = cnt = None
    if want_knn:
        ks = B.lib.cc_db_knn_stride(B.db)
        knn, cnt = np.zeros((nq, L.NQLEV, L.NPIV, ks), L.knn_hit_dt), np.zeros((nq, L.NQLEV, L.NPIV), np.int32)
        kw.update(knn=B.dev_out(knn), knn_cnt=B.dev_out(cnt))
    r = calls.query(B.lib, B.db, epochs, stream=B.stream, **kw)
    B.sync()
    if want_knn:
        r.knn, r.kcnt = B.fetch(knn), B.fetch(cnt)
    return r


def run_verify(B, qdesc, items, qidx=None, mfo=10, **kw):
    if qdesc is not None:
        kw.update(qdesc=B.dev(np.ascontiguousarray(qdesc)), n_desc=len(qdesc))
    r = calls.verify(B.lib, B.db, items, qidx=qidx, levels=None, max_fine_opt=mfo, max_key_dist_sq=float("inf"), stream=B.stream, **kw)
    B.sync()
    return r


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_answers(r, r0, what, match=True):
    same(r.res, r0.res, (what, "res"))
    same(r.rank[0], r0.rank[0], (what, "ranked lists"))
    same(r.rank[1], r0.rank[1], (what, "counts"))
    if r0.detail is not None:
        same(r.detail, r0.detail, (what, "detail"))
    if match:
        same(r.match, r0.match, (what, "match rows"))


# ---- 1. the built merge scenes (the back end's database is constell_cases.database) -------------------------------------------
E_SCENES = ("E proposals", "E rounds 0 63 64 130", "E 65 candidates", "E sentinels, first call", "E sentinels, second call")


def scene_hints(L, sc):
    h = np.zeros(len(sc.hints), L.hint_dt)
    h["cand_gidx"] = sc.base + sc.hints[:, 0]
    h["level"], h["seq_src"], h["seq_tgt"] = sc.hints[:, 1], sc.hints[:, 2], sc.hints[:, 3]
    hi = np.asarray(sc.hints, np.int32).copy()
    hi[:, 0] += sc.base
    return h, hi


def scene_reference(L, oracle, sc):
    """the match oracle's records of a scene, cross-checked against the committed oracle.check_hints_cands"""
    key = ("scene", sc.name)
    if key not in _cache:
        db_desc = K.database(L)
        mr = K.merge_reference(L, oracle, sc)
        _, hi = scene_hints(L, sc)
        exp, ref = expected(sc.tgt, ("E tgt",), db_desc, "E", hi, sim=mr["ref"]["sim"], lb=mr["ref"]["lb"], ub=mr["ref"]["ub"])
        old = mr["cands"]
        assert len(ref) == len(old), (sc.name, len(ref), len(old))
        for k in range(len(old)):
            s = int(old["idx_sel"][k])
            assert ref["cand"][k] == sc.base + old["cand"][k] and ref["n_props"][k] == old["n_props"][k] and ref["idx_sel"][k] == s, (sc.name, k, ref[k], old[k])
            assert ref["survived"][k] == old["survived"][k] and ref["vote_cnt"][k] == old["vote_cnt"][k, s], (sc.name, k, ref[k], old[k])
            assert ref["n_pairs"][k] == old["n_constell"][k, s] and ref["area_perc"][k].tobytes() == old["area_perc"][k, s].tobytes(), (sc.name, k, ref[k], old[k])
        _cache[key] = (exp, ref, mr)
    return _cache[key]


def proposals_scene_facts(L, oracle, sc):
    """what the "E proposals" scene must hold, asserted on the oracle's side"""
    exp, ref, mr = scene_reference(L, oracle, sc)
    assert ref["n_props"].tolist() == [1, 2, 4, 4, 2, 2, 1, 2, 1, 1] and ref["idx_sel"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0], ref
    assert ref["survived"].all() and len(ref) == 10
    assert (ref["vote_cnt"] > ref["n_pairs"]).any(), "an entry whose checks merged the same pairs more than once"
    names = list(K.E_SEQ)
    abc = names.index("joins the first of two that would both accept it")
    levels = set(exp[sc.base + abc][1][:, 0].tolist())
    assert len(levels) >= 2, ("the ABC candidate's set spans two levels", levels)
    assert (ref["idx_sel"] != 0).any(), "an entry whose selected proposal is not the first"
    drop = names.index("a fifth proposal is dropped, the first still joins")
    old = mr["cands"][drop]
    voted = sum(len(mr["ref"]["pairs"][i][1]) for i in range(len(sc.hints)) if sc.hints[i, 0] == drop)
    assert old["n_props"] == 4 and int(old["vote_cnt"].sum()) < voted, ("a fifth proposal was dropped", old, voted)


def check_merge_scenes(B, L, oracle, log=None):
    """case 1: the scenes in order (the two sentinel calls follow each other), every ranked entry against the oracle"""
    scenes = {sc.name: sc for sc in K.merge_scenes(L)}
    db_desc = K.database(L)
    st = new_stats()
    for name in E_SCENES:
        sc = scenes[name]
        exp, ref, mr = scene_reference(L, oracle, sc)
        if name == "E proposals":
            proposals_scene_facts(L, oracle, sc)
        h, hi = scene_hints(L, sc)
        lb, ub = mr["ref"]["lb"], mr["ref"]["ub"]
        r = run_hints(B, sc.tgt, h, lb, ub, mfo=10, ranked=16, matches=0.0)
        cands, n = r.rank
        want = min(16, 10, int(ref["survived"].sum()))
        assert n[0] == want > 0, (name, n, want)
        if name == "E proposals":
            assert n[0] == 10
        check_rows(L, sc.tgt, ("E tgt",), db_desc, "E", hi, cands[0], n[0], r.match[0], 0.0, (name,), st, sim=mr["ref"]["sim"], lb=lb, ub=ub)
        if log is not None:
            log.append("%-28s %2d entries" % (name, int(n[0])))
    report(st, "merge scenes")
    return st


# ---- 2. bit edges -------------------------------------------------------------------------------------------------------------
def bit_edge_scene(L):
    """The E query with level-1 rows 3 and 4 replaced by copies of row 6 and the BCI of anchor (1, 5) naming both in the place of
    row 6: candidate 0's check on that anchor pairs the candidate's contour 6 with the query's 3 and 4 -- bits 63 and 64, either
    side of a word boundary; candidate 1's check on (4, 5) holds (4, 9, 9): bit 399, the last of the set."""
    if "bits" not in _cache:
        sc0 = K.merge_scenes(L)[0]
        K.database(L)
        tgt = sc0.tgt.copy()
        for q in (3, 4):
            tgt["cont"][1][q] = tgt["cont"][1][6]
        b = tgt["bcis"][1, 5].copy()
        pts = [tuple(p) for p in b["pts"][:int(b["n_pts"])].tolist()]
        new = []
        for p in pts:
            new += [(p[0], 3) + p[2:], (p[0], 4) + p[2:]] if p[1] == 6 else [p]
        assert len(new) == len(pts) + 1
        segs = [k for k in range(len(new)) if k == 0 or new[k - 1][2] != new[k][2]] + [len(new)]
        for k, p in enumerate(new):
            b["pts"][k] = p
        b["n_pts"], b["n_segs"] = len(new), len(segs)
        b["segs"][:len(segs)] = segs
        tgt["bcis"][1, 5] = b
        hints = np.array([(sc0.base + 0, 1, 5, 5), (sc0.base + 1, 4, 5, 5)], np.int32)
        _cache["bits"] = (tgt, hints, None, sc0)
    return _cache["bits"]


def check_bit_edges(B, L, oracle):
    """case 2"""
    tgt, hi, _, sc0 = bit_edge_scene(L)
    mr = K.merge_reference(L, oracle, sc0)
    sim = mr["ref"]["sim"]
    # (a level-4 constellation alone weighs 0.1 of its area: the scene's own bars with the area bar taken down)
    lb, ub = K.thresholds(L, neg_est_dist=-1e9, correlation=-1e30, area_perc=0.0)
    db_desc = K.database(L)
    exp, ref = expected(tgt, ("E tgt, bit edges",), db_desc, "E", hi, sim=sim, lb=lb, ub=ub)
    k0, k1 = exp[int(hi[0, 0])][1].tolist(), exp[int(hi[1, 0])][1].tolist()
    assert [1, 6, 3] in k0 and [1, 6, 4] in k0, ("the oracle's set holds bits 63 and 64", k0)
    assert [4, 9, 9] in k1, ("the oracle's set holds bit 399", k1)
    r = run_hints(B, tgt, RC.to_hint_dt(L, hi), lb, ub, mfo=10, ranked=16, matches=0.0)
    cands, n = r.rank
    assert n[0] == 2, n
    st = new_stats()
    check_rows(L, tgt, ("E tgt, bit edges",), db_desc, "E", hi, cands[0], n[0], r.match[0], 0.0, ("bit edges",), st, sim=sim, lb=lb, ub=ub)
    words = {int(c["cand_gidx"]): np.asarray(m["pairs"], np.uint64) for c, m in zip(cands[0][:2], r.match[0][:2])}
    w0, w1 = words[int(hi[0, 0])], words[int(hi[1, 0])]
    assert (int(w0[0]) >> 63) & 1 and int(w0[1]) & 1 and (int(w1[6]) >> (399 - 384)) & 1, (w0, w1)
    # cc_match_pairs round-trips them in key order; a short buffer is not overrun and the count is still the set's
    for g in (int(hi[0, 0]), int(hi[1, 0])):
        m = r.match[0][[int(c["cand_gidx"]) for c in cands[0][:2]].index(g)]
        row = np.ascontiguousarray(m.reshape(1))
        out = np.full((401, 4), 0x55, np.int8)
        got = B.lib.cc_match_pairs(_p(row), _p(out), 400)
        assert got == m["n_pairs"] == len(exp[g][1])
        assert out[:got, :3].tolist() == exp[g][1].tolist() == L.match_pairs(m).tolist() and not out[:got, 3].any() and (out[got:] == 0x55).all()
        assert B.lib.cc_match_pairs(_p(row), _p(out), 2) == got and (out[2:got, 3] == 0).all()
        assert B.lib.cc_match_pairs(_p(row), None, 0) == got and B.lib.cc_match_pairs(None, None, 0) == -1
    return st


# ---- 3. the query flow on the 64-scan loop drive ------------------------------------------------------------------------------
def drive_reference(B, cc, oracle, key):
    """the drive's 64 queries at their own epochs in one call, with hit lists: without and with matches (bar 0)"""
    ck = ("drive", key)
    if ck not in _cache:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        r0 = run_query(B, desc, seeds, want_knn=True, ranked=16, detail=True)
        r = run_query(B, desc, seeds, want_knn=True, ranked=16, detail=True, matches=0.0)
        _cache[ck] = (r0, r)
    return _cache[ck]


def check_drive(B, cc, oracle, key, sim=None):
    """case 3 (and 4's tolerance on every entry): every ranked entry of every query against the oracle fed with the query's own hits"""
    L = B.L
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    r0, r = drive_reference(B, cc, oracle, key)
    cands, n = r.rank
    st = new_stats()
    multi_cands = merged_props = 0
    for q in range(len(desc)):
        if n[q] == 0:
            assert not r.match[q].tobytes().strip(b"\0"), (key, q)
            continue
        hints = RC.hints_of_knn(L, r.knn[q], r.kcnt[q], n_levels=int(dcfg.n_q_levels))
        ref = check_rows(L, desc[q], ("drive", q), desc, "drive", hints, cands[q], n[q], r.match[q], 0.0, (key, q), st, sim=dcfg.cont_sim)
        multi_cands += int((ref["n_props"] > 1).sum())
        merged_props += int((ref["vote_cnt"] > ref["n_pairs"]).sum())
    report(st, "drive, %s" % key)
    print("drive, %s: %d queries with entries, %d multi-proposal candidates, %d selected proposals that merged checks" % (
        key, int((n > 0).sum()), multi_cands, merged_props))
    assert st["entries"] == int(n.sum()) > 0, (key, "at least one query returns an entry")
    return st


# ---- 4. the three bars --------------------------------------------------------------------------------------------------------
def check_bars(B, L, oracle):
    """n_inlier for the bars 0, one between the residuals and 1e9, on the "E proposals" scene (ten entries, 3 .. 15 pairs each)"""
    sc = K.merge_scenes(L)[0]
    exp, ref, mr = scene_reference(L, oracle, sc)
    h, hi = scene_hints(L, sc)
    lb, ub, sim = mr["ref"]["lb"], mr["ref"]["ub"], mr["ref"]["sim"]
    db_desc = K.database(L)
    st = new_stats()
    r = run_hints(B, sc.tgt, h, lb, ub, matches=0.0)
    check_rows(L, sc.tgt, ("E tgt",), db_desc, "E", hi, r.rank[0][0], r.rank[1][0], r.match[0], 0.0, ("bar 0",), st, sim=sim, lb=lb, ub=ub)
    bar = pick_bar(st["res"])
    got = {}
    for px in (0.0, bar, 1e9):
        r1 = run_hints(B, sc.tgt, h, lb, ub, matches=px)
        same_answers(r1, r, ("bar", px), match=False)
        check_rows(L, sc.tgt, ("E tgt",), db_desc, "E", hi, r1.rank[0][0], r1.rank[1][0], r1.match[0], px, ("bar", px), new_stats(), sim=sim, lb=lb, ub=ub)
        got[px] = r1.match[0]["n_inlier"][:10].copy()
    npairs = r.match[0]["n_pairs"][:10]
    print("bars 0 / %.6g / 1e9: inliers %s / %s / %s of %s pairs" % (bar, got[0.0].tolist(), got[bar].tolist(), got[1e9].tolist(), npairs.tolist()))
    assert (got[1e9] == npairs).all() and (got[0.0] <= got[bar]).all() and 0 < int(got[bar].sum()) < int(npairs.sum())


# ---- 5. nothing else moves ----------------------------------------------------------------------------------------------------
def knn_chunks(B):
    out = np.zeros(3, np.int64)
    assert B.lib.cc_db_debug_knn_chunks(B.db, _p(out)) == 0
    return out


def check_nothing_else_moves(B, cc, oracle, key):
    L = B.L
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    r0, r = drive_reference(B, cc, oracle, key)
    same_answers(r, r0, "with and without matches", match=False)
    same(r.kcnt, r0.kcnt, "want_knn counts")
    ks = r.knn.shape[-1]
    live = np.arange(ks)[None, None, None, :] < np.minimum(r.kcnt, ks)[..., None]   # (a list's entries beyond its count are not the call's)
    same(r.knn[live], r0.knn[live], "want_knn hits")
    # match NULL through the new entry points is the old entry point; the retrieval counters move alike
    qs = np.arange(36, 44, dtype=np.int32)
    c0 = knn_chunks(B)
    a = run_query(B, desc[qs], qs, ranked=16, detail=True)
    c1 = knn_chunks(B)
    lb, ub = L.default_thresholds()
    res = np.zeros(len(qs), L.query_result_dt)
    cands, cnt, ro = L.rank_buffers(len(qs), 16)
    det = L.rank_detail_buffer(len(qs), 16)
    qd = B.dev(np.ascontiguousarray(desc[qs]))
    rc = B.lib.cc_db_query_submit_matched(B.db, qd, None, None, len(qs), _p(qs), _b(lb), _b(ub), _p(res), None, None, B.stream, _b(ro), _p(det), None, None)
    assert rc == 0 and B.lib.cc_db_query_wait(B.db) == 0, B.lib.cc_last_error()
    c2 = knn_chunks(B)
    b = run_query(B, desc[qs], qs, ranked=16, detail=True, matches=1.0)
    c3 = knn_chunks(B)
    same(res, a.res, "match NULL: res")
    same(cands, a.rank[0], "match NULL: lists")
    same(cnt, a.rank[1], "match NULL: counts")
    same(det, a.detail, "match NULL: detail")
    same_answers(b, a, "a matched call", match=False)
    assert (c1 - c0).tolist() == (c2 - c1).tolist() == (c3 - c2).tolist() and (c1 - c0).sum() > 0, (c0, c1, c2, c3)
    # the plain entry points without a list: the matched one with rank NULL and match NULL
    p0 = run_query(B, desc[qs], qs)
    res2 = np.zeros(len(qs), L.query_result_dt)
    rc = B.lib.cc_db_query_submit_matched(B.db, qd, None, None, len(qs), _p(qs), _b(lb), _b(ub), _p(res2), None, None, B.stream, None, None, None, None)
    assert rc == 0 and B.lib.cc_db_query_wait(B.db) == 0
    same(res2, p0.res, "rank NULL, match NULL")
    hq = 38
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, r.knn[hq], r.kcnt[hq]))
    h0 = run_hints(B, desc[hq], hints, mfo=dcfg.max_fine_opt, detail=True)
    h1 = run_hints(B, desc[hq], hints, mfo=dcfg.max_fine_opt, detail=True, matches=2.0)
    same_answers(h1, h0, "hint flow", match=False)
    same(h1.scores, h0.scores, "hint scores")
    assert h0.rank[1][0] == r.rank[1][hq] and h1.match[0]["pairs"].tobytes() == r.match[hq]["pairs"].tobytes()


# ---- 6. forms and mixing ------------------------------------------------------------------------------------------------------
def check_forms(B, cc, oracle, key, packed):
    """stored, packed, masked and host forms against the descriptor form; packed: (hot address, feat address, n) of the drive's records"""
    L = B.L
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    r0, r = drive_reference(B, cc, oracle, key)
    qs = np.array([36, 38, 40, 41, 47, 63, 5, 50], np.int32)
    ref = run_query(B, desc[qs], qs, ranked=16, detail=True, matches=0.5)
    assert int(ref.rank[1].sum()) >= 4 and (ref.rank[1] == 0).any()
    same(np.ascontiguousarray(r.match[qs])["pairs"], ref.match["pairs"], "a subset gives the rows of the whole drive")
    stored = run_query(B, None, qs, src=L.PackedSrc(None, None, 0, 0), idx=qs, ranked=16, detail=True, matches=0.5)
    same_answers(stored, ref, "stored")
    pk = run_query(B, None, qs, src=L.PackedSrc(packed[0], packed[1], packed[2], 0), idx=qs, ranked=16, detail=True, matches=0.5)
    same_answers(pk, ref, "packed")
    bits = np.full((2, 2), 0xFFFFFFFF, np.uint32)
    rows = np.array([0, -1, 1, 0, -1, 1, 0, 0], np.int32)
    mk = run_query(B, desc[qs], qs, mask=(B.dev(bits), 2, 2, rows), ranked=16, detail=True, matches=0.5)
    same_answers(mk, ref, "masked (every scan allowed)")
    lb, ub = L.default_thresholds()
    res = np.zeros(len(qs), L.query_result_dt)
    cands, cnt, ro = L.rank_buffers(len(qs), 16)
    det = L.rank_detail_buffer(len(qs), 16)
    mt, mo = L.match_buffers(len(qs), 16, 0.5)
    mt.view(np.uint8)[...] = 0xFF   # rows beyond h_n are zeroed by the device, not by the host
    qd = np.ascontiguousarray(desc[qs])
    hm = L.ScanMaskC(bits.ctypes.data, 2, 2, rows.ctypes.data)
    rc = B.lib.cc_db_query_batch_host_matched(B.db, _p(qd), len(qs), _p(qs), _b(lb), _b(ub), _p(res), _b(ro), _p(det), _b(hm), _b(mo))
    assert rc == 0, B.lib.cc_last_error()
    same(res, ref.res, "host: res")
    same(cands, ref.rank[0], "host: lists")
    same(det, ref.detail, "host: detail")
    same(mt, ref.match, "host: match rows (the buffer was pre-filled with 0xFF)")
    # the hint flow's host form
    hq = 38
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, r.knn[hq], r.kcnt[hq]))
    h1 = run_hints(B, desc[hq], hints, mfo=dcfg.max_fine_opt, matches=0.5)
    res1 = np.zeros(1, L.query_result_dt)
    c1, n1, ro1 = L.rank_buffers(1, 16)
    m1, mo1 = L.match_buffers(1, 16, 0.5)
    m1.view(np.uint8)[...] = 0xFF
    q1 = np.ascontiguousarray(desc[hq:hq + 1])
    rc = B.lib.cc_db_check_hints_host_matched(B.db, _p(q1), _p(hints), len(hints), _b(lb), _b(ub), int(dcfg.max_fine_opt), _p(res1), None, _b(ro1), None, _b(mo1))
    assert rc == 0, B.lib.cc_last_error()
    same(m1, h1.match, "hint flow, host form")
    same(c1, h1.rank[0], "hint flow, host form: lists")
    i38 = int(np.nonzero(qs == hq)[0][0])
    assert m1[0]["pairs"].tobytes() == ref.match[i38]["pairs"].tobytes() and np.array_equal(m1[0]["n_inlier"], ref.match[i38]["n_inlier"])


def check_verify(B, L, oracle):
    """one item of eight candidates on the E scans: one row per surviving candidate (descriptor, host and stored-free forms)"""
    sc = K.merge_scenes(L)[0]
    mr = K.merge_reference(L, oracle, sc)
    db_desc = K.database(L)
    lb, ub, sim = mr["ref"]["lb"], mr["ref"]["ub"], mr["ref"]["sim"]
    items = [[sc.base + k for k in range(8)]]
    q = np.ascontiguousarray(sc.tgt.reshape(1))
    hl, hn = np.zeros((1, L.HINT_MAX), L.hint_dt), np.zeros(1, np.int32)
    r0 = run_verify(B, q, items, ranked=16, detail=True, lb=lb, ub=ub)
    r = run_verify(B, q, items, ranked=16, detail=True, matches=0.0, lb=lb, ub=ub, hints=B.dev_out(hl), n_hints=B.dev_out(hn))
    same_answers(r, r0, "verify", match=False)
    hl, hn = B.fetch(hl), B.fetch(hn)
    h = hl[0, :hn[0]]
    hi = np.stack([h["cand_gidx"], h["level"], h["seq_src"], h["seq_tgt"]], 1).astype(np.int32)
    st = new_stats()
    ref = check_rows(L, sc.tgt, ("E tgt",), db_desc, "E", hi, r.rank[0][0], r.rank[1][0], r.match[0], 0.0, ("verify",), st, sim=sim, lb=lb, ub=ub)
    assert r.rank[1][0] == int(ref["survived"].sum()) == 8, (r.rank[1], ref)
    res = np.zeros(1, L.query_result_dt)
    cands, cnt, ro = L.rank_buffers(1, 16)
    mt, mo = L.match_buffers(1, 16, 0.0)
    mt.view(np.uint8)[...] = 0xFF
    tab = calls.cand_table(items)
    cfg = L.VerifyCfg(0, 10, float("inf"), 0)
    rc = B.lib.cc_db_verify_batch_host_matched(B.db, _p(q), 1, None, _p(tab), 1, _b(cfg), _b(lb), _b(ub), _p(res), _b(ro), None, _b(mo))
    assert rc == 0, B.lib.cc_last_error()
    same(mt, r.match, "verify, host form")
    report(st, "verify")


def check_lanes(B4, cc, oracle, ref_rows):
    """130 queries over four lanes with max_ret 1, 4 and 16: the rows are the prefix of the 64-query call's (B4: a database of the
    drive with four lanes; ref_rows: the drive's answer with matches at bar 0)"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    qs = np.concatenate([np.arange(64), np.arange(64), [38, 40]]).astype(np.int32)
    assert len(qs) == 130
    for k in (1, 4, 16):
        r = run_query(B4, desc[qs], qs, ranked=k, matches=0.0)
        want = np.ascontiguousarray(ref_rows.match[qs][:, :k])
        same(r.match, want, ("four lanes, max_ret", k))
        same(r.rank[0], np.ascontiguousarray(ref_rows.rank[0][qs][:, :k]), ("four lanes, lists", k))
        assert np.array_equal(r.rank[1], np.minimum(ref_rows.rank[1][qs], k))


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def check_refusals(B, cc, oracle, Bdyn):
    """every refusal of the header: nothing is queued, nothing is written, the handle answers as before.  Bdyn: a database of the
    drive in dynamic-threshold mode."""
    L = B.L
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    lb, ub = L.default_thresholds()
    qs = np.array([38, 40], np.int32)
    qd_h = np.ascontiguousarray(desc[qs])
    qd = B.dev(qd_h)
    before = run_query(B, desc[qs], qs, ranked=16, matches=0.0)
    res = np.zeros(2, L.query_result_dt)
    cands, cnt, ro = L.rank_buffers(2, 16)
    mt, mo = L.match_buffers(2, 16, 1.0)
    tab = calls.cand_table([[0, 1], [2]])
    cfg = L.VerifyCfg(0, 5, 1000.0, 0)
    hints = RC.to_hint_dt(L, np.array([[0, 1, 0, 0]], np.int32))

    def every(lib, db, qdev, r, m):
        yield "query_submit", lib.cc_db_query_submit_matched(db, qdev, None, None, 2, _p(qs), _b(lb), _b(ub), _p(res), None, None, B.stream, r, None, None, m)
        yield "query_batch_host", lib.cc_db_query_batch_host_matched(db, _p(qd_h), 2, _p(qs), _b(lb), _b(ub), _p(res), r, None, None, m)
        yield "scan_batch", lib.cc_db_query_scan_batch_submit_matched(db, None, 1, _p(qs), _b(lb), _b(ub), _p(res), r, None, m)
        yield "verify_submit", lib.cc_db_verify_submit_matched(db, qdev, 2, None, None, _p(tab), 2, _b(cfg), _b(lb), _b(ub), _p(res), None, None, B.stream, r, None, m)
        yield "verify_batch_host", lib.cc_db_verify_batch_host_matched(db, _p(qd_h), 2, None, _p(tab), 2, _b(cfg), _b(lb), _b(ub), _p(res), r, None, m)
        yield "check_hints", lib.cc_db_check_hints_matched(db, qdev, _p(hints), 1, _b(lb), _b(ub), 5, _p(res), None, B.stream, r, None, m)
        yield "check_hints_host", lib.cc_db_check_hints_host_matched(db, _p(qd_h), _p(hints), 1, _b(lb), _b(ub), 5, _p(res), None, r, None, m)

    def refused(why, word, lib, db, qdev, r, m):
        seen = 0
        for fn, rc in every(lib, db, qdev, r, m):
            assert rc == EINVAL, (why, fn, rc)
            msg = lib.cc_last_error()
            assert word in msg and fn.split("_")[0].encode() in msg, (why, fn, msg)
            seen += 1
        assert seen == 7

    refused("match without rank", b"comes with rank", B.lib, B.db, qd, None, _b(mo))
    no_rows = L.MatchOut(None, 1.0)   # (named: the library reads the struct through a bare pointer)
    refused("h_match NULL", b"h_match", B.lib, B.db, qd, _b(ro), _b(no_rows))
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        bad_px = L.MatchOut(mt.ctypes.data, bad)
        refused("inlier_px %r" % bad, b"inlier_px", B.lib, B.db, qd, _b(ro), _b(bad_px))
    refused("dynamic thresholds", b"dynamic-threshold", Bdyn.lib, Bdyn.db, Bdyn.dev(qd_h), _b(ro), _b(mo))
    # whatever the underlying call refuses
    for what, r in (("max_ret 17", L.RankOut(cands.ctypes.data, cnt.ctypes.data, 17, 0)), ("h_n NULL", L.RankOut(cands.ctypes.data, None, 16, 0))):
        for fn, rc in every(B.lib, B.db, qd, _b(r), _b(mo)):
            assert rc == EINVAL, (what, fn, rc)
    bad_ub = L.Score.from_buffer_copy(bytes(ub))
    bad_ub.i_ovlp_sum = lb.i_ovlp_sum
    assert B.lib.cc_db_query_submit_matched(B.db, qd, None, None, 2, _p(qs), _b(lb), _b(bad_ub), _p(res), None, None, B.stream, _b(ro), None, None, _b(mo)) == EINVAL
    both = L.PackedSrc(None, None, 0, 0)   # descriptors AND a source
    assert B.lib.cc_db_query_submit_matched(B.db, qd, _b(both), None, 2, _p(qs), _b(lb), _b(ub), _p(res), None, None, B.stream, _b(ro), None, None, _b(mo)) == EINVAL
    assert B.lib.cc_db_query_wait(B.db) == 0 and Bdyn.lib.cc_db_query_wait(Bdyn.db) == 0
    B.sync()
    assert not res.tobytes().strip(b"\0") and not cands.tobytes().strip(b"\0") and not cnt.any() and not mt.tobytes().strip(b"\0"), "a refused call wrote an answer"
    after = run_query(B, desc[qs], qs, ranked=16, matches=0.0)
    same_answers(after, before, "the handle after the refusals")
    # the dynamic database still answers its ranked calls
    d0 = run_query(Bdyn, desc[qs], qs, ranked=16)
    assert d0.res["n_cand_pose"].sum() >= 0
    # Python: matches without ranked is a ValueError before the library is called
    import pytest
    with pytest.raises(ValueError):
        calls.query(B.lib, B.db, qs, qdesc=qd, matches=1.0)
