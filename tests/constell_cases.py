"""TEST INFRASTRUCTURE shared by test_emu_constell.py / test_gpu_constell.py: K4 (csrc/k_check.h) on BUILT scans.

Descriptors are built here (make_scan), not ingested: the header, keys and the levels 0 / 5 of one recorded scan, and for levels
1..4 up to 10 contour rows and the BCIs of the 6 anchors, both chosen by the case.  The builder keeps the BCI invariants (points
ordered by bit_pos, the ring bits are the points' bit positions, a point's level is its ring layer + 1, segs are the starts of the
runs of equal bit_pos plus the end, seq < 10, at most 40 points); every descriptor is rebuilt with oracle.Scan.from_desc and
compared with what the oracle then holds (accepted()) before it is used.

A case is a SLOT: one (level, anchor) of a scan pair, with its own src / tgt anchor rows and BCIs, checked by the hint
(candidate, level, anchor, anchor).  24 slots share a scan pair; a SCENE is one query scan, its candidate scans and a hint list,
run as ONE cc_db_check_hints call per back end.

Two judges, neither of them the product:
  R1  the oracle: orc_check_hints on the scene's hint list (five scores and `passed` per hint, the counters of the result
      record), orc_check_pair per hint (the pair set and T_pass of a passing check).
  R2  a numpy restatement (r2_check): checkSim with every operation rounded in f32 as cc_check_sim writes it, the popcount
      bars on 256-bit integers, the potential pairs with clampAng in f64, the two-pointer window on the sorted keys in the
      reference's f64 expression, the individual similarity of the window's pairs.  It gives ovlp_sum, max_one, in_ang_rng
      and indiv_sim and, beside them, the pair count and the window's start, which no other judge exports.  On a slot whose
      keys are all distinct the sorted order is known, and R2 goes on (r2_b2): the shaft scan in the reference's sequential
      form, the orientation filter with glibc's acosf, the swap-to-back removal -- i_orie_sim, passed and the constellation.
      Where keys tie, those three depend on the order std::sort leaves among equal
      keys, which R2 (a stable sort) does not know.  R2 must agree with R1 on every hint of every scene (reference()) before a
      back end is judged; the edge assertions of a case (its pair count, its window) are made on R2's figures once R1 has
      confirmed R2's scores for that hint.

Compared for equality, no tolerance: the six per-hint figures, the pair set and pair count of every passing check,
cand_aft_check1..3, n_cand_pose, n_cand_tidy, n_res and flags.  Where the device's capacities cut a check (more than 256
potential pairs, a window of more than 63 pairs: CC_QF_CHECK_CAP) the reference, which has none, is no judge of what follows
the cut: such a slot is marked `capped`, the flag must be set, the figures up to the cut are compared; with distinct keys the cut is
deterministic and R2 states the device's outcome, held for equality (r2_tie_free); with ties a passing capped check
must hold 64 entries at most, all of them from the reference's window or the anchor pair, and the anchor pair itself wherever the
orientation filter cannot remove it (a src anchor row without ecc_feat: the `C cap` slots).

T_pass (cc_db_debug_passes) is judged against the closed form at 50 digits on R1's pair list and the f32 pos_means, within
tf_bound(): a running error analysis of the two mean sums, the four covariance sums, sqrt, the two divisions, the rotation of
the mean and atan2.  ASSUMPTION: the f64 atan2 of the device library (and glibc's) is within ATAN2_ULP = 2 ulp; nothing in the
suite holds the device's to it.  The oracle's own T_pass goes through the same check first.  A constellation whose nrm is
below 1e-6 takes the sequential branch on both sides: x and y must then have the oracle's bits."""
import ctypes as C
import math

import mpmath as mp
import numpy as np

import pose_common as PC

F = np.float32
U = 2.0 ** -53
ATAN2_ULP = 2.0
NSLOT_LEV, NSLOT_ANCH = 4, 6
SCORE_FIELDS = ("i_ovlp_sum", "i_ovlp_max_one", "i_in_ang_rng", "i_indiv_sim", "i_orie_sim", "passed")
RES_FIELDS = ("n_res", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy", "n_knn_hits", "flags")
QF_CHECK_CAP = 1
CC_ECAPACITY = -4
PP_SMALL, PP_MAX, CSTL_MAX = 64, 256, 64
PI_F = F(math.pi)
RANGE_F = F(math.pi / 16)
WRAP_T = F(float.fromhex("-0x1.858eb6p+2"))   # CC_B1_WRAP_T


def nf(x, up=True):
    return np.nextafter(F(x), F(np.inf) if up else F(-np.inf))


# ---- 0. the builder -----------------------------------------------------------------------------------------------------
def plain_rows(seed, tf=(0.0, 0.0, 0.0), jitter=0.0, ecc=0):
    """ten rows for each of the levels 1..4: {level: list of row dicts}.  Row (l, s) of every scan made with the same seed is the
    same contour, moved by tf = (x, y, theta) about the image centre, its axis turned by theta plus a row-specific `jitter`."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(25.0, 125.0, (5, 10, 2))
    ang = rng.uniform(-1.5, 1.5, (5, 10))
    jit = np.random.default_rng(seed + 7919).uniform(-1.0, 1.0, (5, 10)) * jitter
    c, s = math.cos(tf[2]), math.sin(tf[2])
    out = {}
    for lev in range(1, 5):
        rows = []
        for q in range(10):
            p = pos[lev, q] - 75.0
            p = np.array([c * p[0] - s * p[1] + 75.0 + tf[0], s * p[0] + c * p[1] + 75.0 + tf[1]])
            a = ang[lev, q] + tf[2] + jit[lev, q]
            rows.append(dict(cell_cnt=200 - 2 * q, pos_mean=F(p), com=F(p), eig_vals=F([4.0, 9.0]), ang=a, vol3_mean=F(1.0), ecc_feat=ecc))
        out[lev] = rows
    return out


def pt(level, seq, bit_pos, theta, r=1.0):
    return (int(level), int(seq), int(bit_pos), float(r), F(theta))


def make_scan(L, rows, bcis):
    """a layouts.scan_desc_dt record.  rows: {level 1..4: <= 10 row dicts}; bcis: {(level, anchor): list of pt()} -- anchors that
    are not named get an empty BCI."""
    d = PC.fixture_desc(L)[0].copy()
    for lev in range(1, 5):
        rs = rows[lev]
        n = len(rs)
        assert n <= 10
        tab = np.zeros(L.MAXC, L.contour_dt)
        for q, r in enumerate(rs):
            t = tab[q]
            t["level"] = lev
            t["poi"] = np.clip(np.nan_to_num(r["pos_mean"]), 0, 149).astype(np.int16)
            t["cell_cnt"] = r["cell_cnt"]
            t["pos_mean"], t["com"] = r["pos_mean"], r["com"]
            t["eig_vals"] = r["eig_vals"]
            if "eig_vecs" in r:
                t["eig_vecs"] = r["eig_vecs"]
            else:
                c, s = F(math.cos(r["ang"])), F(math.sin(r["ang"]))
                t["eig_vecs"] = [c, s, -s, c]   # v00 v10 v01 v11: column 1 = (v01, v11) is the major axis
            v, e = t["eig_vecs"].astype(np.float64), t["eig_vals"].astype(np.float64)
            t["pos_cov"] = [v[0] * v[0] * e[0] + v[2] * v[2] * e[1], v[1] * v[0] * e[0] + v[3] * v[2] * e[1],
                            v[0] * v[1] * e[0] + v[2] * v[3] * e[1], v[1] * v[1] * e[0] + v[3] * v[3] * e[1]]
            t["eccen"] = math.sqrt(max(0.0, 1.0 - float(e[0]) / float(e[1]))) if e[1] > 0 else 0.0
            t["vol3_mean"] = r["vol3_mean"]
            t["ecc_feat"] = r["ecc_feat"]
            tab[q] = t
        d["cont"][lev] = tab
        d["n_cont"][lev] = d["n_stored"][lev] = n
        d["layer_cell_cnt"][lev] = max(1, 2 * sum(int(r["cell_cnt"]) for r in rs))
        for a in range(L.NPIV):
            b = np.zeros((), L.bci_dt)
            b["piv_seq"], b["level"] = a, lev
            pts = sorted(bcis.get((lev, a), []), key=lambda p: p[2])   # stable: the case's order among equal bit_pos stays
            assert len(pts) <= L.BCI_MAXPTS
            bits = [0, 0, 0, 0]
            segs = []
            for k, p in enumerate(pts):
                pl, ps, bp = p[0], p[1], p[2]
                assert 1 <= pl <= 4 and 0 <= ps < 10 and 0 <= bp < 256 and bp >> 6 == pl - 1 and abs(float(p[4])) <= float(PI_F), p
                assert ps < len(rows[pl]), "a point names a stored contour"
                b["pts"][k] = (pl, ps, bp, p[3], p[4])
                bits[bp >> 6] |= 1 << (bp & 63)
                if k == 0 or pts[k - 1][2] != bp:
                    segs.append(k)
            if pts:
                segs.append(len(pts))
            b["n_pts"], b["n_segs"] = len(pts), len(segs)
            b["segs"][:len(segs)] = segs
            b["dist_bin"] = np.array(bits, np.uint64)
            d["bcis"][lev, a] = b
    return d


def accepted(oracle, desc, what):
    """oracle.Scan.from_desc took the descriptor: the rows and BCIs it then holds are those that were given"""
    s = oracle.Scan.from_desc(desc)
    assert s.h, what
    back = s.desc()[0]
    for lev in range(1, 5):
        n = int(desc["n_stored"][lev])
        assert s.ncont(lev) == n and back["n_stored"][lev] == n and back["layer_cell_cnt"][lev] == desc["layer_cell_cnt"][lev], (what, lev)
        for f in ("cell_cnt", "pos_mean", "eig_vals", "eig_vecs", "vol3_mean", "com", "ecc_feat"):
            assert back["cont"][lev][f][:n].tobytes() == desc["cont"][lev][f][:n].tobytes(), (what, lev, f)
        for a in range(6):
            g, h = desc["bcis"][lev, a], back["bcis"][lev, a]
            k, m = int(g["n_pts"]), int(g["n_segs"])
            assert h["n_pts"] == k and h["n_segs"] == m and h["dist_bin"].tobytes() == g["dist_bin"].tobytes(), (what, lev, a)
            assert h["pts"][:k].tobytes() == g["pts"][:k].tobytes() and h["segs"][:m].tobytes() == g["segs"][:m].tobytes(), (what, lev, a)
            assert (np.diff(g["pts"]["bit_pos"][:k].astype(int)) >= 0).all(), (what, lev, a)
    return s


# ---- R2: the numpy restatement --------------------------------------------------------------------------------------------
def _perc(a, b, p):
    with np.errstate(invalid="ignore", divide="ignore"):
        return bool(np.abs(F(F(a - b) / max(a, b))) > p)   # max(NaN-free operands); a NaN quotient compares false


def r2_check_sim(a, b, sim):
    """ContourView::checkSim (contour.h:278-329), every operation rounded in f32 as cc_check_sim writes it"""
    ca, cb = F(a["cell_cnt"]), F(b["cell_cnt"])
    if _perc(ca, cb, F(sim.tp_cell_cnt)) and abs(F(ca - cb)) > F(sim.ta_cell_cnt):
        return False
    for k in (1, 0):
        ea, eb = F(a["eig_vals"][k]), F(b["eig_vals"][k])
        if max(ea, eb) > F(2.0) and _perc(np.sqrt(ea), np.sqrt(eb), F(sim.tp_eigval)):
            return False
    if max(int(a["cell_cnt"]), int(b["cell_cnt"])) > 15 and abs(F(F(a["vol3_mean"]) - F(b["vol3_mean"]))) > F(sim.ta_h_bar):
        return False
    r = []
    for c in (a, b):
        x, y = F(c["com"][0] - c["pos_mean"][0]), F(c["com"][1] - c["pos_mean"][1])
        r.append(np.sqrt(F(F(x * x) + F(y * y))))
    if abs(F(r[0] - r[1])) > F(sim.ta_rcom) and _perc(r[0], r[1], F(sim.tp_rcom)):
        return False
    return True


def _ring(b):
    return sum(int(b["dist_bin"][w]) << (64 * w) for w in range(4))


def r2_pairs(bs, bt):
    """the potential pairs of BCI::checkConstellSim in generation order: [(level, seq_src, seq_tgt)], keys f32 after clampAng"""
    ns, nt = int(bs["n_pts"]), int(bt["n_pts"])
    sp, tp = bs["pts"][:ns], bt["pts"][:nt]
    return pairs_of([(int(p["level"]), int(p["seq"]), int(p["bit_pos"]), 0.0, F(p["theta"])) for p in sp],
                    [(int(p["level"]), int(p["seq"]), int(p["bit_pos"]), 0.0, F(p["theta"])) for p in tp])


def pairs_of(sp, tp):
    """r2_pairs on two lists of pt() in table order (ascending bit_pos)"""
    ids, keys = [], []
    for tl, tq, tb, _, tth in tp:
        for sl, sq, sb, _, sth in sp:
            if tb - 1 <= sb <= tb + 1:
                od = np.float64(F(tth - sth))
                od = F(od - math.floor((od + math.pi) / (2 * math.pi)) * 2 * math.pi)
                ids.append((sl, sq, tq))
                keys.append(od)
    return ids, np.array(keys, F)


def r2_window(keys):
    """the two-pointer loop of contour_mng.h:344-357 on the sorted keys -> (longest, its start)"""
    n = len(keys)
    k = np.sort(keys).astype(np.float64)
    rng = float(RANGE_F)
    beg, longest, p1, p2 = 0, 1, 0, 0
    while p1 < n:
        if float(F(F(k[p2 % n]) - F(k[p1]))) + 2 * math.pi * (p2 // n) > rng:
            p1 += 1
        else:
            if p2 - p1 + 1 > longest:
                longest, beg = p2 - p1 + 1, p1
            p2 += 1
    return longest, beg


def r2_check(src, tgt, lev, s, t, sim, lb):
    """-> dict(anchor, ovlp_sum, max_one, npp, in_ang_rng, beg, indiv_sim, scores [4] as the reference would report them)"""
    o = dict(anchor=False, ovlp_sum=0, max_one=0, npp=-1, in_ang_rng=0, beg=0, indiv_sim=0, keys=None)
    o["anchor"] = r2_check_sim(src["cont"][lev][s], tgt["cont"][lev][t], sim)
    if o["anchor"]:
        bs, bt = src["bcis"][lev, s], tgt["bcis"][lev, t]
        S, T = _ring(bs), _ring(bt)
        m = (1 << 256) - 1
        ov = [bin(S & T).count("1"), bin((S << 1) & m & T).count("1"), bin((S >> 1) & T).count("1")]
        o["ovlp_sum"], o["max_one"] = sum(ov), max(ov)
        if o["ovlp_sum"] >= lb.i_ovlp_sum and o["max_one"] >= lb.i_ovlp_max_one:
            ids, keys = r2_pairs(bs, bt)
            o["npp"], o["keys"], o["ids"] = len(ids), keys, ids
            o["in_ang_rng"], o["beg"] = r2_window(keys)
            if o["in_ang_rng"] >= lb.i_in_ang_rng:
                order = np.argsort(keys, kind="stable")
                n = len(ids)
                win = [ids[order[(o["beg"] + e) % n]] for e in range(o["in_ang_rng"])] + [(lev, s, t)]
                o["window"] = win[:-1]
                o["indiv_sim"] = sum(r2_check_sim(src["cont"][l_][a_], tgt["cont"][l_][b_], sim) for l_, a_, b_ in win)
            if len(ids) and len(set(keys[:PP_MAX].tolist())) == min(len(ids), PP_MAX):
                o.update(r2_tie_free(src, tgt, lev, s, t, sim, lb, ids, keys))
    o["scores"] = [o["ovlp_sum"], o["max_one"], o["in_ang_rng"], o["indiv_sim"]]
    # the device's capacities: CC_PP_MAX potential pairs, CC_CSTL_MAX entries of a window that goes on to stage B2
    o["capped"] = o["npp"] > PP_MAX or (o["in_ang_rng"] >= lb.i_in_ang_rng and o["in_ang_rng"] + 1 > CSTL_MAX)
    return o


_acosf = C.CDLL("libm.so.6").acosf    # glibc's acosf, the reference's std::acos(float)
_acosf.restype, _acosf.argtypes = C.c_float, [C.c_float]


def _nrm(x, y):
    return np.sqrt(F(F(x * x) + F(y * y)))


def _unit(x, y):
    z = F(F(x * x) + F(y * y))
    if z > 0:
        q = np.sqrt(z)
        return F(x / q), F(y / q)
    return x, y


def r2_b2(src, tgt, cstl_in, sim, lb):
    """checkConstellCorrespSim (contour_mng.h:1124-1242) in the reference's sequential form, f32 as written, on a cstl_in list
    whose ORDER is known -> (i_indiv_sim, i_orie_sim, cstl_out or None when a bar ended it)"""
    out = [p for p in cstl_in if r2_check_sim(src["cont"][p[0]][p[1]], tgt["cont"][p[0]][p[2]], sim)]
    if len(out) < lb.i_indiv_sim:
        return len(out), 0, None
    indiv = len(out)
    ps = lambda d, p, k: d["cont"][p[0]][p[k]]["pos_mean"]
    sh_s, sh_t = (F(0), F(0)), (F(0), F(0))
    for i in range(1, min(len(out), 10)):
        for j in range(i):
            a, b = ps(src, out[i], 1), ps(src, out[j], 1)
            cx, cy = F(a[0] - b[0]), F(a[1] - b[1])
            if _nrm(cx, cy) > _nrm(*sh_s):
                sh_s = _unit(cx, cy)
                a, b = ps(tgt, out[i], 2), ps(tgt, out[j], 2)
                sh_t = _unit(F(a[0] - b[0]), F(a[1] - b[1]))
    pi6 = F(math.pi / 6)
    n, i = len(out), 0
    while i < n:
        sc1, tc1 = src["cont"][out[i][0]][out[i][1]], tgt["cont"][out[i][0]][out[i][2]]
        if sc1["ecc_feat"] and tc1["ecc_feat"]:
            th_s = F(_acosf(F(F(sh_s[0] * sc1["eig_vecs"][2]) + F(sh_s[1] * sc1["eig_vecs"][3]))))
            th_t = F(_acosf(F(F(sh_t[0] * tc1["eig_vecs"][2]) + F(sh_t[1] * tc1["eig_vecs"][3]))))
            if abs(F(th_s - th_t)) > pi6 and abs(F(F(math.pi - np.float64(th_s)) - th_t)) > pi6:
                out[i], out[n - 1] = out[n - 1], out[i]
                n -= 1
                continue
        i += 1
    out = out[:n]
    return indiv, n, (out if n >= lb.i_orie_sim else None)


def r2_tie_free(src, tgt, lev, s, t, sim, lb, ids, keys):
    """a check whose keys are all distinct: the sorted order is known, so R2 goes on through stage B2 -- and states the DEVICE's
    outcome where a capacity cuts the check: the first CC_PP_MAX pairs in generation order, their window, its first 63 entries in
    sorted order and the anchor pair.  -> dict(orie_sim, passed, cstl_out; dev = the same under the device's capacities)"""
    o = {}
    for name, cap in (("ref", False), ("dev", True)):
        k, d = (keys[:PP_MAX], ids[:PP_MAX]) if cap else (keys, ids)
        longest, beg = r2_window(k)
        r = dict(in_ang_rng=longest, indiv_sim=0, orie_sim=0, passed=0, cstl=None)
        if longest >= lb.i_in_ang_rng:
            order = np.argsort(k, kind="stable")
            win = [d[order[(beg + e) % len(d)]] for e in range(longest)]
            if cap and longest + 1 > CSTL_MAX:
                win = win[:CSTL_MAX - 1]
            r["indiv_sim"], r["orie_sim"], r["cstl"] = r2_b2(src, tgt, win + [(lev, s, t)], sim, lb)
            r["passed"] = int(r["cstl"] is not None)
        o[name] = r
    return dict(tie_free=o)


# ---- T_pass: the closed form at 50 digits and its bound -----------------------------------------------------------------
def pair_points(src, tgt, pairs):
    S = np.array([src["cont"][l_][a_]["pos_mean"] for l_, a_, _ in pairs], np.float64)
    T = np.array([tgt["cont"][l_][b_]["pos_mean"] for l_, _, b_ in pairs], np.float64)
    return S, T


def tf_exact(S, T):
    """getTFFromConstell's closed form (x, y, theta) and nrm at 50 digits"""
    with mp.workdps(50):
        n = len(S)
        sx, sy = mp.fsum(map(mp.mpf, S[:, 0])) / n, mp.fsum(map(mp.mpf, S[:, 1])) / n
        dx, dy = mp.fsum(map(mp.mpf, T[:, 0])) / n, mp.fsum(map(mp.mpf, T[:, 1])) / n
        s = [mp.mpf(0)] * 4
        for (ax, ay), (bx, by) in zip(S, T):
            a0, a1, b0, b1 = mp.mpf(ax) - sx, mp.mpf(ay) - sy, mp.mpf(bx) - dx, mp.mpf(by) - dy
            s = [s[0] + b0 * a0, s[1] + b0 * a1, s[2] + b1 * a0, s[3] + b1 * a1]
        sn, cs = (s[2] - s[1]) / n, (s[0] + s[3]) / n
        nrm = mp.sqrt(sn * sn + cs * cs)
        r00, r10 = (cs / nrm, sn / nrm) if nrm > 0 else (mp.mpf(1), mp.mpf(0))
        return (float(dx - (r00 * sx - r10 * sy)), float(dy - (r10 * sx + r00 * sy)), float(mp.atan2(r10, r00))), float(nrm)


def tf_bound(S, T, nrm):
    """(bound on |x|, |y| error, bound on the angle error) of an f64 evaluation of the closed form in ANY summation order.
    Running error analysis, first order in U = 2^-53 with (1 + U)^k <= 1 + 1.01 k U for the k <= 200 used here.  Ma, Mb: the
    largest |coordinate| of the src / tgt centres; Da, Db: the largest |centre - mean| per side (from the data).
      a mean of n values: n - 1 additions and a product with 1/n (two roundings): |mean' - mean| <= (n + 2) U M =: da (db)
      a centred value a_i - mean' = A_i - ca + ra_i: A_i the true centred value, ca the mean's error (|ca| <= da, THE SAME for every
        i), ra_i the subtraction's rounding, |ra_i| <= U (Da + da)
      a covariance sum: sum (B_i - cb + rb_i)(A_i - ca + ra_i); the true centred values sum to zero, so the common errors leave
        only n ca cb, and the rest is sum (B_i ra_i + A_i rb_i), n product roundings U Da' Db' (Da' = Da + da ...) and n - 1 additions
        of partial sums <= n Da' Db'; the 1/n adds two roundings: per entry
        e_s <= da db + U (Db Da' + Da Db') + (n + 2) U Da' Db'
        -- this is what keeps the bound meaningful when the tgt centres nearly coincide (Db ~ 1e-6, nrm ~ 1e-6)
      sn = s10 - s01, cs = s00 + s11: e_v <= 2 e_s + U (2 Da' Db')
      nrm = sqrt(sn^2 + cs^2): relative error <= e_v sqrt2 / nrm + 3 U
      r00 = cs / nrm, r10 = sn / nrm: e_r <= e_v / nrm + (e_v sqrt2 / nrm + 4 U)        -- the 1 / nrm amplification
      theta = atan2(r10, r00): the direction (sn, cs) is off by at most e_v sqrt2 / nrm radians (scaling both by 1 / nrm does not
        turn it; the two divisions add 2 U), atan2 itself ATAN2_ULP ulp of a value <= pi: e_th <= e_v sqrt2 / nrm + 2 U + ATAN2_ULP * 2^-51
      t = dm - R sm: |err| <= db + 2 (e_r Ma + da + 3 U Ma) + 2 U (Mb + 2 Ma)"""
    n = len(S)
    Ma, Mb = float(max(np.abs(S).max(), 1.0)), float(max(np.abs(T).max(), 1.0))
    Da, Db = float(np.abs(S - S.mean(0)).max()), float(np.abs(T - T.mean(0)).max())
    da, db = (n + 2) * U * Ma, (n + 2) * U * Mb
    Da1, Db1 = Da + 2 * da, Db + 2 * db      # (twice: Da, Db themselves are computed from a rounded mean)
    e_s = da * db + U * (Db1 * Da1 + Da1 * Db1) + (n + 2) * U * Da1 * Db1
    e_v = 2 * e_s + U * 2 * Da1 * Db1
    if not nrm > 0:
        return float("inf"), float("inf")
    e_dir = e_v * math.sqrt(2) / nrm
    e_r = e_v / nrm + e_dir + 4 * U
    e_th = e_dir + 2 * U + ATAN2_ULP * 2.0 ** -51
    e_t = db + 2 * (e_r * Ma + da + 3 * U * Ma) + 2 * U * (Mb + 2 * Ma)
    return 1.01 * e_t, 1.01 * e_th


def check_tf(tf, src, tgt, pairs, what):
    """tf against the 50-digit closed form on `pairs` -> the largest error / bound"""
    S, T = pair_points(src, tgt, pairs)
    ex, nrm = tf_exact(S, T)
    bt, ba = tf_bound(S, T, nrm)
    et = max(abs(tf[0] - ex[0]), abs(tf[1] - ex[1]))
    ea = abs(math.remainder(tf[2] - ex[2], 2 * math.pi))
    assert et <= bt and ea <= ba, (what, "T_pass", tuple(tf), ex, "errors", et, ea, "bounds", bt, ba, "nrm", nrm)
    return max(et / bt, ea / ba), nrm


# ---- slots and scenes -----------------------------------------------------------------------------------------------------
class Slot:
    """one case.  src_row / tgt_row: changes to the anchor row (dicts); src_bci / tgt_bci: point lists; expect: assertions on the
    references -- anchor (bool), ovlp (sum, max), npp, win, beg, keep (the check gets past the popcount bars), capped"""

    def __init__(self, name, src_row=None, tgt_row=None, src_bci=None, tgt_bci=None, **expect):
        self.name, self.src_row, self.tgt_row = name, src_row or {}, tgt_row or {}
        self.src_bci, self.tgt_bci, self.expect = src_bci, tgt_bci, expect


class Scene:
    def __init__(self, name, tgt, srcs, hints, slots, lb=None, sim=None):
        self.name, self.tgt, self.srcs, self.slots = name, tgt, srcs, slots   # slots[i] belongs to hints[i] (None: a repeat)
        self.hints = np.asarray(hints, np.int32).reshape(-1, 4)                  # (index into srcs, level, seq_src, seq_tgt)
        self.lb, self.sim = lb, sim
        self.base = None   # index of srcs[0] in the back end's database
        self.share = None  # a scene on another scene's scans
        self.expect = {}


def thresholds(L, **kw):
    lb, ub = L.default_thresholds()
    for k, v in kw.items():
        setattr(lb, k, v)
    return lb, ub


DEFAULT_BCI = [pt(1, 6, 20, 0.0), pt(1, 7, 24, 0.25), pt(1, 8, 28, 0.5), pt(2, 6, 64 + 20, 0.75), pt(2, 7, 64 + 24, 1.0)]


def pack(L, name, slots, seed, tf=(3.0, -2.0, 0.3), jitter=0.0, ecc=0, lb=None, rows_fn=None):
    """scenes of up to 24 slots each: slot k of a scan pair sits at (level 1 + k // 6, anchor k % 6)"""
    scenes = []
    for s0 in range(0, len(slots), 24):
        part = slots[s0:s0 + 24]
        rs, rt = plain_rows(seed, jitter=0.0, ecc=ecc), plain_rows(seed, tf, jitter, ecc=ecc)
        if rows_fn:
            rows_fn(rs, rt)
        bs, bt, hints = {}, {}, []
        for k, sl in enumerate(part):
            lev, a = 1 + k // 6, k % 6
            rs[lev][a] = dict(rs[lev][a], **sl.src_row)
            rt[lev][a] = dict(rt[lev][a], **sl.tgt_row)
            bs[(lev, a)] = DEFAULT_BCI if sl.src_bci is None else sl.src_bci
            bt[(lev, a)] = DEFAULT_BCI if sl.tgt_bci is None else sl.tgt_bci
            hints.append((0, lev, a, a))
        scenes.append(Scene("%s/%d" % (name, s0 // 24), make_scan(L, rt, bt), [make_scan(L, rs, bs)], hints, list(part), lb=lb))
    return scenes


# ---- A. the anchor gate and the popcounts -------------------------------------------------------------------------------
def gate_slots():
    S = []

    def add(name, a, b, ok):
        S.append(Slot(name, a, b, anchor=ok))
    # cell_cnt: fails when |d| / max > 0.2 AND |d| > 6 (both strict)
    add("cells perc on the bar (10/50)", dict(cell_cnt=40), dict(cell_cnt=50), True)
    add("cells perc over (11/51)", dict(cell_cnt=40), dict(cell_cnt=51), False)
    add("cells perc under (9/49)", dict(cell_cnt=40), dict(cell_cnt=49), True)
    add("cells delta on the bar (6, perc over)", dict(cell_cnt=20), dict(cell_cnt=26), True)
    add("cells delta over (7, perc over)", dict(cell_cnt=27), dict(cell_cnt=20), False)
    add("cells delta under (5)", dict(cell_cnt=20), dict(cell_cnt=25), True)
    # eigenvalues: sqrt ratio against 0.2, only when max(eig) > 2.0f
    for k, nm in ((1, "major"), (0, "minor")):
        def e(v, k=k):
            return dict(eig_vals=F([v, 30.0]) if k == 0 else F([1.0, v]))
        o = dict(eig_vals=F([16.0, 30.0]) if k == 0 else F([1.0, 16.0]))
        add("eig %s on the bar (4 : 5)" % nm, e(25.0), o, True)
        add("eig %s over (26)" % nm, e(26.0), o, False)
        add("eig %s under (24)" % nm, o, e(24.0), True)
        lo = dict(eig_vals=F([0.5, 30.0]) if k == 0 else F([0.25, 0.5]))
        add("eig %s switch at 2.0: off" % nm, dict(eig_vals=F([2.0, 30.0]) if k == 0 else F([0.25, 2.0])), lo, True)
        add("eig %s switch one float over 2.0: on" % nm, dict(eig_vals=F([nf(2.0), 30.0]) if k == 0 else F([0.25, nf(2.0)])), lo, False)
    # mean height: only when max(cell_cnt) > 15
    add("height switch at 15: off", dict(cell_cnt=15, vol3_mean=F(3.0)), dict(cell_cnt=14, vol3_mean=F(1.0)), True)
    add("height switch at 16: on", dict(cell_cnt=14, vol3_mean=F(3.0)), dict(cell_cnt=16, vol3_mean=F(1.0)), False)
    add("height on the bar", dict(vol3_mean=F(0.0)), dict(vol3_mean=F(0.3)), True)
    add("height one float over", dict(vol3_mean=nf(0.3)), dict(vol3_mean=F(0.0)), False)
    add("height one float under", dict(vol3_mean=F(0.0)), dict(vol3_mean=nf(0.3, False)), True)
    # centre of mass: fails when |r1 - r2| > 0.4 AND perc > 0.25
    z = F([0.0, 0.0])

    def com(r):
        return dict(pos_mean=z, com=F([r, 0.0]))
    add("com delta on the bar", com(0.0), com(F(0.4)), True)
    add("com delta one float over", com(nf(0.4)), com(0.0), False)
    add("com delta one float under", com(0.0), com(nf(0.4, False)), True)
    add("com perc on the bar (1/4)", com(3.0), com(4.0), True)
    add("com perc one float over", com(3.0), com(nf(4.0)), False)
    add("com perc one float under", com(nf(4.0, False)), com(3.0), True)
    # NaN quotients
    add("cell_cnt 0 on both sides", dict(cell_cnt=0), dict(cell_cnt=0), None)
    add("com == pos_mean on both sides", com(0.0), com(0.0), None)
    return S


def ring_slots():
    """bits whose shifted ANDs carry across the 64-bit words, and drop at both ends"""
    S = []

    def add(name, sb, tb, ovlp):
        lev = lambda b: (b >> 6) + 1
        S.append(Slot(name, src_bci=[pt(lev(b), 6 + i % 4, b, 0.1 * i) for i, b in enumerate(sb)],
                      tgt_bci=[pt(lev(b), 6 + i % 4, b, 0.1 * i) for i, b in enumerate(tb)], ovlp=ovlp))
    for w in (63, 127, 191):
        add("src %d, tgt %d: the shl carries" % (w, w + 1), [w], [w + 1], (1, 1))
        add("src %d, tgt %d: the shr carries" % (w + 1, w), [w + 1], [w], (1, 1))
        add("src %d %d, tgt both" % (w, w + 1), [w, w + 1], [w, w + 1], (4, 2))
    add("src 0, tgt 0 1", [0], [0, 1], (2, 1))
    add("src 0 1, tgt 0: bit 0 shifted right drops", [0, 1], [0], (2, 1))
    add("src 255, tgt 254 255", [255], [254, 255], (2, 1))
    add("src 254 255, tgt 255: bit 255 shifted left drops", [254, 255], [255], (2, 1))
    add("src 0 255, tgt 0 255: no wrap around the ring", [0, 255], [0, 255], (2, 2))
    add("every word's ends", [0, 63, 64, 127, 128, 191, 192, 255], [0, 63, 64, 127, 128, 191, 192, 255], (14, 8))
    add("no common bit", [10, 70], [13, 73], (0, 0))
    return S


def a_classes():
    """CC_A_CLASSES, the overlap counts that separate stage A's four size classes, read from the host code that sets them"""
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "contour-context_amd", "csrc", "cc_db_api.inc")).read()
    m = re.search(r"int a_class\[3\] = \{(\d+), (\d+), (\d+)\}", txt)
    assert m, "csrc/cc_db_api.inc: the line `int a_class[3] = {a, b, c};` (CC_A_CLASSES) was not found"
    return tuple(int(v) for v in m.groups())


def class_slots():
    """keepers on both sides of every size-class border (ovlp_sum 7 | 8, 13 | 14, 21 | 22 under the shipped 8, 14, 22) and anchors that
    fail: a run of n consecutive ring bits on both sides gives ovlp_sum 3 n - 2, an isolated common bit one more"""
    S = []
    for run, iso in ((3, 0), (3, 1), (5, 0), (5, 1), (7, 2), (8, 0), (10, 0), (2, 1)) * 2:
        b = [pt(1, q, 20 + q, 0.01 * q) for q in range(run)] + [pt(2, q, 64 + 10 + 5 * q, 0.0) for q in range(iso)]
        S.append(Slot("run of %d bits + %d apart" % (run, iso), src_bci=b, tgt_bci=b, ovlp=(3 * run - 2 + iso, run + iso)))
    for k in range(8):
        S.append(Slot("anchor fails %d" % k, dict(cell_cnt=40), dict(cell_cnt=51), anchor=False))
    return S


# ---- B. pair counts and key orders -----------------------------------------------------------------------------------------
COUNTS = (0, 1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 100, 255, 256, 257, 400)


def _split(n):
    """n = sum over the four layers of a_l * b_l with a_l, b_l <= 10 -> [(a_l, b_l)]"""
    best = None
    prods = sorted({**{(a * b): (a, b) for a in range(11) for b in range(a + 1)}, 0: (3, 0)}.items(), reverse=True)

    def rec(left, k, acc):
        nonlocal best
        if best is not None:
            return
        if k == 4:
            if left == 0:
                best = list(acc)
            return
        for p, ab in prods:
            if p <= left and p * (4 - k) >= left:
                rec(left - p, k + 1, acc + [ab])
    rec(n, 0, [])
    assert best is not None, n
    return best


def count_bcis(n, key_fn, flip=False):
    """src and tgt point lists with exactly n potential pairs: layer l holds a_l src and b_l tgt points in one bin.  The pair
    (tgt i, src j) of the generation order gets key_fn(running pair index) where one side of a layer has a single point (the
    key is then free per pair), else theta_t - theta_s of grid angles."""
    sb, tb, k = [], [], 0
    for l_, (a, b) in enumerate(_split(n)):
        if flip:
            a, b = b, a
        bp = 64 * l_ + 30
        if a == 0 or b == 0:
            # a layer without pairs still carries points: far bins, partners none
            sb += [pt(l_ + 1, q, 64 * l_ + 5, 0.0) for q in range(a)]
            tb += [pt(l_ + 1, q, 64 * l_ + 50, 0.0) for q in range(b)]
            continue
        if b == 1:
            tb.append(pt(l_ + 1, 0, bp, 0.0))
            sb += [pt(l_ + 1, q, bp, -key_fn(k + q)) for q in range(a)]
        elif a == 1:
            sb.append(pt(l_ + 1, 0, bp, 0.0))
            tb += [pt(l_ + 1, q, bp, key_fn(k + q)) for q in range(b)]
        else:
            sb += [pt(l_ + 1, q, bp, -key_fn(k + q) / 2) for q in range(a)]
            tb += [pt(l_ + 1, q, bp, key_fn(k + 7 * q + 3) / 2) for q in range(b)]
        k += a * b
    return sb, tb


def b1_bin(od):
    """cc_b1_bin: the orientation bin of the counting sort, in f32"""
    return min(255, max(0, int(F(F(F(od) + F(3.14159274)) * F(40.7436638)))))


G64 = 1.0 / 64   # grid of exactly representable angles: sums and differences are exact, ties are exact


def key_orders():
    return {
        "equal": lambda k: 0.25,
        "two values": lambda k: 0.25 + G64 * (k % 2),
        "runs": lambda k: G64 * 20 * ((k // 7) % 5),              # runs of 7 ties over five values a window apart: ties lie across every cut
        "descending": lambda k: 1.5 - G64 * (k % 190),
        "organ pipe": lambda k: G64 * min(k % 64, 63 - k % 64),
        "scattered": lambda k: G64 * (((k * 37) % 101) - 50) * 3,  # spread over +-2.4 rad: many counting-sort bins
        "narrow": lambda k: G64 * ((k * 5) % 12),                  # all inside one pi/16 window: the window is the whole list
    }


def sort_slots():
    S = []
    for n in COUNTS:
        for nm in (("equal", "runs", "scattered", "narrow") if n not in (17, 49, 65, 257) else tuple(key_orders())):
            if n == 0 and nm != "equal":
                continue
            sb, tb = count_bcis(n, key_orders()[nm], flip=(n % 2 == 1))
            win = r2_window(pairs_of(sorted(sb, key=lambda p: p[2]), sorted(tb, key=lambda p: p[2]))[1])[0]
            ex = dict(npp=n, capped=(n > PP_MAX or win + 1 > CSTL_MAX) or None)
            if nm in ("equal", "narrow") and 0 < n <= PP_MAX:
                ex["win"] = n
            S.append(Slot("%d pairs, %s keys" % (n, nm), src_bci=sb, tgt_bci=tb, **ex))
    # all keys distinct (key = (100 l + 10 i + j) / 2048, or its negative): R2 knows the order and judges stage B2 as well, and at
    # 64 (longest + 1 = 65), 257 and 400 pairs states what the device's cut leaves, for equality
    for n in (17, 49, 63, 64, 100, 257, 400):
        for sgn in ((1, -1) if n in (49, 64, 257) else (1,)):
            sb, tb = [], []
            for l_, (a_, b_) in enumerate(_split(n)):
                if a_ and b_:
                    sb += [pt(l_ + 1, j, 64 * l_ + 30, -sgn * j / 2048.0) for j in range(a_)]
                    tb += [pt(l_ + 1, i, 64 * l_ + 30, sgn * (100 * l_ + 10 * i) / 2048.0) for i in range(b_)]
            S.append(Slot("%d pairs, distinct %s keys" % (n, "ascending" if sgn > 0 else "descending"), src_bci=sb, tgt_bci=tb, npp=n,
                          capped=(n >= CSTL_MAX) or None, tie_free=True))
    # the depth-limit fallback: key sequences found by the adversary of tests/introsort_adversary.py, on which the restated introsort
    # loop runs out of its 2 floor(log2 n) partitions with more than 16 elements left (asserted).  40 free keys, all inside one
    # window, with ties laid over them: the constellation's order is whatever std::sort's heapsort and insertion sort leave
    import introsort_adversary as IA
    for n in (37, 40):
        v = IA.adversary(n)
        for nm, f in IA.TIES.items():
            k = [f(x, n) for x in v]
            if not IA.deep_on(k):
                continue
            sb, tb = _fan([x / 256.0 for x in k])
            S.append(Slot("deep: %d keys, %s" % (n, nm), src_bci=sb, tgt_bci=tb, npp=n, win=n, deep=True))
    assert sum(bool(x.expect.get("deep")) for x in S) >= 10
    # point tables of 1, 2, 39 and 40 entries: the 12-byte entries are read as 8-byte words
    for ns, nt in ((1, 1), (2, 1), (1, 2), (39, 40), (40, 39), (40, 40), (39, 39), (2, 40), (40, 1)):
        def tab(m, sgn):
            return [pt(1 + q // 10, q % 10, 64 * (q // 10) + 3 * (q % 10) + 2, sgn * G64 * ((q * 11) % 9)) for q in range(m)]
        S.append(Slot("tables of %d and %d points" % (ns, nt), src_bci=tab(ns, -1), tgt_bci=tab(nt, 1), npp=min(ns, nt)))
    # a tgt point whose partners are none, one whose partners are the whole src table
    S.append(Slot("partners: none and all", src_bci=[pt(1, q, 30 + q % 3, -G64 * q) for q in range(10)],
                  tgt_bci=[pt(1, 0, 10, 0.0), pt(1, 1, 31, 0.0), pt(1, 2, 60, 0.5)], npp=10))
    # bit_pos 63 (layer 1) next to 64 (layer 2): the +-1 rule pairs across layers; the pair carries the src level and the tgt seq
    S.append(Slot("pairs across the layer border 63 | 64", src_bci=[pt(1, 1, 62, 0.0), pt(1, 2, 63, 0.0), pt(1, 3, 63, G64), pt(2, 4, 64, 0.0), pt(2, 5, 65, 0.0)],
                  tgt_bci=[pt(1, 6, 63, 0.0), pt(2, 7, 64, G64), pt(2, 8, 64, 0.0)], npp=4 + 4 + 4))
    # clampAng's three branches: theta_t - theta_s at exactly +-pi (f32) and one float inside; -0 and +0 differences
    pi_in = nf(PI_F, False)
    S.append(Slot("differences at +-pi and +-0", src_bci=[pt(1, q, 30, v) for q, v in enumerate((0.0, -0.0, float(PI_F), -float(PI_F), float(pi_in), -float(pi_in)))],
                  tgt_bci=[pt(1, 0, 30, 0.0), pt(1, 1, 30, -0.0), pt(1, 2, 31, float(PI_F)), pt(1, 3, 31, -float(PI_F))], npp=24))
    # keys on both sides of a counting-sort bin edge and in bins 0 and 255 (the large instance: 90 pairs)
    edge = [-float(PI_F), -3.14, float(PI_F), 3.14, float(nf(PI_F, False)), 0.0]
    for b in (1, 64, 128, 129, 200, 255):
        x, hi = F(b / 40.7436638 - math.pi - 1e-3), F(b / 40.7436638 - math.pi + 1e-3)
        assert b1_bin(x) == b - 1 and b1_bin(hi) == b
        while nf(x) != hi:          # bisection on the floats: x stays in bin b - 1, hi in bin b
            m = F((np.float64(x) + np.float64(hi)) / 2)
            m = m if x < m < hi else nf(x)
            x, hi = (m, hi) if b1_bin(m) < b else (x, m)
        assert b1_bin(x) == b - 1 and b1_bin(nf(x)) == b
        edge += [float(x), float(nf(x)), float(nf(x)), float(x)]
    assert len(edge) == 30
    sb, tb = [], []
    for l_ in range(3):
        sb += [pt(l_ + 1, 0, 64 * l_ + 30, 0.0), pt(l_ + 1, 1, 64 * l_ + 30, 0.0), pt(l_ + 1, 2, 64 * l_ + 31, 0.0)]
        tb += [pt(l_ + 1, q, 64 * l_ + 30, edge[10 * l_ + q]) for q in range(10)]
    S.append(Slot("bin edges, bins 0 and 255", src_bci=sb, tgt_bci=tb, npp=90))
    return S


# ---- C. the window -----------------------------------------------------------------------------------------------------------
def _fan(keys, extra_src=(), extra_tgt=()):
    """one tgt point per layer against up to 10 src points: up to 40 potential pairs with the given keys, in this order"""
    assert len(keys) <= 40
    sb, tb = list(extra_src), list(extra_tgt)
    for l_ in range((len(keys) + 9) // 10):
        tb.append(pt(l_ + 1, 0, 64 * l_ + 30, 0.0))
        sb += [pt(l_ + 1, q, 64 * l_ + 30, -float(F(keys[10 * l_ + q]))) for q in range(min(10, len(keys) - 10 * l_))]
    return sb, tb


def window_slots(lb_rng=3):
    S = []

    def add(name, keys, **ex):
        sb, tb = _fan(keys)
        S.append(Slot(name, src_bci=sb, tgt_bci=tb, npp=len(keys), **ex))
    far = [1.0, 2.0, -1.0, -2.0]
    add("window of 1", far, win=1, beg=0)
    add("window of lb - 1", far + [0.1] * (lb_rng - 1), win=lb_rng - 1)
    add("window of lb", far + [0.1] * lb_rng, win=lb_rng)
    add("window of lb + 1", far + [0.1] * (lb_rng + 1), win=lb_rng + 1)
    add("window is the whole list", [G64 * (q % 12) for q in range(40)], win=40, beg=0)
    add("two windows of equal length: the first start wins", [1.0, 1.01, 1.02, -1.0, -1.01, -1.02, 2.5], win=3, beg=0)
    add("two windows of equal length, given in descending order", [2.5, 1.02, 1.01, 1.0, -1.0, -1.01, -1.02][::-1], win=3, beg=0)
    # a non-wrapping difference of exactly (float)(pi / 16) and its two neighbours: `>` keeps the exact one in
    r = float(RANGE_F)
    add("difference exactly pi/16: in", [0.0, 0.05, r, 1.0], win=3, beg=0)
    add("difference one float over pi/16: out", [0.0, 0.05, float(nf(RANGE_F)), 1.0], win=2, beg=0)
    add("difference one float under pi/16: in", [0.0, 0.05, float(nf(RANGE_F, False)), 1.0], win=3, beg=0)
    # a window that wraps past the end: keys near +pi and near -pi; the f32 difference last - first sits at CC_B1_WRAP_T
    for nm, d, win in (("at", WRAP_T, 2), ("one float under", nf(WRAP_T, False), 4), ("one float over", nf(WRAP_T), 2)):
        hi = F(3.0)
        lo = F(hi + d)                     # both sums are exact: lo - hi == d, asserted
        assert F(lo - hi) == d, (nm, lo, hi, d)
        # sorted: lo lo -1 0.5 1.5 hi hi.  The window that starts at the first hi takes both lo (length 4) if and only if the
        # wrapped difference lo - hi passes the test; otherwise the longest is 2 and the first start (lo, index 0) wins
        add("wrapping window, last difference %s CC_B1_WRAP_T" % nm, [float(lo), float(lo), 0.5, float(hi), float(hi), -1.0, 1.5],
            wrap=float(d), win=win, beg=5 if win == 4 else 0)
    add("wrapping window of 4 over a plain one of 3", [3.1, 3.12, -3.1, -3.12, 0.0, 0.01, 0.02], win=4, beg=5)
    return S


def cap_slots():
    """longest + 1 equal to 63, 64 and 65, the constellation cap: 62, 63 and 64 equal keys beside a few far ones"""
    # (six plain slots first: the cap slots then sit on level-2 anchors, whose pair (2, a, a) is not among the level-1 and level-4
    # window pairs -- the anchor pair is in a capped set only if the cut kept it)
    S = [Slot("plain slot %d" % k) for k in range(6)]
    for longest in (62, 63, 64):
        sb, tb = count_bcis(longest, lambda k: 0.25)
        sb, tb = sb + [pt(4, 8, 192 + 50, -2.0), pt(4, 9, 192 + 50, 1.0)], tb + [pt(4, 9, 192 + 50, 0.0)]
        S.append(Slot("longest + 1 = %d" % (longest + 1), src_row=dict(ecc_feat=0), src_bci=sb, tgt_bci=tb, npp=longest + 2, win=longest, capped=(longest + 1 > CSTL_MAX) or None))
    # the same edge with 64 DISTINCT keys: R2 knows the order, states the cut (63 window entries, then the anchor pair) and every
    # figure, the pair set and n_pairs are held for equality -- the anchor pair (2, a, a) is in the set only if the cut kept it last
    S.append(Slot("longest + 1 = 65, distinct keys", src_row=dict(ecc_feat=0), src_bci=[pt(1, j, 30, -j / 2048.0) for j in range(8)],
                  tgt_bci=[pt(1, i, 30, 10 * i / 2048.0) for i in range(8)], npp=64, win=64, capped=True, tie_free=True))
    return S


# ---- D. stage B2 ------------------------------------------------------------------------------------------------------------
def b2_slots():
    S = []
    # ncs = i_indiv_sim - 1, i_indiv_sim, i_indiv_sim + 1: a window of 3 pairs + the anchor, of which src rows 8 and 9 of level 4
    # (b2_rows: a tenth of the cells) are similar to nothing
    for seqs, ncs in (((0, 8, 9), 2), ((0, 1, 9), 3), ((0, 1, 2), 4)):
        S.append(Slot("ncs = %d" % ncs, src_bci=[pt(4, q, 192 + 30, -0.1) for q in seqs], tgt_bci=[pt(4, 0, 192 + 30, 0.0)], npp=3, win=3, ncs=ncs))
    # the shaft scan counts only the first 10 entries: constellations of 2, 9, 10, 11 and more entries
    for n in (1, 8, 9, 10, 11, 20, 38):
        sb, tb = _fan([0.05 + G64 * (q % 3) for q in range(n)])
        S.append(Slot("constellation of %d entries" % (n + 1), src_bci=sb, tgt_bci=tb, npp=n, win=n))
    # shaft sequences where the 1.001 shortcut and the sequential scan could part (b2_rows places the centres).  Ten distinct
    # ascending keys inside one window: the constellation's entries are the src contours 0..9 of the level, in this order
    asc = [0.01 * q for q in range(10)]
    for lev, nm in ((1, "a pair of 0.7 px behind the last sure one (entries 8, 9)"), (2, "two identical centres, z == 0 (entries 8, 9)"),
                    (3, "every pair shorter than a pixel")):
        S.append(Slot("shaft: " + nm, src_bci=[pt(lev, q, 64 * (lev - 1) + 30, -float(F(asc[q]))) for q in range(10)],
                      tgt_bci=[pt(lev, 0, 64 * (lev - 1) + 30, 0.0)], npp=10, win=10))
    return S


def b2_rows_1px(rs, rt):
    """as b2_rows, the close pair of level 1 between 1 px and 1.001 px (asserted on the f32 centres): longer than the running
    unit vector, shorter than the shortcut's `sure` bar -- the scan is murky and replayed, and the pair IS taken"""
    b2_rows(rs, rt, gap=1.0005)
    for rows in (rs, rt):
        d = F(rows[1][9]["pos_mean"][0] - rows[1][8]["pos_mean"][0])
        assert rows[1][9]["pos_mean"][1] == rows[1][8]["pos_mean"][1] and F(1.0) < d < F(1.001), d


def b2_rows(rs, rt, gap=0.7):
    rs[4][8]["cell_cnt"] = rs[4][9]["cell_cnt"] = 20

    def put(rows, lev, q, p):
        rows[lev][q] = dict(rows[lev][q], pos_mean=F(p), com=F(p))
    for rows in (rs, rt):
        p8 = np.float64(rows[1][8]["pos_mean"])
        put(rows, 1, 9, p8 + [gap, 0.0])
        put(rows, 2, 9, np.float64(rows[2][8]["pos_mean"]))
        p0 = np.float64(rows[3][0]["pos_mean"])
        for q in range(1, 10):
            put(rows, 3, q, p0 + [0.09 * q, 0.05 * (q % 3)])


def acos_ladder():
    """CPU search with glibc's acosf (the reference's): the f32 dot products d around 1/2 at which the orientation test
    |acos(d) - acos(0)| > pi/6 && |(pi - acos(d)) - acos(0)| > pi/6 flips, -> (keep side [5], remove side [5]): 1, 2, 3, 5, 8 floats below
    the flip and 0, 1, 2, 4, 7 floats above it -- all within 1e-6 of the bar, far inside the device's 1e-5 switch band"""
    pi6, th_t = F(math.pi / 6), F(_acosf(F(0.0)))

    def rm(d):
        th = F(_acosf(F(d)))
        return bool(abs(F(th - th_t)) > pi6 and abs(F(F(math.pi - np.float64(th)) - th_t)) > pi6)
    lo, hi = F(0.4999), F(0.5001)
    assert not rm(lo) and rm(hi)
    while nf(lo) != hi:
        m = F((np.float64(lo) + np.float64(hi)) / 2)
        m = m if lo < m < hi else nf(lo)
        lo, hi = (lo, m) if rm(m) else (m, hi)

    def step(x, k):
        for _ in range(abs(k)):
            x = nf(x, k > 0)
        return x
    keep, drop = [step(hi, -k) for k in (1, 2, 3, 5, 8)], [step(hi, k) for k in (0, 1, 2, 4, 7)]
    assert not any(rm(d) for d in keep) and all(rm(d) for d in drop), "the test is monotone across the ladder"
    return keep, drop


def acos_rows(rs, rt):
    """level 1: ten contours in a row along x on both sides, so every shaft is (1, 0); tgt axes (0, 1): theta_t = acos(0); src axis
    (d, 0) with d from the ladder: even seqs stay by a few floats, odd seqs are removed by a few floats.  Seq 9 of the src has no
    ecc_feat: its pair stays whatever the angle."""
    keep, drop = acos_ladder()
    for q in range(10):
        d = keep[q // 2] if q % 2 == 0 else drop[q // 2]
        ps, pt_ = F([30.0 + 9 * q, 50.0]), F([30.0 + 9 * q, 60.0])
        rs[1][q] = dict(rs[1][q], pos_mean=ps, com=ps, eig_vecs=F([1.0, 0.0, d, 0.0]), ecc_feat=0 if q == 9 else 1)
        rt[1][q] = dict(rt[1][q], pos_mean=pt_, com=pt_, eig_vecs=F([1.0, 0.0, 0.0, 1.0]), ecc_feat=1)
    for a in range(6):   # the slots' anchors lie on the same lines, to the right: the shaft stays (1, 0) when the anchor pair is among the first ten
        ps, pt_ = F([200.0 + 9 * a, 50.0]), F([200.0 + 9 * a, 60.0])
        rs[2][a] = dict(rs[2][a], pos_mean=ps, com=ps)
        rt[2][a] = dict(rt[2][a], pos_mean=pt_, com=pt_)


def acos_slots():
    """the orientation filter within floats of pi/6 (slots on level-2 anchors without ecc_feat: the anchor pair always stays)"""
    S = [Slot("plain slot %d" % k) for k in range(6)]
    for nm, seqs, stay in (("all ten entries: the odd ones go, the one-sided ninth stays", list(range(10)), 5 + 1), ("the first entry goes", [1, 0, 2, 4, 6, 8], 5),
                           ("the last entry goes", [0, 2, 4, 6, 7], 4), ("all go", [1, 3, 5, 7], 0), ("all but i_orie_sim go", [0, 1, 2, 3, 4, 5, 7], 3),
                           ("none goes", [0, 2, 4, 6, 8], 5), ("ecc_feat on one side only", [0, 2, 4, 9], 4)):
        S.append(Slot("acos: " + nm, src_row=dict(ecc_feat=0), src_bci=[pt(1, q, 30, -0.01 * k) for k, q in enumerate(seqs)], tgt_bci=[pt(1, 0, 30, 0.0)],
                      npp=len(seqs), win=len(seqs), orie=stay + 1, tie_free=True))
    return S


NRM_Z = (1.0, 2.0)   # one float at 1.0 is 1.19e-7


def nrm_rows(rs, rt):
    """every tgt contour at NRM_Z, but (1, 3) one float and (1, 4) twenty floats to its right.  A constellation of the ten level-1
    src contours against ONE of those two, closed by an anchor pair whose tgt sits at NRM_Z, has the cross-covariance
    -eps (a_anchor - src mean) / n in its x row and zero in its y row: nrm = eps |a_anchor - src mean| / n, a few times eps"""
    for lev in range(1, 5):
        for q in range(10):
            z = F([_bump(F(NRM_Z[0]), {3: 1, 4: 20}.get(q, 0) if lev == 1 else 0), NRM_Z[1]])
            rt[lev][q] = dict(rt[lev][q], pos_mean=z, com=z)


def nrm_slots():
    """umeyama on either side of the nrm < 1e-6 switch (slots on level-2 anchors: the anchor's tgt is at NRM_Z)"""
    S = [Slot("plain slot %d" % k) for k in range(6)]
    for t, rng, nm in ((3, (1.5e-7, 8e-7), "just under 1e-6: the sequential branch, x and y to the oracle's bits"),
                       (4, (1.5e-6, 8e-6), "just above 1e-6: the closed form at its largest 1 / nrm")):
        S.append(Slot("nrm " + nm, src_bci=[pt(1, q, 30, -0.01 * q) for q in range(10)], tgt_bci=[pt(1, t, 30, 0.0)], npp=10, win=10, nrm=rng, tie_free=True))
    return S


def deep_rows(rs, rt):
    """rows under which the ORDER of a constellation shows in its pose: every tgt contour at one point, so the cross-covariance is
    exactly zero, nrm = 0 and both sides take the sequential sums with the identity rotation -- T = tgt mean - src mean; and src
    centres whose magnitudes span 2^7 .. 2^-53 (every other one scaled by 2^-30), so that the f64 sum of the src centres is not
    exact and its last bits depend on the order of the list.  x and y must have the oracle's bits (check_scene)."""
    one = F([70.25, 81.5])
    for lev in range(1, 5):
        for q in range(10):
            rt[lev][q] = dict(rt[lev][q], pos_mean=one, com=one)
            if q % 2:
                p = F(np.float64(rs[lev][q]["pos_mean"]) * 2.0 ** -30)
                rs[lev][q] = dict(rs[lev][q], pos_mean=p, com=p)


# ---- the table -----------------------------------------------------------------------------------------------------------------
_cache = {}


def scenes(L):
    """every scene, built once"""
    if "S" in _cache:
        return _cache["S"]
    lb1 = thresholds(L, i_ovlp_sum=0, i_ovlp_max_one=0)[0]      # the popcount bars out of the way: B1 sees every slot
    out = []
    out += pack(L, "A gate", gate_slots(), seed=11)
    out += pack(L, "A rings", ring_slots(), seed=12, lb=lb1)
    # ovlp_sum and max_one exactly on lb, and one under: the rings scene again under bars set from its own slots
    out += pack(L, "A rings, bars (4, 2)", ring_slots(), seed=12, lb=thresholds(L, i_ovlp_sum=4, i_ovlp_max_one=2)[0])
    out += pack(L, "A rings, bars (2, 2)", ring_slots(), seed=12, lb=thresholds(L, i_ovlp_sum=2, i_ovlp_max_one=2)[0])
    ss = sort_slots()
    out += pack(L, "B deep", [x for x in ss if x.expect.get("deep")], seed=20, ecc=0, lb=lb1, rows_fn=deep_rows)
    ss = [x for x in ss if not x.expect.get("deep")]
    out += pack(L, "B sort", [x for x in ss if not x.expect.get("capped")], seed=13, jitter=0.7, ecc=1, lb=lb1)
    out += pack(L, "B sort, capped", [x for x in ss if x.expect.get("capped")], seed=18, jitter=0.7, ecc=1, lb=lb1)
    out += pack(L, "C window", window_slots(), seed=14, jitter=0.7, ecc=1, lb=lb1)
    out += pack(L, "C cap", cap_slots(), seed=15, jitter=0.7, ecc=1, lb=lb1)
    out += pack(L, "D b2", b2_slots(), seed=16, jitter=0.7, ecc=1, lb=lb1, rows_fn=b2_rows)
    out += pack(L, "D b2, no orientation noise", b2_slots(), seed=17, jitter=0.0, ecc=1, lb=lb1, rows_fn=b2_rows)
    out += pack(L, "D b2, a pair of 1.0005 px", b2_slots(), seed=23, jitter=0.7, ecc=1, lb=lb1, rows_fn=b2_rows_1px)
    # umeyama on a pure translation and on rotations next to +-pi (the merge scenes' groups G and H are at +-(pi - 0.025) as well)
    out += pack(L, "D b2, pure translation", b2_slots(), seed=24, tf=(4.0, -3.0, 0.0), jitter=0.7, ecc=1, lb=lb1, rows_fn=b2_rows)
    out += pack(L, "D b2, rotation by pi - 0.01", b2_slots(), seed=25, tf=(2.0, 1.0, math.pi - 0.01), jitter=0.7, ecc=1, lb=lb1, rows_fn=b2_rows)
    out += pack(L, "D b2, rotation by 0.01 - pi", b2_slots(), seed=26, tf=(2.0, 1.0, 0.01 - math.pi), jitter=0.7, ecc=1, lb=lb1, rows_fn=b2_rows)
    out += pack(L, "D nrm", nrm_slots(), seed=28, ecc=0, lb=lb1, rows_fn=nrm_rows)
    out += pack(L, "D acos", acos_slots(), seed=22, ecc=1, lb=lb1, rows_fn=acos_rows)
    cls = pack(L, "A classes", class_slots(), seed=19)
    out += cls
    out += shape_scenes(L, cls[0])
    _cache["S"] = out
    return out


def shape_scenes(L, gate):
    """call shapes of stage A on the size-class scene's scan pair: 1, 64, 65, 1 024, 1 025 and 1 152 = CC_HINT_MAX hints; the
    list opens with a wave of 64 keepers, a wave without one and a wave with one, then cycles through the 24 slots (keepers of
    several overlap sizes and anchors that fail)"""
    lb = gate.lb
    keep = [h for h, s in zip(gate.hints, gate.slots) if s.expect.get("anchor") is None]
    drop = [h for h, s in zip(gate.hints, gate.slots) if s.expect.get("anchor") is False]
    assert len(keep) >= 8 and len(drop) >= 8
    full = [keep[i % len(keep)] for i in range(64)] + [drop[i % len(drop)] for i in range(64)]
    full += [keep[0]] + [drop[i % len(drop)] for i in range(63)]
    while len(full) < L.HINT_MAX:
        full.append(gate.hints[len(full) % len(gate.hints)])
    out = []
    for n in (1, 64, 65, 1024, 1025, L.HINT_MAX):
        sc = Scene("A shapes/%d hints" % n, gate.tgt, gate.srcs, full[:n], [None] * n, lb=lb)
        sc.share = gate
        sc.expect = dict(classes=n >= 64)
        out.append(sc)
    return out


# ---- the judges' answers, computed once ---------------------------------------------------------------------------------------
def database(L):
    """the candidate scans of every scene in one list (a scene's `base` is the index of its first), shared scan pairs once"""
    if "db" not in _cache:
        descs = []
        for sc in scenes(L) + merge_scenes(L):
            if getattr(sc, "share", None) is not None:
                sc.base = sc.share.base
                continue
            sc.base = len(descs)
            descs += sc.srcs
        _cache["db"] = np.array(descs, dtype=L.scan_desc_dt)
    return _cache["db"]


def check_pair(oracle, cand, tgt, level, s, t, sim, lb, ub):
    """oracle.check_pair with room for the reference's uncapped pair sets"""
    oi = np.zeros(8, np.int32)
    tf = np.zeros(3, np.float64)
    pairs = np.zeros((1024, 3), np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    oracle.lib().orc_check_pair(cand.h, tgt.h, level, s, t, C.addressof(sim), C.addressof(lb), C.addressof(ub), p(oi), p(tf), p(pairs))
    return oi, tf, [tuple(int(v) for v in r) for r in pairs[:oi[6]]]


def reference(L, oracle, sc):
    """R1's answers for a scene, R2 held against them, the edge assertions -> dict(res, scores, pairs {hint: (tf, pair list)}, r2)"""
    key = ("ref", sc.name)
    if key in _cache:
        return _cache[key]
    database(L)
    lb, ub = L.default_thresholds()
    lb = sc.lb or lb
    sim = sc.sim or L.default_db_cfg().cont_sim
    otgt = accepted(oracle, sc.tgt, sc.name + " tgt")
    osrc = [accepted(oracle, d, sc.name + " src") for d in sc.srcs]
    # candidates are told apart by their int id: rebuild them with distinct ids
    osrc = [oracle.Scan.from_desc(d, int_id=100 + k) for k, d in enumerate(sc.srcs)]
    res, scores = oracle.check_hints(otgt, osrc, sc.hints, sim=sim, lb=lb, ub=ub, max_fine_opt=10)
    ref = dict(res=res, scores=scores, pairs={}, r2={}, lb=lb, ub=ub, sim=sim, log=[])
    seen = {}
    for i, (ci, lev, s, t) in enumerate(sc.hints.tolist()):
        hk = (ci, lev, s, t)
        if hk in seen:      # a repeated hint: the same check
            j = seen[hk]
            if j in ref["pairs"]:
                ref["pairs"][i] = ref["pairs"][j]
            ref["r2"][i] = ref["r2"][j]
            continue
        seen[hk] = i
        slot = sc.slots[i]
        r2 = r2_check(sc.srcs[ci], sc.tgt, lev, s, t, sim, lb)
        ref["r2"][i] = r2
        what = (sc.name, slot.name if slot else i)
        # R2 against R1: the reference reports a score as far as the check got
        exp4 = list(r2["scores"])
        assert exp4 == scores[i, :4].tolist(), (what, "R2", exp4, "R1", scores[i].tolist())
        if "tie_free" in r2:   # distinct keys: R2 judges the shaft scan and the orientation filter too
            tfr = r2["tie_free"]["ref"]
            assert [tfr["orie_sim"], tfr["passed"]] == scores[i, 4:6].tolist(), (what, "R2 stage B2", tfr["orie_sim"], tfr["passed"], "R1", scores[i].tolist())
        if scores[i, 5]:
            oi, tf, pairs = check_pair(oracle, osrc[ci], otgt, lev, s, t, sim, lb, ub)
            assert oi[:5].tolist() == scores[i, :5].tolist() and oi[5] == 1, (what, oi, scores[i])
            # the oracle exports the proposal's pair SET; the pose was fitted to the LIST.  Point tables name a contour once, so
            # the only entry a list can hold twice is the anchor pair, appended behind a window that already has it
            extra = int(oi[4]) - len(pairs)
            assert extra in (0, 1) and (extra == 0 or (lev, s, t) in pairs), (what, oi, pairs)
            pairs = pairs + [(lev, s, t)] * extra
            if "tie_free" in r2:
                assert sorted(r2["tie_free"]["ref"]["cstl"]) == sorted(pairs), (what, "R2's constellation", r2["tie_free"]["ref"]["cstl"], pairs)
            ref["pairs"][i] = (tf, pairs)
            r, nrm = check_tf(tf, sc.srcs[ci], sc.tgt, pairs, what + ("the oracle's own",))
            ref["log"].append((what, r, nrm, len(pairs)))
            if slot is not None and "nrm" in slot.expect:
                assert slot.expect["nrm"][0] < nrm < slot.expect["nrm"][1], (what, "nrm at 50 digits", nrm)
                ref["nrm_cases"] = ref.get("nrm_cases", []) + [(slot.name, nrm, tf_bound(*pair_points(sc.srcs[ci], sc.tgt, pairs), nrm))]
        if slot is not None:
            edge_assertions(slot, r2, scores[i], what, lb)
    if sc.expect.get("classes"):   # the keepers of the call spread over all four size classes of stage A, in its first wave already
        cl = a_classes()
        for part in (scores[:64], scores):
            kp = part[(part[:, 0] >= lb.i_ovlp_sum) & (part[:, 1] >= lb.i_ovlp_max_one), 0]
            assert set(np.digitize(kp, cl).tolist()) == {0, 1, 2, 3}, (sc.name, cl, sorted(set(kp.tolist())))
    _cache[key] = ref
    return ref


def edge_assertions(slot, r2, sc, what, lb):
    """the case reaches its edge, on the references"""
    ex = slot.expect
    if ex.get("anchor") is not None:
        assert r2["anchor"] == ex["anchor"], (what, "anchor", r2["anchor"])
        if ex["anchor"]:
            assert sc[0] > 0, (what, "R1 saw the anchor pass", sc)
        else:
            assert not sc.any(), (what, "R1 saw the anchor fail", sc)
    assert bool(ex.get("capped")) == r2["capped"], (what, "capped", r2["capped"], r2["npp"], r2["in_ang_rng"])
    if ex.get("deep"):
        import introsort_adversary as IA
        assert IA.deep_on(r2["keys"].tolist()), (what, "the depth limit is not exhausted")
    if ex.get("tie_free"):
        assert "tie_free" in r2, (what, "keys not distinct")
    if "ovlp" in ex:
        assert (r2["ovlp_sum"], r2["max_one"]) == ex["ovlp"] == (sc[0], sc[1]), (what, r2["ovlp_sum"], r2["max_one"], sc)
    if "npp" in ex and r2["npp"] >= 0:
        assert r2["npp"] == ex["npp"], (what, "pairs", r2["npp"])
    if "win" in ex:
        assert r2["in_ang_rng"] == ex["win"] == sc[2], (what, "window", r2["in_ang_rng"], sc)
    if "ncs" in ex:
        assert sc[3] == ex["ncs"] == r2["indiv_sim"], (what, "ncs", sc)
    if "orie" in ex:
        assert sc[3] == ex["npp"] + 1 and sc[4] == ex["orie"], (what, "orientation filter", sc)
    if "beg" in ex:
        assert r2["beg"] == ex["beg"], (what, "window start", r2["beg"])
    if "wrap" in ex:
        k = np.sort(r2["keys"])
        assert float(F(k[0] - k[-1])) == ex["wrap"], (what, float(F(k[0] - k[-1])), ex["wrap"])


def scene_facts(L, oracle):
    """profiles/k4_constell/scenes.txt: per case its pairs, window, ncs, outcome and which B1 instance and sort branch it takes"""
    lines = []
    for sc in scenes(L):
        ref = reference(L, oracle, sc)
        if sc.slots[0] is None:
            lines.append("%-46s %4d hints, %d keepers, res %s" % (sc.name, len(sc.hints), int((ref["scores"][:, 0] > 0).sum()), [int(ref["res"][f]) for f in RES_FIELDS]))
            continue
        for i, slot in enumerate(sc.slots):
            r2, s = ref["r2"][i], ref["scores"][i]
            npp = r2["npp"]
            inst = "-" if npp < 0 else ("small" if npp <= PP_SMALL else ("large, capped" if npp > PP_MAX else "large"))
            n = min(npp, PP_MAX)
            rank = "-" if npp <= 0 else ("rank<=16" if n <= 16 else ("rank<=48/64" if (n <= 48 or npp <= PP_SMALL) else "counting sort"))
            lines.append("%-22s %-52s pairs %4d window %3d@%-3d ncs %2d orie %2d passed %d  B1 %s, %s%s" % (
                sc.name, slot.name, npp, s[2], r2["beg"], s[3], s[4], s[5], inst, rank, ", partitions" if n > 16 else ""))
    return lines


# ---- the comparison of a back end ------------------------------------------------------------------------------------------------
def pair_list(bits):
    out = []
    for wd in range(7):
        m = int(bits[wd])
        while m:
            b = wd * 64 + (m & -m).bit_length() - 1
            m &= m - 1
            out.append((b // 100 + 1, (b % 100) // 10, b % 10))
    return out


def check_scene(B, L, oracle, sc, log=None):
    """one cc_db_check_hints call of the back end against the references.  B.hints(scene, hint array, lb, ub) ->
    (rc, result record, scores, pass records)."""
    ref = reference(L, oracle, sc)
    h = np.zeros(len(sc.hints), L.hint_dt)
    h["cand_gidx"] = sc.base + sc.hints[:, 0]
    h["level"], h["seq_src"], h["seq_tgt"] = sc.hints[:, 1], sc.hints[:, 2], sc.hints[:, 3]
    rc, res, scores, passes = B.hints(sc, h, ref["lb"], ref["ub"])
    got = np.stack([scores[f] for f in SCORE_FIELDS], 1)
    capped = [i for i in range(len(sc.hints)) if ref["r2"][i]["capped"]]
    assert rc == (CC_ECAPACITY if capped else 0), (sc.name, rc)
    assert bool(res["flags"] & QF_CHECK_CAP) == bool(capped), (sc.name, "flags", int(res["flags"]))
    exp = ref["scores"]
    worst = 0.0
    by_hint = {int(p["hint"]): p for p in passes}
    sc.last_passes = by_hint   # (check_merge starts its bar from these)
    for i in range(len(sc.hints)):
        what = (sc.name, sc.slots[i].name if sc.slots[i] else i)
        if i in capped:
            r2 = ref["r2"][i]
            assert got[i, :2].tolist() == exp[i, :2].tolist(), (what, got[i], exp[i])
            if r2["npp"] <= PP_MAX:   # the window was found on the whole list: only the constellation was cut
                assert got[i, 2] == exp[i, 2] and got[i, 3] <= CSTL_MAX, (what, got[i], exp[i])
            if "tie_free" in r2:
                # distinct keys: the cut is deterministic and R2 states its outcome -- every figure, the pair set, n_pairs and
                # T_pass (on R2's list, which ends with the anchor pair unless the filter swapped it away) for equality
                dv = r2["tie_free"]["dev"]
                assert got[i, 2:].tolist() == [dv["in_ang_rng"], dv["indiv_sim"], dv["orie_sim"], dv["passed"]], (what, "capped, tie-free", got[i].tolist(), dv)
                assert (i in by_hint) == bool(dv["passed"]), what
                if dv["passed"]:
                    p = by_hint[i]
                    assert sorted(pair_list(p["pairs"])) == sorted(set(dv["cstl"])) and p["n_pairs"] == len(dv["cstl"]), (what, "capped pair set")
                    worst = max(worst, check_tf(p["tf"], sc.srcs[int(sc.hints[i, 0])], sc.tgt, dv["cstl"], what + (B.name, "capped"))[0])
                continue
            if got[i, 5]:
                p = by_hint[i]
                pl = pair_list(p["pairs"])
                lev, s, t = sc.hints[i, 1:].tolist()
                # (beyond CC_PP_MAX pairs the device's window is that of the first 256 generated pairs, not the reference's)
                pool = r2["window"] if r2["npp"] <= PP_MAX else r2["ids"]
                assert len(pl) <= CSTL_MAX and set(pl) <= set(pool) | {(lev, s, t)}, (what, "a capped constellation", len(pl))
                # the cut keeps 63 window pairs and the anchor pair; where the src anchor row has no ecc_feat the
                # orientation filter cannot take the anchor pair out again, so it must be in the set
                if not sc.srcs[int(sc.hints[i, 0])]["cont"][lev][s]["ecc_feat"]:
                    assert (lev, s, t) in pl, (what, "a capped constellation keeps the anchor pair", pl)
            continue
        assert got[i].tolist() == exp[i].tolist(), (what, "got", got[i].tolist(), "expected", exp[i].tolist())
        if exp[i, 5]:
            tf, pairs = ref["pairs"][i]
            p = by_hint[i]
            assert sorted(pair_list(p["pairs"])) == sorted(set(pairs)) and p["n_pairs"] == exp[i, 4], (what, "pair set", pair_list(p["pairs"]), pairs)
            ci = int(sc.hints[i, 0])
            r, nrm = check_tf(p["tf"], sc.srcs[ci], sc.tgt, pairs, what + (B.name,))
            worst = max(worst, r)
            if nrm < 1e-6:
                # both sides sum sequentially: the same r00, r10.  The angle goes through atan2, a sincos and atan2 again on
                # either side: four library calls of ATAN2_ULP ulp of pi at most between the two figures
                assert p["tf"][0] == tf[0] and p["tf"][1] == tf[1], (what, "sequential branch: the oracle's bits", p["tf"], tf)
                assert abs(math.remainder(p["tf"][2] - tf[2], 2 * math.pi)) <= 4 * ATAN2_ULP * 2.0 ** -51, (what, p["tf"][2], tf[2])
        else:
            assert i not in by_hint, (what, "a pass record for a check that did not pass")
    assert len(by_hint) == int(got[:, 5].sum()), sc.name
    if not capped:
        for f in RES_FIELDS:
            assert res[f] == ref["res"][f], (sc.name, f, int(res[f]), int(ref["res"][f]))
        if ref["res"]["n_res"]:
            assert res["cand_gidx"] == sc.base + ref["res"]["cand_gidx"], sc.name
    if log is not None:
        log.append("%-32s %4d hints  aft_check1..3 %4d %4d %4d  passed %3d  flags %d  T_pass error / bound %.3f" % (
            sc.name, len(sc.hints), res["cand_aft_check1"], res["cand_aft_check2"], res["cand_aft_check3"], int(got[:, 5].sum()), int(res["flags"]), worst))
    return worst


def raw_hints(lib, db, qdesc_addr, h, lb, ub, L, stream=None, mfo=10):
    """cc_db_check_hints + cc_db_debug_passes on a bound library; CC_ECAPACITY is an answer here, not an error"""
    res = np.zeros(1, L.query_result_dt)
    sc = np.zeros(len(h), L.hint_score_dt)
    rc = lib.cc_db_check_hints(db, qdesc_addr, h.ctypes.data, len(h), C.addressof(lb), C.addressof(ub), mfo, res.ctypes.data, sc.ctypes.data, stream)
    if rc not in (0, CC_ECAPACITY):
        raise RuntimeError("cc_db_check_hints: %d %s" % (rc, lib.cc_last_error().decode()))
    out = np.zeros(L.HINT_MAX, L.pass_dbg_dt)
    n = C.c_int()
    rc2 = lib.cc_db_debug_passes(db, out.ctypes.data, len(out), C.byref(n))
    assert rc2 == 0, rc2
    return rc, res[0], sc, out[:n.value].copy()


# ---- E. the merge (K4b) ------------------------------------------------------------------------------------------------------
# Every check of these scenes passes, so the order of the hints is the order of the merge.  A scan's rows come in eight GROUPS,
# (level, seqs 0..4) and (level, seqs 5..9); the tgt rows of a group are the src rows moved by the group's own rigid transform
# T = (x, y, theta) about the origin, and a slot's constellation names rows of its own group only: T_pass of slot (level, a) is the
# transform of group (level, a == 5) up to the f32 rounding of the centres.  Which proposals then accept which checks is read
# off the table; the oracle's export (check_hints_cands) is asserted to agree before a back end is judged.
E_GROUPS = {
    "A": ((1, 0), (3.0, -2.0, 0.30)),
    "B": ((1, 1), (5.5, -2.0, 0.30)),                    # 2.5 px from A: outside
    "C": ((2, 0), (4.25, -2.0, 0.30)),                   # 1.25 px from A and from B: both would accept it
    "D": ((2, 1), (3.0, -2.0, 0.59)),                    # 0.29 rad from A: inside
    "E": ((3, 0), (3.0, -2.0, 0.61)),                    # 0.31 rad from A: outside; 0.02 rad from D
    "F": ((3, 1), (3.0, 1.9, 0.30)),                     # 3.9 px from A
    "G": ((4, 0), (150.0, 150.0, math.pi - 0.025)),
    "H": ((4, 1), (150.0, 150.0, -math.pi + 0.025)),     # 0.05 rad from G, across +-pi
}
E_SEQ = {   # name -> (the groups checked, in order, for ONE candidate; proposals, idx_sel expected of the reference)
    "one proposal": ("AAA", 1, 0),
    "two proposals, tied votes": ("AB", 2, 0),
    "four proposals": ("AFGE", 4, 0),
    "a fifth proposal is dropped, the first still joins": ("AFGEBA", 4, 0),
    "joins the first of two that would both accept it": ("ABC", 2, 0),
    "the second proposal has the most votes": ("ABBB", 2, 1),
    "0.29 rad: joins": ("AD", 1, 0),
    "0.31 rad: a proposal of its own": ("AE", 2, 0),
    "blended across +-pi": ("GHGH", 1, 0),
    "blended across -+pi": ("HGG", 1, 0),
}


def e_hint(cand, g, j=0):
    """the hint of candidate `cand` for group g; the first half of a level has five anchors (j picks one), the second half one"""
    (lev, half), _ = E_GROUPS[g]
    a = 5 if half else j % 5
    return (cand, lev, a, a)


def e_scans(L, shift):
    """(tgt, src): the src rows moved by `shift` as a whole (two kinds of candidate scan with slightly different poses)"""
    rs, rt = plain_rows(21), plain_rows(21)
    for (lev, half), (tx, ty, th) in E_GROUPS.values():
        c, s = math.cos(th), math.sin(th)
        for q in range(5 * half, 5 * half + 5):
            p = np.float64(rs[lev][q]["pos_mean"])
            rs[lev][q] = dict(rs[lev][q], pos_mean=F(p + shift), com=F(p + shift))
            p = np.float64(rs[lev][q]["pos_mean"])
            t = F([c * p[0] - s * p[1] + tx, s * p[0] + c * p[1] + ty])
            rt[lev][q] = dict(rt[lev][q], pos_mean=t, com=t, ang=rs[lev][q]["ang"] + th)
    b = {}
    for lev in range(1, 5):
        for a in range(6):
            b[(lev, a)] = [pt(lev, q, 64 * (lev - 1) + 10 + 4 * i, 0.1 * i) for i, q in enumerate(range(5, 10) if a == 5 else range(5))]
    return make_scan(L, rt, b), make_scan(L, rs, b)


E_NCAND = 70


def merge_scenes(L):
    if "E" in _cache:
        return _cache["E"]
    tgt, sx = e_scans(L, np.zeros(2))
    _, sy = e_scans(L, np.array([0.5, 0.0]))   # (the same tgt: a candidate of the second kind is half a pixel off)
    srcs = [sx if k % 2 == 0 else sy for k in range(E_NCAND)]
    lb = thresholds(L, neg_est_dist=-1e9, correlation=-1e30)[0]   # every candidate that clears the area bar goes on and survives
    out = []

    def add(name, hints, **expect):
        sc = Scene("E " + name, tgt, srcs, hints, [None] * len(hints), lb=lb)
        sc.expect = expect
        if out:
            sc.share = out[0]
        out.append(sc)
    # the proposal table: one candidate per sequence, the candidates' checks interleaved round-robin
    seqs = list(E_SEQ.items())
    hints, k = [], 0
    while any(k < len(s[0]) for _, s in seqs):
        hints += [e_hint(c, s[0][k], k) for c, (_, s) in enumerate(seqs) if k < len(s[0])]
        k += 1
    add("proposals", hints, props=[s[1] for _, s in seqs], idx_sel=[s[2] for _, s in seqs])
    # one scan's checks in positions 0, 63, 64 and 130: three rounds of 64, through `before` / clast
    fill = [e_hint(1 + i % 7, "AFGE"[i % 4], i) for i in range(131)]
    for pos, g in ((0, "A"), (63, "F"), (64, "A"), (130, "G")):
        fill[pos] = e_hint(0, g, pos)
    add("rounds 0 63 64 130", fill, n_cand=8, first=dict(props=3))
    # a scan opened and continued within one round; interleavings
    add("A B A B", [e_hint(i % 2, "AF"[(i // 2) % 2], i) for i in range(140)], n_cand=2)
    add("A x 64, B x 64", [e_hint(i // 64, "AFGE"[i % 4], i) for i in range(128)], n_cand=2)
    # 3 .. 70 candidate scans: the four-wide lookup and its sentinels, the second trip of the lane loop
    for n in (3, 4, 5, 63, 64, 65, 70):
        add("%d candidates" % n, [e_hint(i % n, "AB"[(i // n) % 2], i) for i in range(2 * n)], n_cand=n)
    # a later round must not find a scan in what an EARLIER CALL left behind the candidate list (the four-wide lookup reads up to
    # three entries past the last candidate: the sentinels): a call that numbers scans 0 .. 7, then one that opens five other
    # scans in its first round -- its second round reads entries 4 .. 7 of the list, of which 5 .. 7 are not this call's -- and the
    # scans 6, 7 and 5 in its second
    add("sentinels, first call", [e_hint(c, "A", c) for c in range(8)], n_cand=8)
    add("sentinels, second call", [e_hint(8 + i % 5, "A", i) for i in range(64)] + [e_hint(c, "AF"[i % 2], i) for i, c in enumerate((6, 6, 7, 5, 7))],
        n_cand=8, order=[8, 9, 10, 11, 12, 6, 7, 5])
    # the post bars exactly on lb, `!(x < lb)` kept, and one float under: set from the reference's own figure when the scene is built
    import oracle_py as O
    one = O.check_hints_cands(O.Scan.from_desc(tgt), [O.Scan.from_desc(sx, int_id=100)], [e_hint(0, "A")], lb=lb, ub=thresholds(L)[1])
    assert len(one) == 1 and one["survived"][0] == 1 and one["n_props"][0] == 1
    area = one["area_perc"][0, 0]
    x, y, th = one["tf"][0, 0]
    cx = cy = 150 / 2 - 0.5     # getEstSensTF: T_so^-1 T T_so, T_so the translation to the image centre
    neg = -math.hypot(math.cos(th) * cx - math.sin(th) * cy + x - cx, math.sin(th) * cx + math.cos(th) * cy + y - cy)
    nlo = F(neg) if float(F(neg)) <= neg else nf(neg, False)   # the largest f32 not above the f64 figure: `neg < lb` is false on it
    assert float(nlo) <= neg < float(nf(nlo)) and float(nf(nlo)) - float(nlo) > 1e5 * abs(neg) * U
    for nm, kw, live in (("area on the bar", dict(area_perc=float(area)), 1), ("area one float under the bar", dict(area_perc=float(nf(area))), 0),
                         ("neg_est_dist on the largest f32 not above it", dict(neg_est_dist=float(nlo)), 1),
                         ("neg_est_dist one float under the bar", dict(neg_est_dist=float(nf(nlo))), 0)):
        add(nm, [e_hint(0, "A")], survives=live)
        out[-1].lb = thresholds(L, **dict(dict(neg_est_dist=-1e9, correlation=-1e30), **kw))[0]
    out.append(band_scene(L))
    _cache["E"] = out
    return out


def merge_reference(L, oracle, sc):
    """the oracle's candidates for a scene (CAND_DT) with the scene's edge asserted; the area scenes take their bar from it"""
    key = ("mref", sc.name)
    if key in _cache:
        return _cache[key]
    ref = reference(L, oracle, sc)
    otgt = oracle.Scan.from_desc(sc.tgt)
    osrc = [oracle.Scan.from_desc(d, int_id=100 + k) for k, d in enumerate(sc.srcs)]
    cands = oracle.check_hints_cands(otgt, osrc, sc.hints, sim=ref["sim"], lb=ref["lb"], ub=ref["ub"])
    ex = sc.expect
    assert ref["scores"][:, 5].all(), (sc.name, "every check of a merge scene passes")
    assert len(cands) == ref["res"]["n_cand_pose"] and int(cands["survived"].sum()) == ref["res"]["n_cand_tidy"], sc.name
    if "props" in ex:
        assert cands["n_props"].tolist() == ex["props"] and cands["idx_sel"].tolist() == ex["idx_sel"], (sc.name, cands["n_props"], cands["idx_sel"])
        assert cands["cand"].tolist() == list(range(len(ex["props"])))
    if "n_cand" in ex:
        assert len(cands) == ex["n_cand"], (sc.name, len(cands))
    if "first" in ex:
        assert cands["cand"][0] == 0 and cands["n_props"][0] == ex["first"]["props"], (sc.name, cands[0])
    if ex.get("bands"):
        band_assertions(sc, ref)
    if "survives" in ex:
        assert len(cands) == 1 and cands["survived"][0] == ex["survives"], (sc.name, cands, ref["lb"].area_perc, ref["lb"].neg_est_dist)
    if "order" in ex:
        assert cands["cand"].tolist() == ex["order"], (sc.name, cands["cand"])
    out = dict(cands=cands, ref=ref)
    _cache[key] = out
    return out


def merge_bound(ref, sc, cand):
    """bar on (|x|, |y|; angle) between the back end's and the oracle's f64 replay of addProposal for one candidate.  The two
    replays start from T_pass values that differ by what was OBSERVED on this very call (sc.last_passes against the oracle's,
    each already held to tf_bound by check_scene): d_t, d_a, the largest over the candidate's checks; a weighted mean keeps
    that (the weights sum to 1).  Every merge then adds its own rounding: the two products, the sum and the division of the
    mean (4 U of |t| <= M per coordinate, on either side: 8 U M), and for the angle the difference, the wrap, the product,
    the division and the sum (5 U pi), the sincos that rebuilds the matrix and the atan2 that reads it back on the reference's
    side against the carried angle on the device's (ATAN2_ULP ulp of pi for each of sincos and atan2, on either side)."""
    idx = [i for i in range(len(sc.hints)) if sc.hints[i, 0] == cand]
    dt = da = 0.0
    M = 1.0
    for i in idx:
        tf, got = ref["pairs"][i][0], sc.last_passes[i]["tf"]
        dt = max(dt, abs(got[0] - tf[0]), abs(got[1] - tf[1]))
        da = max(da, abs(math.remainder(got[2] - tf[2], 2 * math.pi)))
        M = max(M, abs(tf[0]), abs(tf[1]))
    m = max(len(idx) - 1, 0)
    return dt + m * 8 * U * M + 2 * U * M, da + m * (10 * U * math.pi + 4 * ATAN2_ULP * 2.0 ** -51) + 2 * U * math.pi, m


def check_merge(B, L, oracle, sc, log=None):
    """a merge scene on a back end: the per-hint figures and the result record as check_scene holds them, then EVERY candidate
    (B.cands(): cc_db_debug_cands) against the oracle's export: order, scan, proposals, whether it went on, and tf_init within
    merge_bound.  -> the largest tf_init error / bound"""
    mr = merge_reference(L, oracle, sc)
    check_scene(B, L, oracle, sc, log)
    got, exp = B.cands(), mr["cands"]
    assert len(got) == len(exp), (sc.name, len(got), len(exp))
    worst, obs = 0.0, 0.0
    for k in range(len(exp)):
        what = (sc.name, "candidate", k)
        c = int(exp["cand"][k])
        assert got["cand_gidx"][k] == sc.base + c and got["n_props"][k] == exp["n_props"][k], (what, got[k], exp[k])
        assert got["refined"][k] == exp["survived"][k], (what, got[k], exp[k])
        if exp["survived"][k]:
            e = exp["tf"][k, exp["idx_sel"][k]]
            bt, ba, m = merge_bound(mr["ref"], sc, c)
            et = max(abs(got["tf_init"][k][0] - e[0]), abs(got["tf_init"][k][1] - e[1]))
            ea = abs(math.remainder(got["tf_init"][k][2] - e[2], 2 * math.pi))
            assert et <= bt and ea <= ba, (what, "tf_init", got["tf_init"][k], e, "errors", et, ea, "bounds", bt, ba, "merges", m)
            worst, obs = max(worst, et / bt, ea / ba), max(obs, et, ea)
        else:
            assert not got["tf_init"][k].any(), what
    if log is not None:
        log.append("%-32s %3d candidates, proposals %s  tf_init error / bound %.3f (largest error %.2e)" % (
            sc.name, len(exp), "".join(str(int(v)) for v in exp["n_props"][:24]), worst, obs))
    return worst


def raw_cands(lib, db, L):
    out = np.zeros(L.HINT_MAX, L.cand_dbg_dt)
    n = C.c_int()
    rc = lib.cc_db_debug_cands(db, out.ctypes.data, len(out), C.byref(n))
    assert rc == 0, rc
    return out[:n.value].copy()


def check_ranked_entries(B, L, oracle, sc):
    """the getter against the *_ranked_detail form on the same hint list: every ranked entry's tf_init is the getter's, bit for bit"""
    from cc_amd import load
    calls = load().calls
    mr = merge_reference(L, oracle, sc)
    h = np.zeros(len(sc.hints), L.hint_dt)
    h["cand_gidx"] = sc.base + sc.hints[:, 0]
    h["level"], h["seq_src"], h["seq_tgt"] = sc.hints[:, 1], sc.hints[:, 2], sc.hints[:, 3]
    lib, db, q, stream = B.raw(sc)
    r = calls.check_hints(lib, db, q, h, mr["ref"]["lb"], mr["ref"]["ub"], 16, stream, ranked=L.RANK_MAX, detail=True)
    B.sync()
    got = {int(c["cand_gidx"]): c for c in raw_cands(lib, db, L)}
    rk, n = r.rank
    assert n[0] == min(L.RANK_MAX, int(mr["cands"]["survived"].sum())) > 0, (sc.name, n)
    for e in range(int(n[0])):
        g = int(rk[0, e]["cand_gidx"])
        assert got[g]["refined"] == 1 and got[g]["tf_init"].tobytes() == r.detail[0, e]["tf_init"].tobytes(), (sc.name, e, got[g], r.detail[0, e])
    return int(n[0])


# ---- F. batches -------------------------------------------------------------------------------------------------------------
def batch_items(L, n_items):
    """(query scenes, items [(query index, database scan)]): one (query, candidate) pair per item -- every scan pair of the A-D
    scenes, then candidates of the merge scenes' query, then the A-D pairs again until n_items"""
    qs, items = [], []
    for sc in scenes(L):
        if sc.share is None:
            items.append((len(qs), sc.base))
            qs.append(sc)
    n_ad = len(items)
    e = merge_scenes(L)[0]
    database(L)
    qs.append(e)
    k = 0
    while len(items) < n_items:
        items.append((len(qs) - 1, e.base + k) if k < E_NCAND and len(items) < n_items - n_ad else items[(len(items)) % n_ad])
        k += 1
    return qs, items[:n_items]


def check_batch(B, L, oracle, n_items, log=None):
    """cc_db_verify_batch on the built scans, the generated hint lists taken back: every item's record equals, byte for byte,
    cc_db_check_hints of its list; the reversed batch returns the same bytes per item.  Every anchor pair of every level is
    hinted (no key bound), so the batch holds the > 64-pair and the capped checks of the B and C scenes: counted with R2."""
    qs, items = batch_items(L, n_items)
    lb, ub = L.default_thresholds()
    sim = L.default_db_cfg().cont_sim
    qdesc = np.array([sc.tgt for sc in qs], dtype=L.scan_desc_dt)
    qidx = np.array([q for q, _ in items], np.int32)
    cands = [[g] for _, g in items]
    res, hints = B.verify(qdesc, qidx, cands)
    rres, rhints = B.verify(qdesc, qidx[::-1].copy(), cands[::-1])
    n_large = n_capped = n_flag = 0
    seen = set()
    for i, (q, g) in enumerate(items):
        assert res[i].tobytes() == rres[len(items) - 1 - i].tobytes() and hints[i].tobytes() == rhints[len(items) - 1 - i].tobytes(), ("reversed", i)
        assert len(hints[i]) > 0 and (hints[i]["cand_gidx"] == g).all(), i
        rc, one, _, _ = B.hints(qs[q], np.ascontiguousarray(hints[i]), lb, ub)
        assert one.tobytes() == res[i].tobytes(), ("item", i, qs[q].name, g, one, res[i])
        assert rc == (CC_ECAPACITY if one["flags"] else 0)
        n_flag += bool(one["flags"] & QF_CHECK_CAP)
        if qs[q].share is None and qs[q].srcs and g == qs[q].base and (q, g) not in seen and not qs[q].name.startswith("E "):
            seen.add((q, g))
            for h in hints[i]:
                r2 = r2_check(qs[q].srcs[0], qs[q].tgt, int(h["level"]), int(h["seq_src"]), int(h["seq_tgt"]), sim, lb)
                n_large += r2["npp"] > PP_SMALL
                n_capped += bool(r2["capped"])
    assert n_large >= 8 and n_capped >= 4 and n_flag >= 2, (n_large, n_capped, n_flag)
    if log is not None:
        log.append("F %s: %d items, %d hints; on the distinct A-D pairs %d checks of > 64 pairs, %d capped; %d items flagged" % (
            B.name, len(items), sum(len(h) for h in hints), n_large, n_capped, n_flag))


# ---- the table under dynamic thresholds --------------------------------------------------------------------------------------
def check_dynamic(B, L, oracle, log=None):
    """every scene of A-E without a capped check once more under cc_db_set_dynamic_thres (the bars rise from check to check, so a
    check cut by a capacity would change the bars of every later one: the reference is no judge there), judged by
    tests/dyn_oracle.check_hints: the six figures per hint and the counters, for equality"""
    import dyn_oracle
    n = 0
    B.dynamic(True)
    try:
        for sc in scenes(L) + merge_scenes(L):
            ref = reference(L, oracle, sc)
            if any(ref["r2"][i]["capped"] for i in range(len(sc.hints))):
                continue
            desc = np.array([sc.tgt] + list(sc.srcs), dtype=L.scan_desc_dt)
            hints = sc.hints.copy()
            eres, esc = dyn_oracle.check_hints(desc, 0, list(range(1, len(desc))), hints, ref["sim"], ref["lb"], ref["ub"])
            h = np.zeros(len(sc.hints), L.hint_dt)
            h["cand_gidx"] = sc.base + sc.hints[:, 0]
            h["level"], h["seq_src"], h["seq_tgt"] = sc.hints[:, 1], sc.hints[:, 2], sc.hints[:, 3]
            rc, res, scores, _ = B.hints(sc, h, ref["lb"], ref["ub"])
            got = np.stack([scores[f] for f in SCORE_FIELDS], 1)
            bad = np.nonzero((got != esc).any(1))[0]
            assert rc == 0 and len(bad) == 0, (sc.name, "dynamic", bad[:5], got[bad[:5]], esc[bad[:5]])
            for f in RES_FIELDS:
                assert res[f] == eres[f], (sc.name, "dynamic", f, int(res[f]), int(eres[f]))
            n += 1
            if log is not None:
                log.append("%-32s dynamic: passed %3d of %4d (constant bars: %3d)" % (sc.name, int(got[:, 5].sum()), len(h), int(ref["scores"][:, 5].sum())))
    finally:
        B.dynamic(False)
    return n


# ---- E, the 1e-9 bands of addProposal's bars ------------------------------------------------------------------------------------
# k_merge.h decides `|t| < 2.0` and `|angle| < 0.3` without sqrt and atan2 unless the value lies within 1e-9 (relative) of its bar;
# inside that band the reference's own expressions decide.  Four checks are placed INSIDE the bands, one on either side of each
# bar, by a CPU search over the f32 centres: a tgt centre with a coordinate near 2^-7 (one float there is 9e-10 px) is moved float
# by float; the pose of the check follows in steps of 1.5e-10 px / 4e-12 rad.  The search runs on fit() / delta(), restatements of
# getTFFromConstell's sequential closed form and of addProposal's delta_T; what it finds is then asserted on the oracle's own
# T_pass values and on which proposal the oracle's export says each check joined.
BAND_P = (3.0, -2.0)
BAND_BASE = [(-30.0, -20.0), (25.0, -28.0), (30.0, 22.0), (-27.0, 26.0)]


def fit(S, T):
    """getTFFromConstell (contour_mng.h:1252-1277 as oracle/orc_contour.h restates it): sequential sums -> (x, y, theta)"""
    n = len(S)
    inv = 1.0 / n
    sx = sy = dx = dy = 0.0
    for (ax, ay), (bx, by) in zip(S, T):
        sx, sy, dx, dy = sx + ax, sy + ay, dx + bx, dy + by
    sx, sy, dx, dy = sx * inv, sy * inv, dx * inv, dy * inv
    s00 = s01 = s10 = s11 = 0.0
    for (ax, ay), (bx, by) in zip(S, T):
        ax, ay, bx, by = ax - sx, ay - sy, bx - dx, by - dy
        s00, s01, s10, s11 = s00 + bx * ax, s01 + bx * ay, s10 + by * ax, s11 + by * ay
    sn, cs = s10 * inv - s01 * inv, s00 * inv + s11 * inv
    nrm = math.sqrt(sn * sn + cs * cs)
    r00, r10 = (cs / nrm, sn / nrm) if nrm > 0 else (1.0, 0.0)
    return dx - (r00 * sx + (-r10) * sy), dy - (r10 * sx + r00 * sy), math.atan2(r10, r00)


def delta(prop, old):
    """addProposal's delta_T = T_prop^-1 * T_old for poses (x, y, theta) -> (squared translation norm, |angle|)"""
    pc, ps = math.cos(prop[2]), math.sin(prop[2])
    oc, os_ = math.cos(old[2]), math.sin(old[2])
    dtx = pc * old[0] + ps * old[1] - (pc * prop[0] + ps * prop[1])
    dty = -ps * old[0] + pc * old[1] - (-ps * prop[0] + pc * prop[1])
    return dtx * dtx + dty * dty, abs(math.atan2(-ps * oc + pc * os_, pc * oc + ps * os_))


def _bump(x, k):
    """the f32 k floats above x"""
    return (np.array([x], F).view(np.int32) + np.int32(k if x > 0 else -k)).view(F)[0]


def band_group(kind, k, dup):
    """(src centres [5], tgt centres [5]) of a group: four centres of BAND_BASE and a fifth whose tgt x is 2^-7 + k floats.
    kind 't': a translation by (5, -2), 2 px from BAND_P; kind 'r': a rotation by 0.3 rad about the origin and BAND_P.
    `dup`: the index of the pair that the anchor repeats at the end of the list"""
    if kind == "p":
        S = [F(p) for p in BAND_BASE] + [F([2.0, 0.0])]
        T = [F(np.float64(p) + BAND_P) for p in S]
    elif kind == "t":
        t = np.array([5.0, -2.0])
        S = [F(p) for p in BAND_BASE] + [F([2.0 ** -7 - t[0], 0.5 - t[1]])]
        T = [F(np.float64(p) + t) for p in S]
        T[4] = F([_bump(F(2.0 ** -7), k), 0.5])
    else:
        c, s = math.cos(0.3), math.sin(0.3)
        q = np.array([2.0 ** -7, 25.0]) - BAND_P
        S = [F(p) for p in BAND_BASE] + [F([c * q[0] + s * q[1], -s * q[0] + c * q[1]])]
        T = [F([c * p[0] - s * p[1] + BAND_P[0], s * p[0] + c * p[1] + BAND_P[1]]) for p in np.float64(S)]
        T[4] = F([_bump(F(2.0 ** -7), k), 25.0])
    return S, T


def _pose(kind, k, dup):
    S, T = band_group(kind, k, dup)
    S, T = [tuple(np.float64(p)) for p in S], [tuple(np.float64(p)) for p in T]
    return fit(S + [S[dup]], T + [T[dup]])


def band_search(kind, dup, side):
    """the k that puts the check's distance (kind 't') or angle (kind 'r') to proposal P inside the 1e-9 band of its bar, under it
    (side -1) or over it (side +1): relative distance to the bar in (5e-11, 6e-10)"""
    P = _pose("p", 0, 0)

    def f(k):
        n2, ang = delta(_pose(kind, k, dup), P)
        return math.sqrt(n2) / 2.0 - 1.0 if kind == "t" else ang / 0.3 - 1.0
    lo, hi = -(1 << 19), 1 << 19
    up = f(hi) > f(lo)
    assert f(lo) * f(hi) < 0, (kind, f(lo), f(hi))
    while hi - lo > 1:
        m = (lo + hi) // 2
        lo, hi = (m, hi) if (f(m) < 0) == up else (lo, m)
    for k in sorted(range(lo - 400, lo + 400), key=lambda k: abs(k - lo)):
        if 5e-11 < side * f(k) < 6e-10:
            return k
    raise AssertionError(("no float inside the band", kind, side))


BAND_CASES = (("t", 5, -1, 1, "0: 2 px less 1e-10: joins"), ("t", 0, +1, 2, "1: 2 px plus 1e-10: a proposal of its own"),
              ("r", 5, -1, 1, "2: 0.3 rad less 1e-10: joins"), ("r", 0, +1, 2, "3: 0.3 rad plus 1e-10: a proposal of its own"))
BAND_SLOT = {0: (1, 5), 1: (2, 0), 2: (2, 5), 3: (3, 0)}   # case -> (level, anchor); proposal P is (1, 0)


def band_scene(L):
    """`E bands`: four candidates (one src scan, four times in the database), each checked with P and then with its own case"""
    if "EB" in _cache:
        return _cache["EB"]
    rs, rt = plain_rows(27), plain_rows(27)
    groups = {(1, 0): band_group("p", 0, 0)}
    for c, (kind, a, side, _, _) in enumerate(BAND_CASES):
        lev = BAND_SLOT[c][0]
        groups[(lev, int(a == 5))] = band_group(kind, band_search(kind, 0, side), 0)   # the anchor repeats the group's first pair
    b = {}
    for (lev, half), (S, T) in groups.items():
        seqs = list(range(5 * half, 5 * half + 5))
        for q, s_, t_ in zip(seqs, S, T):
            rs[lev][q] = dict(rs[lev][q], pos_mean=s_, com=s_)
            rt[lev][q] = dict(rt[lev][q], pos_mean=t_, com=t_)
        a = seqs[0]   # the group's slot: the anchor is its first contour, so the list ends with a repeat of its first pair
        # distinct ascending keys 0.001 i: the list's order is the groups' order, whatever std::sort does with ties
        b[(lev, a)] = ([pt(lev, q, 64 * (lev - 1) + 10 + 4 * i, 0.1 * i) for i, q in enumerate(seqs)],
                       [pt(lev, q, 64 * (lev - 1) + 10 + 4 * i, 0.1 * i + 0.001 * i) for i, q in enumerate(seqs)])
    tgt = make_scan(L, rt, {k: v[1] for k, v in b.items()})
    src = make_scan(L, rs, {k: v[0] for k, v in b.items()})
    hints = []
    for c in range(4):
        lev, a = BAND_SLOT[c]
        a = 5 if a == 5 else 0
        hints += [(c, 1, 0, 0), (c, lev, a, a)]
    sc = Scene("E bands", tgt, [src] * 4, hints, [None] * len(hints), lb=thresholds(L, neg_est_dist=-1e9, correlation=-1e30)[0])
    sc.expect = dict(props=[x[3] for x in BAND_CASES], idx_sel=[0] * 4, bands=True)
    _cache["EB"] = sc
    return sc


def band_assertions(sc, ref):
    """on the ORACLE's T_pass values: every case lies inside the 1e-9 band of its bar, on its side, and outside the first arm"""
    for c, (kind, _, side, _, nm) in enumerate(BAND_CASES):
        P, Q = ref["pairs"][2 * c][0], ref["pairs"][2 * c + 1][0]
        n2, ang = delta(tuple(Q), tuple(P))
        if kind == "t":
            assert 4.0 * (1.0 - 1e-9) <= n2 <= 4.0 * (1.0 + 1e-9) and (math.sqrt(n2) < 2.0) == (side < 0) and ang < 0.01, (nm, n2, ang)
        else:
            pc, ps = math.cos(Q[2]), math.sin(Q[2])
            d00, d10 = pc * math.cos(P[2]) + ps * math.sin(P[2]), -ps * math.cos(P[2]) + pc * math.sin(P[2])
            lim = d00 * 0.30933624960962325
            assert n2 < 1.0 and lim * (1.0 - 1e-9) <= abs(d10) <= lim * (1.0 + 1e-9) and (ang < 0.3) == (side < 0), (nm, n2, abs(d10) / lim - 1, ang)
