"""TEST INFRASTRUCTURE shared by test_emu_gmm_inputs.py / test_gpu_gmm_inputs.py: K5 (csrc/k_gmm.h) on SYNTHETIC ellipse tables.

Descriptors are built here (make_desc), not ingested: the header, keys and BCIs of one recorded scan, and for levels 1..4 contour
rows whose counts, means, eigenvalues and eigenvector angles the case chooses.  Every case first rebuilds its descriptors with
oracle.Scan.from_desc and checks that the oracle took them (accepted()).

  A  cc_gmm_feat (cc_pack_scans -> cc_k_gmm_prep) against a restatement: n_ell / flags from the reference's own loop, the ellipse
     rows bit for bit against an f32 numpy restatement of getManualCov, ac against the full n^2 sum at 50 digits within a DERIVED
     bound (ac_bound).
  B  the pair pre-selection of cc_k_gmm_init (cc_gmm_scan_pairs) through cc_db_pose_*, refine = 0: n_pairs against the ctor's
     expression in numpy f64 (and against the oracle's count), the try value at T_init against oracle.gmm_eval within
     pose_common.TRY_BAR; both init instances.
  C  list-length edges through cc_k_gmm_refine<16|64>: items with exactly N pairs, N on every edge of the list plumbing, against
     oracle.gmm.

A back end provides: L, pack(desc) -> feat bytes [n, FEAT_BYTES]; open(desc, small_grid) -> handle; pose(handle, items, refine,
tries) -> (rows, try values); switch(handle) -> a problem count up to which a chunk surely takes cc_k_gmm_init's wave-per-problem
instance, and for the small_grid handle the count above which it takes the 16-lane one (`n_prob <= gridDim.x` in the kernel,
gridDim.x = tune.gmm of launch_gmm_init in cc_db_api.inc: 4 096 unless CC_GMM_GRID says otherwise when the handle is made).

Islands.  A pair list of exactly N pairs is made of islands: island k holds a_k src and b_k tgt ellipses within 0.4 cell of its
centre (closer than any major axis, >= 2 cells), islands lie >= 40 cells apart, further than 3 (maj_s + maj_t) <= 18 cells plus the
largest displacement a start pose causes (0.71 cell + 0.01 rad x 330 cells = 3.3).  Then N = sum a_k b_k exactly.

The packed in-between lists.  cc_k_gmm_refine<16> takes the lists of 97..256 pairs (four to a wave, 32 records each in LDS) once a
chunk selects >= CC_GMM_PACK_MIN_PROBLEMS = 3 072 problems.  A pose chunk holds at most 1 024 items (cc_db::QB), so no pose call
reaches that with the shipped threshold: the harness runner builds a second library with the threshold at 8 (the macro is
#ifndef-guarded; nothing else differs) and runs part C on it, where the call of 21 items packs them and the call of 4 does not.
On the device that branch is reached by the query flows alone."""
import hashlib
import json
import math
import os

import mpmath as mp
import numpy as np

import pose_common as PC
from primitive_cases import ErrBound as _EB
from ranked_common import TOL

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gmm_inputs_ac.json")
NLV, ECAP = 4, 320
U = 2.0 ** -53
EXP_ULP = 2.0    # ASSUMPTION: the library exp of the device (and glibc's) is within 2 ulp; nothing in the suite holds the device's to it
NINF = float("-inf")

feat_dt = np.dtype([("n_ell", "<i4", (NLV,)), ("flags", "<i4"), ("pad", "<i4", (3,)), ("ac", "<f8"), ("ell", "<f4", (NLV, ECAP, 8))])
assert feat_dt.itemsize == 41000


# ---- 0. synthetic ellipse tables ----------------------------------------------------------------------------------------
def base_desc(L):
    return PC.fixture_desc(L)[0].copy()


def level(cell_cnt, pos, eig, ang, n_cont=None, full=None):
    """one level's contour rows: cell_cnt [n] non-increasing (the table's order), pos [n, 2], eig [n, 2] (minor, major), ang [n]
    (the eigenvectors are the rotation by ang, rounded to f32); n_cont defaults to n, full (layer_cell_cnt) to twice the sum (every
    row is then used by the 95 % rule)"""
    cc = np.asarray(cell_cnt, np.int64).reshape(-1)
    n = len(cc)
    assert n <= ECAP and (np.diff(cc) <= 0).all() and (n == 0 or (cc.min() >= 1 and cc.max() < 32768)), "rows in sorted order, int16 counts"
    return {"cell_cnt": cc, "pos": np.asarray(pos, np.float32).reshape(n, 2), "eig": np.asarray(eig, np.float32).reshape(n, 2),
            "ang": np.asarray(ang, np.float64).reshape(n), "n_cont": n if n_cont is None else int(n_cont),
            "full": int(2 * cc.sum()) if full is None else int(full)}


def empty_level():
    return level([], np.zeros((0, 2)), np.zeros((0, 2)), [], full=0)


def make_desc(L, levels):
    """a layouts.scan_desc_dt record: the recorded scan's header, keys and BCIs, levels 1..4 from `levels` (four level() dicts)"""
    d = base_desc(L)
    assert len(levels) == NLV
    for li, lv in enumerate(levels):
        lev = li + 1
        n = len(lv["cell_cnt"])
        d["n_cont"][lev], d["n_stored"][lev], d["layer_cell_cnt"][lev] = lv["n_cont"], n, lv["full"]
        rows = np.zeros(L.MAXC, L.contour_dt)
        c, s = np.cos(lv["ang"]).astype(np.float32), np.sin(lv["ang"]).astype(np.float32)
        rows["level"][:n] = lev
        rows["poi"][:n] = np.clip(np.nan_to_num(lv["pos"]), 0, 149).astype(np.int16)
        rows["cell_cnt"][:n] = lv["cell_cnt"]
        rows["pos_mean"][:n] = lv["pos"]
        rows["eig_vals"][:n] = lv["eig"]
        rows["eig_vecs"][:n] = np.stack([c, s, -s, c], 1)   # v00 v10 v01 v11
        cov = ell_rows(rows[:n])
        rows["pos_cov"][:n] = cov[:, [0, 2, 1, 3]]
        with np.errstate(invalid="ignore", divide="ignore"):
            rows["eccen"][:n] = np.nan_to_num(np.sqrt(np.maximum(0, 1 - lv["eig"][:, 0] / lv["eig"][:, 1])))
        rows["vol3_mean"][:n] = 1.0
        rows["com"][:n] = lv["pos"]
        d["cont"][lev] = rows
    return d


def stack(descs, L):
    return np.array(descs, dtype=L.scan_desc_dt)


def accepted(oracle, desc, what):
    """oracle.Scan.from_desc took the descriptor: the rows it holds are the rows that were given"""
    s = oracle.Scan.from_desc(desc)
    assert s.h, what
    back = s.desc()[0]
    for lev in range(1, NLV + 1):
        n = int(desc["n_stored"][lev])
        assert s.ncont(lev) == n and back["n_stored"][lev] == n and back["layer_cell_cnt"][lev] == desc["layer_cell_cnt"][lev], (what, lev)
        for f in ("cell_cnt", "pos_mean", "eig_vals", "eig_vecs"):
            assert back["cont"][lev][f][:n].tobytes() == desc["cont"][lev][f][:n].tobytes(), (what, lev, f)
    return s


# ---- A. references ----------------------------------------------------------------------------------------------------------
def ell_rows(rows):
    """getManualCov (contour.h:376-378) in f32, every product and every sum rounded once, in cc_k_gmm_prep's association;
    -> [n, 8] f32: c00 c01 c10 c11 mx my w maj"""
    f = np.float32
    v00, v10, v01, v11 = (rows["eig_vecs"][:, k].astype(f) for k in range(4))
    e0, e1 = rows["eig_vals"][:, 0].astype(f), rows["eig_vals"][:, 1].astype(f)
    with np.errstate(invalid="ignore"):
        a00, a01, a10, a11 = v00 * e0, v01 * e1, v10 * e0, v11 * e1
        out = np.stack([a00 * v00 + a01 * v01, a00 * v10 + a01 * v11, a10 * v00 + a11 * v01, a10 * v10 + a11 * v11,
                        rows["pos_mean"][:, 0], rows["pos_mean"][:, 1], rows["cell_cnt"].astype(f), np.sqrt(e1)], 1)
    assert out.dtype == f
    return out


def select_ref(desc, lev):
    """the reference's own loop (correlation.h:49-82, as oracle/orc_gmm.h:144-153) over the stored rows -> (n_ell, flags): a row
    the loop wants beyond the stored ones is flags bit 2"""
    full, run, n = int(desc["layer_cell_cnt"][lev]), 0, 0
    for j in range(int(desc["n_cont"][lev])):
        if run * 1.0 / full >= 0.95:
            break
        if j >= int(desc["n_stored"][lev]):
            return n, 4
        run += int(desc["cont"][lev]["cell_cnt"][j])
        n += 1
    return n, 0


def feat_ref(desc):
    """(n_ell [4], flags, [ell [n, 8] per level]) of one descriptor"""
    n_ell, flags, ells = [], 0, []
    for lev in range(1, NLV + 1):
        n, f = select_ref(desc, lev)
        n_ell.append(n)
        flags |= f
        ells.append(ell_rows(desc["cont"][lev][:n]))
    return np.array(n_ell, np.int32), flags, ells


def drop_mask(E):
    """cc_k_gmm_prep's f32 drop test on every pair (i, j) of one level -> bool [n, n]"""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = E[:, None, 4] - E[None, :, 4], E[:, None, 5] - E[None, :, 5]
        t00, t01, t10, t11 = (E[:, None, k] + E[None, :, k] for k in range(4))
        tr, det = t00 + t11, t00 * t11 - t01 * t10
        return (dx * dx + dy * dy > f(400) * tr) & (det > f(1e-4) * tr * tr)


def _div(a, b):
    v = a.v / b.v
    return _EB(v, (a.e + np.abs(v) * b.e) / (np.abs(b.v) - b.e) + U * np.abs(v))


def _sqrt(a):
    v = np.sqrt(a.v)
    return _EB(v, a.e / (2 * np.sqrt(a.v - a.e)) + U * v)


def self_term_bound(A, B):
    """cc_gmm_self_term (and GMMPair's autocorr lambda with quadExp: the same operations in the same order) followed operation by
    operation in half-ulps, as primitive_cases.gmm_term_bound follows cc_gmm_term; exp at EXP_ULP plus e^|dx| - 1 for its argument's
    error.  A, B [m, 8] f32 -> (value, bound of its absolute error) [m] f64"""
    a, b = [_EB(A[:, k].astype(np.float64)) for k in range(8)], [_EB(B[:, k].astype(np.float64)) for k in range(8)]
    n00, n01, n10, n11 = ((a[k] + b[k]).scale(2) for k in range(4))
    mx, my = a[4] - b[4], a[5] - b[5]
    det = n00 * n11 - n10 * n01
    assert (det.v > 2 * det.e).all(), "the bound needs det N safely positive"
    inv = _div(_EB(np.ones_like(det.v)), det)
    i00, i10, i01, i11 = n11 * inv, -(n10 * inv), -(n01 * inv), n00 * inv
    h0, h1 = mx.scale(-0.5), my.scale(-0.5)
    r0, r1 = h0 * i00 + h1 * i10, h0 * i01 + h1 * i11
    x = r0 * mx + r1 * my
    ev = np.exp(x.v)
    ex = _EB(ev, ev * (np.expm1(x.e) + 2 * U * EXP_ULP))
    t = _div(a[6] * b[6], _sqrt(det)) * ex
    return t.v, t.e * (1 + 1e-6)


def _mp_terms(E):
    """the self term of every pair i <= j of one level at 50 digits -> (sum over the ORDERED pairs, list of (i, j, term))"""
    mp.mp.dps = 50
    M = [[mp.mpf(float(x)) for x in row] for row in E]
    n, tot, terms = len(M), mp.mpf(0), []
    for i in range(n):
        a = M[i]
        for j in range(i, n):
            b = M[j]
            n00, n01, n10, n11 = 2 * (a[0] + b[0]), 2 * (a[1] + b[1]), 2 * (a[2] + b[2]), 2 * (a[3] + b[3])
            mx, my = a[4] - b[4], a[5] - b[5]
            det = n00 * n11 - n10 * n01
            q = -(mx * mx * n11 - mx * my * (n01 + n10) + my * my * n00) / (2 * det)
            t = a[6] * b[6] / mp.sqrt(det) * mp.exp(q)
            terms.append(t)
            tot += t if i == j else 2 * t
    return tot, terms


_golden = None


def ac_exact(ells):
    """The full ordered n^2 sum of correlation.h:102-119 over the four levels at 50 digits, and the exact mass of the pairs
    cc_k_gmm_prep's f32 test drops -> (sum, dropped mass) as mpf.  ~0.1 ms per pair: the values of the committed cases are kept in
    tests/golden/gmm_inputs_ac.json under the SHA-1 of the f32 ellipse rows they were computed from, and recomputed when a table's
    hash is not there (`PYTHONPATH=oracle python tests/gmm_cases.py` rewrites the file)."""
    mp.mp.dps = 50
    global _golden
    if _golden is None:
        _golden = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    key = hashlib.sha1(b"|".join(np.ascontiguousarray(E).tobytes() for E in ells)).hexdigest()
    if key not in _golden:
        tot, drop = mp.mpf(0), mp.mpf(0)
        for E in ells:
            t, terms = _mp_terms(E)
            tot += t
            iu = np.triu_indices(len(E))
            dm = drop_mask(E)[iu]
            for k in np.nonzero(dm)[0]:
                drop += 2 * terms[k]   # (a dropped pair is off the diagonal: |m|^2 > 0)
        _golden[key] = [mp.nstr(tot, 45), mp.nstr(drop, 45)]
    tot, drop = _golden[key]
    return mp.mpf(tot), mp.mpf(drop)


def ac_bound(ells, exact, oracle_sum=False):
    """The derived bound of |ac - exact|.  Device: per evaluated pair i <= j the running bound of cc_gmm_self_term (doubled off the
    diagonal: the doubling is exact), plus (ceil(T / 256) + 8) u of the sum for the T evaluated terms, all >= 0 (one lane's
    sequential part, six shuffle steps, four partials), plus the mass of the dropped pairs.  The oracle's sequential sum of all
    n^2 terms: the same per-term bound, (T - 1) u, nothing dropped.  -> (bound, T)"""
    per, T = 0.0, 0
    for E in ells:
        n = len(E)
        if n == 0:
            continue
        i, j = np.triu_indices(n)
        keep = np.ones(len(i), bool) if oracle_sum else ~drop_mask(E)[i, j]
        i, j = i[keep], j[keep]
        _, e = self_term_bound(E[i], E[j])
        per += float((e * np.where(i == j, 1.0, 2.0)).sum())
        T += (n * n) if oracle_sum else len(i)
    S = float(exact[0])
    if oracle_sum:
        return per + (T - 1) * U * S, T
    return per + (-(-T // 256) + 8) * U * S + float(exact[1]), T


def finite_case(ells):
    """every evaluated pair has finite inputs and det N > 0 (else the reference value is not finite: class comparison)"""
    for E in ells:
        if not np.isfinite(E).all():
            return False
        if len(E):
            t = [E[:, None, k].astype(np.float64) + E[None, :, k] for k in range(4)]
            if not (t[0] * t[3] - t[1] * t[2] > 1e-9 * (t[0] + t[3]) ** 2).all():
                return False
    return True


# ---- A. cases -----------------------------------------------------------------------------------------------------------
def _cloud(rng, n, span=60.0, w0=None):
    """n ellipses scattered over span x span cells: minor axis 1..3, major 1..6 cells, all weights distinct"""
    e1 = rng.uniform(1.0, 36.0, n)
    e0 = np.minimum(e1, rng.uniform(1.0, 9.0, n))
    w0 = (400 + n) if w0 is None else w0
    return level(w0 - np.arange(n), rng.uniform(20, 20 + span, (n, 2)), np.stack([e0, e1], 1), rng.uniform(-np.pi, np.pi, n))


def _cut_level(rng, n_rows, cut, n_cont=None, cnt=10):
    """n_rows equal contours of `cnt` cells whose 95 % cut falls on contour `cut` (the first row NOT used); cut None: no cut"""
    lv = _cloud(rng, n_rows)
    lv["cell_cnt"][:] = cnt
    lv["n_cont"] = n_rows if n_cont is None else n_cont
    lv["full"] = 10 ** 7 if cut is None else int(cut * cnt / 0.95)
    return lv


def _f32_step_pairs():
    """pairs of round ellipses (C = 2.5 I exactly, tr = 10: 400 tr = 4 000) whose f32 dx^2 + dy^2 is one f32 step under 4 000,
    4 000 itself and one step over it: a at (0, Y), b at (x, Y + y), Y a multiple of 4 096 and y of 1 / 8 (both differences exact),
    x found by a search over the f32 values from 63.24 up; each pair 4 096 cells from the next"""
    f = np.float32
    want = [np.nextafter(f(4000), f(0)), f(4000), np.nextafter(f(4000), f(1e9))]
    cand = [f(63.24)]
    for _ in range(6000):
        cand.append(np.nextafter(cand[-1], f(100)))
    cand = np.array(cand, f)
    pos = []
    for k, wv in enumerate(want):
        hit = None
        for y in (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0):
            idx = np.nonzero(cand * cand + f(y) * f(y) == wv)[0]
            if len(idx):
                hit = (cand[idx[0]], f(y))
                break
        assert hit is not None, ("no f32 offset gives", wv)
        Y = f(4096.0 * (k + 1))
        a, b = np.array([0, Y], f), np.array([hit[0], Y + hit[1]], f)
        d = b - a
        assert d[0] * d[0] + d[1] * d[1] == wv, (k, a, b)
        pos += [a, b]
    n = len(pos)
    return level(500 - np.arange(n), np.array(pos), np.full((n, 2), 2.5), np.zeros(n))


def feat_cases(L):
    """[(name, descriptor)] of part A, eleven descriptors"""
    rng = np.random.default_rng(20240)
    out = []
    for name, counts in (("counts 0 1 2 3", (0, 1, 2, 3)), ("counts 63 64 65 127", (63, 64, 65, 127)), ("counts 128 129 255 256", (128, 129, 255, 256)),
                         ("counts 257 319 320 5", (257, 319, 320, 5))):
        out.append((name, make_desc(L, [_cloud(rng, n, span=40.0 + n / 4) if n else empty_level() for n in counts])))
    # the 95 % rule
    exact = _cloud(rng, 12)
    exact["cell_cnt"][:] = [40, 30, 20, 5, 1, 1, 1, 1, 1, 1, 1, 1]   # 95 cells before row 3 + ... : the run is 95 after row 3
    exact["full"] = 100
    under = _cloud(rng, 12)
    under["cell_cnt"][:] = [40, 30, 20, 4, 1, 1, 1, 1, 1, 1, 1, 1]   # 94 after row 3, 95 after row 4
    under["full"] = 100
    out.append(("95 % exactly, one under, cut on 63, on 64", make_desc(L, [exact, under, _cut_level(rng, 80, 63), _cut_level(rng, 80, 64)])))
    out.append(("cut on 65, on 128; n_cont > n_stored cut inside, cut beyond",
                make_desc(L, [_cut_level(rng, 80, 65), _cut_level(rng, 140, 128), _cut_level(rng, 320, 300, n_cont=400), _cut_level(rng, 320, None, n_cont=400)])))
    # the drop test
    spot = _cloud(rng, 160)
    spot["pos"][:] = np.float32([75.25, 61.5])
    g = np.arange(256)
    lattice = level(700 - g, np.stack([40.0 * (g % 16), 40.0 * (g // 16)], 1), np.tile([1.0, 4.0], (256, 1)), rng.uniform(-np.pi, np.pi, 256))
    out.append(("one spot, wide lattice, f32 steps of the drop test, odd n", make_desc(L, [spot, lattice, _f32_step_pairs(), _cloud(rng, 7, span=8.0)])))
    # what the kernel's comment sends "the exact way": held in value where N stays finite, in class where it does not
    out.append(("near-singular finite N", make_desc(L, [_thin_level(), empty_level(), _cloud(rng, 5, span=6.0), empty_level()])))
    for name, edit in (("eig_vals[0] = 0", _zero_minor), ("both eigenvalues 0", _zero_both), ("a pos_mean NaN", _nan_mean)):
        lv = _cloud(rng, 6, span=6.0)
        edit(lv)
        out.append((name, make_desc(L, [_cloud(rng, 5, span=6.0), lv, empty_level(), _cloud(rng, 4, span=6.0)])))
    return out


def _zero_minor(lv):
    lv["eig"][2, 0] = 0.0


def _zero_both(lv):
    lv["eig"][2] = (0.0, 0.0)


def _nan_mean(lv):
    lv["pos"][2, 1] = np.nan


def _thin_level():
    """nine ellipses of eigenvalues 0.002 and 36 (axes 0.045 x 6 cells), all at the angle 0.5, strung along their major axis at 0..4,
    200, 201, 400 and 401 cells: N / 2 of every pair has det <= 1e-4 tr^2 in f32, so the f32 drop test is bypassed although most
    pairs lie further apart than |m|^2 = 400 tr; N stays positive definite and ac finite"""
    t = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 200.0, 201.0, 400.0, 401.0])
    pos = np.array([30.0, 40.0]) + t[:, None] * np.array([math.cos(0.5), math.sin(0.5)]) + 0.01 * np.arange(9)[:, None] * np.array([-math.sin(0.5), math.cos(0.5)])
    return level(300 - np.arange(9), pos, np.tile([0.002, 36.0], (9, 1)), np.full(9, 0.5))


def bypassed(E):
    """pairs of one level that the drop test would lose by distance but keeps because N / 2 is not safely positive definite in f32"""
    f = np.float32
    dx, dy = E[:, None, 4] - E[None, :, 4], E[:, None, 5] - E[None, :, 5]
    t00, t01, t10, t11 = (E[:, None, k] + E[None, :, k] for k in range(4))
    tr, det = t00 + t11, t00 * t11 - t01 * t10
    return (dx * dx + dy * dy > f(400) * tr) & ~(det > f(1e-4) * tr * tr)


def check_feat(B, oracle, log=None):
    """part A on one back end; returns the largest observed error / bound ratio of ac"""
    L = B.L
    cases = feat_cases(L)
    desc = stack([d for _, d in cases], L)
    scans = [accepted(oracle, desc[i], cases[i][0]) for i in range(len(desc))]
    raw = B.pack(desc)
    assert raw.shape[1] == feat_dt.itemsize
    feat = np.frombuffer(np.ascontiguousarray(raw).tobytes(), feat_dt)
    worst, worst_o = 0.0, 0.0
    zero = np.zeros(3)
    seen = {"flag": 0, "noflag": 0, "nonfinite": 0}
    for i, (name, _) in enumerate(cases):
        n_ell, flags, ells = feat_ref(desc[i])
        f = feat[i]
        assert f["n_ell"].tolist() == n_ell.tolist(), (name, f["n_ell"], n_ell)
        assert int(f["flags"]) == flags, (name, int(f["flags"]), flags)
        ns, _, _ = oracle.gmm_counts(scans[i], scans[i], zero)
        assert ns.tolist() == n_ell.tolist(), (name, "the oracle's own ellipse counts", ns, n_ell)
        seen["flag" if flags else "noflag"] += 1
        for li in range(NLV):
            got = f["ell"][li][:n_ell[li]]
            assert got.view(np.uint32).tolist() == ells[li].view(np.uint32).tolist(), (name, "level", li + 1, "ellipse rows differ from the f32 restatement")
        o_ac = oracle.gmm_eval(scans[i], scans[i], zero, zero)[2][0]
        if not finite_case(ells):
            seen["nonfinite"] += 1
            same = (np.isnan(o_ac) and np.isnan(f["ac"])) or (np.isinf(o_ac) and f["ac"] == o_ac) or \
                   (np.isfinite(o_ac) and np.isfinite(f["ac"]) and abs(f["ac"] - o_ac) <= 1e-12 * abs(o_ac))
            print("A %-60s not finite in the reference: oracle %r, got %r" % (name, o_ac, float(f["ac"])))
            assert same, (name, o_ac, f["ac"])
            continue
        exact = ac_exact(ells)
        S = float(exact[0])
        assert float(exact[1]) < 2.0 ** -53 * S, (name, "the dropped pairs weigh", float(exact[1]), "of", S)
        bo, To = ac_bound(ells, exact, oracle_sum=True)
        eo = float(abs(mp.mpf(float(o_ac)) - exact[0]))
        bd, Td = ac_bound(ells, exact)
        ed = float(abs(mp.mpf(float(f["ac"])) - exact[0]))
        if name == "near-singular finite N":
            assert bypassed(ells[0]).sum() >= 40 and not drop_mask(ells[0]).any(), "the thin ellipses should bypass the drop test"
        if "wide lattice" in name:
            iu = np.triu_indices(len(ells[1]))
            assert drop_mask(ells[1])[iu].mean() > 0.95, "the lattice should lose over 95 % of its pairs"
            assert ells[2].shape[0] == 6 and drop_mask(ells[2])[[0, 2, 4], [1, 3, 5]].tolist() == [False, False, True], "one step under, on, over 400 tr"
        ro, rd = (eo / bo if bo else 0.0), (ed / bd if bd else 0.0)
        line = "A %-60s n_ell %-22s T %6d of %6d  bound %.2e rel  oracle err/bound %.3f  %s err/bound %.3f (err %.2e rel)" % (
            name, n_ell.tolist(), Td, sum(len(E) * (len(E) + 1) // 2 for E in ells), bd / S if S else 0.0, ro, B.name, rd, ed / S if S else 0.0)
        print(line)
        if log is not None:
            log.append(line)
        assert eo <= bo, (name, "the oracle's own ac misses the bound", eo, bo)
        assert ed <= bd, (name, "ac", float(f["ac"]), "exact", S, "error", ed, "bound", bd)
        worst, worst_o = max(worst, rd), max(worst_o, ro)
    assert seen["flag"] == 1 and seen["nonfinite"] == 3, seen
    return worst, worst_o


# ---- B / C. pose descriptors -------------------------------------------------------------------------------------------
def _grid_level(rng, n, dx=0.0, w0=900):
    """n ellipses on a 20-column grid of 30-cell steps, major axis 2 cells (9 for every seventh: it reaches its four neighbours)"""
    i = np.arange(n)
    e1 = np.where(i % 7 == 3, 81.0, 4.0)
    return level(w0 - i, np.stack([30.0 * (i % 20) + 5 + dx, 30.0 * (i // 20) + 5], 1), np.stack([e1 / 2, e1], 1), rng.uniform(-np.pi, np.pi, n))


def squares(N):
    """N as a sum of squares, greedy, each root <= 48 and the first square at most 0.55 N: an item then has at least two large
    islands (a single island leaves the rotation about it nearly free, and the refinement without a unique optimum)"""
    out = []
    first = N >= 8
    while N > 0:
        m = min(48, int(math.isqrt(int(0.55 * N) if first else N)))
        first = False
        out.append(m)
        N -= m * m
    return out


def island_centres(rng, k, lo=20.0, hi=250.0, sep=40.0):
    c = []
    while len(c) < k:
        p = rng.uniform(lo, hi, 2)
        if all(np.hypot(*(p - q)) >= sep for q in c):
            c.append(p)
    return c


def island_desc(L, rng, sizes_per_level, centres_per_level, shift=None):
    """one descriptor whose level li holds islands of sizes_per_level[li] ellipses at centres_per_level[li] (+ shift[li])"""
    lv = []
    for li in range(NLV):
        sz = sizes_per_level[li]
        n = int(sum(sz))
        if n == 0:
            lv.append(empty_level())
            continue
        pos = np.concatenate([np.asarray(c) + (0 if shift is None else np.asarray(shift[li])) + rng.uniform(-0.28, 0.28, (m, 2))
                              for m, c in zip(sz, centres_per_level[li])])
        order = rng.permutation(n)   # the table's order is by weight, not by island
        e1 = rng.uniform(4.0, 9.0, n)
        lv.append(level(1000 - np.arange(n), pos[order], np.stack([rng.uniform(1.0, 4.0, n), e1], 1), rng.uniform(-np.pi, np.pi, n)))
    return make_desc(L, lv)


C_COUNTS = (1, 2, 16, 17, 32, 33, 96, 97, 128, 129, 256, 257, 500, 501, 1279, 1280, 1281, 1400, 1401, 2304, 2305)
PLACES = (0.0, 4000.0, -4000.0, 4095.5, 4096.5)
GRAZE_EPS = (2.0 ** -20, 2.0 ** -40, 2.0 ** -46)
SRC_A, SRC_B, TGT_X, TGT_Y = (1, 15, 16, 17), (63, 64, 65, 320), (1, 7, 8, 9), (63, 64, 65, 320)


class PoseSet:
    """the descriptors of parts B and C (one database holds them all) and their items"""

    def __init__(self, L):
        rng = np.random.default_rng(77)
        self.L, self.desc, self.items, self.kind = L, [], [], []

        def add(d):
            self.desc.append(d)
            return len(self.desc) - 1
        # grazing: one src ellipse; five tgt ellipses 10^3 cells apart in y, at x = place - threshold
        self.graze, self.expect = [], {}
        for maj in (0.5, 60.0, "off the f32 grid"):
            e = np.float32(0.3 if isinstance(maj, str) else maj * maj)
            src = level([500], [[10.0, 20.0]], [[e / 2, e]], [0.3])
            thr = 3.0 * float(np.float32(np.sqrt(e) + np.sqrt(e)))
            tx_pos = np.float32(np.array(PLACES) - thr)
            if isinstance(maj, str):
                # With this axis the threshold has bits below the f32 step at 4 000 (2.4e-4), and each tgt is moved along the f32
                # grid until the f32 image of a src 2^-20 INSIDE the threshold lies clearly outside it (rounded up by more than
                # the slack): only the margin of the conservative f32 test keeps such a pair.
                n_moved = 0
                for k in range(5):
                    x = tx_pos[k]
                    for _ in range(64):
                        sx = float(x) + thr * (1.0 - 2.0 ** -20)
                        if float(np.float32(np.float32(sx) - x)) > thr * (1.0 + 1e-6):
                            tx_pos[k], n_moved = x, n_moved + 1
                            break
                        x = np.nextafter(x, np.float32(1e9))
                assert n_moved >= 4, "the tgts near +-4 000 and 4 096 should find such a place"
            tgt = level(500 - np.arange(5), np.stack([tx_pos, 20.0 + 1000.0 * np.arange(5)], 1), np.tile([e / 2, e], (5, 1)), 0.7 * np.arange(5))
            s, t = add(make_desc(L, [src, empty_level(), empty_level(), empty_level()])), add(make_desc(L, [tgt, empty_level(), empty_level(), empty_level()]))
            for k in range(5):
                for eps in GRAZE_EPS:
                    for sg in (-1.0, 1.0):
                        dist = thr * (1.0 + sg * eps)
                        tf = (float(tx_pos[k]) + dist - 10.0, 1000.0 * k, 0.0)
                        self._item(t, s, tf, "graze maj %s place %g eps %+.0e" % (maj, PLACES[k], sg * eps))
                        self.graze.append(len(self.items) - 1)
        # chunk shapes: every (src count, tgt count) of the two lists on some level
        tg = {}
        for name, cnts in (("X", TGT_X), ("Y", TGT_Y)):
            tg[name] = add(make_desc(L, [_grid_level(rng, n, dx=0.4) for n in cnts]))
        for cnts in (SRC_A, SRC_B):
            for r in range(4):
                s = add(make_desc(L, [_grid_level(rng, cnts[(li + r) % 4]) for li in range(NLV)]))
                for name in ("X", "Y"):
                    self._item(tg[name], s, (0.3, -0.2, 0.002), "chunk shapes src %s rot %d tgt %s" % (cnts, r, name))
        # the only hits on the last tgt of a full chunk, the first of the next, and the last of a partial chunk; empty levels between
        far = level(900 - np.arange(100), np.stack([35.0 * np.arange(100), np.full(100, 50.0)], 1), np.tile([2.0, 4.0], (100, 1)), rng.uniform(-3, 3, 100))
        hit = level([300, 200, 100], far["pos"][[63, 64, 99]] + 0.3, np.tile([2.0, 4.0], (3, 1)), [0.1, 0.2, 0.3])
        t, s = add(make_desc(L, [far, empty_level(), empty_level(), far])), add(make_desc(L, [hit, empty_level(), empty_level(), hit]))
        self._item(t, s, (0.0, 0.0, 0.0), "chunk edges")
        z = add(make_desc(L, [empty_level()] * 4))
        self._item(z, z, (0.0, 0.0, 0.0), "all levels empty")
        self._item(t, z, (0.0, 0.0, 0.0), "empty src")
        # dense blocks: level li's tgt island stands 1 000 cells along direction li from its src island
        cen = [[np.array([60.0, 70.0])], [np.array([80.0, 50.0])], [np.array([100.0, 90.0])], []]
        dirs = [(1000.0, 0.0), (0.0, 1000.0), (-1000.0, 0.0), (0.0, 0.0)]
        s = add(island_desc(L, rng, [[64], [16], [320], []], cen))
        t = add(island_desc(L, rng, [[64], [64], [320], []], cen, shift=dirs))
        self.dense = {}
        for li, name in enumerate(("64 x 64", "16 x 64", "320 x 320")):
            self._item(t, s, (dirs[li][0] + 0.2, dirs[li][1] - 0.1, 0.0), "dense " + name)
            self.dense[name] = len(self.items) - 1
            self.expect[len(self.items) - 1] = (64 * 64, 16 * 64, 320 * 320)[li]
        # the lane-by-lane filing at its flush edge: four src ellipses reach all 64 tgts of a chunk, a fifth (20 cells off) only the
        # first tgt, whose major axis is 9 cells: the block's 257 hits arrive as 64, 64, 64, 64, 1
        P0 = np.array([120.0, 140.0])
        e1 = np.full(64, 4.0)
        e1[0] = 81.0
        t = add(make_desc(L, [level(900 - np.arange(64), P0 + rng.uniform(-0.28, 0.28, (64, 2)), np.stack([e1 / 2, e1], 1), rng.uniform(-3, 3, 64)),
                              empty_level(), empty_level(), empty_level()]))
        sp = P0 + rng.uniform(-0.28, 0.28, (5, 2))
        sp[4] = P0 + (20.0, 0.0)
        s = add(make_desc(L, [level(900 - np.arange(5), sp, np.tile([2.0, 4.0], (5, 1)), rng.uniform(-3, 3, 5)), empty_level(), empty_level(), empty_level()]))
        self._item(t, s, (0.1, 0.1, 0.0), "flush edge 4 x 64 + 1")
        self.expect[len(self.items) - 1] = 257
        self.n_b = len(self.items)
        # part C: N = sum of squares, an island of m ellipses per square, src = tgt = the same descriptor
        self.c_items = {}
        signs = [(1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1), (1, 1, -1), (-1, -1, 1)]
        for k, N in enumerate(C_COUNTS):
            sq = squares(N)
            per = [[m for j, m in enumerate(sq) if j % NLV == li] for li in range(NLV)]
            per = per[k % NLV:] + per[:k % NLV]   # which level holds the largest island changes from item to item
            assert all(sum(p) <= ECAP for p in per)
            cen = island_centres(rng, len(sq))
            cpl, it = [], iter(cen)
            for p in per:
                cpl.append([next(it) for _ in p])
            d = add(island_desc(L, rng, per, cpl))
            self._item(d, d, np.array(signs[k % 6]) * np.array([0.5, 0.5, 0.01]), "C %d pairs" % N)
            self.c_items[N] = len(self.items) - 1
        self.desc = stack(self.desc, L)
        self.items_arr = L.pose_items([i[0] for i in self.items], [i[1] for i in self.items], [i[2] for i in self.items])

    def _item(self, q, gidx, tf, kind):
        self.items.append((q, gidx, np.asarray(tf, np.float64)))
        self.kind.append(kind)


_sets = {}


def pose_set(L, oracle):
    if "P" not in _sets:
        P = PoseSet(L)
        P.scans = [accepted(oracle, P.desc[i], ("pose descriptor", i)) for i in range(len(P.desc))]
        P.feat = [feat_ref(P.desc[i]) for i in range(len(P.desc))]
        _sets["P"] = P
    return _sets["P"]


def pairs_ref(fs, ft, tf):
    """GMMPair's ctor (correlation.h:85-96) in numpy f64 on the restated tables: T_init applied as written (R mu + t, the matrix
    entries cos / sin of the C library), kept if sqrt(dx^2 + dy^2) < 3.0 * f64(f32(maj_s + maj_t)) -> [(si, ti) index arrays per level]"""
    c, s = math.cos(tf[2]), math.sin(tf[2])
    out = []
    for li in range(NLV):
        Es, Et = fs[2][li], ft[2][li]
        mx, my = Es[:, 4].astype(np.float64), Es[:, 5].astype(np.float64)
        sx, sy = c * mx + (-s) * my + tf[0], s * mx + c * my + tf[1]
        dx, dy = sx[:, None] - Et[None, :, 4].astype(np.float64), sy[:, None] - Et[None, :, 5].astype(np.float64)
        thr = 3.0 * (Es[:, None, 7] + Et[None, :, 7]).astype(np.float64)
        out.append(np.nonzero(np.sqrt(dx * dx + dy * dy) < thr))
    return out


def smallest_term(fs, ft, tf, sel, nrm):
    """the smallest selected pair's term at T_init over sqrt(ac_src ac_tgt), in plain f64 (for the assertion on the reference only)"""
    c, s = math.cos(tf[2]), math.sin(tf[2])
    R = np.array([[c, -s], [s, c]])
    small = np.inf
    for li in range(NLV):
        si, ti = sel[li]
        if not len(si):
            continue
        Es, Et = fs[2][li][si].astype(np.float64), ft[2][li][ti].astype(np.float64)
        Cs = Es[:, :4].reshape(-1, 2, 2)
        N = 2.0 * (R @ Cs @ R.T + Et[:, :4].reshape(-1, 2, 2))
        mu = Es[:, 4:6] @ R.T + np.array(tf[:2]) - Et[:, 4:6]
        det = N[:, 0, 0] * N[:, 1, 1] - N[:, 0, 1] * N[:, 1, 0]
        E = mu[:, 0] ** 2 * N[:, 1, 1] - mu[:, 0] * mu[:, 1] * (N[:, 0, 1] + N[:, 1, 0]) + mu[:, 1] ** 2 * N[:, 0, 0]
        small = min(small, float((Es[:, 6] * Et[:, 6] / np.sqrt(det) * np.exp(-E / (2 * det))).min()))
    return small / nrm


def _run_split(B, h, items, refine, tries, per_call):
    """the items in calls of at most per_call, rows in item order"""
    rs, ts = [], []
    for b0 in range(0, len(items), per_call):
        r, t = B.pose(h, items[b0:b0 + per_call], refine, None if tries is None else np.ascontiguousarray(tries[b0:b0 + per_call]))
        rs.append(r)
        ts.append(t)
    return np.concatenate(rs), (None if tries is None else np.concatenate(ts))


def check_selection(B, oracle, skip=()):
    """part B.  skip: kinds a back end leaves out (named in its module)"""
    L = B.L
    P = pose_set(L, oracle)
    idx = [i for i in range(P.n_b) if P.kind[i] not in skip]
    items = P.items_arr[idx]
    tries = np.ascontiguousarray(items["tf"][:, None, :])
    h = B.open(P.desc, small_grid=False)
    sw = B.switch(h)
    # once as short calls: the wave-per-problem instance (a chunk of at most `sw` problems)
    per = min(sw, 64)
    rw, tw = _run_split(B, h, items, 0, tries, per)
    # ... and once in a call whose chunks all hold more than the switch point: two chunks of n / 2, n a multiple of 128
    h2 = B.open(P.desc, small_grid=True)
    sw2 = B.switch(h2)
    n_big = max(128 * (-(-len(items) // 128)), 128 * (-(-(2 * sw2 + 2) // 128)))
    assert n_big // 2 > sw2 and n_big // 2 <= 1024, (n_big, sw2)
    rep = np.arange(n_big) % len(items)
    rg, tg = B.pose(h2, items[rep], 0, np.ascontiguousarray(tries[rep]))
    rg, tg = rg[:len(items)], tg[:len(items)]
    mx = {"try": 0.0, "same": 0.0}
    n_sel = {0: 0, 1: 0}
    for k, i in enumerate(idx):
        q, g, tf = P.items[i]
        what = (i, P.kind[i])
        sel = pairs_ref(P.feat[g], P.feat[q], tf)
        n_ref = sum(len(s[0]) for s in sel)
        _, _, on = oracle.gmm_counts(P.scans[g], P.scans[q], tf)
        assert int(on.sum()) == n_ref, (what, "the oracle's count against the numpy expression", on, n_ref)
        assert n_ref == P.expect.get(i, n_ref), (what, "the layout does not give the intended count", n_ref)
        assert int(rw[k]["n_pairs"]) == n_ref, (what, "n_pairs, wave per problem", int(rw[k]["n_pairs"]), n_ref)
        assert int(rg[k]["n_pairs"]) == n_ref, (what, "n_pairs, 16 lanes per problem", int(rg[k]["n_pairs"]), n_ref)
        if i in P.graze:
            n_sel[min(n_ref, 1)] += 1
        if n_ref == 0:
            assert tw[k, 0] == 0.0 and tg[k, 0] == 0.0, what
            continue
        cost, _, ac = oracle.gmm_eval(P.scans[g], P.scans[q], tf, tf)
        nrm = math.sqrt(ac[0] * ac[1])
        ref = -cost / nrm
        small = smallest_term(P.feat[g], P.feat[q], tf, sel, nrm)
        assert small > 1e3 * PC.TRY_BAR, (what, "a lost pair would hide under the bar", small)
        mx["try"] = max(mx["try"], abs(tw[k, 0] - ref), abs(tg[k, 0] - ref))
        mx["same"] = max(mx["same"], abs(tw[k, 0] - tg[k, 0]), abs(rw[k]["corr_init"] - rg[k]["corr_init"]))
        for r in (rw[k], rg[k]):   # (the try is cc_k_pose_eval's sum over the codes init filed, corr_init is init's own sum)
            mx["try"] = max(mx["try"], abs(r["corr_init"] - ref))
            assert abs(r["corr_init"] - ref) < PC.TRY_BAR, (what, "corr_init", r["corr_init"], ref, n_ref)
        assert abs(tw[k, 0] - ref) < PC.TRY_BAR, (what, "wave per problem", tw[k, 0], ref, n_ref)
        assert abs(tg[k, 0] - ref) < PC.TRY_BAR, (what, "16 lanes per problem", tg[k, 0], ref, n_ref)
        assert abs(tw[k, 0] - tg[k, 0]) <= PC.SAME_BAR and abs(rw[k]["corr_init"] - rg[k]["corr_init"]) <= PC.SAME_BAR, what
        assert abs(tw[k, 0] - rw[k]["corr_init"]) < PC.INIT_BAR, what
    assert n_sel[0] >= 10 and n_sel[1] >= 10, ("the grazing items should fall on both sides", n_sel)
    line = "B %s: %d items (short calls of <= %d items; the large call: %d-problem grid, %d items); max |try, corr_init - oracle| %.2e, between the instances %.2e; grazing items selected / not %d / %d" % (
        B.name, len(idx), per, sw2, n_big, mx["try"], mx["same"], n_sel[1], n_sel[0])
    print(line)
    return line


def check_lists(B, oracle):
    """part C; returns the rows.  The 97..256 items run twice: with all the items (21 selected problems) and in a call of their own
    (4): a library whose CC_GMM_PACK_MIN_PROBLEMS lies between the two sends the first run to the packed 16-lane instance."""
    L = B.L
    P = pose_set(L, oracle)
    idx = [P.c_items[N] for N in C_COUNTS]
    items = P.items_arr[idx]
    h = B.open(P.desc, small_grid=False)
    res, _ = B.pose(h, items, 1, None)
    mid = [k for k, N in enumerate(C_COUNTS) if 97 <= N <= 256]
    res2, _ = B.pose(h, items[mid], 1, None)   # the in-between items in a call of their own (few problems: a wave each)
    mx = {"corr_init": 0.0, "corr": 0.0, "tf": 0.0}
    for k, N in enumerate(C_COUNTS):
        q, g, tf = P.items[idx[k]]
        r = res[k]
        what = ("C", N)
        _, _, on = oracle.gmm_counts(P.scans[g], P.scans[q], tf)
        assert int(on.sum()) == N, (what, "the layout does not give N pairs in the reference", on)
        ci, co, tfo, st = oracle.gmm(P.scans[g], P.scans[q], tf)
        assert int(st[1]) >= 0, (what, "the oracle's own line search fails from this start: choose another layout", st)
        assert int(r["n_pairs"]) == N, (what, int(r["n_pairs"]))
        assert r["flags"] & L.PF_REFINED, what
        mx["corr_init"] = max(mx["corr_init"], abs(ci - r["corr_init"]))
        mx["corr"] = max(mx["corr"], abs(co - r["correlation"]))
        mx["tf"] = max(mx["tf"], float(PC.tf_diff(tfo, r["tf"]).max()))
        assert abs(ci - r["corr_init"]) < TOL, (what, ci, r["corr_init"])
        assert abs(co - r["correlation"]) < TOL, (what, co, r["correlation"])
        assert PC.tf_diff(tfo, r["tf"]).max() < TOL, (what, tfo, r["tf"])
        assert (int(st[0]), int(st[1])) == (int(r["iterations"]), int(r["termination"])), (what, st, r["iterations"], r["termination"])
    PC.rows_close(res2, res[mid], "the 97..256 items in a call of their own")
    two = max(np.abs(res2["correlation"] - res[mid]["correlation"]).max(), float(PC.tf_diff(res2["tf"], res[mid]["tf"]).max()))
    line = "C %s: %d items, every one compared in full; max |corr_init| %.2e |corr| %.2e |tf| %.2e; the 97..256 items between their two calls %.2e" % (
        B.name, len(idx), mx["corr_init"], mx["corr"], mx["tf"], two)
    print(line)
    return res


def write_golden():
    """rewrite tests/golden/gmm_inputs_ac.json from the cases above"""
    import oracle_py
    global _golden
    _golden = {}
    for nm, d in feat_cases(oracle_py.L):
        e = feat_ref(d)[2]
        if finite_case(e):
            print(nm, ac_exact(e))
    json.dump(_golden, open(GOLDEN, "w"), indent=0, sort_keys=True)


if __name__ == "__main__":   # PYTHONPATH=oracle python tests/gmm_cases.py
    write_golden()
