"""TEST INFRASTRUCTURE: a plain numpy restatement of the retrieval-key phase (ContourManager::makeContoursRecurs, the part that fills
layer_keys_; gaussPDF of tools/algos.h), independent of the oracle's C++ and of the device code, with a verdict on every component:
decidable to the bit, or provably ambiguous.

Every step of a key component is an individually rounded IEEE operation in a fixed order -- restated here with numpy's f32 / f64
scalars operation by operation -- except one f64 exp per (cell, division).  That one is computed here in long double and rounded
the way the reference rounds it (to f64, then to f32), and a term is AMBIGUOUS when an error of W * 2^-53 relative to the exact
value, in either direction, can move that f32.  A ring component is ambiguous when any of its terms is.

W, in units of u = 2^-53 (half an ulp of an f64 significand; one ulp of a value is at most 2 u of it).  With s = the double
sqrt(2 * M_PI) and E = exp(z) / s the exact quotient (z = -u^2 / 2 is exact in f64: u is an f32):
  * the reference computes fl(glibc exp(z) / s): exp within 1 ulp (glibc documents less) = 2 u, the quotient's rounding 1 u: 3 u;
  * the device computes fl(cc_exp_nonpos(z) * C), C = 0.3989422804014327: exp within EXP_NONPOS_ULP ulp (csrc/cc_fmath.h derives
    it, tests/primitive_cases.py holds the device to it) = 2 * EXP_NONPOS_ULP u, the product's rounding 1 u, and |C * s - 1| / u
    for multiplying by C where the reference divides by s (computed below in long double: 0.375 u);
  * this module's own exp / division in long double: 2^-10 u each at most (LD_SLACK of primitive_cases.py), 2 * LD_SLACK with room.
W = max(3, 2 * EXP_NONPOS_ULP + 1 + |C * s - 1| / u) + 2 * LD_SLACK, second-order terms (u^2) being far below the slack: 4.08.
The expected share of ambiguous terms is W * 2^-53 * 2^24 * 2 ~ 1.5e-8."""
import numpy as np

from primitive_cases import EXP_NONPOS_ULP, LD_SLACK

LD = np.longdouble
F32, F64 = np.float32, np.float64
M_PI = 3.14159265358979323846
DEV_INV_SQRT_2PI = 0.3989422804014327            # the constant csrc/k_contours.h multiplies by
SQRT_2PI = np.sqrt(F64(2.0) * F64(M_PI))         # what the reference divides by: std::sqrt(2 * M_PI * sd * sd), sd = 1
U = LD(2.0) ** -53
CONST_DIST_U = float(abs(LD(DEV_INV_SQRT_2PI) * LD(SQRT_2PI) - LD(1)) / U)
W = max(3.0, 2.0 * EXP_NONPOS_ULP + 1.0 + CONST_DIST_U) + 2.0 * LD_SLACK
assert np.finfo(LD).nmant >= 63, "the reference's exp needs a long double wider than f64"
assert CONST_DIST_U < 1.0 and 3.0 < W < 5.0, (CONST_DIST_U, W)

NLEV, NPIV, KEY_DIM, NBIN, DIV_PER_BIN = 6, 6, 10, 7, 5
NDIV = NBIN * DIV_PER_BIN
RTOL_AMBIGUOUS = 1e-5


def _to_f32(x):
    """long double -> f64 -> f32, the reference's two roundings (`return` of a double expression from gaussPDF<float>)"""
    return np.asarray(x, LD).astype(F64).astype(F32)


def roi_list(bev, pix_rc, cfg, v_cen):
    """The RoI cells of an anchor at v_cen (f32 pair), in raster order: (f32 distances, `higher` counts)."""
    n_row, n_col = int(cfg.n_row), int(cfg.n_col)
    grads = np.array([cfg.lv_grads[i] for i in range(NLEV)], F32)
    pad = int(np.ceil(F32(cfg.roi_radius) + F32(1.0)))
    r_cen, c_cen = int(v_cen[0]), int(v_cen[1])
    r_min, r_max = max(0, r_cen - pad), min(n_row - 1, r_cen + pad)
    c_min, c_max = max(0, c_cen - pad), min(n_col - 1, c_cen + pad)
    rr, cc = np.meshgrid(np.arange(r_min, r_max + 1), np.arange(c_min, c_max + 1), indexing="ij")
    cell = (rr * n_col + cc).ravel()                       # raster order
    h = bev[cell]
    dx = pix_rc[cell, 0] - F32(v_cen[0])
    dy = pix_rc[cell, 1] - F32(v_cen[1])
    dist = np.sqrt(dx * dx + dy * dy)                      # f32 arrays: each product, the sum and the root rounded once
    assert dist.dtype == F32
    keep = (dist.astype(F64) < F64(F32(cfg.roi_radius)) - 1e-2) & (h > grads[1])
    higher = (h[:, None] > grads[None, 1:]).sum(1)
    return dist[keep], higher[keep].astype(np.int32)


def ring_components(dist, higher, roi_radius):
    """-> (seven f32 ring components, seven ambiguity flags) of a list"""
    n = len(dist)
    roi = F32(roi_radius)
    div_len = F32(roi / F32(NDIV))
    bin_len = F32(roi / F32(NBIN))
    xg = np.array([F32(F64(F32(F32(d) * div_len)) + 0.5 * F64(div_len)) for d in range(NDIV)], F32)
    divs = np.zeros(NDIV, F32)
    amb_div = np.zeros(NDIV, bool)
    if n:
        u = (xg[None, :] - dist[:, None]).astype(F32)      # [n, 35], one f32 subtraction each
        z = -0.5 * u.astype(F64) * u.astype(F64)           # exact
        e = np.exp(z.astype(LD)) / LD(SQRT_2PI)
        pdf = _to_f32(e)
        amb = _to_f32(e * (LD(1) - LD(W) * U)) != _to_f32(e * (LD(1) + LD(W) * U))
        term = (higher.astype(F32)[:, None] * pdf).astype(F32)
        divs = np.add.accumulate(term, axis=0, dtype=F32)[-1]   # sequential, in list order; never np.sum (pairwise)
        amb_div = amb.any(0)
    rings = np.zeros(NBIN, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = F64(bin_len) / np.sqrt(F64(n))             # n = 0: inf, and 0 * inf = NaN as in the reference
        for b in range(NBIN):
            ring = F32(0.0)
            for d in range(DIV_PER_BIN):
                ring = F32(ring + divs[b * DIV_PER_BIN + d])
            rings[b] = F32(F64(ring) * scale)
    return rings, amb_div.reshape(NBIN, DIV_PER_BIN).any(1)


def key_reference(bev, pix_rc, cont, n_stored, cfg):
    """bev [n_cell] f32 and pix_rc [n_cell, 2] f32 of one scan, cont = its descriptor's contour rows [6][..] (pos_mean, cell_cnt,
    eig_vals), n_stored [6], cfg the manager config -> (keys [6, 6, 10] f32, ambiguous [6, 6, 10] bool, n_list [6, 6] int: the RoI
    list length of each valid anchor, -1 for an anchor without a key)."""
    bev = np.ascontiguousarray(bev, F32).reshape(-1)
    pix_rc = np.ascontiguousarray(pix_rc, F32).reshape(-1, 2)
    keys = np.zeros((NLEV, NPIV, KEY_DIM), F32)
    ambiguous = np.zeros((NLEV, NPIV, KEY_DIM), bool)
    n_list = np.full((NLEV, NPIV), -1, np.int64)
    for ll in range(NLEV):
        acc = 0
        for seq in range(min(int(cfg.piv_firsts), NPIV)):
            if seq < int(n_stored[ll]):
                acc += int(cont[ll][seq]["cell_cnt"])
            if not (seq < int(n_stored[ll]) and int(cont[ll][seq]["cell_cnt"]) >= int(cfg.min_cont_key_cnt)):
                continue
            row = cont[ll][seq]
            dist, higher = roi_list(bev, pix_rc, cfg, row["pos_mean"].astype(F32))
            n_list[ll, seq] = len(dist)
            cnt = F32(int(row["cell_cnt"]))
            keys[ll, seq, 0] = np.sqrt(F32(F32(row["eig_vals"][1]) * cnt))
            keys[ll, seq, 1] = np.sqrt(F32(F32(row["eig_vals"][0]) * cnt))
            keys[ll, seq, 2] = F32(np.sqrt(F64(acc)))
            keys[ll, seq, 3:], ambiguous[ll, seq, 3:] = ring_components(dist, higher, cfg.roi_radius)
    return keys, ambiguous, n_list


def check_keys(ref_keys, ambiguous, got_keys, ignore=None):
    """The verdict: a component that is not ambiguous has the reference's bits (NaN meets NaN), an ambiguous one lies within
    RTOL_AMBIGUOUS of it.  `ignore` [6, 6, 10] bool takes components out (the rings of an anchor whose list the device clamps).
    Raises AssertionError naming the offenders; returns the number of ambiguous components compared."""
    ref = np.asarray(ref_keys, F32).reshape(NLEV, NPIV, KEY_DIM)
    got = np.asarray(got_keys, F32).reshape(NLEV, NPIV, KEY_DIM)
    amb = np.asarray(ambiguous, bool).reshape(ref.shape)
    use = np.ones(ref.shape, bool) if ignore is None else ~np.asarray(ignore, bool).reshape(ref.shape)
    same = (ref.view(np.uint32) == got.view(np.uint32)) | (np.isnan(ref) & np.isnan(got))
    with np.errstate(invalid="ignore"):
        near = np.abs(got.astype(F64) - ref.astype(F64)) <= RTOL_AMBIGUOUS * np.abs(ref.astype(F64))
    bad = use & ~np.where(amb, same | near, same)
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError("%d key components differ from the key reference, first: %s" % (
            len(idx), ["(level %d, seq %d, k %d) ref %r (0x%08x) got %r (0x%08x)%s" % (
                l, s, k, float(ref[l, s, k]), int(ref.view(np.uint32)[l, s, k]), float(got[l, s, k]), int(got.view(np.uint32)[l, s, k]),
                " ambiguous" if amb[l, s, k] else "") for l, s, k in idx[:6]]))
    return int((amb & use).sum())


def scan_reference(oracle_scan, oracle_desc, cfg):
    """key_reference on an oracle.Scan and its exported descriptor record"""
    bev, pix = oracle_scan.bev()
    return key_reference(bev, pix, oracle_desc["cont"], oracle_desc["n_stored"], cfg)

