"""TEST INFRASTRUCTURE: cases, references and checks of the primitives every kernel stands on, shared by
tests/test_emu_primitives.py (CPU harness), tests/test_gpu_primitives.py (MI355X), tests/test_sort_replica.py and
tests/test_atan2f_replica.py.  A check takes a probe backend of tests/dev_probe.py (`P`) and, where device and harness must
agree bit for bit, the other backend (`other`); it returns the figures it observed (docs: DESIGN.md section 6).

References: plain numpy on the lanes' operands, exact integer / fractions.Fraction arithmetic, numpy.longdouble (64-bit
mantissa) for bulk passes and mpmath at 50 digits for the sampled and the worst arguments."""
import ctypes as C
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the bulk references need the 80-bit long double"

# ---------------------------------------------------------------------------------------------------------------------
# A. row and wave collectives (csrc/cc_group.h)
# ---------------------------------------------------------------------------------------------------------------------
BALLOT, SCAN, SUM_I, OR_U, BEST, BCAST, SUM_D, QUAD, SHR, SHL1, GSUM64, WSCAN, MASK, BITS = range(14)
GROUP_OPS = {"ballot": BALLOT, "scan_incl": SCAN, "sum_i": SUM_I, "or_u": OR_U, "best": BEST, "bcast": BCAST, "sum_d": SUM_D,
             "quad_bcast": QUAD, "row_shr": SHR, "row_shl1": SHL1, "mbcnt_mask_lane": MASK, "push_sign_brev": BITS}
WAVE_OPS = {"gsum64": GSUM64, "wave_scan": WSCAN}   # every lane of the wave takes part (the headers' contract)
N_BLOCKS = 64
SENT_I = np.int32(0x5A5A5A5A)
SENT_D = np.uint64(0x7FF8DEADBEEF0001)
# all 15 non-empty sets of rows with the others returned early, then the two if / else patterns
MODES = list(range(1, 16)) + [16, 17]


def _rand_doubles(rng, n):
    """mixed signs, magnitudes 1e-300 .. 1e300: the order of addition shows in a sum"""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-300, 300, n)).astype(np.float64)


def _special_f32_bits(rng, n):
    sp = np.array([0x00000000, 0x80000000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x00000001, 0x80000001, 0x007FFFFF,
                   0x807FFFFF, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000], np.uint32)
    a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    k = rng.random(n) < 0.5
    a[k] = sp[rng.integers(0, len(sp), int(k.sum()))]
    return a.view(np.int32)


def group_operands(op, block, seed):
    """one operand set: a, b (int32), d (float64) per thread, m (uint64) per wave"""
    rng = np.random.default_rng(seed)
    n = N_BLOCKS * block
    a = rng.integers(-2 ** 24, 2 ** 24 + 1, n).astype(np.int32)
    b = rng.integers(-2 ** 24, 2 ** 24 + 1, n).astype(np.int32)
    d = _rand_doubles(rng, n)
    m = rng.integers(0, 2 ** 64, n // 64, dtype=np.uint64)
    m[0], m[1] = 0, 0xFFFFFFFFFFFFFFFF
    if op == BALLOT:   # predicate densities 0, 1/16, 1/2, 1: a quarter of the workgroups each
        dens = np.repeat(np.array([0.0, 1 / 16, 0.5, 1.0]), n // 4)
        a = ((a & ~1) | (rng.random(n) < dens)).astype(np.int32)
    elif op == OR_U:
        a = (rng.integers(0, 2 ** 32, n, dtype=np.uint64) & rng.integers(0, 2 ** 32, n, dtype=np.uint64)
             & rng.integers(0, 2 ** 32, n, dtype=np.uint64)).astype(np.uint32).view(np.int32)
    elif op == BEST:   # many ties in a, and in (a, b)
        a = rng.integers(-2, 2, n).astype(np.int32)
        b = rng.integers(0, 6, n).astype(np.int32)
    elif op == BCAST:
        d = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)
    elif op in (QUAD, BITS):
        a = _special_f32_bits(rng, n)
        b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)
    elif op in (SHR, SHL1):
        a = (a | 1).astype(np.int32)   # never 0: the zeros beyond a row's ends are the primitive's
    return a, b, d, m


def _sum_d_rows(v):
    """the double sum over the 16 lanes of each row in the association csrc/cc_group.h spells out: xor 1, xor 2, half-row
    mirror, row mirror (every step an IEEE addition of two f64 values, as numpy's)"""
    sl = np.arange(16)
    v = v + v[:, sl ^ 1]
    v = v + v[:, sl ^ 2]
    v = v + v[:, (sl & 8) | (7 - (sl & 7))]
    v = v + v[:, 15 - sl]
    return v


def group_expected(op, a, b, d, m):
    """(ints [n, 4], doubles [n]) every lane would hold with every lane taking part; m: the wave's mask, per thread"""
    n = len(a)
    ei = np.zeros((n, 4), np.int32)
    ed = np.zeros(n, np.float64)
    A, B, D = a.reshape(-1, 16), b.reshape(-1, 16), d.reshape(-1, 16)
    sl = np.arange(16)
    lane = (np.arange(n) & 63).astype(np.uint64)
    with np.errstate(all="ignore"):
        if op == BALLOT:
            ei[:, 0] = np.repeat((((A & 1).astype(np.int64)) << sl).sum(1), 16)
        elif op == SCAN:
            ei[:, 0] = np.cumsum(A.astype(np.int64), 1).ravel()
        elif op == SUM_I:
            ei[:, 0] = np.repeat(A.astype(np.int64).sum(1), 16)
        elif op == OR_U:
            ei[:, 0] = np.repeat(np.bitwise_or.reduce(A, 1), 16)
        elif op == BEST:
            amax = A.max(1, keepdims=True)
            bmin = np.where(A == amax, B, np.iinfo(np.int32).max).min(1)
            ei[:, 0], ei[:, 1] = np.repeat(amax[:, 0], 16), np.repeat(bmin, 16)
        elif op == BCAST:
            src = B & 15
            ei[:, 0] = np.take_along_axis(A, src, 1).ravel()
            ed = np.take_along_axis(D.view(np.uint64), src.astype(np.int64), 1).ravel().view(np.float64)
        elif op == SUM_D:
            ed = _sum_d_rows(D).ravel()
        elif op == GSUM64:
            w = d.reshape(-1, 64)
            l64 = np.arange(64)
            w = w + w[:, l64 ^ 32]
            w = w + w[:, l64 ^ 16]
            ed = _sum_d_rows(w.reshape(-1, 16)).ravel()
        elif op == QUAD:
            q = a.reshape(-1, 4)
            for k in range(4):
                ei[:, k] = np.repeat(q[:, k], 4)
        elif op == SHR:
            for k, dist in enumerate((1, 2, 4, 8)):
                s = np.zeros_like(A)
                s[:, dist:] = A[:, :-dist]
                ei[:, k] = s.ravel()
        elif op == SHL1:
            s = np.zeros_like(A)
            s[:, :-1] = A[:, 1:]
            ei[:, 0] = s.ravel()
        elif op == WSCAN:
            w = np.cumsum(a.reshape(-1, 64).astype(np.int64), 1)
            ei[:, 0] = w.ravel()
            ei[:, 1] = np.repeat(w[:, 63], 64)
        elif op == MASK:
            below = m & ((np.uint64(1) << lane) - np.uint64(1))
            ei[:, 0] = [bin(int(x)).count("1") for x in below]
            ei[:, 1] = ((m >> lane) & np.uint64(1)).astype(np.int32)
        elif op == BITS:
            ua, ub = a.view(np.uint32).astype(np.uint64), b.view(np.uint32).astype(np.uint64)
            ei[:, 0] = (((ub << np.uint64(1)) | (ua >> np.uint64(31))) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
            rev = np.zeros(n, np.uint64)
            for i in range(32):
                rev |= ((ua >> np.uint64(i)) & np.uint64(1)) << np.uint64(31 - i)
            ei[:, 1] = rev.astype(np.uint32).view(np.int32)
        else:
            raise ValueError(op)
    return ei, ed


def check_group(P, op, block):
    """One primitive under every divergence pattern (MODES) with `block` threads per workgroup.  Lanes that take part hold
    the reference's value computed from their own row's operands; lanes that returned early keep the caller's fill."""
    s0, s1 = group_operands(op, block, 1000 + op), group_operands(op, block, 2000 + op)
    n = N_BLOCKS * block
    hs = [P.dev(x) for x in s0[:3]] + [P.dev(x) for x in s1[:3]] + [P.dev(s0[3])]
    row = (np.arange(n) >> 4) & 3
    m0 = np.repeat(s0[3], 64)
    e0 = group_expected(op, s0[0], s0[1], s0[2], m0)
    e1 = group_expected(op, s1[0], s1[1], s1[2], ~m0)
    modes = MODES if op not in (GSUM64, WSCAN) else [15]
    for mode in modes:
        oi, od = P.dev(np.full((n, 4), SENT_I, np.int32)), P.dev(np.full(n, SENT_D, np.uint64))
        P.call("probe_group", op, mode, N_BLOCKS, block, *hs, oi, od)
        gi, gd = P.get(oi), P.get(od)
        if mode < 16:
            active, first = ((mode >> row) & 1) == 1, np.ones(n, bool)
        else:
            active, first = np.ones(n, bool), ((row & 1) == 0 if mode == 16 else row == 0)
        wi = np.where(first[:, None], e0[0], e1[0])
        wd = np.where(first, e0[1].view(np.uint64), e1[1].view(np.uint64))
        wi = np.where(active[:, None], wi, SENT_I)
        wd = np.where(active, wd, SENT_D)
        bad = np.nonzero((gi != wi).any(1) | (gd != wd))[0]
        assert len(bad) == 0, "op %d mode %d block %d: %d lanes differ, first thread %d (row %d lane %d): got %s / %#x, want %s / %#x" % (
            op, mode, block, len(bad), bad[0], row[bad[0]], bad[0] & 15, gi[bad[0]], int(gd[bad[0]]), wi[bad[0]], int(wd[bad[0]]))
        if op in (SUM_D, GSUM64):   # every lane of a problem holds the same bits
            g = gd[active].reshape(-1, 16 if op == SUM_D else 64)
            assert (g == g[:, :1]).all()
    return len(modes)


def check_uniform(P):
    """cc_wave_id, cc_uniform_i, cc_uniform_ptr in a 256-thread workgroup: the wave's index and the wave's own value"""
    rng = np.random.default_rng(7)
    vals = rng.integers(-2 ** 31, 2 ** 31, N_BLOCKS * 4).astype(np.int32)
    out = P.dev(np.full((N_BLOCKS * 256, 3), SENT_I, np.int32))
    P.call("probe_uniform", N_BLOCKS, P.dev(vals), out)
    g = P.get(out)
    t = np.arange(N_BLOCKS * 256)
    assert np.array_equal(g[:, 0], (t >> 6) & 3)
    assert np.array_equal(g[:, 1], vals[t >> 6])
    assert np.array_equal(g[:, 2], vals[t >> 6])


def round_fraction_to_f32(v):
    """the f32 nearest to the exact rational v, ties to even (subnormals and overflow included), as a Python float"""
    if v == 0:
        return 0.0
    s, v = (-1.0, -v) if v < 0 else (1.0, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()   # 2^(e-1) <= v < 2^(e+1)
    if Fraction(2) ** e > v:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)
    r = round(v / q) * q                                        # round(Fraction): half to even
    return s * (float("inf") if r >= Fraction(2) ** 128 else float(r))


def pk_fma_cases(n_pairs=2048):
    """(a, b, c) f32 triples, two per cc_f2: random magnitudes; c = -fl(a b) (+- an ulp), where the fused result is the
    product's rounding error and a separate multiply and add gives 0 or an ulp; sums that land between two floats"""
    rng = np.random.default_rng(17)
    n = 2 * n_pairs
    a = (rng.choice([-1, 1], n) * 2.0 ** rng.uniform(-20, 20, n)).astype(np.float32)
    b = (rng.choice([-1, 1], n) * 2.0 ** rng.uniform(-20, 20, n)).astype(np.float32)
    c = (rng.choice([-1, 1], n) * 2.0 ** rng.uniform(-40, 40, n)).astype(np.float32)
    k = np.arange(n) % 4
    p = (a * b).astype(np.float32)
    c[k == 1] = -p[k == 1]
    c[k == 2] = np.nextafter(-p[k == 2], np.float32(np.inf) * rng.choice([-1, 1], int((k == 2).sum())).astype(np.float32))
    c[k == 3] = (p[k == 3] * np.float32(2.0 ** -12)).astype(np.float32)   # a b + c needs more than 24 bits
    a[:4] = np.float32([1e-20, 3e-23, 1.5e19, 1.0000001])   # subnormal and near-overflow results
    b[:4] = np.float32([1e-20, 1e-20, 1.5e19, 1.0000001])
    c[:4] = np.float32([1e-42, -1e-45, 1e38, -1.0000002])
    want = np.array([round_fraction_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    np.float64).astype(np.float32)   # exact: the values are f32 already
    with np.errstate(all="ignore"):
        unfused = ((a * b).astype(np.float32) + c).astype(np.float32)
    return a, b, c, want, unfused


def check_pk_fma(P):
    a, b, c, want, unfused = pk_fma_cases()
    nz = want != 0   # an exact zero's sign is the addition's, not the rounding's
    assert (unfused.view(np.uint32) != want.view(np.uint32))[nz].sum() > len(a) // 8, "the cases must tell a fused from an unfused result"
    out = P.dev(np.zeros(len(a), np.float32))
    P.call("probe_pk_fma", P.dev(a), P.dev(b), P.dev(c), out, len(a) // 2)
    g = P.get(out)
    bad = np.nonzero((g.view(np.uint32) != want.view(np.uint32)) & nz | ((g != 0) & ~nz))[0]
    assert len(bad) == 0, [(a[i], b[i], c[i], want[i], g[i]) for i in bad[:5]]


def check_load3f(P):
    """12- and 16-byte strides from bases that are 4, 8 and 12 bytes past a 16-byte boundary"""
    rng = np.random.default_rng(19)
    n = 1000
    words = rng.integers(0, 2 ** 32, 4 * n + 8, dtype=np.uint64).astype(np.uint32)
    for off in (4, 8, 12):
        for stride in (12, 16):
            assert off + (n - 1) * stride + 12 <= words.nbytes
            out = P.dev(np.zeros((n, 3), np.uint32))
            P.call("probe_load3f", P.dev(words, offset=off), stride, out, n)
            idx = (off + np.arange(n) * stride) // 4
            want = np.stack([words[idx], words[idx + 1], words[idx + 2]], 1)
            assert np.array_equal(P.get(out), want), (off, stride)


# ---------------------------------------------------------------------------------------------------------------------
# B. f64 routines (csrc/cc_fmath.h, cc_gmm_term)
# ---------------------------------------------------------------------------------------------------------------------
EXP_NONPOS_ULP = 1.35   # csrc/cc_fmath.h derives it
RSQRT_ULP = 1.0 + 1e-6  # csrc/cc_fmath.h derives it
LD_SLACK = 2.0 ** -10   # a long double result is within one of its own ulps = 2^-11 f64 ulp of the exact value
N_BULK = 2_000_000


def ulp_err(got, exact):
    """|got - exact| in units of the f64 ulp at `exact` (2^-1074 below the normal range); exact: longdouble array"""
    _, e = np.frexp(exact)
    ulp = np.ldexp(LD(1), np.maximum(e - 53, -1074))
    return (np.abs(got.astype(LD) - exact) / ulp).astype(np.float64)


def ulp_err_mp(got, exact):
    import mpmath as mp
    _, e = mp.frexp(exact)
    return float(abs(mp.mpf(float(got)) - exact) / mp.ldexp(1, max(int(e) - 53, -1074)))


def _run_f64(P, fn, x):
    out = P.dev(np.full(len(x), np.nan))
    P.call(fn, P.dev(x), out, len(x))
    return P.get(out)


def _same_bits(a, b):
    return a.view(np.uint64) == b.view(np.uint64)


def exp_args():
    rng = np.random.default_rng(23)
    C64 = 92.33248261689366
    k = rng.integers(-68000, 0, 20000).astype(np.float64) + 0.5
    ties = k / C64   # z * (64 / ln 2) lands on, or an ulp beside, a tie of rint
    parts = [rng.uniform(-1, 0, 500_000), rng.uniform(-40, 0, 500_000), rng.uniform(-740, 0, 500_000),
             rng.uniform(-740, -708, 40_000),   # results in the subnormal range
             ties, np.nextafter(ties, 0), np.nextafter(ties, -1000),
             np.array([-0.0, 0.0, -740.0, np.nextafter(-740.0, -1000), -741.0, -745.2, -1e3, -1e300, -np.inf, -5e-324, -1e-300])]
    n = sum(len(p) for p in parts)
    z = np.concatenate(parts + [-np.exp(-40 * rng.random(N_BULK - n))])
    assert len(z) == N_BULK and (z <= 0).all()
    return z


def _mp_pass(z, got, err_ld, exact_fn, n_sample=2000, n_worst=100):
    """the 100 worst of the bulk pass and 2 000 sampled arguments against mpmath at 50 digits: the largest error in ulp"""
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(29)
    idx = np.concatenate([np.argsort(err_ld)[-n_worst:], rng.integers(0, len(z), n_sample)])
    return max(ulp_err_mp(got[i], exact_fn(mp.mpf(float(z[i])))) for i in idx)


def check_exp_nonpos(P, other=None):
    import mpmath as mp
    z = exp_args()
    got = _run_f64(P, "probe_exp_nonpos", z)
    if other is not None:   # IEEE fma, rint, ldexp with contraction off on both sides: the same bits
        ref = _run_f64(other, "probe_exp_nonpos", z)
        bad = np.nonzero(~_same_bits(got, ref))[0]
        assert len(bad) == 0, (len(bad), [(z[i], got[i], ref[i]) for i in bad[:5]])
    low = z < -740.0
    assert (got[low].view(np.uint64) == 0).all(), "below -740 the routine returns +0"
    assert got[z == 0].tolist() == [1.0, 1.0]
    zz, gg = z[~low], got[~low]
    err = ulp_err(gg, np.exp(zz.astype(LD)))
    print("cc_exp_nonpos on %s: max %.4f ulp against long double over %d arguments" % (P.name, err.max(), len(zz)))
    assert err.max() <= EXP_NONPOS_ULP + LD_SLACK, (err.max(), zz[err.argmax()])
    worst = _mp_pass(zz, gg, err, mp.exp)
    print("cc_exp_nonpos on %s: max %.4f ulp against mpmath (100 worst + 2000 sampled)" % (P.name, worst))
    assert worst <= EXP_NONPOS_ULP, worst
    return worst


def rsqrt_args():
    rng = np.random.default_rng(31)
    den = rng.integers(1, 2 ** 52, 50_000, dtype=np.uint64).view(np.float64)   # denormals, every width
    pow4 = 4.0 ** np.arange(-511, 512)
    sp = np.array([5e-324, 1e-323, 2.2250738585072014e-308, 2.225073858507201e-308, 1e308, 1.7976931348623157e308, 1.0, 2.0, 3.0, 4.0])
    n_main = N_BULK - len(den) - len(pow4) - len(sp)
    return np.concatenate([np.exp(80 * (rng.random(n_main) - 0.5)), den, pow4, sp])


def check_rsqrt(P, other=None):
    import mpmath as mp
    x = rsqrt_args()
    got = _run_f64(P, "probe_rsqrt", x)
    err = ulp_err(got, LD(1) / np.sqrt(x.astype(LD)))
    print("cc_rsqrt on %s: max %.4f ulp against long double over %d arguments" % (P.name, err.max(), len(x)))
    assert err.max() <= RSQRT_ULP + 2 * LD_SLACK, (err.max(), x[err.argmax()])   # reference: a rounded root, then a rounded quotient
    worst = _mp_pass(x, got, err, lambda v: 1 / mp.sqrt(v))
    print("cc_rsqrt on %s: max %.4f ulp against mpmath (100 worst + 2000 sampled)" % (P.name, worst))
    assert worst <= RSQRT_ULP, worst
    if other is not None:   # the seeds differ (v_rsq_f64 against 1 / sqrt), the bar holds for both: at most two ulp apart
        ref = _run_f64(other, "probe_rsqrt", x)
        apart = np.abs(got.view(np.int64) - ref.view(np.int64)).max()
        print("cc_rsqrt: %s and %s differ in %d of %d results, by at most %d ulp" % (P.name, other.name, int((~_same_bits(got, ref)).sum()), len(x), apart))
        assert apart <= 2
    # outside the domain x > 0, finite: what the header documents
    edge = _run_f64(P, "probe_rsqrt", np.array([0.0, np.inf]))
    assert np.isnan(edge).all(), edge
    return worst


def sqrt_args():
    rng = np.random.default_rng(37)
    k = rng.integers(1, 2 ** 26, 200_000).astype(np.float64) * 2.0 ** rng.integers(-100, 100, 200_000)   # k * k is exact
    sq = k * k
    return np.concatenate([np.exp(rng.uniform(-700, 700, 350_000)), sq, np.nextafter(sq, 0), np.nextafter(sq, np.inf),
                           rng.integers(1, 2 ** 52, 49_990, dtype=np.uint64).view(np.float64),
                           np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, np.inf, 1.0, 2.0, 4.0, 0.25])])


def check_sqrt(P):
    """sqrt(double) as the translation unit's flags compile it: correctly rounded (cc_gmm_pair_near relies on it)"""
    x = sqrt_args()
    assert len(x) == 1_000_000
    got = _run_f64(P, "probe_sqrt", x)
    bad = np.nonzero(~_same_bits(got, np.sqrt(x)))[0]
    assert len(bad) == 0, (len(bad), [(x[i], got[i]) for i in bad[:5]])


class _EB:
    """a computed f64 quantity and a bound of its absolute error, both per pair: the running error analysis of one IEEE
    operation after the other (u = 2^-53 of the result per operation, operand errors propagated to first order with the
    second-order product kept)"""
    U = 2.0 ** -53

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    def _r(self, v, e):
        return _EB(v, e + _EB.U * np.abs(v))

    def __neg__(self):
        return _EB(-self.v, self.e)

    def scale(self, k):   # by a power of two: exact
        return _EB(self.v * k, self.e * abs(k))

    def __add__(self, o):
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._r(self.v - o.v, self.e + o.e)

    def _pe(self, o):
        return np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e

    def __mul__(self, o):
        return self._r(self.v * o.v, self._pe(o))

    def fma(self, o, c):   # self * o + c, one rounding
        return self._r(self.v * o.v + c.v, self._pe(o) + c.e)


ErrBound = _EB   # (gmm_cases.py follows cc_gmm_self_term with it)


def gmm_term_cases(n=2000):
    """raw [n, 14] f32 (src cov, tgt cov, src mean, tgt mean, weights) and pose [n, 6] f64 (px py cos sin cos2 sin2): ellipses
    with axes from the point_sigma floor (1.0) to 50 px at every orientation, built in f32 the way cc_k_gmm_prep builds them;
    the transformed src mean within the pre-selection radius 3 (maj_s + maj_t) of the tgt mean; theta over the full circle"""
    rng = np.random.default_rng(43)

    def ell():
        e1 = np.exp(rng.uniform(0, np.log(50.0), n)).astype(np.float32)
        e0 = np.minimum(e1, np.exp(rng.uniform(0, np.log(50.0), n))).astype(np.float32)
        e0[rng.random(n) < 0.25] = 1.0   # the floor itself
        a = rng.uniform(-np.pi, np.pi, n)
        v00, v10, v01, v11 = [x.astype(np.float32) for x in (np.cos(a), np.sin(a), -np.sin(a), np.cos(a))]
        a00, a01, a10, a11 = v00 * e0, v01 * e1, v10 * e0, v11 * e1
        return np.stack([a00 * v00 + a01 * v01, a00 * v10 + a01 * v11, a10 * v00 + a11 * v01, a10 * v10 + a11 * v11], 1), np.sqrt(e1)
    cs, majs = ell()
    ct, majt = ell()
    th = rng.uniform(-np.pi, np.pi, n)
    th[:4] = [0.0, np.pi, -np.pi, np.pi / 2]
    sm = rng.uniform(0, 150, (n, 2)).astype(np.float32)
    t = rng.uniform(-20, 20, (n, 2))
    c, s = np.cos(th), np.sin(th)
    moved = np.stack([c * sm[:, 0] - s * sm[:, 1] + t[:, 0], s * sm[:, 0] + c * sm[:, 1] + t[:, 1]], 1)
    rho = 3.0 * (majs + majt).astype(np.float64) * rng.random(n) * 0.999
    rho[:8] = 0.0
    phi = rng.uniform(0, 2 * np.pi, n)
    tm = (moved - np.stack([rho * np.cos(phi), rho * np.sin(phi)], 1)).astype(np.float32)
    w = rng.integers(1, 5000, (n, 2)).astype(np.float32)
    raw = np.ascontiguousarray(np.concatenate([cs, ct, sm, tm, w], 1), np.float32)
    pose = np.ascontiguousarray(np.stack([t[:, 0], t[:, 1], c, s, np.cos(2 * th), np.sin(2 * th)], 1), np.float64)
    return raw, pose


def gmm_term_exact(raw, pose):
    """The formula in the comment above cc_gmm_term at 50 digits, for the numbers the kernel is given (the four
    trigonometric values as they are): N = 2 (R C_s R^T + C_t) with R C R^T = m I + [p q; q -p] + a J, mu = R m_s + t - m_t,
    term = -w_s w_t / sqrt(det N) exp(-mu^T adj(N) mu / (2 det N)), and its derivatives by x, y and theta (d/dtheta of the
    four trigonometric values: c' = -s, s' = c, c2' = -2 s2, s2' = 2 c2).  -> [n, 4] mpf"""
    import mpmath as mp
    mp.mp.dps = 50
    out = []
    for f, ps in zip(raw, pose):
        s00, s01, s10, s11, t00, t01, t10, t11, smx, smy, tmx, tmy, ws, wt = [mp.mpf(float(x)) for x in f]
        px, py, c, s, c2, s2 = [mp.mpf(float(x)) for x in ps]
        m, d, b, a = (s00 + s11) / 2, (s00 - s11) / 2, (s01 + s10) / 2, (s10 - s01) / 2
        p, q = d * c2 - b * s2, d * s2 + b * c2
        dp, dq = -2 * q, 2 * p
        N = mp.matrix([[2 * (m + p + t00), 2 * (q - a + t01)], [2 * (q + a + t10), 2 * (m - p + t11)]])
        dN = mp.matrix([[2 * dp, 2 * dq], [2 * dq, -2 * dp]])
        mu = mp.matrix([c * smx - s * smy + px - tmx, s * smx + c * smy + py - tmy])
        dmu = mp.matrix([-s * smx - c * smy, c * smx - s * smy])
        adj = lambda M: mp.matrix([[M[1, 1], -M[0, 1]], [-M[1, 0], M[0, 0]]])
        det = N[0, 0] * N[1, 1] - N[0, 1] * N[1, 0]
        ddet = dN[0, 0] * N[1, 1] + N[0, 0] * dN[1, 1] - dN[0, 1] * N[1, 0] - N[0, 1] * dN[1, 0]
        A, dA = adj(N), adj(dN)
        E = (mu.T * A * mu)[0]
        dE_mu = (A + A.T) * mu                       # dE / d mu
        dE_t = (dE_mu.T * dmu)[0] + (mu.T * dA * mu)[0]
        Q = -E / (2 * det)
        v = -ws * wt / mp.sqrt(det) * mp.exp(Q)
        Qx, Qy = -dE_mu[0] / (2 * det), -dE_mu[1] / (2 * det)
        Qt = -(dE_t * det - E * ddet) / (2 * det * det)
        out.append([v, v * Qx, v * Qy, v * (Qt - ddet / (2 * det))])
    return out


def gmm_term_bound(raw, pose):
    """A bound of the absolute error of cc_gmm_term's four results per pair: cc_gmm_make_pair and cc_gmm_term followed
    operation by operation (the ~95 roundings the comment counts), cc_rsqrt entering with its bar (RSQRT_ULP ulp, an ulp
    being at most 2 u relative) plus half the relative error of its argument, cc_exp_nonpos with its bar (EXP_NONPOS_ULP)
    plus e^|dQ| - 1 for the absolute error dQ of its argument.  Cancellation (det N of two elongated, aligned ellipses; E for
    mu along N's major axis) enters through the absolute errors of the cancelling operands, which is why the bound is per
    pair and not one number.  -> [n, 4] f64"""
    f = [_EB(raw[:, k].astype(np.float64)) for k in range(14)]
    s00, s01, s10, s11, t00, t01, t10, t11, smx, smy, tmx, tmy, ws, wt = f
    px, py, c, s, c2, s2 = [_EB(pose[:, k]) for k in range(6)]
    # cc_gmm_make_pair
    sm, sa = (s00 + s11).scale(0.5), (s10 - s01).scale(0.5)
    a01, a10 = (t01 - sa).scale(2), (t10 + sa).scale(2)
    sd, sb = (s00 - s11).scale(0.5), (s01 + s10).scale(0.5)
    a00, a11 = (sm + t00).scale(2), (sm + t11).scale(2)
    as_, ap, w = a01 + a10, a01 * a10, ws * wt
    # cc_gmm_term
    p, q = sd.fma(c2, -(sb * s2)), sd.fma(s2, sb * c2)
    p2, q2 = p.scale(2), q.scale(2)
    n00, n11 = a00 + p2, a11 - p2
    nx = q.scale(4).fma(_EB(np.ones_like(q.v)), as_)
    det = n00.fma(n11, -q2.fma(q2 + as_, ap))
    ddet = q.fma(n00 - n11, -(p * nx)).scale(4)
    g0, g1 = -s.fma(smx, c * smy), c.fma(smx, -(s * smy))
    m0, m1 = g1 + (px - tmx), (py - tmy) - g0
    m00, m11, m01 = m0 * m0, m1 * m1, m0 * m1
    E = m00.fma(n11, m11.fma(n00, -(m01 * nx)))
    inner = (g0.fma(m1, m0 * g1)).fma(nx, p.scale(8) * m01)
    dE = ((m0 * g0).fma(n11, (m1 * g1) * n00)).scale(2).fma(_EB(np.ones_like(q.v)), q.scale(4).fma(m00 - m11, -inner))
    assert (det.v > 2 * det.e).all()
    U = _EB.U
    rv = 1.0 / np.sqrt(det.v)
    r = _EB(rv, rv * (0.5 * det.e / (det.v - det.e) + 2 * U * RSQRT_ULP))
    idet = r * r
    hi = idet.scale(-0.5)
    Q = hi * E
    assert (Q.v <= 0).all() and (Q.v > -740).all()
    ev = np.exp(Q.v)
    ex = _EB(ev, ev * (np.expm1(Q.e) + 2 * U * EXP_NONPOS_ULP))
    v = -(w * r) * ex
    gx = v * (hi * m0.scale(2).fma(n11, -(m1 * nx)))
    gy = v * (hi * m1.scale(2).fma(n00, -(m0 * nx)))
    half = _EB(np.full_like(q.v, 0.5))
    gt = v * (idet * dE.scale(-0.5).fma(_EB(np.ones_like(q.v)), -(ddet * (Q + half))))
    return np.stack([v.e, gx.e, gy.e, gt.e], 1) * (1 + 1e-6)   # the bound itself is computed in f64


_gmm_ref = {}


def check_gmm_term(P):
    """cc_gmm_term's value and three gradient components against the formula at 50 digits; every error is at most the pair's
    composed bound (gmm_term_bound).  Figures are relative to the term's own value |v|, in units of u = 2^-53.
    Observed, harness and MI355X alike: 812 u (value), 2 787 u / 2 450 u / 5.6e5 u (gx, gy, gt: the lever arm of theta) at
    the pairs where det N cancels most; the bound allows up to 6.4e3 u and 4.6e6 u there; no error is above 0.67 of its
    bound."""
    raw, pose = gmm_term_cases()
    if "exact" not in _gmm_ref:   # computed once, shared, never changed
        _gmm_ref["exact"] = gmm_term_exact(raw, pose)
        _gmm_ref["bound"] = gmm_term_bound(raw, pose)
    exact, bound = _gmm_ref["exact"], _gmm_ref["bound"]
    out = P.dev(np.full((len(raw), 4), np.nan))
    P.call("probe_gmm_term", P.dev(raw), P.dev(pose), out, len(raw))
    got = P.get(out)
    import mpmath as mp
    err = np.array([[float(abs(mp.mpf(float(g)) - e)) for g, e in zip(gr, er)] for gr, er in zip(got, exact)])
    vabs = np.array([float(abs(er[0])) for er in exact])
    rel, brel = err / vabs[:, None] / _EB.U, bound / vabs[:, None] / _EB.U
    print("cc_gmm_term on %s: max error / |v| in u: value %.1f, gx %.1f, gy %.1f, gt %.1f; largest bound %.3g (value), %.3g (gradient); "
          "largest error / bound %.3f" % (P.name, rel[:, 0].max(), rel[:, 1].max(), rel[:, 2].max(), rel[:, 3].max(), brel[:, 0].max(),
                                          brel[:, 1:].max(), (err / bound).max()))
    bad = np.nonzero((err > bound).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], err[bad[:3]], bound[bad[:3]])
    return rel.max(0)


# ---------------------------------------------------------------------------------------------------------------------
# C. bit-for-bit carriers (csrc/cc_stats.h, csrc/cc_sort.h, csrc/k_knn.h)
# ---------------------------------------------------------------------------------------------------------------------
def atan2f_args(n):
    """(y, x): differences of contour centres inside the 150 x 150 BEV, random bit patterns (NaN / inf removed), the special
    cases crossed with each other"""
    rng = np.random.default_rng(3)
    a = (rng.uniform(0, 150, n) - rng.uniform(0, 150, n)).astype(np.float32)
    b = (rng.uniform(0, 150, n) - rng.uniform(0, 150, n)).astype(np.float32)
    c = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    d = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    ok = np.isfinite(c) & np.isfinite(d)
    sp = np.array([0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 3e38, -3e38, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25, 2.0 ** -29], np.float32)
    sy, sx = np.meshgrid(sp, sp)
    y = np.ascontiguousarray(np.concatenate([a, c[ok], sy.ravel()]), np.float32)
    x = np.ascontiguousarray(np.concatenate([b, d[ok], sx.ravel()]), np.float32)
    return y, x


def acosf_args(n):
    """dot products of unit vectors, cosines pushed a little beyond +-1 (NaN), random bit patterns, the special cases"""
    rng = np.random.default_rng(5)
    a = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    b = np.clip(np.cos(rng.uniform(0, np.pi, n)).astype(np.float32) * np.float32(1.0000001), -2, 2).astype(np.float32)
    c = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    c = c[np.isfinite(c)]
    sp = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.49999997, 0.50000006, 2.0 ** -58, 2.0 ** -57, 1.0000001, -1.0000001, 3e38], np.float32)
    return np.ascontiguousarray(np.concatenate([a, b, c, sp]), np.float32)


def libm_atan2f(y, x):
    import oracle_py
    want = np.zeros_like(y)
    oracle_py.lib().orc_atan2f(C.c_void_p(y.ctypes.data), C.c_void_p(x.ctypes.data), C.c_void_p(want.ctypes.data), C.c_long(len(y)))
    return want


def libm_acosf(x):
    import oracle_py
    want = np.zeros_like(x)
    oracle_py.lib().orc_acosf(C.c_void_p(x.ctypes.data), C.c_void_p(want.ctypes.data), C.c_long(len(x)))
    return want


def _run_f32(P, fn, *ins):
    out = P.dev(np.zeros(len(ins[0]), np.float32))
    P.call(fn, *[P.dev(v) for v in ins], out, len(ins[0]))
    return P.get(out)


def check_atan2f(P, other=None, n=1_000_000):
    y, x = atan2f_args(n)
    got = _run_f32(P, "probe_atan2f", y, x)
    want = libm_atan2f(y, x)
    bad = np.nonzero(want.view(np.uint32) != got.view(np.uint32))[0]
    assert len(bad) == 0, (len(bad), [(float(y[i]), float(x[i]), float(want[i]), float(got[i])) for i in bad[:5]])
    if other is not None:
        ref = _run_f32(other, "probe_atan2f", y, x)
        assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))
    return len(y)


def check_acosf(P, other=None, n=1_000_000):
    x = acosf_args(n)
    assert (np.abs(x) > 1).sum() > 1000   # the |x| > 1 NaNs are among the cases
    got = _run_f32(P, "probe_acosf", x)
    want = libm_acosf(x)
    same = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
    bad = np.nonzero(~same)[0]
    assert len(bad) == 0, (len(bad), x[bad[:5]], want[bad[:5]], got[bad[:5]])
    if other is not None:
        ref = _run_f32(other, "probe_acosf", x)
        assert ((ref.view(np.uint32) == got.view(np.uint32)) | (np.isnan(ref) & np.isnan(got))).all()
    return len(x)


def eigen2f_args(n=100_000):
    """covariance triples (m00, m10, m11): random SPD matrices of every elongation, equal diagonals, zero off-diagonal,
    near-singular and exactly singular ones, raw second moments of a few cells"""
    rng = np.random.default_rng(41)
    th = rng.uniform(0, np.pi, n)
    l1 = rng.uniform(0.05, 2500, n)
    l0 = l1 * 10.0 ** -rng.uniform(0, 7, n)
    c, s = np.cos(th), np.sin(th)
    m = np.stack([c * c * l0 + s * s * l1, c * s * (l0 - l1), s * s * l0 + c * c * l1], 1).astype(np.float32)
    k = np.arange(n) % 8
    m[k == 1, 2] = m[k == 1, 0]                                  # equal diagonals
    m[k == 2, 1] = 0                                             # zero off-diagonal
    m[k == 3, 1] = np.sqrt(m[k == 3, 0] * m[k == 3, 2])          # singular up to f32 rounding
    q = rng.integers(0, 150, (n, 2)).astype(np.float32)
    m[k == 4] = np.stack([q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 1] * q[:, 1]], 1)[k == 4]   # rank one, exact
    m[:4] = np.float32([[0, 0, 0], [1, 0, 1], [0, 1, 0], [1e-30, 1e-30, 1e-30]])
    return np.ascontiguousarray(m)


def _run_eigen2f(P, m):
    out = P.dev(np.zeros((len(m), 6), np.float32))
    P.call("probe_eigen2f", P.dev(m), out, len(m))
    return P.get(out)


def check_eigen2f(P, other=None):
    """against the oracle's own restatement of Eigen's solver (oracle/orc_math.h) on a sample, bit for bit; the device also
    against the harness on all of them"""
    import oracle_py
    m = eigen2f_args()
    got = _run_eigen2f(P, m)
    lib = oracle_py.lib()
    m4, ev, vec = np.zeros(4, np.float32), np.zeros(2, np.float32), np.zeros(4, np.float32)
    for i in range(0, len(m), 20):
        m4[:] = (m[i, 0], m[i, 1], m[i, 1], m[i, 2])
        lib.orc_eigen2f(m4.ctypes.data, ev.ctypes.data, vec.ctypes.data)
        want = np.float32([ev[0], ev[1], vec[0], vec[2], vec[1], vec[3]])   # the oracle's vectors are row-major
        assert np.array_equal(want.view(np.uint32), got[i].view(np.uint32)), (i, m[i], want, got[i])
    if other is not None:
        ref = _run_eigen2f(other, m)
        bad = np.nonzero((ref.view(np.uint32) != got.view(np.uint32)).any(1))[0]
        assert len(bad) == 0, (len(bad), m[bad[:3]], ref[bad[:3]], got[bad[:3]])
    return len(m)


def killer(n):
    """A sequence on which median-of-3 quicksort degenerates (Musser's construction), so that introsort's depth limit is
    reached and the heapsort branch runs: the wave replay must hand such input to the serial replica."""
    k = n // 2
    a = np.zeros(n, np.int32)
    for i in range(1, k + 1):
        if i % 2 == 1:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


SORT_LENGTHS = list(range(0, 40)) + [63, 64, 65, 100, 128, 129, 257, 320, 1000]
SORT_KEY_RANGES = (2, 5, 40, 5000)


def sort_desc_cases():
    """int32 key arrays: tie-heavy random keys of every length class and key range; sorted, reversed and all-equal inputs;
    inputs that drive introsort into its heapsort branch"""
    rng = np.random.default_rng(5)
    cases = []
    for n in SORT_LENGTHS:
        for hi in SORT_KEY_RANGES:
            cases.append(rng.integers(3, 3 + hi, n).astype(np.int32))
    for n in (17, 33, 200, 320):
        cases += [np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)[::-1].copy(), np.full(n, 7, np.int32)]
    for n in (64, 200, 320, 2000):
        cases.append(killer(n))
        cases.append(-killer(n) + 5000)
    return cases


def sort_asc_f_cases():
    rng = np.random.default_rng(1)
    return [np.round(rng.uniform(-3.2, 3.2, n), 1).astype(np.float32) for n in (0, 1, 16, 17, 40, 123, 256, 1000)]   # many exact ties


def _pack_cases(cases):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in cases])]).astype(np.int32)
    arr = np.concatenate([(c.astype(np.uint32) << 16) | np.arange(len(c), dtype=np.uint32) for c in cases]).astype(np.uint32)
    return arr, offs


def check_sort_desc(P, oracle, wave):
    """std_sort as one lane / std_sort_wave as one wave per array, all cases in one launch, against the real std::sort"""
    cases = sort_desc_cases()
    assert all(len(c) < 4096 for c in cases)
    arr, offs = _pack_cases(cases)
    h = P.dev(arr)
    if wave:
        P.call("probe_sort_desc_wave", h, P.dev(arr), P.dev(offs), len(cases))
    else:
        P.call("probe_sort_desc", h, P.dev(offs), len(cases))
    g = P.get(h)
    for k, keys in enumerate(cases):
        assert np.array_equal(g[offs[k]:offs[k + 1]] & 0xFFFF, oracle.sort_desc_perm(keys)), (len(keys), keys[:8])
    return len(cases)


def check_sort_asc_f(P, oracle):
    cases = sort_asc_f_cases()
    dt = np.dtype([("k", "<f4"), ("idx", "<i4")])
    offs = np.concatenate([[0], np.cumsum([len(c) for c in cases])]).astype(np.int32)
    arr = np.zeros(offs[-1], dt)
    arr["k"] = np.concatenate(cases)
    arr["idx"] = np.concatenate([np.arange(len(c)) for c in cases])
    h = P.dev(arr)
    P.call("probe_sort_asc_f", h, P.dev(offs), len(cases))
    g = P.get(h)
    for k, keys in enumerate(cases):
        assert np.array_equal(g["idx"][offs[k]:offs[k + 1]], oracle.sort_asc_perm_f(keys)), len(keys)


def bitonic_cases():
    """(R, kind, keys): random keys, padding keys (0xFFFFFFFF) on half the places, many equal buckets"""
    rng = np.random.default_rng(11)
    out = []
    for r in (1, 4, 8):
        for kind in range(3):
            n = 1024 * r
            a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
            if kind == 1:
                a[rng.integers(0, n, n // 2)] = 0xFFFFFFFF
            if kind == 2:
                a = (rng.integers(0, 50, n).astype(np.uint32) << 13) | np.arange(n, dtype=np.uint32)
            out.append((r, kind, a))
    return out


def scan_cases():
    """(n, values to sum, values for the running maximum)"""
    rng = np.random.default_rng(12)
    return [(n, rng.integers(0, 3, n).astype(np.int32), np.where(rng.random(n) < 0.05, np.arange(n), 0).astype(np.int32))
            for n in (64, 1024, 2048, 8192)]


def check_block_sort_and_scans(P):
    for r, kind, a in bitonic_cases():
        h = P.dev(a)
        P.call("probe_block_bitonic", h, r)
        assert np.array_equal(P.get(h), np.sort(a)), (r, kind)
    for n, v, hmax in scan_cases():
        h = P.dev(v)
        P.call("probe_block_scan", h, n, 0)
        assert np.array_equal(P.get(h), np.cumsum(v)), n
        h = P.dev(hmax)
        P.call("probe_block_scan", h, n, 1)
        assert np.array_equal(P.get(h), np.maximum.accumulate(hmax)), n
