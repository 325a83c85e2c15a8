"""TEST INFRASTRUCTURE for the typed-coordinate ingest (cc_ingest_coords and its siblings, include/cont2_amd_coords.h): the numpy
restatement of the three conversion steps, the builders of coordinate streams (records and columns of f32 / f64 / i32), the cases --
each asserts on the numpy / oracle side that it reaches the edge it is named after -- a driver of the calls on the CPU harness, and
the check both the harness and the GPU tests run: the oracle on the converted points p, and the bytes of cc_ingest_points on the
packed {12, 0} records p."""
import ctypes as C
import mmap
from fractions import Fraction

import numpy as np

from parity import compare_desc, terrain_scan
from point_filter import boundary_indices
from point_layouts import NAN_FILL, PointsApi, apply_tf, random_tfs

F32, F64, I32 = 0, 1, 2
DTYPES = {F32: np.float32, F64: np.float64, I32: np.int32}
STRIDE_MAX = 256
Q10 = 1024.0   # clouds quantised to multiples of 2^-10 m


class CoordSrc(C.Structure):
    """cc_coord_src_t"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("type", C.c_int32), ("stride_bytes", C.c_int32), ("scale", C.c_double * 3)]


# ---- the specification, restated: one numpy ufunc call per step, on float64, then the narrowing ----
def spec(v, type, scale=None, origin=None):
    """v [n, 3] of the source's dtype -> p [n, 3] f32.  scale: 3 values (I32 only), origin: 3 values or None (0.0)."""
    v = np.asarray(v)
    assert v.dtype == DTYPES[type]
    X = v.astype(np.float64)                                             # step 1
    if type == I32:
        X = np.multiply(X, np.asarray(scale, np.float64).reshape(1, 3))  # ... one f64 product
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        D = np.subtract(X, o.reshape(1, 3))                              # step 2: one f64 subtraction
        return D.astype(np.float32)                                      # step 3: IEEE round to nearest even; overflow gives +-inf


# the wrong variants a conversion could be, for the cases that must tell them apart
def wrong_truncated(v, type, scale, origin):
    """step 3 by truncation towards zero"""
    X = np.asarray(v).astype(np.float64)
    if type == I32:
        X = np.multiply(X, np.asarray(scale, np.float64).reshape(1, 3))
    D = np.subtract(X, (np.zeros(3) if origin is None else np.asarray(origin, np.float64)).reshape(1, 3))
    with np.errstate(all="ignore"):
        p = D.astype(np.float32)
        over = np.abs(p.astype(np.float64)) > np.abs(D)
        return np.where(over, np.nextafter(p, np.float32(0)), p).astype(np.float32)


def wrong_f32_subtraction(v, type, scale, origin):
    """narrowing first, the subtraction in f32: what a caller's `X.astype(f32) - O.astype(f32)` does"""
    X = np.asarray(v).astype(np.float64)
    if type == I32:
        X = np.multiply(X, np.asarray(scale, np.float64).reshape(1, 3))
    o = (np.zeros(3) if origin is None else np.asarray(origin, np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        return np.subtract(X.astype(np.float32), o.reshape(1, 3))


def wrong_fused(v, type, scale, origin):
    """I32: v * scale - origin as ONE operation rounded once (a fused multiply-add), exactly, by rational arithmetic"""
    assert type == I32
    v = np.asarray(v)
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    out = np.zeros(v.shape, np.float32)
    for k in range(3):
        s, ok = Fraction(float(scale[k])), Fraction(float(o[k]))
        out[:, k] = np.array([float(int(a) * s - ok) for a in v[:, k]], np.float64).astype(np.float32)   # float(Fraction) rounds to nearest even
    return out


def cells(p, cfg):
    """the cell (row, col) of every point of p [n, >= 2] f32 as the reference bins it, -1 outside the map (numpy floor on f32, for
    the tests' own assertions that a variant MOVES points; the library is held against the oracle, never against this)"""
    x_lo, y_lo = -0.5 * cfg.n_row * cfg.reso_row, -0.5 * cfg.n_col * cfg.reso_col
    with np.errstate(all="ignore"):
        r = np.floor((p[:, 0].astype(np.float64) - x_lo) / cfg.reso_row)
        c = np.floor((p[:, 1].astype(np.float64) - y_lo) / cfg.reso_col)
    ok = (r >= 0) & (r < cfg.n_row) & (c >= 0) & (c < cfg.n_col)
    return np.where(ok, r * cfg.n_col + c, -1)


# ---- streams: how a scan's coordinates lie in memory ----
class Place:
    """Where x, y, z of every point lie.  records(stride, (ox, oy, oz)): ONE array of `stride`-byte records with the elements at those
    byte offsets; columns(stride): THREE separately allocated arrays, elements `stride` bytes apart (default: the element size).
    base_shift: the first byte sits that far behind a 16-byte boundary; fill: a seed for random bytes between the elements (else
    NaN bit patterns)."""

    def __init__(self, kind, stride, offsets=(0, 0, 0), base_shift=0, fill=None):
        self.kind, self.stride, self.offsets, self.base_shift, self.fill = kind, stride, offsets, base_shift, fill

    @classmethod
    def records(cls, stride, offsets, base_shift=0, fill=None):
        return cls("records", stride, offsets, base_shift, fill)

    @classmethod
    def columns(cls, stride=None, base_shift=0, fill=None):
        return cls("columns", stride, (0, 0, 0), base_shift, fill)

    def build(self, v, exact=False, alloc=None):
        """v [n, 3] -> (buffers: uint8 arrays, streams: [(buffer index, byte offset of the first element)] for x, y, z, stride).
        exact: every buffer holds EXACTLY the bytes its streams span (alloc(nbytes) makes it: a guard-page buffer, say)"""
        v = np.ascontiguousarray(v)
        n, elem = len(v), v.dtype.itemsize
        stride = self.stride or elem
        assert stride % elem == 0 and all(o % elem == 0 for o in self.offsets)

        def raw(nbytes, seed):
            if exact:
                b = alloc(nbytes) if alloc else np.zeros(nbytes, np.uint8)
            else:
                w = np.zeros(nbytes + 48, np.uint8)
                s = (-w.ctypes.data) % 16 + self.base_shift
                b = w[s:s + nbytes]
                assert b.ctypes.data % 16 == self.base_shift % 16
            if self.fill is not None:
                b[:] = np.random.default_rng(self.fill + seed).integers(0, 256, nbytes, dtype=np.uint8)
            else:
                b[:nbytes // 4 * 4].view(np.uint32)[:] = NAN_FILL
            return b

        def put(b, at, col):
            rows = np.lib.stride_tricks.as_strided(b[at:], (n, elem), (stride, 1))
            rows[:] = np.ascontiguousarray(col).view(np.uint8).reshape(n, elem)

        if self.kind == "records":
            lo, hi = min(self.offsets), max(self.offsets)
            assert hi + elem <= stride
            nbytes = (n - 1) * stride + (hi - lo) + elem if exact else n * stride
            b = raw(nbytes, 0)
            first = lo if exact else 0
            for k in range(3):
                put(b, self.offsets[k] - first, v[:, k])
            return [b], [(0, self.offsets[k] - first) for k in range(3)], stride
        bufs = []
        for k in range(3):
            b = raw((n - 1) * stride + elem, k)
            put(b, 0, v[:, k])
            bufs.append(b)
        return bufs, [(k, 0) for k in range(3)], stride


def guarded(nbytes):
    """nbytes of memory whose last byte lies in front of an inaccessible page: a read of one element too many faults"""
    page = mmap.PAGESIZE
    total = (nbytes + page - 1) // page * page + page
    m = mmap.mmap(-1, total)
    base = C.addressof(C.c_char.from_buffer(m))
    libc = C.CDLL(None, use_errno=True)
    assert libc.mprotect(C.c_void_p(base + total - page), C.c_size_t(page), 0) == 0
    a = np.frombuffer(m, np.uint8, nbytes, offset=total - page - nbytes)
    assert a.ctypes.data + nbytes == base + total - page
    return a


class Case:
    """Scans of raw coordinates v [n, 3] (one dtype), the conversion's parameters and how the coordinates lie in memory."""

    def __init__(self, name, raws, type, place, scale=None, origins=None, tfs=None):
        self.name, self.raws, self.type, self.place, self.tfs = name, [np.ascontiguousarray(r, DTYPES[type]) for r in raws], type, place, tfs
        self.scale = None if scale is None else np.asarray(scale, np.float64).reshape(3)
        self.origins = None if origins is None else np.ascontiguousarray(np.asarray(origins, np.float64).reshape(len(raws), 3))
        assert (self.scale is not None) == (type == I32)

    def offs(self):
        return np.concatenate([[0], np.cumsum([len(s) for s in self.raws])]).astype(np.int64)

    def p(self):
        """the f32 points the library is specified to see: [n, 4] per scan (w = 0)"""
        out = []
        for i, r in enumerate(self.raws):
            q = np.zeros((len(r), 4), np.float32)
            q[:, :3] = spec(r, self.type, self.scale, None if self.origins is None else self.origins[i])
            out.append(q)
        return out

    def variant(self, fn):
        return [fn(r, self.type, self.scale, None if self.origins is None else self.origins[i]) for i, r in enumerate(self.raws)]

    def moved(self):
        ps = self.p()
        return ps if self.tfs is None else [apply_tf(s, m) for s, m in zip(ps, self.tfs)]

    def packed(self):
        """the {12, 0} records of p: what cc_ingest_points is given for the byte comparison"""
        return np.ascontiguousarray(np.concatenate([q[:, :3] for q in self.p()], 0)).reshape(-1).view(np.uint8)

    def build(self, exact=False, alloc=None):
        return self.place.build(np.concatenate(self.raws, 0), exact, alloc)

    def repeat(self, n_scans):
        """the case with its scans repeated to n_scans (4: split sweep + merge kernel; 9: one workgroup per scan)"""
        idx = [i % len(self.raws) for i in range(n_scans)]
        return Case(self.name, [self.raws[i] for i in idx], self.type, self.place, self.scale, None if self.origins is None else self.origins[idx],
                    None if self.tfs is None else np.stack([self.tfs[i] for i in idx]))


def _sizes(n_scans, n0=9001, step=499):
    return [n0 + step * i for i in range(n_scans)]   # 9 001 .. 13 000: several chunks, part boundaries inside the data


def quantised(s):
    """an f32 cloud [n, >= 3] on the 2^-10 m lattice, as f64 [n, 3]"""
    return np.round(s[:, :3].astype(np.float64) * Q10) / Q10 + 0.0   # (+ 0.0: no -0.0, which a shift by an origin and back would not return)


def geo_origins(n_scans, seed=5):
    """a different origin per scan near (448 000, 5 412 000, 300), each a multiple of 2^-10"""
    rng = np.random.default_rng(seed)
    o = np.array([448000.0, 5412000.0, 300.0]) + np.round(rng.uniform(-500.0, 500.0, (n_scans, 3)) * Q10) / Q10
    assert len({tuple(r) for r in o}) == n_scans
    return o


def to_i32(local, scale, origin):
    """the integers whose spec conversion lies nearest to `local` [n, 3]: v = round((local + origin) / scale)"""
    return np.round((local.astype(np.float64) + np.asarray(origin).reshape(1, 3)) / np.asarray(scale).reshape(1, 3)).astype(np.int64).astype(np.int32)


# ---- the cases ----
def case_georef(n_scans=4, seed=600, sizes=None):
    """1: georeferenced f64 [N, 3]: local clouds on the 2^-10 lattice, shifted in f64 by an origin per scan"""
    sizes = sizes or _sizes(n_scans)
    local = [quantised(terrain_scan(seed + i, n=n, scale=1.3 + 0.1 * (i % 4))) for i, n in enumerate(sizes)]
    O = geo_origins(len(sizes), seed)
    case = Case("georeferenced f64", [q + O[i] for i, q in enumerate(local)], F64, Place.records(24, (0, 8, 16)), origins=O)
    for q, p in zip(local, case.p()):
        assert p[:, :3].astype(np.float64).tobytes() == q.tobytes(), "the spec recovers the quantised cloud bit for bit"
    return case


def assert_georef_edge(oracle, cfg, case):
    """the naively cast cloud is another scan: its BEV differs from the right one in at least 20 cells"""
    right = oracle.Scan(case.p()[0], cfg).bev()[0]
    naive = np.zeros((len(case.raws[0]), 4), np.float32)
    naive[:, :3] = wrong_f32_subtraction(case.raws[0], F64, None, case.origins[0])
    wrong = oracle.Scan(naive, cfg).bev()[0]
    assert (right != wrong).sum() >= 20, (right != wrong).sum()
    assert len({tuple(o) for o in case.origins[:4]}) == min(4, len(case.origins)), "every scan has a different origin"


def _edge_values():
    """f64 values D whose narrowing is an edge, as (base, nudge): exactly halfway between two f32 (to both parities) -- nudge 0 -- and
    one f64 ulp on either side of that -- nudge -1 / +1; the f32 within one ulp of cell borders of both resolutions of the tests
    (multiples of 3), of x_lo / x_hi (+-75) and of the blind disc's radius (3)"""
    base, nudge = [], []
    for b in [3.0, 6.0, 9.0, 12.0, 24.0, 33.0, 48.0, 63.0, 72.0, 75.0]:
        for sgn in (1.0, -1.0):
            f = np.float32(sgn * b)
            lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
            lo2, hi2 = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            for a, c in ((lo2, lo), (lo, f), (f, hi), (hi, hi2)):   # midpoints whose even neighbour is the lower one and the upper one
                mid = (np.float64(a) + np.float64(c)) / 2
                base += [mid, mid, mid]
                nudge += [0, -1, 1]
            base += [np.float64(lo), np.float64(f), np.float64(hi)]
            nudge += [0, 0, 0]
    return np.array(base, np.float64), np.array(nudge)


def _nudged(x, nudge):
    return np.where(nudge < 0, np.nextafter(x, -np.inf), np.where(nudge > 0, np.nextafter(x, np.inf), x))


def case_rounding_f64(n_scans=4, seed=620, with_origin=True):
    """2 (f64): terrain with edge values spliced into x or y, high above everything near them.  Without an origin the stored value IS
    D, and "one f64 ulp on either side" is D's.  With an origin (multiples of 4 near the UTM one) the stored X = D + O is exact for
    the midpoints and the f32 themselves, and one ulp of X on either side is the nearest the input can come to them."""
    E, nudge = _edge_values()
    m = len(E)
    raws, O = [], np.array([[448000.0 + 4 * i, 5412000.0 - 8 * i, 300.0] for i in range(n_scans)]) if with_origin else None
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        local = terrain_scan(seed + i, n=n, scale=1.2)[:, :3].astype(np.float64)
        at = rng.choice(n, 2 * m, replace=False)
        k = np.arange(m)
        other = -60.0 + 1.5 * (k % 80) + 0.375   # the other coordinate: inside a cell at both resolutions
        local[at[:m], 0], local[at[:m], 1] = E, other
        local[at[m:], 1], local[at[m:], 0] = E, other
        local[at, 2] = 20.0 + 0.01 * np.arange(2 * m)
        blind = at[:m][np.abs(np.abs(E) - 3.0) < 1e-3]
        local[blind, 1] = 0.0   # on the x axis: x^2 + y^2 against blind_sq = 9 is decided by x's last bit
        X = local + O[i] if with_origin else local
        if with_origin:
            assert np.array_equal(X[at[:m], 0] - O[i, 0], E) and np.array_equal(X[at[m:], 1] - O[i, 1], E), "the stored midpoints are exact"
        X[at[:m], 0] = _nudged(X[at[:m], 0], nudge)
        X[at[m:], 1] = _nudged(X[at[m:], 1], nudge)
        raws.append(X)
    return Case("rounding f64" + (" with an origin" if with_origin else ""), raws, F64, Place.records(24, (0, 8, 16)), origins=O)


def fused_triples(axis_offset=2000, scale=0.001):
    """(v, origin) for one axis with `scale`, found with rational arithmetic: the exact v * scale - origin rounds to another f32 than
    the twice-rounded spec, and the two land in different cells.  v = -(1 / scale) * a is a whole number of metres -a; the origin
    -axis_offset + 2^-19 puts D = -(a - axis_offset) - 2^-19 exactly halfway between the cell border -n and the f32 below it; the f64
    product has already dropped the scale's representation error, which the fused form still sees.  Whichever sign that error has, one
    of the four mirrored constructions works: all are tried and the one with the most differences is returned."""
    q = int(round(1 / scale))
    best = None
    for vs in (-1, 1):
        for ms in (-1, 1):
            o = vs * axis_offset + ms * 2.0 ** -19
            v = np.array([vs * q * (axis_offset + n) for n in range(33, 64)], np.int32).reshape(-1, 1).repeat(3, 1)
            a = spec(v, I32, [scale] * 3, [o] * 3)[:, 0]
            b = wrong_fused(v, I32, [scale] * 3, [o] * 3)[:, 0]
            moved = int((np.floor(a.astype(np.float64)) != np.floor(b.astype(np.float64))).sum())
            if best is None or moved > best[0]:
                best = (moved, v[:, 0].copy(), o)
    assert best[0] >= 20, best[0]
    return best[1], best[2]


def case_rounding_i32(n_scans=4, seed=640):
    """2 (i32): triples (v, scale, origin) whose exact v * scale - origin rounds differently from the twice-rounded spec, in x and in y"""
    scale = np.array([0.001, 0.001, 0.001])
    vx, ox = fused_triples(2000)
    vy, oy = fused_triples(3000)
    origin = np.array([ox, oy, 100.0])
    raws = []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        local = terrain_scan(seed + i, n=n, scale=1.2)[:, :3]
        v = to_i32(local, scale, origin)
        at = rng.choice(n, len(vx) + len(vy), replace=False)
        k = np.arange(len(vx))
        inside = to_i32(np.stack([-50.0 + 3.0 * k + 0.4, -50.0 + 3.0 * k + 0.4, 0 * k], 1), scale, origin)
        v[at[:len(vx)], 0], v[at[:len(vx)], 1] = vx, inside[:, 1]
        v[at[len(vx):], 1], v[at[len(vx):], 0] = vy, inside[:len(vy), 0]
        v[at, 2] = to_i32(np.stack([0 * at, 0 * at, 20.0 + 0.01 * np.arange(len(at))], 1).astype(np.float64), scale, origin)[:, 2]
        raws.append(v)
    return Case("rounding i32", raws, I32, Place.records(12, (0, 4, 8)), scale=scale, origins=np.tile(origin, (n_scans, 1)))


def assert_variant_matters(case, cfg, fn, what):
    """a wrong conversion changes the f32 bits of at least 50 points and moves at least 5 of them to another cell"""
    bits = moved = 0
    for p, w in zip(case.p()[:4], case.variant(fn)[:4]):
        d = (p[:, :3].view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).any(axis=1)
        bits += int(d.sum())
        moved += int((cells(p, cfg) != cells(w, cfg)).sum())
    assert bits >= 50 and moved >= 5, (what, bits, moved)


def case_types(variant, n_scans=4, seed=660):
    """3: the element types and the shapes of the streams"""
    sizes = _sizes(n_scans)
    local = [terrain_scan(seed + 10 * variant + i, n=n, scale=1.3) for i, n in enumerate(sizes)]
    O = geo_origins(n_scans, seed + variant)
    f64 = [quantised(s) + O[i] for i, s in enumerate(local)]
    f32 = [s[:, :3] for s in local]
    las_scale, file_off = np.array([0.001, 0.001, 0.001]), np.array([448000.0, 5412000.0, 0.0])
    las_origin = O - file_off   # LAS: X_world = v * scale + file offset; the call's origin folds the file offset in
    i32 = [to_i32(quantised(s), las_scale, las_origin[i]) for i, s in enumerate(local)]
    las = dict(scale=las_scale, origins=las_origin)
    return [
        lambda: Case("f64 columns", f64, F64, Place.columns(), origins=O),
        lambda: Case("f64 records of 32 B, x y z at 0 16 8", f64, F64, Place.records(32, (0, 16, 8), fill=seed), origins=O),
        lambda: Case("f32 columns", f32, F32, Place.columns()),
        lambda: Case("f32 records of 48 B, x y z at 8 24 40", f32, F32, Place.records(48, (8, 24, 40))),
        lambda: Case("i32 records of 20 B", i32, I32, Place.records(20, (0, 4, 8), fill=seed), **las),
        lambda: Case("i32 records of 28 B", i32, I32, Place.records(28, (0, 4, 8)), **las),
        lambda: Case("i32 columns", i32, I32, Place.columns(), **las),
        lambda: Case("f64 stride 256", f64, F64, Place.records(STRIDE_MAX, (8, 128, 248), fill=seed), origins=O),
        lambda: Case("f64 base 8 bytes off", f64, F64, Place.records(24, (0, 8, 16), base_shift=8), origins=O),
        lambda: Case("f32 base 4 bytes off", f32, F32, Place.columns(base_shift=4)),
        lambda: Case("i32 base 4 bytes off", i32, I32, Place.records(12, (0, 4, 8), base_shift=4), **las),
    ][variant]()


N_TYPES = 11


def case_special(type, n_scans=4, seed=700):
    """4: f64 NaN, +-inf and +-1e300 in x or y, -0.0; INT32_MIN / INT32_MAX: all rejected (or, for -0.0, kept at 0); z stays finite"""
    raws = []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        local = terrain_scan(seed + i, n=n, scale=1.3)[:, :3].astype(np.float64)
        at = rng.choice(n, n // 4, replace=False)
        axis = rng.integers(0, 2, len(at))
        if type == F64:
            local[at, axis] = np.resize(np.array([np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300, -0.0, 3.5e38, -3.5e38]), len(at))
            raws.append(local)
        else:
            v = to_i32(local, [0.001] * 3, [0.0] * 3)
            v[at, axis] = np.resize(np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0], np.int64), len(at)).astype(np.int32)
            raws.append(v)
    if type == F64:
        return Case("special f64", raws, F64, Place.columns())
    return Case("special i32", raws, I32, Place.records(12, (0, 4, 8)), scale=[0.001] * 3)


def assert_special_edge(case):
    for r, p in zip(case.raws, case.p()):
        bad = ~np.isfinite(p[:, 0]) | ~np.isfinite(p[:, 1])
        if case.type == F64:
            assert bad.sum() > 1000 and np.isinf(p[np.abs(r[:, 0]) == 1e300, 0]).all() and np.isinf(p[np.abs(r[:, 0]) == 3.5e38, 0]).all(), "overflow gives +-inf"
            assert (np.signbit(p[:, :2]) & (p[:, :2] == 0)).sum() > 50, "-0.0 stays -0.0"
        else:
            assert (np.abs(p[:, :2]) > 2.0e6).sum() > 500, "INT32_MIN / INT32_MAX are far outside the map"
        assert np.isfinite(p[:, 2]).all()


def case_boundaries(n_scans=4, seed=720, chunk=4096):
    """5: the records on both sides of every chunk and split-part boundary are each the highest point of a cell of its own, at a
    georeferenced f64 position: the cell is right only if that record's conversion is"""
    raws, O = [], geo_origins(n_scans, seed)
    for i, n in enumerate(_sizes(n_scans)):
        local = quantised(terrain_scan(seed + i, n=n, scale=1.2))
        at = boundary_indices(n, chunk)
        k = np.arange(len(at))
        local[at, 0], local[at, 1] = 10.5 + (k % 20) * 1.5 + 2.0 ** -10, -20.25 + (k // 20) * 3.0
        local[at, 2] = 30.0 + k
        raws.append(local + O[i])
    return Case("boundaries", raws, F64, Place.records(32, (0, 16, 8)), origins=O)


def assert_boundary_edge(oracle, cfg, case, chunk=4096):
    n = len(case.raws[0])
    at = boundary_indices(n, chunk)
    bev = oracle.Scan(case.p()[0], cfg).bev()[0]
    assert (bev >= 30.0 + cfg.lidar_height).sum() == len(at), "every boundary record owns a cell of its own"


def case_with_tf(n_scans=4, seed=740):
    """6: with h_tf: the matrix sees p"""
    c = case_georef(n_scans, seed)
    return Case("with h_tf", c.raws, F64, Place.records(24, (0, 8, 16)), origins=c.origins, tfs=random_tfs(n_scans, seed=seed, max_tilt_deg=2.0, max_shift=3.0))


def case_identity(layout, n_scans=4, seed=760):
    """7: F32, consecutive, no origin: cc_ingest_points with that {stride, offset}"""
    stride, off = layout
    return Case("identity", [terrain_scan(seed + i, n=n, scale=1.3)[:, :3] for i, n in enumerate(_sizes(n_scans))], F32, Place.records(stride, (off, off + 4, off + 8)))


# ---- the CPU harness' driver ----
class CoordsApi(PointsApi):
    """point_layouts.PointsApi plus the calls that take coordinate streams."""

    def _dbg(self, n, debug):
        if not debug:
            return None, None
        L, ncell = self.L, self._cfg.n_row * self._cfg.n_col
        dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32), "labels": np.zeros((n, L.NLEV, ncell), np.int16)}
        st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
        return dbg, C.cast(st, C.c_void_p)

    @staticmethod
    def src(bufs, streams, stride, type, scale=None, first=0):
        """-> CoordSrc whose streams begin at point `first`"""
        a = [bufs[b].ctypes.data + o + first * stride for b, o in streams]
        sc = [1.0, 1.0, 1.0] if scale is None else [float(v) for v in scale]
        return CoordSrc(a[0], a[1], a[2], type, stride, (C.c_double * 3)(*sc))

    @staticmethod
    def _p(a, dt):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dt)
        return a, C.c_void_p(a.ctypes.data)

    def ingest_coords_rc(self, ctx, src, offsets, origin=None, tf=None, debug=False):
        """cc_ingest_coords: (rc, descriptors, debug outputs or None).  src: a CoordSrc or None (a NULL source)"""
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        dbg, dbg_p = self._dbg(n, debug)
        (_o, op), (_t, tp) = self._p(origin, np.float64), self._p(tf, np.float32)
        rc = self.lib.cc_ingest_coords(ctx, C.byref(src) if src is not None else None, C.c_void_p(offsets.ctypes.data), n, op, tp, C.c_void_p(desc.ctypes.data), dbg_p, None)
        return rc, desc, dbg

    def ingest_coords_host_rc(self, ctx, src, offsets, origin=None, tf=None, want_bev=False):
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        (_o, op), (_t, tp) = self._p(origin, np.float64), self._p(tf, np.float32)
        rc = self.lib.cc_ingest_coords_host(ctx, C.byref(src) if src is not None else None, C.c_void_p(offsets.ctypes.data), n, op, tp, C.c_void_p(desc.ctypes.data),
                                            C.c_void_p(bev.ctypes.data) if want_bev else None)
        return rc, desc, bev

    def scan_ingest_coords_rc(self, ctx, src, n_points, origin=None, tf=None):
        """cc_scan_ingest_coords -> (rc, the scan's descriptor or None)"""
        sc = C.c_void_p()
        (_o, op), (_t, tp) = self._p(origin, np.float64), self._p(tf, np.float32)
        rc = self.lib.cc_scan_ingest_coords(ctx, C.byref(src) if src is not None else None, C.c_int64(n_points), op, tp, 0, C.byref(sc))
        return rc, (self._take(sc)[0] if rc == 0 else None)


class EmuDriver:
    """how the shared check below reaches the library on the CPU harness (numpy in, numpy out)"""
    float_exact = True

    def __init__(self, L):
        self.api = CoordsApi(L)

    def context(self, cfg, n):
        return self.api.create(cfg, max_batch=n)

    def close(self, ctx):
        self.api.lib.cc_destroy(ctx)

    def coords(self, ctx, case):
        bufs, streams, stride = case.build()
        src = self.api.src(bufs, streams, stride, case.type, case.scale)
        rc, d, dbg = self.api.ingest_coords_rc(ctx, src, case.offs(), case.origins, case.tfs, debug=True)
        self.api.chk(rc, "cc_ingest_coords")
        rc, plain, _ = self.api.ingest_coords_rc(ctx, src, case.offs(), case.origins, case.tfs)
        assert rc == 0 and plain.tobytes() == d.tobytes(), "with / without debug outputs"
        return d, dbg

    def points(self, ctx, case):
        return self.api.ingest_points(ctx, case.packed(), (12, 0), case.offs(), tf=case.tfs, debug=True)


def check_case(drv, oracle, cfg, case, ctx=None):
    """The coordinate call on `case`: (a) bev, pix_rc, label images and descriptor of every scan against the oracle on the points p
    (moved by the scan's matrix when the case has one; points with a non-finite x or y, which the library rejects and the reference
    does not define, left out); (b) the bytes against cc_ingest_points on the packed p.  Returns the descriptors and debug outputs."""
    own = ctx is None
    if own:
        ctx = drv.context(cfg, len(case.raws))
    d, dbg = drv.coords(ctx, case)
    r, rdbg = drv.points(ctx, case)
    if own:
        drv.close(ctx)
    report = []
    if d.tobytes() != r.tobytes():
        report.append("%s: the descriptors differ from cc_ingest_points' on the packed p" % case.name)
    for k in ("bev", "pix_rc", "labels"):
        if np.asarray(dbg[k]).tobytes() != np.asarray(rdbg[k]).tobytes():
            report.append("%s: %s differs from cc_ingest_points' on the packed p" % (case.name, k))
    seen = {}
    for i, s in enumerate(case.moved()):
        key = id(case.raws[i])   # (a repeated scan: the oracle once)
        if key not in seen:
            o = oracle.Scan(s[np.isfinite(s[:, 0]) & np.isfinite(s[:, 1])], cfg)
            seen[key] = (o.bev(), o.labels(), o.desc()[0])
        (ob, opix), olab, od = seen[key]
        if not np.array_equal(ob, dbg["bev"][i]):
            report.append("%s scan %d: bev differs from the oracle on p (%d cells)" % (case.name, i, int((ob != np.asarray(dbg["bev"][i]).reshape(ob.shape)).sum())))
        if not np.array_equal(opix, dbg["pix_rc"][i]):
            report.append("%s scan %d: pix_rc differs" % (case.name, i))
        if not np.array_equal(olab, dbg["labels"][i]):
            report.append("%s scan %d: label images differ" % (case.name, i))
        report += ["%s scan %d: %s" % (case.name, i, m) for m in compare_desc(od, d[i], float_exact=drv.float_exact)]
    assert not report, "\n".join(report[:30])
    return d, dbg
