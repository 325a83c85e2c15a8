"""TEST INFRASTRUCTURE for the rig ingest (cc_ingest_rig and its siblings, include/cont2_amd_rig.h): the numpy restatement of the cloud Q
the library is specified to see -- every segment moved by its mode (point_layouts.apply_tf, point_motion.apply_motion on the segment's
SLICE of the pool), the x of every record the rule drops (point_filter.Rule.keeps) replaced by a quiet NaN -- the case builders, each
with an assertion on the ORACLE's side that it reaches the edge it is named after, a driver of the calls on the CPU harness, and the one
check both the harness and the GPU tests run: the oracle on the kept, moved points, and the bytes of cc_ingest_batch on Q."""
import ctypes as C

import numpy as np

from parity import compare_desc, terrain_scan
from point_filter import F32, QNAN, U8, U16, U32, Rule, drop_classes, kitti_labels, repack_with_words
from point_layouts import Layout, PointsApi, apply_tf, rigid
from point_motion import TIME_F32, TIME_U32, apply_motion, cells, time_bins, u32_bits_as_f32

RIG_SEG_MAX = 16
NONE, TF, MOTION = 0, 1, 2
EMPTY = -999.0   # a cell above it is occupied


class RigSegment(C.Structure):
    """cc_rig_segment_t"""
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_int64), ("layout", Layout), ("mode", C.c_int32), ("filter_offset", C.c_int32),
                ("tf", C.c_float * 12), ("time_offset", C.c_int32), ("time_type", C.c_int32), ("t_begin", C.c_float), ("scale", C.c_float),
                ("knot0", C.c_int32), ("n_knots", C.c_int32)]


class Motion:
    """a segment's motion mode: t_begin is the f32 that goes into the slot (TIME_U32: point_motion.u32_bits_as_f32 of the u32)"""

    def __init__(self, time_offset, time_type, t_begin, scale, knot0, n_knots, words):
        self.time_offset, self.time_type, self.t_begin, self.scale, self.knot0, self.n_knots = time_offset, time_type, np.float32(t_begin), np.float32(scale), knot0, n_knots
        self.words = np.ascontiguousarray(words, np.uint32)


class Seg:
    """One segment: records xyzi [n, 4] f32 packed as `layout` (base `shift` bytes behind a 16-byte boundary), a mode -- tf (12 values),
    motion (a Motion) or neither -- and its filter word: flt = (byte offset, the words in the rule's dtype) or None."""

    def __init__(self, xyzi, layout=(16, 0), shift=0, tf=None, motion=None, flt=None, fill=None):
        self.xyzi, self.layout, self.shift, self.tf, self.motion, self.flt, self.fill = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4), layout, shift, tf, motion, flt, fill
        assert tf is None or motion is None

    def __len__(self):
        return len(self.xyzi)

    def moved(self, pool, clamp_to_pool=False):
        """what the library is specified to see of the segment's records, the filter aside: [n, 4] f32, w = 0.  clamp_to_pool: the
        WRONG reading in which a time beyond the slice's end reaches the knots behind the slice (for the cases' own assertions)."""
        if self.motion is not None:
            m = self.motion
            knots = np.asarray(pool, np.float32).reshape(-1, 12)
            sl = knots[m.knot0:] if clamp_to_pool else knots[m.knot0:m.knot0 + m.n_knots]
            return apply_motion(self.xyzi, m.words, m.time_type, m.t_begin, m.scale, sl) if len(self) else np.zeros((0, 4), np.float32)
        if self.tf is not None:
            return apply_tf(self.xyzi, self.tf)
        out = np.zeros((len(self), 4), np.float32)
        out[:, :3] = self.xyzi[:, :3]
        return out

    def keep(self, rule):
        return np.ones(len(self), bool) if self.flt is None else rule.keeps(self.flt[1])

    def buffer(self):
        fields = []
        if self.motion is not None:
            fields.append((self.motion.time_offset, self.motion.words))
        if self.flt is not None:
            fields.append(self.flt)
        return repack_with_words(self.xyzi, self.layout[0], self.layout[1], fields, self.shift, self.fill)

    def fill_c(self, g, ptr):
        """the segment into the cc_rig_segment_t g, its records at address ptr (None: no records)"""
        g.points, g.n_points, g.layout = ptr, len(self), Layout(*self.layout)
        g.mode = MOTION if self.motion is not None else TF if self.tf is not None else NONE
        g.filter_offset = -1 if self.flt is None else self.flt[0]
        if self.tf is not None:
            g.tf[:] = [float(v) for v in np.asarray(self.tf, np.float32).reshape(12)]
        if self.motion is not None:
            m = self.motion
            g.time_offset, g.time_type, g.scale, g.knot0, g.n_knots = m.time_offset, m.time_type, float(m.scale), m.knot0, m.n_knots
            C.memmove(C.addressof(g) + RigSegment.t_begin.offset, np.float32(m.t_begin).tobytes(), 4)   # (the bits, whatever they spell)


class Case:
    """scans: a list of scans, each a list of Seg; pools [n_scans, P, 12] f32 or None; rule: a point_filter.Rule (its offset is not
    read) or None."""

    def __init__(self, name, scans, pools=None, rule=None):
        self.name, self.scans, self.rule = name, scans, rule
        self.pools = None if pools is None else np.ascontiguousarray(np.asarray(pools, np.float32).reshape(len(scans), -1, 12))

    def n_pool(self):
        return 0 if self.pools is None else self.pools.shape[1]

    def _pool(self, i):
        return None if self.pools is None else self.pools[i]

    def moved(self, i, clamp_to_pool=False):
        return np.concatenate([s.moved(self._pool(i), clamp_to_pool) for s in self.scans[i]], 0)

    def keep(self, i):
        return np.concatenate([s.keep(self.rule) for s in self.scans[i]])

    def q(self, i):
        """Q: the moved records, dropped x = NaN -- what cc_ingest_batch is handed for the byte comparison"""
        out = self.moved(i)
        out[~self.keep(i), 0] = QNAN
        return out

    def kept(self, i):
        return self.moved(i)[self.keep(i)]

    def repeat(self, n_scans):
        idx = [i % len(self.scans) for i in range(n_scans)]
        return Case(self.name, [self.scans[i] for i in idx], None if self.pools is None else self.pools[idx], self.rule)

    def take(self, idx):
        return Case(self.name, [self.scans[i] for i in idx], None if self.pools is None else self.pools[list(idx)], self.rule)

    def table(self, place=None):
        """-> (array of RigSegment, int32 scan_segs, what they point to).  place(buffer, shift) -> (address, keep-alive) puts a segment's
        records where the call reads them (default: where numpy has them)."""
        place = place or (lambda buf, shift: (buf.ctypes.data, buf))
        arr = (RigSegment * max(sum(len(sc) for sc in self.scans), 1))()
        scan_segs, held, k = np.zeros(len(self.scans) + 1, np.int32), [], 0
        for i, sc in enumerate(self.scans):
            for s in sc:
                ptr = None
                if len(s):
                    ptr, h = place(s.buffer(), s.shift)
                    held.append(h)
                s.fill_c(arr[k], ptr)
                k += 1
            scan_segs[i + 1] = k
        return arr, scan_segs, held


def assert_keeps(case, at_least=11):
    """every scan of a case keeps more than 10 records, unless the case is named for the opposite"""
    for i in range(len(case.scans)):
        assert int(case.keep(i).sum()) >= at_least, (case.name, i)


def _sizes(n_scans, n0=9001, step=499):
    return [n0 + step * i for i in range(n_scans)]   # 9 001 .. 13 000 records: several chunks, split-part boundaries inside the data


def shift_knots(n_knots, seed=0):
    """knots that differ by whole metres in x and by a yaw of a few degrees from one to the next: a wrong knot lands in another cell"""
    rng = np.random.default_rng(seed)
    return np.stack([rigid(np.deg2rad(rng.uniform(-3, 3)), t=(float(k % 9) - 4.0, float((k * 5) % 7) - 3.0, 0.0), dtype=np.float32).reshape(12) for k in range(n_knots)])


def x_knots(n_knots):
    """pure translations in x by (k mod 8) metres: a point's column and height stay, its row tells the knot"""
    return np.stack([rigid(0.0, t=(float(k % 8), 0.0, 0.0), dtype=np.float32).reshape(12) for k in range(n_knots)])


def _time_words(bins, n_knots):
    """f32 time words that land in the middle of the given bins with t_begin 0 and scale n_knots (u = bin + 0.5)"""
    return ((np.asarray(bins) + np.float32(0.5)) / np.float32(n_knots)).astype(np.float32).view(np.uint32)


# ---- boundaries ----
LAYOUT_A, LAYOUT_B = (32, 0), (48, 8)   # time f32 at 12 / 4 (in front of x), label u32 at 16 / 0


def boundary_cuts(n, chunk, d):
    """where the segments of a boundary scan begin: d records off every split-part boundary (8 parts of ceil(n / 8)) and off the first
    multiples of the chunk, RIG_SEG_MAX - 1 cuts at the most"""
    per = (n + 7) // 8
    cuts = [p * per + d for p in range(1, 8)]
    k = 1
    while len(cuts) < RIG_SEG_MAX - 1 and k * chunk + d < n - 4:
        if k * chunk + d not in cuts:
            cuts.append(k * chunk + d)
        k += 1
    return sorted(cuts)


def case_boundaries(n_scans=4, seed=700, chunk=4096):
    """Segment boundaries -1 / 0 / +1 records off every chunk and every split-part boundary (scan i: (-1, 0, +1, 0)[i mod 4]), the record
    shape, the word offsets and the slice changing at each.  Around a cut c the records c - 2 and c + 1 are dropped, c - 1 sits in the
    last bin of its slice and c in the first of the next one; each of the four is higher than anything else, in a column of its own."""
    scans, pools = [], []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = terrain_scan(seed + i, n=n, scale=1.2)
        lab = kitti_labels(rng, s, share=0.04, high=False)
        cuts = boundary_cuts(n, chunk, (-1, 0, 1, 0)[i % 4])
        bins = rng.integers(0, 4, n)
        t = 0
        for c in cuts:
            for j, (b, dropped) in zip((c - 2, c - 1, c, c + 1), ((2, True), (3, False), (0, False), (1, True))):
                s[j, 0], s[j, 1], s[j, 2] = 10.5, -36.25 + t, 30.0 + t
                bins[j] = b
                lab[j] = (lab[j] & np.uint32(0xFFFF0000)) | np.uint32(252 + t % 8 if dropped else 7)
                t += 1
        segs, edges = [], [0] + cuts + [n]
        for k in range(len(edges) - 1):
            a, b = edges[k], edges[k + 1]
            lay, t_off, f_off = (LAYOUT_A, 12, 16) if k % 2 == 0 else (LAYOUT_B, 4, 0)
            segs.append(Seg(s[a:b], lay, motion=Motion(t_off, TIME_F32, 0.0, 4.0, 4 * k, 4, _time_words(bins[a:b], 4)), flt=(f_off, lab[a:b]), fill=seed + k))
        scans.append(segs)
        pools.append(x_knots(64))
    c = Case("boundaries", scans, pools, drop_classes(0, U32, mask=0xFFFF))
    assert_keeps(c)
    return c


# ---- ties across segments ----
def case_ties(dropped, n_scans=4, seed=720):
    """Two segments whose records fall into the same 36 cells with heights on one 6-value lattice.  dropped: the earlier segment's records
    at the top height are dropped, so the later segment owns those cells -- pix_rc changes, bev does not; otherwise nothing is dropped
    and the earlier segment owns them."""
    scans, pools = [], []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = np.zeros((n, 4), np.float32)
        s[:, 0], s[:, 1] = rng.uniform(10.0, 16.0, n), rng.uniform(-3.0, 3.0, n)
        s[:, 2] = rng.integers(0, 6, n) * 0.5 - 1.0
        h = n // 2 + 3
        tag = np.where((s[:h, 2] == 1.5) & dropped, 1, 0).astype(np.uint8)
        bins = rng.integers(0, 2, n - h)
        scans.append([Seg(s[:h], (32, 0), tf=rigid(0.0, t=(0.25, 0.0, 0.0), dtype=np.float32).reshape(12), flt=(17, tag), fill=seed),
                      Seg(s[h:], (32, 0), motion=Motion(20, TIME_F32, 0.0, 2.0, 1, 2, _time_words(bins, 2)))])
        pools.append(np.stack([rigid(0.0, t=(0.0, 0.0, 9.0), dtype=np.float32).reshape(12)] + [rigid(0.0, t=(0.125 * k, 0.0, 0.0), dtype=np.float32).reshape(12) for k in (1, 2)]))
    c = Case("ties, the earlier one dropped" if dropped else "ties", scans, pools, Rule(0, U8, kept=[True, False], keep_other=1))
    assert_keeps(c)
    return c


# ---- slices ----
def case_slices(n_scans=4, seed=740):
    """Two motion segments on the slices [0, 16) and [16, 48) of one pool of 48.  A third of the times lies beyond the slice's end (they
    clamp to ITS last knot, not to the neighbour's first or the pool's last), a tenth before t_begin, some are NaN (its first knot)."""
    scans, pools = [], []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = terrain_scan(seed + i, n=n, scale=1.3)
        h = n // 2 + 1
        segs = []
        for part, (k0, nk, ttype) in zip((s[:h], s[h:]), ((0, 16, TIME_F32), (16, 32, TIME_U32))):
            m = len(part)
            u = rng.uniform(-0.15, 1.5, m)   # in sweeps: [0, 1) is the slice
            if ttype == TIME_F32:
                t = (2.0 + u * 0.1).astype(np.float32)
                t[rng.choice(m, m // 50, replace=False)] = np.float32(np.nan)
                mo = Motion(28, TIME_F32, 2.0, nk / 0.1, k0, nk, t.view(np.uint32))
            else:   # u32 nanoseconds from 4 000 000 000 on, wrapping; a time before t_begin wraps to a huge one: the slice's LAST knot
                w = (np.uint64(4000000000) + (np.maximum(u, 0.0) * 1e8).astype(np.uint64)).astype(np.uint32)
                mo = Motion(28, TIME_U32, u32_bits_as_f32(4000000000), nk / 1e8, k0, nk, w)
            segs.append(Seg(part, (32, 0), motion=mo))
        scans.append(segs)
        pools.append(shift_knots(48, seed + i))
    c = Case("slices", scans, pools)
    return c


def assert_slices(cfg, case):
    """the case fails if the clamp used the pool's size: the two readings put hundreds of records into different cells"""
    for i in range(len(case.scans)):
        seg0 = case.scans[i][0]
        m = seg0.motion
        b = time_bins(m.words, m.time_type, m.t_begin, m.scale, 48)   # the bins a clamp to the pool would give
        assert (b >= 16).sum() > 500 and (b == 0).sum() > 200 and np.isnan(m.words.view(np.float32)).sum() > 20
        right, wrong = cells(cfg, seg0.moved(case.pools[i])), cells(cfg, seg0.moved(case.pools[i], clamp_to_pool=True))
        assert ((right != wrong) & (b >= 16)).sum() > 300, "clamping to the pool moves records to other cells"
        assert np.array_equal(right[b < 16], wrong[b < 16])


# ---- a mixed scan ----
MIXED_KINDS = ("u8", "u16", "u32", "range")
_MIXED_OFFS = {"u8": (13, 17, 3, 19), "u16": (14, 18, 2, 18), "u32": (12, 20, 0, 16), "range": (12, 20, 0, 16)}   # the word's offset in segments 0 .. 3


def case_mixed(kind, n_scans=4, seed=760):
    """none, tf, f32-time and u32-time segments in one scan; layouts {16, 0}, {32, 0}, {48, 8} with the time word in front of x, {20, 0},
    and a base at 4 mod 16; the filter word -- a u8, u16 or u32 class (200 .. 207 are the dropped ones; a u32 carries an instance id in
    its high half) or an f32 under the range rule -- at another offset in every segment; one unfiltered segment."""
    scans, pools = [], []
    dtype = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "range": np.float32}[kind]
    offs = _MIXED_OFFS[kind]
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = terrain_scan(seed + i, n=n, scale=1.3)
        e = [0, n // 5 + 1, 2 * n // 5 - 3, 3 * n // 5 + 2, 4 * n // 5 - 1, n]
        p = [s[e[k]:e[k + 1]] for k in range(5)]

        def word(k):
            if kind == "range":
                v = rng.uniform(0.0, 1.0, len(p[k])).astype(np.float32)
                v[::97] = np.float32(np.nan)
                return v
            w = kitti_labels(rng, p[k], share=0.08)
            cls = np.where((w & np.uint32(0xFFFF)) >= 252, (w & np.uint32(0xFFFF)) - 52, w & np.uint32(0xFFFF))
            return ((w & np.uint32(0xFFFF0000)) | cls).astype(np.uint32) if kind == "u32" else cls.astype(dtype)

        tfs = [rigid(0.3, 0.01, -0.02, (1.5, -2.0, 0.1), np.float32).reshape(12), rigid(-1.1, 0.0, 0.02, (-3.0, 0.5, -0.1), np.float32).reshape(12)]
        t2 = (5.0 + rng.uniform(-0.01, 0.12, len(p[2]))).astype(np.float32)
        w3 = (np.uint64(1000) + rng.integers(0, 120000000, len(p[3])).astype(np.uint64)).astype(np.uint32)
        scans.append([
            Seg(p[0], (16, 0), flt=(offs[0], word(0)), fill=seed),
            Seg(p[1], (32, 0), tf=tfs[0], flt=(offs[1], word(1)), fill=seed + 1),
            Seg(p[2], (48, 8), motion=Motion(4, TIME_F32, 5.0, 24 / 0.1, 0, 24, t2.view(np.uint32)), flt=(offs[2], word(2)), fill=seed + 2),
            Seg(p[3], (20, 0), motion=Motion(12, TIME_U32, u32_bits_as_f32(1000), 8 / 1e8, 24, 8, w3), flt=(offs[3], word(3)), fill=seed + 3),
            Seg(p[4], (16, 0), shift=4, tf=tfs[1]),
        ])
        pools.append(shift_knots(32, seed + i))
    if kind == "range":
        rule = Rule(0, F32, lo=0.1, hi=0.9)
    else:
        rule = drop_classes(0, {"u8": U8, "u16": U16, "u32": U32}[kind], dropped=range(200, 208), n_classes=208, mask=0xFF if kind == "u8" else 0xFFFF)
    c = Case("mixed, %s" % kind, scans, pools, rule)
    assert_keeps(c)
    for i in range(n_scans):
        k = c.keep(i)
        assert 0.03 < 1.0 - k.mean() < 0.4 and k[-len(scans[i][4]):].all()
    return c


# ---- empties and limits ----
def case_empties(n_scans=4, seed=780):
    """empty segments first, in the middle and last, and a segment whose records are all dropped"""
    scans, pools = [], []
    none = np.zeros((0, 4), np.float32)
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = terrain_scan(seed + i, n=n, scale=1.3)
        a, b = n // 3, 2 * n // 3
        lab = kitti_labels(rng, s)
        gone = np.full(b - a, 255, np.uint32)
        bins = rng.integers(0, 8, n - b)
        scans.append([Seg(none, (32, 0), tf=shift_knots(1)[0]), Seg(s[:a], (16, 0), flt=(12, lab[:a])), Seg(none, (16, 0)), Seg(none, (48, 8), motion=Motion(4, TIME_F32, 0.0, 1.0, 0, 8, [])),
                      Seg(s[a:b], (32, 0), flt=(16, gone), fill=seed), Seg(s[b:], (32, 0), motion=Motion(12, TIME_F32, 0.0, 8.0, 0, 8, _time_words(bins, 8)), flt=(24, lab[b:])),
                      Seg(none, (16, 0), flt=(12, np.zeros(0, np.uint32)))])
        pools.append(shift_knots(8, seed + i))
    c = Case("empties", scans, pools, drop_classes(0, U32, mask=0xFFFF))
    assert_keeps(c)
    assert all(not c.scans[i][4].keep(c.rule).any() for i in range(n_scans))
    return c


def case_all_dropped(n_scans=4, seed=800):
    """scans whose records are all dropped: n_pix 0, the empty descriptor (the limits on a scan count records)"""
    scans = []
    for i, n in enumerate(_sizes(n_scans)):
        s = terrain_scan(seed + i, n=n, scale=1.3)
        h = n // 2
        scans.append([Seg(s[:h], (16, 0), flt=(12, np.full(h, 252, np.uint32))), Seg(s[h:], (32, 0), tf=shift_knots(1)[0], flt=(20, np.full(n - h, 259, np.uint32)))])
    c = Case("everything dropped", scans, None, drop_classes(0, U32, mask=0xFFFF))
    assert all(not c.keep(i).any() for i in range(n_scans))
    return c


def case_max_segments(n_scans=4, seed=820):
    """CC_RIG_SEG_MAX segments with a pool of 64: every segment a slice of 4"""
    scans, pools = [], []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = terrain_scan(seed + i, n=n, scale=1.3)
        lab = kitti_labels(rng, s)
        e = np.linspace(0, n, RIG_SEG_MAX + 1).astype(int)
        bins = rng.integers(0, 4, n)
        scans.append([Seg(s[e[k]:e[k + 1]], (32, 0), motion=Motion(12, TIME_F32, 0.0, 4.0, 4 * k, 4, _time_words(bins[e[k]:e[k + 1]], 4)), flt=(16, lab[e[k]:e[k + 1]])) for k in range(RIG_SEG_MAX)])
        pools.append(shift_knots(64, seed + i))
    c = Case("max segments", scans, pools, drop_classes(0, U32, mask=0xFFFF))
    assert_keeps(c)
    return c


# ---- the edges, asserted on the oracle's side ----
def assert_edge(oracle, cfg, case, i=0):
    """the oracle on all the moved records against the oracle on the kept ones"""
    (ab, ap), (kb, kp) = oracle.Scan(case.moved(i), cfg).bev(), oracle.Scan(case.kept(i), cfg).bev()
    if case.name == "boundaries":
        n_cuts = len(case.scans[i]) - 1
        assert n_cuts >= 9 and (ab >= 30.0).sum() == 4 * n_cuts and (kb >= 30.0).sum() == 2 * n_cuts, "the dropped spikes own cells unless the filter sees them"
        k, mv = case.keep(i), case.moved(i)
        first = np.cumsum([len(s) for s in case.scans[i]])[:-1]
        assert (mv[first - 1, 0] != mv[first, 0]).all() and k[first].all() and k[first - 1].all() and not k[first - 2].any() and not k[first + 1].any()
    if case.name == "ties, the earlier one dropped":
        same = (kb > EMPTY) & (kb == ab)
        assert (same & (ap != kp).any(axis=1)).sum() >= 5, "the later segment owns the cell: pix_rc changes, bev does not"
    if case.name == "ties":
        assert case.keep(i).all()
        (fb, fp) = oracle.Scan(case.scans[i][0].moved(case.pools[i]), cfg).bev()   # the earlier segment alone
        (lb, _lp) = oracle.Scan(case.scans[i][1].moved(case.pools[i]), cfg).bev()
        tied = (fb > EMPTY) & (fb == lb)
        assert tied.sum() >= 5 and np.array_equal(ap[tied], fp[tied]), "among equal heights the earlier segment's record owns the cell"
    if case.name == "empties":
        assert ((ab > EMPTY) & (kb < ab)).sum() >= 20


# ---- the CPU harness' driver ----
class RigApi(PointsApi):
    """point_layouts.PointsApi plus the rig calls."""

    def _dbg(self, n, debug):
        if not debug:
            return None, None
        ncell = self._cfg.n_row * self._cfg.n_col
        dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32), "labels": np.zeros((n, self.L.NLEV, ncell), np.int16)}
        st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
        return dbg, C.cast(st, C.c_void_p)

    @staticmethod
    def _args(pools, flt):
        kn = None if pools is None else np.ascontiguousarray(pools, np.float32)
        return kn, (C.c_void_p(kn.ctypes.data) if kn is not None else None), (0 if kn is None else kn.reshape(len(kn), -1).shape[1] // 12), (C.byref(flt) if flt is not None else None)

    def ingest_rig_rc(self, ctx, arr, scan_segs, pools, flt, debug=False, n_pool=None):
        """cc_ingest_rig on a raw array of cc_rig_segment_t: (rc, descriptors, debug outputs or None).  pools [n, P, 12] or None; flt: a
        point_filter.Filter or None"""
        scan_segs = np.ascontiguousarray(scan_segs, np.int32)
        n = len(scan_segs) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        dbg, dbg_p = self._dbg(n, debug)
        kn, kn_p, P, flt_p = self._args(pools, flt)
        rc = self.lib.cc_ingest_rig(ctx, arr, C.c_void_p(scan_segs.ctypes.data), n, kn_p, P if n_pool is None else n_pool, flt_p, C.c_void_p(desc.ctypes.data), dbg_p, None)
        return rc, desc, dbg

    def ingest_rig_host_rc(self, ctx, arr, scan_segs, pools, flt, want_bev=False, n_pool=None):
        scan_segs = np.ascontiguousarray(scan_segs, np.int32)
        n = len(scan_segs) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        kn, kn_p, P, flt_p = self._args(pools, flt)
        rc = self.lib.cc_ingest_rig_host(ctx, arr, C.c_void_p(scan_segs.ctypes.data), n, kn_p, P if n_pool is None else n_pool, flt_p, C.c_void_p(desc.ctypes.data),
                                         C.c_void_p(bev.ctypes.data) if want_bev else None)
        return rc, desc, bev

    def scan_ingest_rig_rc(self, ctx, arr, s0, n_segs, pool, flt, n_pool=None):
        """cc_scan_ingest_rig for the n_segs segments from arr[s0] on -> (rc, the scan's descriptor or None)"""
        sc = C.c_void_p()
        kn, kn_p, P, flt_p = self._args(None if pool is None else np.asarray(pool, np.float32).reshape(1, -1, 12), flt)
        rc = self.lib.cc_scan_ingest_rig(ctx, C.byref(arr, s0 * C.sizeof(RigSegment)), n_segs, kn_p, P if n_pool is None else n_pool, flt_p, 0, C.byref(sc))
        return rc, (self._take(sc)[0] if rc == 0 else None)


def c_rule(case):
    """the case's rule as the C struct (and what it points to)"""
    return (None, None) if case.rule is None else case.rule.c()


class EmuDriver:
    """how the shared check reaches the library on the CPU harness (numpy in, numpy out; "device" pointers are host pointers there)"""
    float_exact = True

    def __init__(self, L):
        self.api = RigApi(L)

    def context(self, cfg, n):
        return self.api.create(cfg, max_batch=n)

    def close(self, ctx):
        self.api.lib.cc_destroy(ctx)

    def rig(self, ctx, case):
        arr, scan_segs, _held = case.table()
        f, _bits = c_rule(case)
        rc, d, dbg = self.api.ingest_rig_rc(ctx, arr, scan_segs, case.pools, f, debug=True)
        self.api.chk(rc, "cc_ingest_rig")
        rc, plain, _ = self.api.ingest_rig_rc(ctx, arr, scan_segs, case.pools, f)
        assert rc == 0 and plain.tobytes() == d.tobytes(), "with / without debug outputs"
        return d, dbg

    def batch(self, ctx, clouds):
        offs = np.concatenate([[0], np.cumsum([len(q) for q in clouds])]).astype(np.int64)
        return self.api.ingest(ctx, np.concatenate(clouds, 0), offs, debug=True)


def check_case(drv, oracle, cfg, case, ctx=None):
    """The rig call on `case`: (1) bev, pix_rc, label images and descriptor of every scan that keeps more than 10 records against the
    oracle on its kept, moved points; (2) the bytes of cc_ingest_batch on the numpy-built Q, dropped x = NaN; (3) with and without
    debug outputs the same bytes (the driver's).  Returns the descriptors and debug outputs."""
    own = ctx is None
    if own:
        ctx = drv.context(cfg, len(case.scans))
    d, dbg = drv.rig(ctx, case)
    qs, seen_q = [], {}
    for i in range(len(case.scans)):
        key = id(case.scans[i])
        if key not in seen_q:
            seen_q[key] = case.q(i)
        qs.append(seen_q[key])
    r, rdbg = drv.batch(ctx, qs)
    if own:
        drv.close(ctx)
    report = []
    if d.tobytes() != r.tobytes():
        report.append("%s: the descriptors differ from cc_ingest_batch's on Q" % case.name)
    for k in ("bev", "pix_rc", "labels"):
        if np.asarray(dbg[k]).tobytes() != np.asarray(rdbg[k]).tobytes():
            report.append("%s: %s differs from cc_ingest_batch's on Q" % (case.name, k))
    seen = {}
    for i in range(len(case.scans)):
        key = id(case.scans[i])
        if key not in seen:
            pts = case.kept(i)
            if len(pts) <= 10:
                seen[key] = None
            else:
                o = oracle.Scan(pts, cfg)
                seen[key] = (o.bev(), o.labels(), o.desc()[0])
        if seen[key] is None:
            continue
        (ob, opix), olab, od = seen[key]
        if not np.array_equal(ob, dbg["bev"][i]):
            report.append("%s scan %d: bev differs from the oracle on the kept, moved points" % (case.name, i))
        if not np.array_equal(opix, dbg["pix_rc"][i]):
            report.append("%s scan %d: pix_rc differs" % (case.name, i))
        if not np.array_equal(olab, dbg["labels"][i]):
            report.append("%s scan %d: label images differ" % (case.name, i))
        report += ["%s scan %d: %s" % (case.name, i, m) for m in compare_desc(od, d[i], float_exact=drv.float_exact)]
    assert not report, "\n".join(report[:30])
    return d, dbg
