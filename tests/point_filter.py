"""TEST INFRASTRUCTURE for the filtered ingest (cc_ingest_points_filtered and its siblings, include/cont2_amd_filter.h): the numpy
restatement of the two rules, a builder of records that carry filter words, the cases -- each asserts on the ORACLE's side that it
reaches the edge it is named after -- a driver of the calls on the CPU harness, and the check both the harness and the GPU tests run:
the oracle on the kept records alone, and the bytes of cc_ingest_points on the records whose dropped x are NaN."""
import ctypes as C

import numpy as np

from parity import compare_desc, terrain_scan
from point_layouts import NAN_FILL, PointsApi, apply_tf, random_tfs

CLASSES_MAX = 4096
U8, U16, U32, F32 = 0, 1, 2, 3
DTYPES = {U8: np.uint8, U16: np.uint16, U32: np.uint32, F32: np.float32}
NAMES = {U8: "u8", U16: "u16", U32: "u32"}
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
MOVING = range(252, 260)   # SemanticKITTI's moving-object classes


class Filter(C.Structure):
    """cc_point_filter_t"""
    _fields_ = [("offset", C.c_int32), ("type", C.c_int32), ("shift", C.c_int32), ("mask", C.c_uint32), ("n_classes", C.c_int32),
                ("keep_other", C.c_int32), ("lo", C.c_float), ("hi", C.c_float), ("keep_bits", C.c_void_p)]


class Rule:
    """One filter: where the word sits, its type, and the class rule (shift, mask, n_classes, keep_other, kept: bool [n_classes]) or the
    range rule (lo, hi).  keeps(words) is the specification in numpy; c() the C struct; python(cc) the package's PointFilter."""

    def __init__(self, offset, type, shift=0, mask=0xFFFFFFFF, kept=None, keep_other=1, lo=0.0, hi=0.0):
        self.offset, self.type, self.shift, self.mask, self.keep_other, self.lo, self.hi = offset, type, shift, mask, keep_other, lo, hi
        self.kept = None if kept is None else np.asarray(kept, bool)
        self.n_classes = 0 if kept is None else len(self.kept)

    def bits(self):
        b = np.zeros(((self.n_classes + 31) // 32) * 32, bool)
        b[:self.n_classes] = self.kept
        return np.ascontiguousarray(np.packbits(b, bitorder="little").view(np.uint32))

    def c(self):
        """-> (Filter, what it points to)"""
        if self.type == F32:
            return Filter(self.offset, F32, 0, 0, 0, 0, self.lo, self.hi, None), None
        bits = self.bits()
        return Filter(self.offset, self.type, self.shift, self.mask, self.n_classes, self.keep_other, 0.0, 0.0, bits.ctypes.data), bits

    def python(self, cc):
        if self.type == F32:
            return cc.PointFilter.range(self.offset, self.lo, self.hi)
        return cc.PointFilter.classes(self.offset, NAMES[self.type], keep=np.flatnonzero(self.kept).tolist(), n_classes=self.n_classes, shift=self.shift,
                                      mask=self.mask, other="keep" if self.keep_other else "drop")

    def keeps(self, words):
        """words: the filter word of every record, in its own dtype -> bool [n]"""
        words = np.asarray(words)
        assert words.dtype == DTYPES[self.type], (words.dtype, self.type)
        if self.type == F32:
            with np.errstate(invalid="ignore"):
                return (np.float32(self.lo) <= words) & (words <= np.float32(self.hi))
        cls = (words.astype(np.uint64) >> np.uint64(self.shift)) & np.uint64(self.mask)
        inside = cls < self.n_classes
        return np.where(inside, self.kept[np.where(inside, cls, 0).astype(np.int64)], bool(self.keep_other))


def drop_classes(offset, type, dropped=MOVING, n_classes=260, **kw):
    kept = np.ones(n_classes, bool)
    kept[list(dropped)] = False
    return Rule(offset, type, kept=kept, **kw)


def repack_with_words(xyzi, stride, off, fields, base_shift=0, fill=None):
    """point_layouts.repack with extra fields: fields = [(byte offset, array [n] of u8 / u16 / u32 / f32), ...] written into every
    record; every other byte holds NaN bit patterns, or -- fill: a seed -- random bytes.  Returns a uint8 array whose data pointer is
    16-byte aligned + base_shift."""
    xyzi = np.ascontiguousarray(xyzi, np.float32)
    n = len(xyzi)
    words = np.full(n * (stride // 4) + 8, NAN_FILL, np.uint32)
    if fill is not None:
        words[:] = np.random.default_rng(fill).integers(0, 2 ** 32, len(words), dtype=np.uint64).astype(np.uint32)
    shift = ((-words.ctypes.data) % 16 + base_shift) // 4
    rec = words[shift:shift + n * (stride // 4)].reshape(n, stride // 4)
    rec[:, off // 4:off // 4 + 3] = xyzi[:, :3].view(np.uint32)
    raw = rec.view(np.uint8).reshape(n, stride)
    for o, a in fields:
        a = np.ascontiguousarray(a)
        assert len(a) == n and o % a.dtype.itemsize == 0
        raw[:, o:o + a.dtype.itemsize] = a.view(np.uint8).reshape(n, a.dtype.itemsize)
    out = rec.reshape(-1).view(np.uint8)
    assert out.ctypes.data % 16 == base_shift % 16
    return out


def nan_x(scan, keep):
    """the scan with the x of every dropped record replaced by a quiet NaN: what the filtered call is specified to equal"""
    s = np.array(scan, np.float32, copy=True)
    s[~keep, 0] = QNAN
    return s


class Case:
    """Scans [n, 4] f32 with their filter words (one array per scan), the rule, and the record shape they are packed into."""

    def __init__(self, name, scans, words, rule, layout=(16, 0), base_shift=0, tfs=None, extra=None, fill=None):
        self.name, self.scans, self.words, self.rule, self.layout, self.base_shift, self.tfs, self.fill = name, scans, words, rule, layout, base_shift, tfs, fill
        self.extra = extra or [[] for _ in scans]   # further fields per scan: [(offset, array)]
        self.keep = [rule.keeps(w) for w in words]

    def offs(self):
        return np.concatenate([[0], np.cumsum([len(s) for s in self.scans])]).astype(np.int64)

    def buffer(self, scans=None):
        scans = self.scans if scans is None else scans
        fields = [(self.rule.offset, np.concatenate(self.words))]
        for k in range(len(self.extra[0])):
            fields.append((self.extra[0][k][0], np.concatenate([e[k][1] for e in self.extra])))
        return repack_with_words(np.concatenate(scans, 0), self.layout[0], self.layout[1], fields, self.base_shift, self.fill)

    def kept_scans(self):
        """the records the oracle sees: the kept ones alone, in their order, moved by the scan's matrix when the case has one"""
        out = [s[k] for s, k in zip(self.scans, self.keep)]
        return out if self.tfs is None else [apply_tf(s, m) for s, m in zip(out, self.tfs)]

    def all_scans(self):
        return self.scans if self.tfs is None else [apply_tf(s, m) for s, m in zip(self.scans, self.tfs)]

    def repeat(self, n_scans):
        """the case with its scans repeated to n_scans (4: split sweep + merge kernel; 9: one workgroup per scan)"""
        idx = [i % len(self.scans) for i in range(n_scans)]
        return Case(self.name, [self.scans[i] for i in idx], [self.words[i] for i in idx], self.rule, self.layout, self.base_shift,
                    None if self.tfs is None else np.stack([self.tfs[i] for i in idx]), [self.extra[i] for i in idx], self.fill)


def kitti_labels(rng, s, share=0.08, high=True):
    """SemanticKITTI words for scan s: static classes 0 .. 99, `share` of the records moving (252 .. 259) in runs of 20 - 60 consecutive
    records (a moving object is a run of neighbouring firings), biased to the upper third of the heights when `high`; in the high 16
    bits a random instance id, which the rule must ignore."""
    n = len(s)
    cls = rng.integers(0, 100, n).astype(np.uint32)
    moving = np.zeros(n, bool)
    while moving.sum() < share * n:
        a = int(rng.integers(0, n))
        moving[a:a + int(rng.integers(20, 60))] = True
    if high:
        moving |= (s[:, 2] > np.quantile(s[:, 2], 0.67)) & (rng.random(n) < 0.15)
    cls[moving] = rng.integers(252, 260, int(moving.sum())).astype(np.uint32)
    return (rng.integers(1, 2 ** 16, n).astype(np.uint32) << np.uint32(16)) | cls


def _sizes(n_scans, n0=9001, step=499):
    return [n0 + step * i for i in range(n_scans)]   # 9 001 .. 13 000: several chunks, part boundaries inside the data


def case_dropped_maxima(n_scans=4, seed=300):
    """1: dropped records are cells' maxima -- the cells' heights and positions change"""
    scans = [terrain_scan(seed + i, n=n, scale=1.3 + 0.1 * (i % 4)) for i, n in enumerate(_sizes(n_scans))]
    words = [kitti_labels(np.random.default_rng(seed + 50 + i), s) for i, s in enumerate(scans)]
    return Case("dropped maxima", scans, words, drop_classes(12, U32, mask=0xFFFF))


def case_first_of_equals(n_scans=4, seed=320):
    """2: the dropped record is the first of several equal heights in its cell -- pix_rc changes, bev does not.  36 cells, hundreds of
    records each, heights on a 6-value lattice; a third of the records is dropped at random."""
    scans, words = [], []
    for i, n in enumerate(_sizes(n_scans)):
        rng = np.random.default_rng(seed + i)
        s = np.zeros((n, 4), np.float32)
        s[:, 0], s[:, 1] = rng.uniform(10.0, 16.0, n), rng.uniform(-3.0, 3.0, n)
        s[:, 2] = rng.integers(0, 6, n) * 0.5 - 1.0
        scans.append(s)
        words.append(np.where(rng.random(n) < 0.33, 1, 0).astype(np.uint8))
    return Case("first of equals", scans, words, Rule(17, U8, kept=[True, False], keep_other=1), layout=(32, 0), fill=seed)


def case_extremes(n_scans=4, seed=340):
    """3: the dropped records hold the scan's highest and lowest points -- max_bin_val / min_bin_val change"""
    scans = [terrain_scan(seed + i, n=n, scale=1.5) for i, n in enumerate(_sizes(n_scans))]
    words = []
    for s in scans:
        lo, hi = np.quantile(s[:, 2], [0.01, 0.99])
        words.append(np.where((s[:, 2] <= lo) | (s[:, 2] >= hi), 300, 7).astype(np.uint16))
    return Case("extremes", scans, words, Rule(18, U16, kept=np.ones(256, bool), keep_other=0), layout=(32, 0))


def boundary_indices(n, chunk):
    """the records on both sides of every chunk boundary (`chunk`: 4 096 on the device, 1 024 on the CPU harness; a multiple of 1 024
    either way, so 4 095 / 4 096 / 8 191 / 8 192 are among them) and of every split-part boundary (8 parts of ceil(n / 8) records)"""
    per = (n + 7) // 8
    idx = {k * 1024 + d for k in range(1, n // 1024 + 1) for d in (-1, 0)} | {p * per + d for p in range(1, 8) for d in (-1, 0)}
    assert chunk % 1024 == 0 and {4095, 4096, 8191, 8192} <= idx
    return np.array(sorted(i for i in idx if 0 <= i < n))


def case_boundaries(n_scans=4, seed=360, chunk=4096):
    """4: dropped records at 4 095 / 4 096 / 8 191 / 8 192 and on both sides of every split-part boundary; each of them is higher than
    anything near it, so it would own its cell and the scan's maximum if the filter missed it"""
    scans, words = [], []
    for i, n in enumerate(_sizes(n_scans)):
        s = terrain_scan(seed + i, n=n, scale=1.2)
        at = boundary_indices(n, chunk)
        w = np.full(n, 5, np.uint32)
        w[at] = 252 + np.arange(len(at)) % 8
        s[at, 2] = 30.0 + np.arange(len(at), dtype=np.float32)
        k = np.arange(len(at))   # a cell of its own each, inside the map and outside the blind disc at both resolutions of the tests
        s[at, 0], s[at, 1] = 10.5 + (k % 20) * 1.5, -20.25 + (k // 20) * 3.0
        scans.append(s)
        words.append(w)
    return Case("boundaries", scans, words, drop_classes(4, U32), layout=(48, 8))


def case_shift_mask(variant, n_scans=4, seed=380):
    """8: shift / mask combinations on random words; n_classes of 1, 32, 33 and 4 096; classes beyond the table under both keep_other"""
    rng = np.random.default_rng(seed + variant)
    type, off, layout, shift, mask, n_classes, other = [
        (U32, 12, (16, 0), 0, 0x1, 1, 1),            # n_classes 1: class 0 by the table, class 1 by keep_other
        (U32, 12, (16, 0), 31, 0xFFFFFFFF, 1, 0),    # the top bit alone
        (U32, 20, (32, 0), 16, 0x3F, 32, 1),         # a 6-bit field, half of it beyond the table, kept
        (U32, 20, (32, 0), 16, 0x3F, 32, 0),         # ... dropped
        (U16, 18, (32, 0), 4, 0xFF, 33, 0),          # bit 32: the table's second word
        (U16, 30, (32, 0), 3, 0x1FFF, 4096, 1),      # the largest table, the record's last two bytes, half of the classes beyond it
        (U32, 4, (48, 8), 20, 0xFFFFFFFF, 4096, 0),  # every class inside the largest table
        (U8, 17, (32, 0), 7, 0xFFFFFFFF, 1, 1),      # a mask wider than the word: the neighbouring bytes must not reach the class
        (U8, 19, (32, 0), 0, 0xFFFFFFFF, 33, 1),     # ... the dword's last byte
        (U8, 16, (20, 0), 2, 0x3F, 32, 0),           # a run-time stride, the record's tail
    ][variant]
    kept = rng.random(n_classes) < 0.5
    kept[[0, n_classes - 1]] = [True, False] if n_classes > 1 else [not other]
    scans = [terrain_scan(seed + 10 * variant + i, n=n, scale=1.3) for i, n in enumerate(_sizes(n_scans))]
    words = [rng.integers(0, 2 ** 32, len(s), dtype=np.uint64).astype(DTYPES[type]) for s in scans]
    c = Case("shift / mask %d" % variant, scans, words, Rule(off, type, shift, mask, kept, other), layout=layout, fill=seed + variant)
    cls = [(w.astype(np.uint64) >> np.uint64(shift)) & np.uint64(mask) for w in words]
    if variant not in (6,):
        assert all((k >= n_classes).sum() > 500 for k in cls), "classes beyond the table"
    assert all(200 < k.sum() < len(k) - 200 for k in c.keep)
    return c


N_SHIFT_MASK = 10


def case_layout(variant, n_scans=4, seed=420):
    """7: the record shapes of the issue, with SemanticKITTI's rule or a tag byte / ring word"""
    scans = [terrain_scan(seed + i, n=n, scale=1.3) for i, n in enumerate(_sizes(n_scans))]
    rngs = [np.random.default_rng(seed + 30 + i) for i in range(n_scans)]
    if variant == 0:     # {16, 0}, u32 at 12: SemanticKITTI, an instance id in the high bits
        return Case("kitti labels", scans, [kitti_labels(r, s) for r, s in zip(rngs, scans)], drop_classes(12, U32, mask=0xFFFF))
    if variant == 1:     # {32, 0}: a tag byte at 17 (0 valid, 1 .. 3 noise kinds) beside a ring word at 18 that the call ignores
        tags = [np.where(r.random(len(s)) < 0.12, r.integers(1, 4, len(s)), 0).astype(np.uint8) for r, s in zip(rngs, scans)]
        rings = [[(18, r.integers(0, 64, len(s)).astype(np.uint16))] for r, s in zip(rngs, scans)]
        return Case("tag byte", scans, tags, Rule(17, U8, kept=[True], keep_other=0), layout=(32, 0), extra=rings, fill=seed)
    if variant == 2:     # {32, 0}: the even rings of the u16 at 18, beside the tag byte
        rings = [(np.arange(len(s)) // 128 % 64).astype(np.uint16) for s in scans]
        tags = [[(17, r.integers(0, 4, len(s)).astype(np.uint8))] for r, s in zip(rngs, scans)]
        return Case("ring subset", scans, rings, Rule(18, U16, kept=np.arange(64) % 2 == 0, keep_other=0), layout=(32, 0), extra=tags, fill=seed)
    if variant == 3:     # {48, 8}: the word in front of xyz
        return Case("word in front of xyz", scans, [kitti_labels(r, s) for r, s in zip(rngs, scans)], drop_classes(0, U32, mask=0xFFFF), layout=(48, 8))
    return Case("base 4 bytes off", scans, [kitti_labels(r, s) for r, s in zip(rngs, scans)], drop_classes(12, U32, mask=0xFFFF), base_shift=4)


N_LAYOUTS = 5


def case_range(variant, n_scans=4, seed=460):
    """9: the range rule: a band; lo == hi; (-inf, inf) keeps every non-NaN; a NaN word is dropped; -0.0 against lo = 0"""
    scans = [terrain_scan(seed + i, n=n, scale=1.3) for i, n in enumerate(_sizes(n_scans))]
    words = []
    for i, s in enumerate(scans):
        rng = np.random.default_rng(seed + 40 + i)
        v = rng.uniform(0.0, 1.0, len(s)).astype(np.float32)
        special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 0.25, np.nextafter(np.float32(0.25), np.float32(0)), np.nextafter(np.float32(0.25), np.float32(1)),
                            0.75, np.nextafter(np.float32(0.75), np.float32(1)), -1e-45, 1e-45], np.float32)
        at = rng.choice(len(s), len(s) // 3, replace=False)
        v[at] = np.resize(special, len(at))
        words.append(v)
    lo, hi = [(0.25, 0.75), (0.25, 0.25), (-np.inf, np.inf), (0.0, np.inf), (-np.inf, -0.0), (0.75, 0.25)][variant]
    c = Case("range %d" % variant, scans, words, Rule(12, F32, lo=lo, hi=hi))
    for w, k in zip(words, c.keep):
        assert not k[np.isnan(w)].any() and np.isnan(w).sum() > 100, "a NaN word is dropped"
        neg0 = (w == 0) & np.signbit(w)
        if variant == 2:
            assert k[~np.isnan(w)].all()
        if variant == 3:
            assert neg0.sum() > 50 and k[neg0].all() and not k[w < 0].any(), "-0.0 passes lo = 0"
        if variant == 4:
            assert k[(w == 0) & ~np.signbit(w)].all() and not k[w > 0].any(), "+0.0 passes hi = -0.0"
        if variant == 1:
            assert 50 < k.sum() == (w == np.float32(0.25)).sum()
        if variant == 5:
            assert not k.any()   # an empty band: everything is dropped
    return c


N_RANGES = 6


def case_everything(kind, n_scans=4, seed=500):
    """5 / 6: everything kept; everything dropped; all but 5 records dropped"""
    scans = [terrain_scan(seed + i, n=n, scale=1.3) for i, n in enumerate(_sizes(n_scans))]
    words = [np.random.default_rng(seed + i).integers(0, 200, len(s)).astype(np.uint32) for i, s in enumerate(scans)]
    if kind == "kept":
        return Case("everything kept", scans, words, drop_classes(12, U32, dropped=range(200, 260)))
    if kind == "dropped":
        return Case("everything dropped", scans, words, Rule(12, U32, kept=np.zeros(200, bool), keep_other=0))
    for s, w in zip(scans, words):   # five records of class 201, far apart, inside the map
        at = np.linspace(100, len(s) - 100, 5).astype(int)
        w[at] = 201
        s[at, 0], s[at, 1] = 20.0 + np.arange(5), -10.0 + 3 * np.arange(5)
    return Case("all but five dropped", scans, words, Rule(12, U32, kept=np.arange(202) == 201, keep_other=0))


def case_with_tf(n_scans=4, seed=540):
    """10: with h_tf -- the filter looks at the record, the matrix moves the kept points"""
    c = case_dropped_maxima(n_scans, seed)
    return Case("with h_tf", c.scans, c.words, c.rule, layout=(32, 0), tfs=random_tfs(n_scans, seed=seed, max_tilt_deg=2.0, max_shift=3.0))


# ---- the edges, asserted on the oracle's side: the oracle on all records against the oracle on the kept ones ----
def oracle_pair(oracle, cfg, case, i=0):
    a, k = oracle.Scan(case.all_scans()[i], cfg), oracle.Scan(case.kept_scans()[i], cfg)
    (ab, ap), (kb, kp) = a.bev(), k.bev()
    return a.desc()[0], k.desc()[0], ab, ap, kb, kp


def assert_edge(oracle, cfg, case):
    da, dk, ab, ap, kb, kp = oracle_pair(oracle, cfg, case)
    occupied = kb > -999.0
    if case.name in ("dropped maxima", "with h_tf", "kitti labels"):
        lower = occupied & (kb < ab)
        assert lower.sum() >= 20 and (ap[lower] != kp[lower]).any(axis=1).sum() >= 20, "cells whose maximum is dropped change height and position"
        assert ((ab > -999.0) & ~occupied).sum() >= 1, "cells that only dropped records reach become empty"
    if case.name == "first of equals":
        same_height = occupied & (kb == ab)
        assert (same_height & (ap != kp).any(axis=1)).sum() >= 5, "cells whose first record at the maximum is dropped keep the height, not the position"
    if case.name == "extremes":
        assert da["max_bin_val"] > dk["max_bin_val"] and da["min_bin_val"] < dk["min_bin_val"]
    if case.name == "boundaries":
        assert da["max_bin_val"] >= 30.0 + 2.0 and dk["max_bin_val"] < 20.0
        assert (ab >= 30.0).sum() >= 20 and not (kb >= 30.0).any()


# ---- the CPU harness' driver ----
class FilterApi(PointsApi):
    """point_layouts.PointsApi plus the calls that take a filter."""

    def _dbg(self, n, debug):
        if not debug:
            return None, None
        L, ncell = self.L, self._cfg.n_row * self._cfg.n_col
        dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32), "labels": np.zeros((n, L.NLEV, ncell), np.int16)}
        st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
        return dbg, C.cast(st, C.c_void_p)

    def ingest_filtered_rc(self, ctx, buf, layout, flt, offsets, tf=None, debug=False):
        """cc_ingest_points_filtered: (rc, descriptors, debug outputs or None).  flt: a Filter or None (a NULL filter)"""
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        dbg, dbg_p = self._dbg(n, debug)
        tfa = self._tf(tf)
        rc = self.lib.cc_ingest_points_filtered(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.byref(flt) if flt is not None else None,
                                                C.c_void_p(offsets.ctypes.data), n, C.c_void_p(tfa.ctypes.data) if tfa is not None else None,
                                                C.c_void_p(desc.ctypes.data), dbg_p, None)
        return rc, desc, dbg

    def ingest_filtered_host_rc(self, ctx, buf, layout, flt, offsets, tf=None, want_bev=False):
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        tfa = self._tf(tf)
        rc = self.lib.cc_ingest_points_filtered_host(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.byref(flt) if flt is not None else None,
                                                     C.c_void_p(offsets.ctypes.data), n, C.c_void_p(tfa.ctypes.data) if tfa is not None else None,
                                                     C.c_void_p(desc.ctypes.data), C.c_void_p(bev.ctypes.data) if want_bev else None)
        return rc, desc, bev

    def scan_ingest_filtered_rc(self, ctx, buf, layout, flt, n_points, tf=None):
        """cc_scan_ingest_points_filtered on the caller's own buffer -> (rc, the scan's descriptor or None)"""
        sc = C.c_void_p()
        tfa = self._tf(tf)
        rc = self.lib.cc_scan_ingest_points_filtered(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.byref(flt) if flt is not None else None,
                                                     C.c_int64(n_points), C.c_void_p(tfa.ctypes.data) if tfa is not None else None, 0, C.byref(sc))
        return rc, (self._take(sc)[0] if rc == 0 else None)


class EmuDriver:
    """how the shared check below reaches the library on the CPU harness (numpy in, numpy out)"""
    float_exact = True

    def __init__(self, L):
        self.api = FilterApi(L)

    def context(self, cfg, n):
        return self.api.create(cfg, max_batch=n)

    def close(self, ctx):
        self.api.lib.cc_destroy(ctx)

    def filtered(self, ctx, case, buf):
        f, _bits = case.rule.c()
        rc, d, dbg = self.api.ingest_filtered_rc(ctx, buf, case.layout, f, case.offs(), case.tfs, debug=True)
        self.api.chk(rc, "cc_ingest_points_filtered")
        rc, plain, _ = self.api.ingest_filtered_rc(ctx, buf, case.layout, f, case.offs(), case.tfs)
        assert rc == 0 and plain.tobytes() == d.tobytes(), "with / without debug outputs"
        return d, dbg

    def points(self, ctx, case, buf):
        return self.api.ingest_points(ctx, buf, case.layout, case.offs(), tf=case.tfs, debug=True)


def check_case(drv, oracle, cfg, case, ctx=None):
    """The filtered call on `case`: (a) bev, pix_rc, label images and descriptor of every scan against the oracle on the kept records
    alone (scans that keep more than 10); (b) the bytes of cc_ingest_points on the records whose dropped x are NaN.  Returns the
    descriptors and debug outputs."""
    own = ctx is None
    if own:
        ctx = drv.context(cfg, len(case.scans))
    d, dbg = drv.filtered(ctx, case, case.buffer())
    r, rdbg = drv.points(ctx, case, case.buffer([nan_x(s, k) for s, k in zip(case.scans, case.keep)]))
    if own:
        drv.close(ctx)
    report = []
    if d.tobytes() != r.tobytes():
        report.append("%s: the descriptors differ from cc_ingest_points' on the NaN-substituted records" % case.name)
    for k in ("bev", "pix_rc", "labels"):
        if np.asarray(dbg[k]).tobytes() != np.asarray(rdbg[k]).tobytes():
            report.append("%s: %s differs from cc_ingest_points' on the NaN-substituted records" % (case.name, k))
    seen = {}
    for i, s in enumerate(case.kept_scans()):
        if len(s) <= 10:
            continue
        key = (id(case.scans[i]), id(case.words[i]))   # (a repeated scan: the oracle once)
        if key not in seen:
            o = oracle.Scan(s, cfg)
            seen[key] = (o.bev(), o.labels(), o.desc()[0])
        (ob, opix), olab, od = seen[key]
        if not np.array_equal(ob, dbg["bev"][i]):
            report.append("%s scan %d: bev differs from the oracle on the kept records" % (case.name, i))
        if not np.array_equal(opix, dbg["pix_rc"][i]):
            report.append("%s scan %d: pix_rc differs" % (case.name, i))
        if not np.array_equal(olab, dbg["labels"][i]):
            report.append("%s scan %d: label images differ" % (case.name, i))
        report += ["%s scan %d: %s" % (case.name, i, m) for m in compare_desc(od, d[i], float_exact=drv.float_exact)]
    assert not report, "\n".join(report[:30])
    return d, dbg
