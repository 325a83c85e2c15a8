"""TEST INFRASTRUCTURE for the per-point-time entry points (cc_ingest_points_motion and its siblings, include/cont2_amd.h): the numpy
restatement of what the library is specified to do with a time word and a scan's knot matrices, a builder of records that carry a
time word, and a driver of the calls on the CPU harness."""
import ctypes as C

import numpy as np

from point_layouts import NAN_FILL, PointsApi, apply_tf, rigid

KNOTS_MAX = 64
TIME_F32, TIME_U32 = 0, 1


class Motion(C.Structure):
    """cc_point_motion_t"""
    _fields_ = [("time_offset", C.c_int32), ("time_type", C.c_int32), ("n_knots", C.c_int32), ("pad_", C.c_int32)]


def time_bins(w, time_type, t_begin, scale, n_knots):
    """The bin of every time word w (uint32 [n]: the 4 bytes as they lie in the record), in np.float32 operations only:
       F32: u = (t - t_begin) * scale;  U32: u = (float)(uint32)(w - tb) * scale, tb = the bits of t_begin, modulo 2^32
       b = trunc(min(max(u, 0), K - 1)), NaN counts as 0 (clamped before the conversion)."""
    w = np.ascontiguousarray(w, np.uint32)
    scale = np.float32(scale)
    with np.errstate(all="ignore"):
        if time_type == TIME_F32:
            u = (w.view(np.float32) - np.float32(t_begin)) * scale
        else:
            tb = np.asarray(t_begin, np.float32).reshape(1).view(np.uint32)[0]   # t_begin: the f32 whose bits are the u32 (u32_bits_as_f32)
            u = (w - tb).astype(np.float32) * scale     # uint32 arithmetic wraps; the conversion rounds to nearest even
        assert u.dtype == np.float32
        u = np.where(u > np.float32(0), u, np.float32(0))                     # (a NaN fails the compare: 0)
        u = np.where(u < np.float32(n_knots - 1), u, np.float32(n_knots - 1))
    return u.astype(np.int64)


def apply_motion(xyz, w, time_type, t_begin, scale, knots):
    """The points the library is specified to see: every point moved by the knot of its bin, with apply_tf's operations.
    xyz [n, >= 3] f32, w uint32 [n], knots [K, 12] f32; returns [n, 4] f32 (w = 0) in the original order."""
    knots = np.asarray(knots, np.float32).reshape(-1, 12)
    b = time_bins(w, time_type, t_begin, scale, len(knots))
    out = np.zeros((len(xyz), 4), np.float32)
    for k in np.unique(b):
        m = b == k
        out[m] = apply_tf(np.asarray(xyz, np.float32)[m], knots[k])
    return out


def u32_bits_as_f32(v):
    """the f32 whose bits are the u32 v: what goes into the t_begin slot of a CC_TIME_U32 call"""
    return np.array([v], np.uint32).view(np.float32)[0]


def repack_with_time(xyzi, w, stride, off, time_off, base_shift=0):
    """point_layouts.repack with the time word w (uint32 [n]) at byte `time_off` of every record."""
    xyzi = np.ascontiguousarray(xyzi, np.float32)
    n = len(xyzi)
    words = np.full(n * (stride // 4) + 8, NAN_FILL, np.uint32)
    shift = ((-words.ctypes.data) % 16 + base_shift) // 4
    rec = words[shift:shift + n * (stride // 4)].reshape(n, stride // 4)
    rec[:, off // 4:off // 4 + 3] = xyzi[:, :3].view(np.uint32)
    rec[:, time_off // 4] = np.ascontiguousarray(w, np.uint32)
    out = rec.reshape(-1).view(np.uint8)
    assert out.ctypes.data % 16 == base_shift % 16
    return out


def random_knots(n_scans, n_knots, seed, max_shift=4.0):
    """[n_scans, K, 12] f32: rigid motions that differ by metres from knot to knot, so that a wrong bin is visible."""
    rng = np.random.default_rng(seed)
    tilt = np.deg2rad(3.0)
    return np.stack([np.stack([rigid(rng.uniform(-np.pi, np.pi), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt),
                                     (rng.uniform(-max_shift, max_shift), rng.uniform(-max_shift, max_shift), rng.uniform(-0.5, 0.5)),
                                     np.float32).reshape(12) for _ in range(n_knots)]) for _ in range(n_scans)])


class MotionApi(PointsApi):
    """point_layouts.PointsApi plus the calls that take a time word and knots."""

    @staticmethod
    def _args(motion, t_begin, scale, knots, n):
        mo = None if motion is None else Motion(int(motion[0]), int(motion[1]), int(motion[2]), 0)
        tm = None if t_begin is None else np.ascontiguousarray(np.stack([np.asarray(t_begin, np.float32).reshape(n),
                                                                         np.asarray(scale, np.float32).reshape(n)], 1))
        kn = None if knots is None else np.ascontiguousarray(np.asarray(knots, np.float32).reshape(n, -1))
        return mo, tm, kn

    def ingest_motion_rc(self, ctx, buf, layout, motion, offsets, t_begin, scale, knots, debug=False):
        """cc_ingest_points_motion: (rc, descriptors, debug outputs or None).  motion: (time_offset, time_type, n_knots) or None;
        t_begin / scale: [n] (None: a NULL h_time); knots [n, K, 12] (None: NULL)."""
        L = self.L
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, L.scan_desc_dt)
        ncell = self._cfg.n_row * self._cfg.n_col
        dbg, dbg_p = None, None
        if debug:
            dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32),
                   "labels": np.zeros((n, L.NLEV, ncell), np.int16)}
            st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
            dbg_p = C.cast(st, C.c_void_p)
        mo, tm, kn = self._args(motion, t_begin, scale, knots, n)
        ptr = buf if isinstance(buf, int) else buf.ctypes.data
        rc = self.lib.cc_ingest_points_motion(ctx, C.c_void_p(ptr), self._lay(layout), C.byref(mo) if mo is not None else None,
                                              C.c_void_p(offsets.ctypes.data), n, C.c_void_p(tm.ctypes.data) if tm is not None else None,
                                              C.c_void_p(kn.ctypes.data) if kn is not None else None, C.c_void_p(desc.ctypes.data), dbg_p, None)
        return rc, desc, dbg

    def ingest_motion(self, ctx, buf, layout, motion, offsets, t_begin, scale, knots, debug=False):
        rc, desc, dbg = self.ingest_motion_rc(ctx, buf, layout, motion, offsets, t_begin, scale, knots, debug)
        self.chk(rc, "cc_ingest_points_motion")
        return (desc, dbg) if debug else desc

    def ingest_motion_host_rc(self, ctx, buf, layout, motion, offsets, t_begin, scale, knots, want_bev=False):
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        mo, tm, kn = self._args(motion, t_begin, scale, knots, n)
        rc = self.lib.cc_ingest_points_motion_host(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.byref(mo) if mo is not None else None,
                                                   C.c_void_p(offsets.ctypes.data), n, C.c_void_p(tm.ctypes.data) if tm is not None else None,
                                                   C.c_void_p(kn.ctypes.data) if kn is not None else None, C.c_void_p(desc.ctypes.data),
                                                   C.c_void_p(bev.ctypes.data) if want_bev else None)
        return rc, desc, bev

    def scan_ingest_motion_rc(self, ctx, buf, layout, motion, n_points, t_begin, scale, knots):
        """cc_scan_ingest_points_motion on the caller's own buffer -> (rc, the scan's descriptor or None)"""
        sc = C.c_void_p()
        mo, tm, kn = self._args(motion, None if t_begin is None else [t_begin], None if scale is None else [scale],
                                None if knots is None else np.asarray(knots, np.float32).reshape(1, -1), 1)
        rc = self.lib.cc_scan_ingest_points_motion(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.byref(mo) if mo is not None else None,
                                                   C.c_int64(n_points), C.c_void_p(tm.ctypes.data) if tm is not None else None,
                                                   C.c_void_p(kn.ctypes.data) if kn is not None else None, 0, C.byref(sc))
        return rc, (self._take(sc)[0] if rc == 0 else None)

    def motion_knots(self, pose_begin, pose_end, ref=1.0, K=32):
        pb = np.ascontiguousarray(np.asarray(pose_begin, np.float64).reshape(12))
        pe = np.ascontiguousarray(np.asarray(pose_end, np.float64).reshape(12))
        out = np.zeros((K, 12), np.float32)
        self.lib.cc_motion_knots(C.c_void_p(pb.ctypes.data), C.c_void_p(pe.ctypes.data), C.c_double(ref), C.c_int(K), C.c_void_p(out.ctypes.data))
        return out


SWEEP = np.float32(0.1)   # the tests' sweeps last 0.1 time units


def bin_edge_inputs(n=9001, K=16):
    """f32 time words for n points: exactly on every bin boundary and 1 ulp either side, below t_begin, far above the end, +-inf,
    NaN, repeated to n.  Returns (words uint32 [n], t_begin, scale); asserts that bins 0 and K - 1 are reached by clamping and by NaN."""
    tb, scale = np.float32(0.25), np.float32(K) / SWEEP
    edges = (tb + np.arange(K + 1, dtype=np.float32) / scale).astype(np.float32)
    special = np.concatenate([edges, np.nextafter(edges, np.float32(np.inf)), np.nextafter(edges, np.float32(-np.inf)),
                              np.array([tb - 1.0, -1e30, tb + 100.0, 1e30, np.inf, -np.inf, np.nan, -np.nan, tb], np.float32)]).astype(np.float32)
    t = np.resize(special, n).astype(np.float32)
    w = t.view(np.uint32)
    b = time_bins(w, TIME_F32, tb, scale, K)
    with np.errstate(all="ignore"):
        u = (t - tb) * scale
        assert ((u < 0) & (b == 0)).sum() > 50 and ((u > K) & (b == K - 1)).sum() > 50 and (np.isnan(t) & (b == 0)).sum() > 50
        assert (np.isposinf(t) & (b == K - 1)).sum() > 20 and (np.isneginf(t) & (b == 0)).sum() > 20
    assert set(np.unique(b)) == set(range(K))
    assert np.all(time_bins(w, TIME_F32, tb, 0.0, K) == 0)   # scale 0: u is 0, or NaN (inf * 0) for an infinite time: bin 0 either way
    return w, tb, scale


def tie_inputs(n_scans=6, n0=6001):
    """Scans whose points fall into a few cells, hundreds each, with a random bin per point; the knots shift z by a binary fraction
    (exact in f32) and the raw heights are lowered by their bin's shift, so the MOVED heights lie on one 6-value lattice whatever the
    bin: equal maxima in one cell come from points of different bins.  Returns (scans, words, t_begin [n], scale [n], knots [n, K, 12])."""
    K = 4
    lifts = np.float32([0.0, 0.5, 1.0, 1.5])
    knots1 = np.stack([rigid(0.0, t=(0.0, 0.0, float(z)), dtype=np.float32).reshape(12) for z in lifts])
    scans, words = [], []
    for i in range(n_scans):
        rng = np.random.default_rng(50 + i)
        n = n0 + 8 * i
        s = np.zeros((n, 4), np.float32)
        s[:, 0], s[:, 1] = rng.uniform(10.0, 16.0, n), rng.uniform(-3.0, 3.0, n)
        b = rng.integers(0, K, n)
        s[:, 2] = rng.integers(0, 6, n) * 0.5 - 1.0 - lifts[b]
        scans.append(s)
        words.append(((b + np.float32(0.5)) / np.float32(K)).astype(np.float32).view(np.uint32))   # t_begin 0, scale K: u = b + 0.5
    return scans, words, np.zeros(n_scans, np.float32), np.full(n_scans, K, np.float32), np.tile(knots1, (n_scans, 1, 1))


def cells(cfg, q):
    """cell index (or -1) of every point of q, as cc_point_cell computes it at a power-of-two resolution"""
    x, y = q[:, 0], q[:, 1]
    hr, hc = cfg.n_row // 2, cfg.n_col // 2
    ok = (np.abs(x) <= hr * cfg.reso_row) & (np.abs(y) <= hc * cfg.reso_col) & ~(x * x + y * y < cfg.blind_sq)
    row = np.floor(x / cfg.reso_row).astype(np.int64) + hr
    col = np.floor(y / cfg.reso_col).astype(np.int64) + hc
    return np.where(ok & (row > 0), row * cfg.n_col + col, -1)


def assert_ties_across_bins(cfg, moved, words, t_begin, scale, n_knots, at_least=10):
    """at least `at_least` cells of every scan have their maximum reached by points of several bins"""
    for i, (m, w) in enumerate(zip(moved, words)):
        c, b = cells(cfg, m), time_bins(w, TIME_F32, t_begin[i], scale[i], n_knots)
        tied = 0
        for cell in np.unique(c[c >= 0]):
            top = (c == cell) & (m[:, 2] == m[c == cell, 2].max())
            tied += len(np.unique(b[top])) > 1
        assert tied >= at_least, (i, tied)
