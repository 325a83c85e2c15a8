"""TEST INFRASTRUCTURE for the point-layout / per-scan-transform entry points (cc_ingest_points and its siblings,
include/cont2_amd.h): numpy restatements of what the library is specified to do, and a driver of the new calls on the CPU
harness (emu_api.EmuApi drives the old ones)."""
import ctypes as C

import numpy as np

import emu_api

NAN_FILL = np.uint32(0x7FC00BAD)   # a quiet-NaN bit pattern: what the bytes of a record that are not x, y, z hold in these tests


def repack(xyzi, stride, off, base_shift=0):
    """The coordinates of [n, 4] f32 KITTI records as n records of `stride` bytes with x, y, z at byte `off`; every other
    byte holds NaN bit patterns.  Returns a uint8 array whose data pointer is 16-byte aligned + base_shift (a multiple of 4)."""
    xyzi = np.ascontiguousarray(xyzi, np.float32)
    n = len(xyzi)
    words = np.full(n * (stride // 4) + 8, NAN_FILL, np.uint32)
    shift = ((-words.ctypes.data) % 16 + base_shift) // 4
    rec = words[shift:shift + n * (stride // 4)].reshape(n, stride // 4)
    rec[:, off // 4:off // 4 + 3] = xyzi[:, :3].view(np.uint32)
    out = rec.reshape(-1).view(np.uint8)
    assert out.ctypes.data % 16 == base_shift % 16
    return out


def apply_tf(xyzi, m):
    """x' = ((m00 x + m01 y) + m02 z) + m03 and rows 1, 2 likewise, in f32, every product and sum rounded once -- the library's
    stated operation order (np.float32 products and sums, no `@`).  xyzi [n, 4] f32, m 12 values; returns [n, 4] f32 (w = 0)."""
    m = np.asarray(m, np.float32).reshape(12)
    x, y, z = (np.ascontiguousarray(xyzi[:, i], np.float32) for i in range(3))
    out = np.zeros((len(xyzi), 4), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3]
    assert out.dtype == np.float32
    return out


def rigid(yaw, roll=0.0, pitch=0.0, t=(0.0, 0.0, 0.0), dtype=np.float64):
    """Row-major 3 x 4 [R | t], R = Rz(yaw) Ry(pitch) Rx(roll), angles in radians."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return np.concatenate([R, np.asarray(t, np.float64).reshape(3, 1)], 1).astype(dtype)


def inverse(m):
    """[R | t]^-1 = [R^T | -R^T t] in f64 (3 x 4)."""
    m = np.asarray(m, np.float64).reshape(3, 4)
    Rt = m[:, :3].T
    return np.concatenate([Rt, -(Rt @ m[:, 3:])], 1)


def random_tfs(n, seed, max_tilt_deg=4.0, max_shift=3.0):
    """n different transforms: any yaw, a few degrees of roll and pitch, a translation.  [n, 12] f32."""
    rng = np.random.default_rng(seed)
    tilt = np.deg2rad(max_tilt_deg)
    return np.stack([rigid(rng.uniform(-np.pi, np.pi), rng.uniform(-tilt, tilt), rng.uniform(-tilt, tilt),
                           (rng.uniform(-max_shift, max_shift), rng.uniform(-max_shift, max_shift), rng.uniform(-0.5, 0.5)), np.float32).reshape(12)
                     for _ in range(n)])


def border_scan(seed, n=4000):
    """Points around the +-75 m border of the map and around the 4 m blind disc: a shift of a few metres moves some in and some out."""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 4), np.float32)
    k = n // 2
    s[:k, 0] = np.where(rng.random(k) < 0.5, 1, -1) * rng.uniform(70.0, 80.0, k)
    s[:k, 1] = rng.uniform(-80.0, 80.0, k)
    ang, r = rng.uniform(0, 2 * np.pi, n - k), rng.uniform(0.5, 9.0, n - k)
    s[k:, 0], s[k:, 1] = r * np.cos(ang), r * np.sin(ang)
    s[:, 2] = rng.uniform(-1.5, 2.5, n)
    return s


class Layout(C.Structure):
    _fields_ = [("stride_bytes", C.c_int32), ("xyz_offset", C.c_int32)]


class PointsApi(emu_api.EmuApi):
    """emu_api.EmuApi plus the calls that take a point layout and a per-scan transform."""

    @staticmethod
    def _lay(layout):
        return None if layout is None else C.byref(Layout(int(layout[0]), int(layout[1])))

    @staticmethod
    def _tf(tf):
        return None if tf is None else np.ascontiguousarray(np.asarray(tf, np.float32).reshape(-1, 12))

    def ingest_points_rc(self, ctx, buf, layout, offsets, tf=None, debug=False):
        """cc_ingest_points: (rc, descriptors, debug outputs or None)"""
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
        tfa = self._tf(tf)
        ptr = buf if isinstance(buf, int) else buf.ctypes.data
        rc = self.lib.cc_ingest_points(ctx, C.c_void_p(ptr), self._lay(layout), C.c_void_p(offsets.ctypes.data), n,
                                       C.c_void_p(tfa.ctypes.data) if tfa is not None else None, C.c_void_p(desc.ctypes.data), dbg_p, None)
        return rc, desc, dbg

    def ingest_points(self, ctx, buf, layout, offsets, tf=None, debug=False):
        rc, desc, dbg = self.ingest_points_rc(ctx, buf, layout, offsets, tf, debug)
        self.chk(rc, "cc_ingest_points")
        return (desc, dbg) if debug else desc

    def ingest_points_host(self, ctx, buf, layout, offsets, tf=None, want_bev=False):
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        tfa = self._tf(tf)
        self.chk(self.lib.cc_ingest_points_host(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.c_void_p(offsets.ctypes.data), n,
                                                C.c_void_p(tfa.ctypes.data) if tfa is not None else None, C.c_void_p(desc.ctypes.data),
                                                C.c_void_p(bev.ctypes.data) if want_bev else None), "cc_ingest_points_host")
        return (desc, bev) if want_bev else desc

    def _take(self, sc):
        p = C.c_void_p()
        self.chk(self.lib.cc_scan_desc(sc, C.byref(p)), "cc_scan_desc")
        d = np.frombuffer(C.string_at(p, self.L.scan_desc_dt.itemsize), self.L.scan_desc_dt).copy()
        self.chk(self.lib.cc_scan_release(sc), "cc_scan_release")
        return d

    def scan_ingest_points(self, ctx, buf, layout, n_points, tf=None):
        """cc_scan_ingest_points on the caller's own buffer -> the scan's descriptor"""
        sc = C.c_void_p()
        tfa = self._tf(tf)
        self.chk(self.lib.cc_scan_ingest_points(ctx, C.c_void_p(buf.ctypes.data), self._lay(layout), C.c_int64(n_points),
                                                C.c_void_p(tfa.ctypes.data) if tfa is not None else None, 0, C.byref(sc)), "cc_scan_ingest_points")
        return self._take(sc)[0]

    def scan_ingest_points_batch(self, ctx, bufs, layout, tf=None):
        """The records of every scan written to a staging slot as they are (bytes), one cc_scan_ingest_points_batch -> descriptors"""
        stride = 16 if layout is None else int(layout[0])
        n = len(bufs)
        ptrs = (C.c_void_p * n)()
        cnt = (C.c_int64 * n)()
        cap = max((len(b) + 15) // 16 for b in bufs)
        for i, b in enumerate(bufs):
            p = self.lib.cc_stage_points_slot(ctx, cap, i)
            assert p, self.lib.cc_last_error()
            C.memmove(p, b.ctypes.data, len(b))
            ptrs[i] = p
            cnt[i] = len(b) // stride
        out = (C.c_void_p * n)()
        tfa = self._tf(tf)
        self.chk(self.lib.cc_scan_ingest_points_batch(ctx, ptrs, self._lay(layout), cnt, n, C.c_void_p(tfa.ctypes.data) if tfa is not None else None, out),
                 "cc_scan_ingest_points_batch")
        return np.concatenate([self._take(C.c_void_p(out[i])) for i in range(n)])
