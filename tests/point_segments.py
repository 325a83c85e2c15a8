"""TEST INFRASTRUCTURE for the segment entry points (cc_ingest_segments and its siblings, include/cont2_amd.h): the ctypes mirror of
cc_point_segment_t, a builder that lays a scan's segments out in memory and restates in numpy the cloud Q the library is
specified to see, and a driver of the calls on the CPU harness."""
import ctypes as C

import numpy as np

from point_layouts import Layout, PointsApi, apply_tf, repack

SEG_MAX = 32


class Segment(C.Structure):
    """cc_point_segment_t"""
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_int64), ("layout", Layout), ("has_tf", C.c_int32), ("pad_", C.c_int32),
                ("tf", C.c_float * 12)]


def moved(xyzi, tf):
    """What the library sees of a segment: T(points) for a segment with a matrix, the coordinates' bits otherwise.  [n, 4] f32, w = 0."""
    if tf is not None:
        return apply_tf(xyzi, tf)
    out = np.zeros((len(xyzi), 4), np.float32)
    out[:, :3] = np.asarray(xyzi, np.float32)[:, :3]
    return out


def cloud_q(scan):
    """Q = T_0(segment 0) ++ T_1(segment 1) ++ ... for a scan given as [(xyzi, layout, tf, base_shift), ...]"""
    return np.concatenate([moved(x, tf) for (x, _lay, tf, _sh) in scan], 0)


class Segments:
    """The segments of a call in memory: every segment's records in an allocation of its own (`bufs` keeps them alive), the array of
    cc_point_segment_t, the scans' first-segment indices, and the numpy cloud Q of every scan.
    scans: a list of scans, each a list of (xyzi [n, 4] f32, (stride, xyz_offset) or None, 12 values or None, base_shift); a segment of
    no points gets a NULL pointer."""

    def __init__(self, scans):
        n = sum(len(s) for s in scans)
        self.arr = (Segment * max(n, 1))()
        self.bufs = []
        self.scan_segs = np.zeros(len(scans) + 1, np.int32)
        self.q = [cloud_q(s) for s in scans]
        k = 0
        for i, scan in enumerate(scans):
            for (xyzi, lay, tf, shift) in scan:
                g = self.arr[k]
                stride, off = (16, 0) if lay is None else lay
                if len(xyzi):
                    buf = repack(xyzi, stride, off, base_shift=shift)
                    self.bufs.append(buf)
                    g.points = buf.ctypes.data
                g.n_points = len(xyzi)
                if lay is not None:
                    g.layout = Layout(stride, off)
                if tf is not None:
                    g.has_tf = 1
                    g.tf[:] = [float(v) for v in np.asarray(tf, np.float32).reshape(12)]
                k += 1
            self.scan_segs[i + 1] = k
        self.n_scans = len(scans)


class SegmentsApi(PointsApi):
    """point_layouts.PointsApi plus the calls that take a scan as a list of segments."""

    def _dbg(self, n):
        ncell = self._cfg.n_row * self._cfg.n_col
        dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32),
               "labels": np.zeros((n, self.L.NLEV, ncell), np.int16)}
        st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
        return dbg, st

    def ingest_segments_rc(self, ctx, arr, scan_segs, debug=False):
        """cc_ingest_segments on a raw array of cc_point_segment_t: (rc, descriptors, debug outputs or None)"""
        scan_segs = np.ascontiguousarray(scan_segs, np.int32)
        n = len(scan_segs) - 1
        desc = np.zeros(n, self.L.scan_desc_dt)
        dbg, st = self._dbg(n) if debug else (None, None)
        rc = self.lib.cc_ingest_segments(ctx, arr, C.c_void_p(scan_segs.ctypes.data), n, C.c_void_p(desc.ctypes.data),
                                         C.cast(st, C.c_void_p) if debug else None, None)
        return rc, desc, dbg

    def ingest_segments(self, ctx, segs, debug=False):
        rc, desc, dbg = self.ingest_segments_rc(ctx, segs.arr, segs.scan_segs, debug)
        self.chk(rc, "cc_ingest_segments")
        return (desc, dbg) if debug else desc

    def ingest_segments_host(self, ctx, segs, want_bev=False):
        n = segs.n_scans
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        self.chk(self.lib.cc_ingest_segments_host(ctx, segs.arr, C.c_void_p(segs.scan_segs.ctypes.data), n, C.c_void_p(desc.ctypes.data),
                                                  C.c_void_p(bev.ctypes.data) if want_bev else None), "cc_ingest_segments_host")
        return (desc, bev) if want_bev else desc

    def scan_ingest_segments(self, ctx, segs, scan, want_bev=False):
        """cc_scan_ingest_segments for scan `scan` of `segs` -> its descriptor (and its max-height image)"""
        s0, s1 = int(segs.scan_segs[scan]), int(segs.scan_segs[scan + 1])
        sc = C.c_void_p()
        self.chk(self.lib.cc_scan_ingest_segments(ctx, C.byref(segs.arr, s0 * C.sizeof(Segment)), s1 - s0, 1 if want_bev else 0, C.byref(sc)),
                 "cc_scan_ingest_segments")
        bev = None
        if want_bev:
            p = C.c_void_p()
            self.chk(self.lib.cc_scan_bev(sc, C.byref(p)), "cc_scan_bev")
            ncell = self._cfg.n_row * self._cfg.n_col
            bev = np.frombuffer(C.string_at(p, 4 * ncell), np.float32).copy()
        d = self._take(sc)[0]
        return (d, bev) if want_bev else d
