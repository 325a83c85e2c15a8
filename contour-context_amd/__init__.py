"""contour-context_amd: MI355X-native hot path of lewisjiang/contour-context (cont2contops).

Python host glue over the C-ABI shared library `libcont2_amd.so` (include/cont2_amd.h).  PyTorch is
used only for device memory, streams and torch.distributed plumbing; all compute is in the HIP
kernels under csrc/.  There is no CPU fallback: creating a Context without a HIP device fails.

The directory name carries a hyphen (it mirrors the reference's name), so it is loaded by path:
    import importlib.util; spec = importlib.util.spec_from_file_location("contour_context_amd", ".../__init__.py")
`load()` in the repo-root helper `cc_amd.py` does exactly that.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, _HERE)
import abi  # noqa: E402
import calls  # noqa: E402
import layouts as L  # noqa: E402
import synth  # noqa: E402,F401
import sharding  # noqa: E402,F401

LIB_PATH = os.path.join(_HERE, "libcont2_amd.so")
_SRCS = ["cont2_amd.hip", "cc_dev.h", "cc_group.h", "cc_hostcfg.h", "cc_sort.h", "cc_stats.h", "cc_fmath.h", "k_rasterize.h", "k_image.h", "k_contours.h", "k_contours_list.h",
         "k_knn.h", "k_knn_list.h", "k_mask.h", "k_check.h", "k_merge.h", "k_gmm.h", "k_gmm_hess.h", "k_match.h", "k_verify.h", "k_pose.h", "k_prep_packed.h", "cc_hostdb.h", "cc_db_api.inc", "cc_comm.inc"]

# how every gfx950 code object of this project that includes csrc/ headers is compiled: the library below and the device
# probe library of the test suite (tests/dev_probe.py), so that what the probes measure is the code the library runs
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value"]


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", s) for s in _SRCS] + [os.path.join(_HERE, "..", "include", h) for h in ["cont2_amd.h"] + list(abi.EXTENSIONS) + list(abi.ADDONS)]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(s) <= os.path.getmtime(LIB_PATH) for s in srcs):
        return LIB_PATH
    cmd = ["hipcc"] + HIPCC_FLAGS + [os.path.join(_HERE, "csrc", "cont2_amd.hip"), "-ldl", "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None

EXPORTS = list(abi.SIGNATURES)  # every symbol include/cont2_amd.h declares
EXPORTS_EXT = [s for table in abi.EXTENSIONS.values() for s in table]  # ... and every symbol of the extension headers beside it
EXPORTS_ADDON = [s for table in abi.ADDONS.values() for s in table]  # ... and of the add-on headers (abi.ADDONS: open-ended)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libcont2_amd.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        _lib = abi.bind(C.CDLL(os.environ.get("CC_AMD_LIB") or LIB_PATH))  # CC_AMD_LIB: tuning aid (another build of the same library)
    return _lib


CCError, CC_ECAPACITY = calls.CCError, calls.CC_ECAPACITY


def _chk(rc, what, tolerate=()):
    return calls.chk(lib(), rc, what, tolerate)


def _ret(*parts):
    """the parts a call has, as a tuple; a lone part as itself"""
    out = tuple(p for p in parts if p is not None)
    return out if len(out) > 1 else out[0]


class IngestDebug(C.Structure):
    _fields_ = [("d_bev", C.c_void_p), ("d_pix_rc", C.c_void_p), ("d_labels", C.c_void_p)]


DESC_BYTES = L.scan_desc_dt.itemsize

POINT_LAYOUTS = {"xyzi": (16, 0), "xyz": (12, 0)}   # names Context.ingest takes for cc_point_layout_t {stride_bytes, xyz_offset}


def _point_layout(layout):
    """None, "xyz" / "xyzi" or a (stride_bytes, xyz_offset) pair -> L.PointLayout or None (the library checks the values)."""
    if layout is None:
        return None
    if isinstance(layout, str):
        if layout not in POINT_LAYOUTS:
            raise ValueError("unknown point layout %r (known: %s, or a (stride_bytes, xyz_offset) pair)" % (layout, sorted(POINT_LAYOUTS)))
        layout = POINT_LAYOUTS[layout]
    return L.PointLayout(int(layout[0]), int(layout[1]))


def _scan_tf(tf, n):
    """[n, 3, 4] or [n, 12] -> contiguous f32 [n, 12] (host), or None"""
    if tf is None:
        return None
    tf = np.ascontiguousarray(np.asarray(tf, np.float32).reshape(len(tf), -1))
    if tf.shape != (n, 12):
        raise ValueError("tf must hold a 3 x 4 matrix per scan: [%d, 3, 4] or [%d, 12], got %s" % (n, n, tf.shape))
    return tf


TIME_TYPES = {"f32": L.TIME_F32, "u32": L.TIME_U32}   # names Context.ingest takes for cc_point_motion_t.time_type


def _scan_motion(motion, t_begin, scale, knots, tf, n):
    """The motion arguments of ingest() / ingest_host() -> (L.PointMotion, [n, 2] f32 times, [n, K * 12] f32 knots), all host.
    t_begin: [n] f32 -- for "u32" times either a uint32 array (its bits are passed on) or the f32 that carry those bits."""
    if tf is not None:
        raise ValueError("motion and tf exclude each other (compose the per-scan matrix into the knots)")
    if knots is None or t_begin is None or scale is None:
        raise ValueError("motion needs t_begin, scale and knots")
    time_offset, time_type = motion
    if time_type not in TIME_TYPES:
        raise ValueError("unknown time type %r (known: %s)" % (time_type, sorted(TIME_TYPES)))
    knots = np.ascontiguousarray(np.asarray(knots, np.float32).reshape(len(knots), -1))
    if knots.shape[0] != n or knots.shape[1] == 0 or knots.shape[1] % 12 != 0:
        raise ValueError("knots must hold K 3 x 4 matrices per scan: [%d, K, 3, 4] or [%d, K, 12], got %s" % (n, n, knots.shape))
    t_begin = np.asarray(t_begin)
    tb = t_begin.astype(np.uint32).view(np.float32) if t_begin.dtype.kind in "ui" else t_begin.astype(np.float32)
    tm = np.ascontiguousarray(np.stack([tb.reshape(n), np.asarray(scale, np.float32).reshape(n)], 1))
    return L.PointMotion(int(time_offset), TIME_TYPES[time_type], knots.shape[1] // 12, 0), tm, knots


class PointFilter:
    """Which records an ingest keeps, by ONE word of the record itself (include/cont2_amd_filter.h): the keep= of Context.ingest /
    ingest_host.  The result is ingest()'s for the kept records alone, in their order.  Made by classes() or range()."""

    def __init__(self, c_struct, bits):
        self._c, self._bits = c_struct, bits   # (the struct points into bits)

    @classmethod
    def classes(cls, offset, dtype, keep=None, drop=None, n_classes=None, shift=0, mask=None, other="keep"):
        """An integer word ("u8" | "u16" | "u32") at byte `offset` of every record: class = (word >> shift) & mask.  Exactly one of
        keep / drop lists classes; n_classes (default: the largest one listed + 1, at most 4096) bounds the table, and a class at or
        beyond it is kept or dropped as other = "keep" | "drop" says.  SemanticKITTI's moving objects:
        PointFilter.classes(12, "u32", drop=range(252, 260), mask=0xFFFF)."""
        return cls(*calls.class_filter(offset, dtype, keep, drop, n_classes, shift, mask, other))

    @classmethod
    def range(cls, offset, lo, hi):
        """An f32 word at byte `offset`: kept iff lo <= v <= hi (a NaN is dropped; lo / hi may be infinite)."""
        return cls(*calls.range_filter(offset, lo, hi))


def _keep_filter(keep, motion):
    if not isinstance(keep, PointFilter):
        raise ValueError("keep must be a PointFilter (PointFilter.classes / PointFilter.range)")
    if motion is not None:
        raise ValueError("keep together with motion is Context.ingest_rig's (one SegMotion segment per scan, its keep_offset the word's offset)")
    return keep._c


def _coord_streams(xyz, on_device):
    """The xyz of Context.ingest_coords / ingest_coords_host -> (address of the first x, y, z, dtype, stride in bytes, device).
    One 2-D tensor / array [N, >= 3] of any strides, or three 1-D ones of equal dtype and stride; nothing is copied."""
    def addr(t):
        return t.data_ptr() if on_device else t.ctypes.data

    def strides(t):
        return [s * t.element_size() for s in t.stride()] if on_device else list(t.strides)

    if isinstance(xyz, (tuple, list)):
        if len(xyz) != 3 or any(getattr(t, "ndim", 0) != 1 for t in xyz):
            raise ValueError("xyz must be one 2-D [N, >= 3] tensor or a tuple of three 1-D tensors")
        a, b, c = xyz
        if not (a.dtype == b.dtype == c.dtype and len(a) == len(b) == len(c) and strides(a) == strides(b) == strides(c)):
            raise ValueError("the three coordinate columns must have one dtype, one length and one stride")
        ptrs, stride, first = [addr(t) for t in xyz], strides(a)[0], a
    else:
        if getattr(xyz, "ndim", 0) != 2 or xyz.shape[1] < 3:
            raise ValueError("xyz must be one 2-D [N, >= 3] tensor or a tuple of three 1-D tensors")
        st = strides(xyz)
        ptrs, stride, first = [addr(xyz) + k * st[1] for k in range(3)], st[0], xyz
    if on_device and not all(t.is_cuda for t in (xyz if isinstance(xyz, (tuple, list)) else [xyz])):
        raise ValueError("ingest_coords takes CUDA tensors (ingest_coords_host: numpy arrays)")
    return ptrs[0], ptrs[1], ptrs[2], first.dtype, stride, (first.device if on_device else None)


def motion_knots(pose_begin, pose_end, ref=1.0, K=32):
    """Knot matrices of a sweep from the poses (3 x 4 [R | p], sensor to world) at its begin and end (cc_motion_knots): knot k =
    T(ref)^-1 T((k + 0.5) / K) with the rotation interpolated on SO(3) and the position linearly; ref in [0, 1] is the instant the
    scan is referred to (1: the sweep's end).  Returns [K, 3, 4] f32."""
    if K < 1:
        raise ValueError("K must be at least 1")
    pb = np.ascontiguousarray(np.asarray(pose_begin, np.float64).reshape(12))
    pe = np.ascontiguousarray(np.asarray(pose_end, np.float64).reshape(12))
    out = np.zeros((int(K), 3, 4), np.float32)
    lib().cc_motion_knots(pb.ctypes.data, pe.ctypes.data, float(ref), int(K), out.ctypes.data)
    return out


RANGE_WORDS = {"u16": (L.RANGE_U16, np.uint16), "u32": (L.RANGE_U32, np.uint32), "f32": (L.RANGE_F32, np.float32)}   # names Context.range_sensor takes
RANGE_ORDERS = {"row": L.RANGE_ROW_MAJOR, "col": L.RANGE_COL_MAJOR}


def _range_model(rows, cols, word, order, range_scale, beam_alt, beam_az_off, col_az, origin, col_knot, K):
    """The arguments of Context.range_sensor -> (L.RangeModel, the arrays it points to).  Shapes and names are checked here, values
    by the library."""
    if word not in RANGE_WORDS:
        raise ValueError("unknown range word %r (known: %s)" % (word, sorted(RANGE_WORDS)))
    if order not in RANGE_ORDERS:
        raise ValueError("unknown storage order %r (known: %s)" % (order, sorted(RANGE_ORDERS)))
    rows, cols, K = int(rows), int(cols), int(K)
    row_tab, col_cs = L.range_tables(beam_alt, np.zeros(rows) if beam_az_off is None else beam_az_off, col_az)
    if row_tab.shape != (rows, 4):
        raise ValueError("beam_alt / beam_az_off must hold %d angles (one per row), got %d" % (rows, len(row_tab)))
    if col_cs.shape != (cols, 2):
        raise ValueError("col_az must hold %d angles (one per column), got %d" % (cols, len(col_cs)))
    knot = None
    if col_knot is not None:
        knot = np.asarray(col_knot).reshape(-1)
        if knot.dtype.kind not in "iu":
            raise ValueError("col_knot must hold integers, got %s" % knot.dtype)
        if knot.size and (int(knot.min()) < -2 ** 31 or int(knot.max()) >= 2 ** 31):
            raise ValueError("col_knot does not fit 32-bit integers")
        knot = np.ascontiguousarray(knot.astype(np.int32))   # (the library checks the range 0 .. K - 1)
        if knot.shape != (cols,):
            raise ValueError("col_knot must hold %d knot indices (one per column), got %d" % (cols, len(knot)))
    n, z = origin
    m = L.RangeModel(rows, cols, RANGE_WORDS[word][0], RANGE_ORDERS[order], float(range_scale), float(n), float(z), K, row_tab.ctypes.data,
                     col_cs.ctypes.data, knot.ctypes.data if knot is not None else None)
    return m, (row_tab, col_cs, knot)


class RangeSensor:
    """cc_range_sensor: a range sensor's model with its tables on the device (Context.range_sensor makes one)."""

    def __init__(self, ctx, model, word):
        self.ctx, self.rows, self.cols, self.K, self.word = ctx, model.n_rows, model.n_cols, model.n_knots, word
        h = C.c_void_p()
        _chk(lib().cc_range_sensor_create(ctx.h, C.addressof(model), C.byref(h)), "cc_range_sensor_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().cc_range_sensor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _knots(self, knots, n):
        """[n, K, 3, 4] or [n, K, 12] -> contiguous f32 [n, K * 12] (host); None exactly when the sensor has no knots"""
        if (knots is None) != (self.K == 0):
            raise ValueError("knots come with a sensor made with K >= 1, and only with one (K = %d)" % self.K)
        if knots is None:
            return None
        knots = np.ascontiguousarray(np.asarray(knots, np.float32).reshape(n, -1))
        if knots.shape != (n, self.K * 12):
            raise ValueError("knots must hold K = %d 3 x 4 matrices per scan: [%d, %d, 3, 4], got %s" % (self.K, n, self.K, knots.shape))
        return knots


def _segment_table(scans, device):
    """[[(points, layout, tf), ...], ...] -> (array of L.PointSegment, int32 [n + 1] first-segment indices).  points: contiguous CUDA
    tensors (device=True) or numpy arrays holding the records as they are; None or an empty one for a segment without points."""
    n_seg = sum(len(sc) for sc in scans)
    arr = (L.PointSegment * max(n_seg, 1))()
    scan_segs = np.zeros(len(scans) + 1, np.int32)
    k = 0
    for i, sc in enumerate(scans):
        for (pts, layout, tf) in sc:
            g = arr[k]
            lay = _point_layout(layout)
            stride = 16 if lay is None else lay.stride_bytes
            if lay is not None:
                g.layout = lay
            if pts is not None:
                if device:
                    assert pts.is_cuda and pts.is_contiguous()
                    nbytes, ptr = pts.numel() * pts.element_size(), pts.data_ptr()
                else:
                    assert pts.flags["C_CONTIGUOUS"]
                    nbytes, ptr = pts.nbytes, pts.ctypes.data
                if stride <= 0 or nbytes % stride != 0:
                    raise ValueError("segment %d of scan %d: %d bytes are not whole records of %d bytes" % (k - scan_segs[i], i, nbytes, stride))
                g.n_points = nbytes // stride
                g.points = ptr if nbytes else None
            if tf is not None:
                tf = np.asarray(tf, np.float32).reshape(-1)
                if tf.shape != (12,):
                    raise ValueError("a segment's tf is a 3 x 4 matrix (12 values)")
                g.has_tf = 1
                g.tf[:] = tf.tolist()
            k += 1
        scan_segs[i + 1] = k
    return arr, scan_segs


class SegMotion:
    """The motion mode of a segment of Context.ingest_rig (include/cont2_amd_rig.h): the record's 4-byte time word at byte
    `time_offset` ("f32" | "u32"), t_begin (for "u32" an integer: its bits are passed on) and scale (bins per time unit), and the
    segment's slice [knot0, knot0 + n_knots) of its scan's knot pool: the record is moved by knot
    knot0 + trunc(clamp((t - t_begin) * scale, 0, n_knots - 1))."""

    def __init__(self, time_offset, type, t_begin, scale, knot0, n_knots):
        if type not in TIME_TYPES:
            raise ValueError("unknown time type %r (known: %s)" % (type, sorted(TIME_TYPES)))
        self.time_offset, self.type, self.scale, self.knot0, self.n_knots = int(time_offset), type, float(scale), int(knot0), int(n_knots)
        tb = np.asarray(t_begin)
        self.t_begin = (tb.astype(np.uint32) if type == "u32" and tb.dtype.kind in "ui" else tb.astype(np.float32)).reshape(1).tobytes()   # the slot's 4 bytes


def _rig_table(scans, device):
    """[[(points, layout, mode, keep_offset), ...], ...] -> (array of L.RigSegment, int32 [n + 1] first-segment indices); points and
    layout as _segment_table takes them; mode: None, a 3 x 4 / 12-value matrix or a SegMotion; keep_offset: the byte offset of the
    segment's filter word, or None."""
    n_seg = sum(len(sc) for sc in scans)
    arr = (L.RigSegment * max(n_seg, 1))()
    scan_segs = np.zeros(len(scans) + 1, np.int32)
    k = 0
    for i, sc in enumerate(scans):
        for (pts, layout, mode, keep_offset) in sc:
            g = arr[k]
            lay = _point_layout(layout)
            stride = 16 if lay is None else lay.stride_bytes
            if lay is not None:
                g.layout = lay
            if pts is not None:
                if device:
                    assert pts.is_cuda and pts.is_contiguous()
                    nbytes, ptr = pts.numel() * pts.element_size(), pts.data_ptr()
                else:
                    assert pts.flags["C_CONTIGUOUS"]
                    nbytes, ptr = pts.nbytes, pts.ctypes.data
                if stride <= 0 or nbytes % stride != 0:
                    raise ValueError("segment %d of scan %d: %d bytes are not whole records of %d bytes" % (k - scan_segs[i], i, nbytes, stride))
                g.n_points = nbytes // stride
                g.points = ptr if nbytes else None
            if isinstance(mode, SegMotion):
                g.mode = L.RIG_MOTION
                g.time_offset, g.time_type, g.scale, g.knot0, g.n_knots = mode.time_offset, TIME_TYPES[mode.type], mode.scale, mode.knot0, mode.n_knots
                C.memmove(C.addressof(g) + L.RigSegment.t_begin.offset, mode.t_begin, 4)   # (a u32's bits, untouched by a float conversion)
            elif mode is not None:
                tf = np.asarray(mode, np.float32).reshape(-1)
                if tf.shape != (12,):
                    raise ValueError("a segment's mode is None, a 3 x 4 matrix (12 values) or a SegMotion")
                g.mode = L.RIG_TF
                g.tf[:] = tf.tolist()
            g.filter_offset = -1 if keep_offset is None else int(keep_offset)
            k += 1
        scan_segs[i + 1] = k
    return arr, scan_segs


def _rig_args(knots, keep, n):
    """knots [n, P, 3, 4] / [n, P, 12] or None, keep: a PointFilter or None -> (f32 [n, P * 12] or None, P, L.PointFilterC or None)"""
    kn, n_pool = None, 0
    if knots is not None:
        kn = np.ascontiguousarray(np.asarray(knots, np.float32).reshape(len(knots), -1))
        if kn.shape[0] != n or kn.shape[1] == 0 or kn.shape[1] % 12 != 0:
            raise ValueError("knots must hold a pool of P 3 x 4 matrices per scan: [%d, P, 3, 4] or [%d, P, 12], got %s" % (n, n, kn.shape))
        n_pool = kn.shape[1] // 12
    if keep is not None and not isinstance(keep, PointFilter):
        raise ValueError("keep must be a PointFilter (PointFilter.classes / PointFilter.range)")
    return kn, n_pool, (None if keep is None else keep._c)


def comm_from_env():
    """cc_comm_create_from_env: (handle, rank, world) from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_PORT (one node)."""
    h, r, w = C.c_void_p(), C.c_int(), C.c_int()
    _chk(lib().cc_comm_create_from_env(C.byref(h), C.byref(r), C.byref(w)), "cc_comm_create_from_env")
    return h, r.value, w.value


def comm_allgather(comm, d_send, d_recv, bytes_per_rank, stream):
    _chk(lib().cc_comm_allgather_packed(comm, d_send, d_recv, bytes_per_rank, stream), "cc_comm_allgather_packed")


def comm_destroy(comm):
    lib().cc_comm_destroy(comm)


def packed_sizes():
    hb, fb = C.c_size_t(), C.c_size_t()
    lib().cc_packed_sizes(C.byref(hb), C.byref(fb))
    return int(hb.value), int(fb.value)


class Context:
    """cc_ctx: per-device ingest context (ContourManager constructor's role, contour_mng.h:478-498)."""

    def __init__(self, device=0, cfg=None, max_batch=512):
        import torch
        if not torch.cuda.is_available():
            raise CCError("no HIP device: the product path has no CPU fallback")
        self.cfg = cfg or L.default_manager_cfg()
        self.device = device
        self.max_batch = max_batch
        h = C.c_void_p()
        _chk(lib().cc_create(device, C.addressof(self.cfg), max_batch, C.byref(h)), "cc_create")
        self.h = h
        self.n_cell = self.cfg.n_row * self.cfg.n_col

    def close(self):
        if getattr(self, "h", None):
            lib().cc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def ingest(self, xyzi, offsets, out=None, debug=False, layout=None, tf=None, motion=None, t_begin=None, scale=None, knots=None, keep=None):
        """xyzi: torch float32 CUDA tensor [total_points, 4]; offsets: int64 host array [n+1] (in points).
        layout: where x, y, z sit in a record -- None / "xyzi" (16-byte KITTI records), "xyz" (packed, 12 bytes) or a
        (stride_bytes, xyz_offset) pair; with a layout `xyzi` is any contiguous CUDA tensor holding the records (cc_ingest_points).
        tf: one row-major 3 x 4 f32 matrix per scan ([n, 3, 4] or [n, 12], host), applied to every point while it is loaded.
        motion: (time_offset, "f32" | "u32") -- every record carries a 4-byte time word at that byte offset and every point is
        moved by the knot matrix of its time bin (cc_ingest_points_motion): knots [n, K, 3, 4] or [n, K, 12], t_begin [n] and
        scale [n] (bins per time unit), all host; bin = trunc(clamp((t - t_begin) * scale, 0, K - 1)).  Not together with tf.
        keep: a PointFilter -- records are dropped by a label / ring / intensity word of their own while they are rasterised
        (cc_ingest_points_filtered): the result is that of the kept records alone.  With layout and tf; together with motion it is
        ingest_rig()'s (one SegMotion segment per scan).
        Returns a torch uint8 CUDA tensor [n, DESC_BYTES] (array of cc_scan_desc_t) (+ debug dict)."""
        import torch
        if motion is None and (knots is not None or t_begin is not None or scale is not None):
            raise ValueError("knots, t_begin and scale come with motion=(time_offset, type)")
        flt = None if keep is None else _keep_filter(keep, motion)
        assert xyzi.is_cuda and xyzi.is_contiguous() and (layout is not None or xyzi.dtype == torch.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if out is None:
            out = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=xyzi.device)
        dbg_p, dbg = None, None
        if debug:
            dbg = {"bev": torch.empty((n, self.n_cell), dtype=torch.float32, device=xyzi.device),
                   "pix_rc": torch.empty((n, self.n_cell, 2), dtype=torch.float32, device=xyzi.device),
                   "labels": torch.empty((n, L.NLEV, self.n_cell), dtype=torch.int16, device=xyzi.device)}
            st = IngestDebug(dbg["bev"].data_ptr(), dbg["pix_rc"].data_ptr(), dbg["labels"].data_ptr())
            dbg_p = C.addressof(st)
        stream = torch.cuda.current_stream(xyzi.device).cuda_stream
        if motion is not None:
            lay = _point_layout(layout)
            mo, tm, kn = _scan_motion(motion, t_begin, scale, knots, tf, n)
            _chk(lib().cc_ingest_points_motion(self.h, xyzi.data_ptr(), C.addressof(lay) if lay is not None else None, C.addressof(mo),
                                               offsets.ctypes.data, n, tm.ctypes.data, kn.ctypes.data, out.data_ptr(), dbg_p, stream),
                 "cc_ingest_points_motion")
        elif flt is not None:
            _chk(calls.ingest_points_filtered(lib(), self.h, xyzi.data_ptr(), _point_layout(layout), flt, offsets, _scan_tf(tf, n), out.data_ptr(), dbg_p,
                                              stream), "cc_ingest_points_filtered")
        elif layout is None and tf is None:
            _chk(lib().cc_ingest_batch(self.h, xyzi.data_ptr(), offsets.ctypes.data, n, out.data_ptr(), dbg_p, stream),
                 "cc_ingest_batch")
        else:
            lay, tfa = _point_layout(layout), _scan_tf(tf, n)
            _chk(lib().cc_ingest_points(self.h, xyzi.data_ptr(), C.addressof(lay) if lay is not None else None, offsets.ctypes.data, n,
                                        tfa.ctypes.data if tfa is not None else None, out.data_ptr(), dbg_p, stream), "cc_ingest_points")
        return (out, dbg) if debug else out

    def ingest_coords(self, xyz, offsets, origin=None, scale=None, tf=None, out=None, debug=False):
        """Coordinates of another type or shape than ingest()'s records, read where they lie (cc_ingest_coords,
        include/cont2_amd_coords.h).  xyz: ONE 2-D CUDA tensor [N, >= 3] -- columns 0 - 2 are x, y, z, ANY strides are taken: a
        float64 [N, 3], a view t[:, 2:5] of a wider tensor, a transposed [3, N].T, all without a copy -- or a tuple of three 1-D
        CUDA tensors of equal dtype and stride (three columns).  dtype float32, float64 or int32 (anything else: ValueError).
        origin: [n, 3] float64 on the host, subtracted in f64 BEFORE the narrowing to f32 (a georeferenced cloud's local origin);
        scale: 3 values (or one), with int32 only -- p = float(double(v) * scale - origin), every step rounded once; tf: as for
        ingest(), applied to p.  The result is ingest()'s for the packed f32 points p.  Returns ingest()'s outputs."""
        import torch
        x, y, z, dtype, stride, dev = _coord_streams(xyz, True)
        src = calls.coord_src(x, y, z, dtype, stride, scale)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        if out is None:
            out = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=dev)
        dbg_p, dbg = None, None
        if debug:
            dbg = {"bev": torch.empty((n, self.n_cell), dtype=torch.float32, device=dev),
                   "pix_rc": torch.empty((n, self.n_cell, 2), dtype=torch.float32, device=dev),
                   "labels": torch.empty((n, L.NLEV, self.n_cell), dtype=torch.int16, device=dev)}
            st = IngestDebug(dbg["bev"].data_ptr(), dbg["pix_rc"].data_ptr(), dbg["labels"].data_ptr())
            dbg_p = C.addressof(st)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _chk(calls.ingest_coords(lib(), self.h, src, offsets, origin, _scan_tf(tf, n), out.data_ptr(), dbg_p, stream), "cc_ingest_coords")
        return (out, dbg) if debug else out

    def ingest_coords_host(self, xyz, offsets, origin=None, scale=None, tf=None):
        """ingest_coords() with numpy arrays: host coordinates in (one 2-D array of any strides, or a tuple of three 1-D arrays), host
        descriptors out (cc_ingest_coords_host).  Exactly the bytes the streams span are copied to the device."""
        x, y, z, dtype, stride, _ = _coord_streams(xyz, False)
        src = calls.coord_src(x, y, z, dtype, stride, scale)
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        out = np.zeros(n, L.scan_desc_dt)
        _chk(calls.ingest_coords(lib(), self.h, src, offsets, origin, _scan_tf(tf, n), out.ctypes.data, host=True), "cc_ingest_coords_host")
        return out

    def range_sensor(self, rows, cols, word="u16", order="row", range_scale=0.001, beam_alt=None, beam_az_off=None, col_az=None, origin=(0.0, 0.0),
                     col_knot=None, K=0):
        """A range sensor (cc_range_sensor_create): images of rows x cols words ("u16" | "u32" | "f32") stored "row"-major (pixel j =
        row * cols + col) or "col"-major (firing after firing), range_scale metres per unit of the word.  beam_alt / beam_az_off: the
        beams' altitude and azimuth offset, col_az: the firings' encoder azimuth, all in radians -- the tables are made in f64 and
        rounded to f32.  origin = (distance of the beam origin from the rotation axis, its height).  K knots per scan (0: none) and
        col_knot [cols]: the knot of every firing (None: all 0)."""
        if beam_alt is None or col_az is None:
            raise ValueError("range_sensor needs beam_alt and col_az")
        m, keep = _range_model(rows, cols, word, order, range_scale, beam_alt, beam_az_off, col_az, origin, col_knot, K)
        return RangeSensor(self, m, word)   # (the tables are copied before the call returns; `keep` lives until here)

    def ingest_ranges(self, sensor, ranges, knots=None, out=None, debug=False):
        """Range images rasterised in place (cc_ingest_ranges): `ranges` is a contiguous CUDA tensor of n * rows * cols words of the
        sensor's type (any shape; int16 / int32 tensors stand for u16 / u32), knots [n, K, 3, 4] or [n, K, 12] host matrices (None
        exactly for a sensor with K = 0): every pixel is moved by the knot of its column.  Returns ingest()'s outputs."""
        import torch
        if sensor.ctx is not self:
            raise ValueError("the sensor belongs to another context")
        assert ranges.is_cuda and ranges.is_contiguous()
        wbytes = np.dtype(RANGE_WORDS[sensor.word][1]).itemsize
        if ranges.element_size() != wbytes or (sensor.word == "f32") != ranges.dtype.is_floating_point:
            raise ValueError("the sensor's words are %s, the tensor holds %s" % (sensor.word, ranges.dtype))
        hw = sensor.rows * sensor.cols
        if ranges.numel() == 0 or ranges.numel() % hw != 0:
            raise ValueError("%d words are not whole images of %d x %d" % (ranges.numel(), sensor.rows, sensor.cols))
        n = ranges.numel() // hw
        kn = sensor._knots(knots, n)
        if out is None:
            out = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=ranges.device)
        dbg_p, dbg = None, None
        if debug:
            dbg = {"bev": torch.empty((n, self.n_cell), dtype=torch.float32, device=ranges.device),
                   "pix_rc": torch.empty((n, self.n_cell, 2), dtype=torch.float32, device=ranges.device),
                   "labels": torch.empty((n, L.NLEV, self.n_cell), dtype=torch.int16, device=ranges.device)}
            st = IngestDebug(dbg["bev"].data_ptr(), dbg["pix_rc"].data_ptr(), dbg["labels"].data_ptr())
            dbg_p = C.addressof(st)
        stream = torch.cuda.current_stream(ranges.device).cuda_stream
        _chk(lib().cc_ingest_ranges(self.h, sensor.h, ranges.data_ptr(), n, kn.ctypes.data if kn is not None else None, out.data_ptr(), dbg_p, stream),
             "cc_ingest_ranges")
        return (out, dbg) if debug else out

    def ingest_ranges_host(self, sensor, ranges, knots=None):
        """ingest_ranges() from a host array of the sensor's word type: host descriptors out."""
        if sensor.ctx is not self:
            raise ValueError("the sensor belongs to another context")
        ranges = np.ascontiguousarray(ranges, RANGE_WORDS[sensor.word][1])
        hw = sensor.rows * sensor.cols
        if ranges.size == 0 or ranges.size % hw != 0:
            raise ValueError("%d words are not whole images of %d x %d" % (ranges.size, sensor.rows, sensor.cols))
        n = ranges.size // hw
        kn = sensor._knots(knots, n)
        out = np.zeros(n, L.scan_desc_dt)
        _chk(lib().cc_ingest_ranges_host(self.h, sensor.h, ranges.ctypes.data, n, kn.ctypes.data if kn is not None else None, out.ctypes.data, None),
             "cc_ingest_ranges_host")
        return out

    def _images(self, height, pos_rc):
        """the shape checks ingest_images / ingest_images_host share (torch tensors or numpy arrays) -> the number of images"""
        if height.ndim not in (2, 3):
            raise ValueError("height must be [n, n_cell] or [n, n_row, n_col], got %s" % (tuple(height.shape),))
        n = int(height.shape[0])
        if (height.ndim == 2 and height.shape[1] != self.n_cell) or (height.ndim == 3 and tuple(height.shape[1:]) != (self.cfg.n_row, self.cfg.n_col)):
            raise ValueError("height must hold %d x %d images, got %s" % (self.cfg.n_row, self.cfg.n_col, tuple(height.shape)))
        if pos_rc is not None and (pos_rc.shape[0] != n or pos_rc.shape[-1] != 2 or int(np.prod(pos_rc.shape[1:])) != 2 * self.n_cell):
            raise ValueError("pos_rc must be [%d, %d, 2], got %s" % (n, self.n_cell, tuple(pos_rc.shape)))
        return n

    def ingest_images(self, height, pos_rc=None, min_height=None, out=None, debug=False):
        """Descriptors from caller-made max-height images (cc_ingest_images, include/cont2_amd_images.h): no points are read.
        height: float32 CUDA tensor [n, n_cell] or [n, n_row, n_col], contiguous -- image heights (z + lidar_height), the layout of
        ingest(debug=True)'s "bev"; pos_rc: float32 CUDA [n, n_cell, 2] of (row_f, col_f) like "pix_rc", or None for the cell
        centres; min_height: n host values that become min_bin_val, or None for the minimum over the occupied cells.  A cell is
        occupied iff row >= 1 and h > -1000 (NaN is empty); a position component that is NaN or more than half a cell from its
        cell's centre is replaced by the centre's.  Returns what ingest() returns."""
        import torch
        assert height.is_cuda and height.is_contiguous() and height.dtype == torch.float32
        assert pos_rc is None or (pos_rc.is_cuda and pos_rc.is_contiguous() and pos_rc.dtype == torch.float32)
        n = self._images(height, pos_rc)
        if out is None:
            out = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=height.device)
        dbg_p, dbg = None, None
        if debug:
            dbg = {"bev": torch.empty((n, self.n_cell), dtype=torch.float32, device=height.device),
                   "pix_rc": torch.empty((n, self.n_cell, 2), dtype=torch.float32, device=height.device),
                   "labels": torch.empty((n, L.NLEV, self.n_cell), dtype=torch.int16, device=height.device)}
            st = IngestDebug(dbg["bev"].data_ptr(), dbg["pix_rc"].data_ptr(), dbg["labels"].data_ptr())
            dbg_p = C.addressof(st)
        stream = torch.cuda.current_stream(height.device).cuda_stream
        _chk(calls.ingest_images(lib(), self.h, height.data_ptr(), None if pos_rc is None else pos_rc.data_ptr(), n, min_height, out.data_ptr(), dbg_p,
                                 stream), "cc_ingest_images")
        return (out, dbg) if debug else out

    def ingest_images_host(self, height, pos_rc=None, min_height=None, want_bev=False):
        """ingest_images() from host arrays (numpy f32, the same shapes): host descriptors out (cc_ingest_images_host); with want_bev
        followed by the images as the library read them [n, n_cell]."""
        height = np.ascontiguousarray(height, np.float32)
        pos_rc = None if pos_rc is None else np.ascontiguousarray(pos_rc, np.float32)
        n = self._images(height, pos_rc)
        out = np.zeros(n, L.scan_desc_dt)
        bev = np.zeros((n, self.n_cell), np.float32) if want_bev else None
        _chk(calls.ingest_images(lib(), self.h, height.ctypes.data, None if pos_rc is None else pos_rc.ctypes.data, n, min_height, out.ctypes.data,
                                 host=True, bev=bev.ctypes.data if want_bev else None), "cc_ingest_images_host")
        return (out, bev) if want_bev else out

    def path_counts(self):
        """Which body of K2 took the context's scans so far (cc_ingest_path_counts, include/cont2_amd_paths.h; waits for the queued ingest calls):
        {"mid": scans the list kernel handed to cc_k_contours_mid, "why": those by reason (configuration, entries / slots, components
        per level, member-list padding), "big": scans handed on to cc_k_contours_big}.  The difference of two readings counts the
        calls between them."""
        out = (C.c_int32 * 6)()
        _chk(lib().cc_ingest_path_counts(self.h, out), "cc_ingest_path_counts")
        return {"mid": int(out[0]), "why": [int(v) for v in out[1:5]], "big": int(out[5])}

    def ingest_segments(self, scans, out=None, debug=False):
        """Every scan from an ordered list of point segments, each with its own record shape and transform (cc_ingest_segments):
        scans = [[(points, layout, tf), ...], ...] with `points` a contiguous CUDA tensor holding the segment's records (read in
        place; the tensors of one call may be separate allocations), `layout` as ingest() takes it and `tf` a 3 x 4 / 12-value
        array or None.  The result is ingest()'s for the cloud T_0(segment 0) ++ T_1(segment 1) ++ ... of every scan.
        Returns a torch uint8 CUDA tensor [n, DESC_BYTES] (+ debug dict)."""
        import torch
        arr, scan_segs = _segment_table(scans, device=True)
        n = len(scans)
        dev = next((p.device for sc in scans for (p, _l, _t) in sc if p is not None), torch.device("cuda", self.device))
        if out is None:
            out = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=dev)
        dbg_p, dbg = None, None
        if debug:
            dbg = {"bev": torch.empty((n, self.n_cell), dtype=torch.float32, device=dev),
                   "pix_rc": torch.empty((n, self.n_cell, 2), dtype=torch.float32, device=dev),
                   "labels": torch.empty((n, L.NLEV, self.n_cell), dtype=torch.int16, device=dev)}
            st = IngestDebug(dbg["bev"].data_ptr(), dbg["pix_rc"].data_ptr(), dbg["labels"].data_ptr())
            dbg_p = C.addressof(st)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _chk(lib().cc_ingest_segments(self.h, C.addressof(arr), scan_segs.ctypes.data, n, out.data_ptr(), dbg_p, stream), "cc_ingest_segments")
        return (out, dbg) if debug else out

    def ingest_segments_host(self, scans):
        """ingest_segments() from host records (numpy arrays of any dtype holding the records as they are): host descriptors out."""
        arr, scan_segs = _segment_table(scans, device=False)
        out = np.zeros(len(scans), L.scan_desc_dt)
        _chk(lib().cc_ingest_segments_host(self.h, C.addressof(arr), scan_segs.ctypes.data, len(scans), out.ctypes.data, None),
             "cc_ingest_segments_host")
        return out

    def ingest_rig(self, scans, knots=None, keep=None, out=None, debug=False):
        """A rig's sensors de-skewed, filtered and joined in one sweep (cc_ingest_rig, include/cont2_amd_rig.h): scans =
        [[(points, layout, mode, keep_offset), ...], ...], at most RIG_SEG_MAX segments per scan.  points, layout: as for
        ingest_segments(); mode: None (the points as they are), a 3 x 4 / 12-value matrix, or a SegMotion(time_offset, type, t_begin,
        scale, knot0, n_knots) -- the record is de-skewed by its time word with the segment's slice of the scan's knot pool;
        keep_offset: the byte offset of the segment's filter word, or None for a segment that is not filtered.  knots: the pools,
        [n, P, 3, 4] or [n, P, 12] on the host (None: no segment is in motion mode); keep: ONE PointFilter for all segments (its own
        offset is not read).  The result is ingest()'s for the moved records of every scan in the order given, the dropped ones left
        out.  Returns a torch uint8 CUDA tensor [n, DESC_BYTES] (+ debug dict)."""
        import torch
        arr, scan_segs = _rig_table(scans, device=True)
        n = len(scans)
        kn, n_pool, flt = _rig_args(knots, keep, n)
        dev = next((p.device for sc in scans for (p, _l, _m, _k) in sc if p is not None), torch.device("cuda", self.device))
        if out is None:
            out = torch.empty((n, DESC_BYTES), dtype=torch.uint8, device=dev)
        dbg_p, dbg = None, None
        if debug:
            dbg = {"bev": torch.empty((n, self.n_cell), dtype=torch.float32, device=dev),
                   "pix_rc": torch.empty((n, self.n_cell, 2), dtype=torch.float32, device=dev),
                   "labels": torch.empty((n, L.NLEV, self.n_cell), dtype=torch.int16, device=dev)}
            st = IngestDebug(dbg["bev"].data_ptr(), dbg["pix_rc"].data_ptr(), dbg["labels"].data_ptr())
            dbg_p = C.addressof(st)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _chk(lib().cc_ingest_rig(self.h, C.addressof(arr), scan_segs.ctypes.data, n, kn.ctypes.data if kn is not None else None, n_pool,
                                 C.addressof(flt) if flt is not None else None, out.data_ptr(), dbg_p, stream), "cc_ingest_rig")
        return (out, dbg) if debug else out

    def ingest_rig_host(self, scans, knots=None, keep=None):
        """ingest_rig() from host records (numpy arrays of any dtype holding the records as they are): host descriptors out."""
        arr, scan_segs = _rig_table(scans, device=False)
        n = len(scans)
        kn, n_pool, flt = _rig_args(knots, keep, n)
        out = np.zeros(n, L.scan_desc_dt)
        _chk(lib().cc_ingest_rig_host(self.h, C.addressof(arr), scan_segs.ctypes.data, n, kn.ctypes.data if kn is not None else None, n_pool,
                                      C.addressof(flt) if flt is not None else None, out.ctypes.data, None), "cc_ingest_rig_host")
        return out

    def pack(self, desc):
        """Full descriptors (torch uint8 CUDA [n, DESC_BYTES]) -> (hot [n, HOT_BYTES], feat [n, FEAT_BYTES]): the compact
        per-scan records the database keeps and the ranks exchange (59 KB instead of 169 KB per scan)."""
        import torch
        n = desc.shape[0]
        hb, fb = packed_sizes()
        hot = torch.empty((n, hb), dtype=torch.uint8, device=desc.device)
        feat = torch.empty((n, fb), dtype=torch.uint8, device=desc.device)
        stream = torch.cuda.current_stream(desc.device).cuda_stream
        _chk(lib().cc_pack_scans(self.h, desc.data_ptr(), n, hot.data_ptr(), feat.data_ptr(), stream), "cc_pack_scans")
        return hot, feat

    def gate_mask(self, xy, gates, row_words=None):
        """Rows of a position prior, made on the device (cc_mask_gates): xy float32 CUDA [n_scans, 2], the scans' positions;
        gates float32 CUDA [n_rows, 3] of (x, y, radius).  Returns the int32 CUDA table [n_rows, row_words] (row_words defaults
        to ceil(n_scans / 32)) in which bit g of row r is set iff scan g lies within gate r's circle, the f32 sum
        dx * dx + dy * dy <= radius * radius as written; hand it to ScanMask(bits, rows)."""
        import torch
        assert xy.is_cuda and gates.is_cuda and xy.dtype == torch.float32 and gates.dtype == torch.float32
        xy, gates = xy.contiguous().reshape(-1, 2), gates.contiguous().reshape(-1, 3)
        n, nr = int(xy.shape[0]), int(gates.shape[0])
        rw = max((n + 31) // 32, 1) if row_words is None else int(row_words)
        bits = torch.empty((nr, max(rw, 1)), dtype=torch.int32, device=xy.device)
        stream = torch.cuda.current_stream(xy.device).cuda_stream
        _chk(lib().cc_mask_gates(self.h, xy.data_ptr(), n, gates.data_ptr(), nr, bits.data_ptr(), rw, stream), "cc_mask_gates")
        return bits

    def ingest_host(self, xyzi, offsets, layout=None, tf=None, motion=None, t_begin=None, scale=None, knots=None, keep=None):
        """Host records in, host descriptors out.  layout / tf / motion, t_begin, scale, knots, keep: as for ingest(); with a layout
        `xyzi` is a contiguous numpy array of any dtype holding the records as they are."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        out = np.zeros(n, L.scan_desc_dt)
        if motion is None and (knots is not None or t_begin is not None or scale is not None):
            raise ValueError("knots, t_begin and scale come with motion=(time_offset, type)")
        if keep is not None:
            flt = _keep_filter(keep, motion)
            xyzi = np.ascontiguousarray(xyzi, np.float32) if layout is None else np.ascontiguousarray(xyzi)
            _chk(calls.ingest_points_filtered(lib(), self.h, xyzi.ctypes.data, _point_layout(layout), flt, offsets, _scan_tf(tf, n), out.ctypes.data,
                                              host=True), "cc_ingest_points_filtered_host")
            return out
        if motion is not None:
            lay = _point_layout(layout)
            mo, tm, kn = _scan_motion(motion, t_begin, scale, knots, tf, n)
            xyzi = np.ascontiguousarray(xyzi)
            _chk(lib().cc_ingest_points_motion_host(self.h, xyzi.ctypes.data, C.addressof(lay) if lay is not None else None, C.addressof(mo),
                                                    offsets.ctypes.data, n, tm.ctypes.data, kn.ctypes.data, out.ctypes.data, None),
                 "cc_ingest_points_motion_host")
            return out
        if layout is None and tf is None:
            xyzi = np.ascontiguousarray(xyzi, np.float32)
            _chk(lib().cc_ingest_host(self.h, xyzi.ctypes.data, offsets.ctypes.data, n, out.ctypes.data), "cc_ingest_host")
            return out
        xyzi = np.ascontiguousarray(xyzi, np.float32) if layout is None else np.ascontiguousarray(xyzi)
        lay, tfa = _point_layout(layout), _scan_tf(tf, n)
        _chk(lib().cc_ingest_points_host(self.h, xyzi.ctypes.data, C.addressof(lay) if lay is not None else None, offsets.ctypes.data, n,
                                         tfa.ctypes.data if tfa is not None else None, out.ctypes.data, None), "cc_ingest_points_host")
        return out


def desc_to_numpy(desc_tensor):
    """torch uint8 [n, DESC_BYTES] (any device) -> numpy structured array of cc_scan_desc_t."""
    return desc_tensor.cpu().numpy().view(L.scan_desc_dt).reshape(-1)


def match_pairs(row):
    """The matched contour pairs of one L.ranked_match_dt record (an entry of the array matches=inlier_px returns), in key
    order -> int8 [n_pairs, 3] of (level, seq_src, seq_tgt): the database scan's contour seq_src and the query's seq_tgt of that
    level.  cc_match_pairs in C."""
    return L.match_pairs(row)


class Packed:
    """Packed records as the query of Database.query / verify / score_poses (and their _submit forms) in the place of `qdesc`:
    hot / feat are the tensors Context.pack returns (or records gathered from another rank, or a saved map), idx names the
    record of every query (None: query i is record i).  Where the call has its own selector (verify's qidx, score_poses' q) that
    one names the records and idx must be None."""

    def __init__(self, hot, feat, idx=None):
        assert hot.is_cuda and feat.is_cuda and hot.is_contiguous() and feat.is_contiguous() and feat.shape[0] == hot.shape[0]
        self.hot, self.feat = hot, feat
        self.idx = None if idx is None else np.ascontiguousarray(idx, np.int32).reshape(-1)
        self.device = hot.device

    def _src(self):
        return L.PackedSrc(self.hot.data_ptr(), self.feat.data_ptr(), int(self.hot.shape[0]), 0)


class Stored:
    """Scans of the database itself as the query (Database.stored makes one): idx names them by database index."""

    def __init__(self, db, idx=None):
        self.db = db
        self.idx = None if idx is None else np.ascontiguousarray(list(idx) if isinstance(idx, range) else idx, np.int32).reshape(-1)
        self.device = None

    def _src(self):
        return L.PackedSrc(None, None, 0, 0)


def _is_src(q):
    return isinstance(q, (Packed, Stored))


class ScanMask:
    """The scans that may answer a query (the mask= of Database.query / query_submit): bits is an int32 or uint32 CUDA tensor
    [n_rows, row_words] -- bit g & 31 of word g >> 5 of a row set = scan g may answer -- and rows names one row per query
    (-1: no restriction; many queries may share a row).  A masked query behaves as if the other scans' keys were not in the
    database's trees.  The table must stay unchanged until the call it is handed to has been waited for."""

    def __init__(self, bits, rows):
        import torch
        assert bits.is_cuda and bits.dim() == 2 and bits.is_contiguous() and bits.dtype in (torch.int32, torch.uint32)
        self.bits = bits
        self.rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        self.device = bits.device

    @classmethod
    def from_allowed(cls, allowed, rows=None, device="cuda", n_db=None):
        """allowed: a bool array [n_rows, n_db] or a list of index arrays (n_db: the number of scans the rows cover, by default
        the largest index + 1), packed on the host and uploaded.  rows: the row of every query (default: query i names row i)."""
        import torch
        tab = L.pack_mask_rows(allowed, n_db=n_db)
        bits = torch.from_numpy(tab.view(np.int32)).to(device)
        return cls(bits, np.arange(len(tab), dtype=np.int32) if rows is None else rows)

    def _c(self):
        return self.bits.data_ptr(), int(self.bits.shape[0]), int(self.bits.shape[1]), self.rows


class ScanLists:
    """The scans that may answer a query as index lists (the among= of Database.query / query_submit; include/cont2_amd_lists.h):
    list r is idx[off[r] : off[r + 1]] -- strictly increasing database indices, at most L.LIST_SCANS_MAX of them -- and rows names
    one list per query (-1: no restriction; many queries may share a list).  A listed query answers exactly like the masked
    query whose row has the list's bits set, but its retrieval reads the listed scans' keys only: its cost follows the list, not
    the map (about 1 us per listed scan per 1 024 queries; it meets the masked walk near 960 scans per list at 5 000 scans:
    DESIGN.md 3.13).  Everything is host memory and is read before the call returns; nothing has to be kept alive."""

    def __init__(self, idx, off, rows):
        self.idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        self.off = np.ascontiguousarray(off, np.int32).reshape(-1)
        self.rows = np.ascontiguousarray(rows, np.int32).reshape(-1)

    @classmethod
    def from_lists(cls, lists, rows=None):
        """lists: a sequence of index sequences, taken as they are (nothing is sorted or de-duplicated: the library refuses a list
        that is not strictly increasing).  rows: the list of every query (default: query i names list i)."""
        ls = [np.asarray(l, np.int64).reshape(-1) for l in lists]
        off = np.zeros(len(ls) + 1, np.int64)
        np.cumsum([len(l) for l in ls], out=off[1:])
        idx = np.concatenate(ls) if ls else np.zeros(0, np.int64)
        return cls(idx, off, np.arange(len(ls), dtype=np.int32) if rows is None else rows)

    @classmethod
    def from_gates(cls, xy, gates, rows=None):
        """The lists of a position prior, made on the host: xy [n_scans, 2] the scans' positions, gates [n_rows, 3] of (x, y,
        radius), numpy arrays or tensors.  List r holds the set bits of Context.gate_mask's row r (the same f32 expression)."""
        to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)  # noqa: E731
        idx, off = L.gate_lists(to_np(xy), to_np(gates))
        return cls(idx, off, np.arange(len(off) - 1, dtype=np.int32) if rows is None else rows)

    def lists(self):
        """the lists as numpy arrays"""
        return [self.idx[self.off[r]:self.off[r + 1]] for r in range(len(self.off) - 1)]

    def _c(self):
        return self.idx, self.off, self.rows


class Database:
    """cc_db: device-resident ContourDB (contour_db.h:673-845) + batched queryRangedKNN."""

    def __init__(self, ctx, cfg=None, capacity=8192):
        self.ctx = ctx
        self.cfg = cfg or L.default_db_cfg()
        h = C.c_void_p()
        _chk(lib().cc_db_create(ctx.h, C.addressof(self.cfg), capacity, C.byref(h)), "cc_db_create")
        self.h = h
        self._pending = []  # what the library reads or writes until query_wait

    def close(self):
        if getattr(self, "h", None):
            lib().cc_db_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return lib().cc_db_size(self.h)

    @property
    def knn_stride(self):
        """Last dimension of the hit array query(want_knn=True) returns: KNN_MAX for nnk <= KNN_MAX, else KNN_MAX_LARGE."""
        return lib().cc_db_knn_stride(self.h)

    def add_scans(self, desc, ts, seeds):
        """desc: torch uint8 CUDA [n, DESC_BYTES]; ts float64 [n]; seeds int32 [n] (the reference passes the scan's
        assigned seq to pushAndBalance, batch_bin_test.cpp:236)."""
        import torch
        ts = np.ascontiguousarray(ts, np.float64)
        seeds = np.ascontiguousarray(seeds, np.int32)
        n = desc.shape[0]
        assert desc.is_cuda and desc.dtype == torch.uint8 and desc.is_contiguous() and len(ts) == n and len(seeds) == n
        stream = torch.cuda.current_stream(desc.device).cuda_stream
        _chk(lib().cc_db_add_scans(self.h, desc.data_ptr(), n, ts.ctypes.data, seeds.ctypes.data, stream), "cc_db_add_scans")

    def stored(self, idx=None):
        """The database's own scans as the query of query / verify / score_poses (and their _submit forms): scan idx[i] is query
        i (an int names one scan; None leaves the naming to the call's own selector -- verify's qidx, score_poses' q).  Nothing is
        excluded: scan g queried at epoch g is the online loop's query of g, at a later epoch the answer may be g itself."""
        return Stored(self, None if idx is None else ([idx] if isinstance(idx, (int, np.integer)) else idx))

    def _source(self, q, rows=False):
        """A query argument -- a descriptor tensor, a Packed or a Stored -- checked -> (the keywords that name it to a flow of
        `calls`, its device, the stream the call is queued on).  rows: the flow indexes the descriptors (uint8 [n, DESC_BYTES])."""
        import torch
        if _is_src(q):
            if isinstance(q, Stored) and q.db is not self:
                raise ValueError("the stored scans belong to another database")
            kw = {"src": q._src(), "idx": q.idx}
            dev = q.device if q.device is not None else torch.device("cuda", self.ctx.device)
        else:
            assert q.is_cuda and q.is_contiguous()
            kw, dev = {"qdesc": q.data_ptr()}, q.device
            if rows:
                assert q.dtype == torch.uint8 and q.dim() == 2 and q.shape[1] == DESC_BYTES
                kw["n_desc"] = q.shape[0]
        return kw, dev, torch.cuda.current_stream(dev).cuda_stream

    def _held(self, *objs):
        """A new entry of the pending list that holds `objs` (the query's tensors or source, the mask) -> the list in it to which
        the submit appends its host buffers before the library is called: a submit that fails may have queued some chunks."""
        keep = []
        self._pending.append((objs, keep))
        return keep

    def _query_kw(self, qdesc, epochs, mask, among=None):
        """what query() and query_submit() hand to calls.query for their query, epochs, mask and lists -> (keywords, device, nq)"""
        if mask is not None and not isinstance(mask, ScanMask):
            raise TypeError("mask must be a ScanMask")
        if among is not None and not isinstance(among, ScanLists):
            raise TypeError("among must be a ScanLists")
        if mask is not None and among is not None:
            raise ValueError("give the scans that may answer as mask= or as among=, not both")
        kw, dev, stream = self._source(qdesc)
        epochs = np.ascontiguousarray(epochs, np.int32).reshape(-1)
        assert "src" in kw or qdesc.shape[0] == len(epochs)
        kw.update(epochs=epochs, stream=stream, mask=None if mask is None else mask._c(), among=None if among is None else among._c())
        return kw, dev, len(epochs)

    def add_scans_prepare(self, desc):
        """Queue the device half of add_scans(desc, ...) on the current stream without waiting (cc_db_add_scans_prepare)."""
        import torch
        assert desc.is_cuda and desc.dtype == torch.uint8 and desc.is_contiguous()
        stream = torch.cuda.current_stream(desc.device).cuda_stream
        _chk(lib().cc_db_add_scans_prepare(self.h, desc.data_ptr(), desc.shape[0], stream), "cc_db_add_scans_prepare")

    _detail_args = staticmethod(calls.detail_buffer)  # (kept under this name for tests/test_emu_ranked_detail.py, which asks it for the refusal)

    def query(self, qdesc, epochs, lb=None, ub=None, want_knn=False, allow_flagged=False, ranked=None, detail=False, mask=None, matches=None,
              among=None):
        """qdesc: torch uint8 CUDA [nq, DESC_BYTES]; epochs int32 [nq] (DB state each query sees).
        In the place of qdesc: self.stored(idx) -- scans of this database by index -- or Packed(hot, feat, idx): the query comes
        from the packed records instead of from descriptors (cc_db_query_submit_packed + the wait), with the same answers.
        Returns numpy structured array of cc_query_result_t (+ knn hits / counts as torch tensors).
        allow_flagged: a query that met an internal capacity (cc_query_result_t.flags != 0) makes the library return
        CC_ECAPACITY with every result delivered; True hands the results back (the caller looks at `flags`) instead of raising.
        ranked=K (1..RANK_MAX): the ranked list of every query's refined candidates as well (cc_db_query_submit_ranked): the return
        value is followed by (cands [nq, K] of L.ranked_cand_dt, counts [nq]); entry 0 of a list is the candidate the result names.
        The ranked form is query_submit(ranked=K) + query_wait(): a batch of a full chunk or more goes out in whole chunks, lane
        after lane, where the plain synchronous call cuts one chunk per lane -- the same answers, scheduled differently.
        detail=True (with ranked=K): followed by a [nq, K] array of L.ranked_detail_dt as well -- per entry the curvature of
        -correlation at its pose (hess, grad) and the refinement's start, initial correlation, iterations, termination and pair
        count (cc_db_query_submit_ranked_detail).  Without ranked it is a ValueError.
        mask=ScanMask(...): only the scans of each query's row may answer (cc_db_query_submit_masked + the wait): the retrieval
        runs as if the other scans' keys were not in the trees.  It combines with every form above.
        matches=inlier_px (with ranked=K; >= 0): followed by a [nq, K] array of L.ranked_match_dt as well -- per entry the matched
        contour pairs its pose was built from (the selected proposal's constellation as a 400-bit set: match_pairs(row) lists
        them), the proposal's votes and area, and the pairs' residuals at the entry's pose: rms, max and how many lie within
        inlier_px pixels (cc_db_query_submit_matched).  It combines with stored / Packed queries, mask= and detail=True; a
        database in dynamic-threshold mode refuses it.  Without ranked it is a ValueError.
        among=ScanLists(...): only the scans of each query's LIST may answer (cc_db_query_submit_listed + the wait): the answers of
        the mask whose rows hold the lists' bits, from a retrieval that reads the listed scans' keys only.  It combines with every
        form above except mask= (giving both is a ValueError)."""
        import torch
        kw, dev, nq = self._query_kw(qdesc, epochs, mask, among)
        knn = cnt = None
        if want_knn:
            ks = self.knn_stride
            knn = torch.zeros((nq, L.NQLEV, L.NPIV, ks, L.knn_hit_dt.itemsize), dtype=torch.uint8, device=dev)
            cnt = torch.zeros((nq, L.NQLEV, L.NPIV), dtype=torch.int32, device=dev)
            kw.update(knn=knn.data_ptr(), knn_cnt=cnt.data_ptr())
        r = calls.query(lib(), self.h, lb=lb, ub=ub, ranked=ranked, detail=detail, matches=matches,
                        tolerate=(CC_ECAPACITY,) if allow_flagged else (), **kw)
        if want_knn:
            knn, cnt = knn.cpu().numpy().view(L.knn_hit_dt).reshape(nq, L.NQLEV, L.NPIV, ks), cnt.cpu().numpy()
        return _ret(r.res, knn, cnt, r.rank, r.detail, r.match)

    def query_submit(self, qdesc, epochs, lb=None, ub=None, ranked=None, detail=False, mask=None, matches=None, among=None):
        """Asynchronous form of query(): queues the batch and returns the result array, which is only valid after
        query_wait() (cc_db_query_submit / cc_db_query_wait).  qdesc may be overwritten by work queued afterwards on the
        current stream.  ranked=K: returns (results, (cands [nq, K], counts [nq])), all of them valid after query_wait();
        with detail=True followed by the [nq, K] detail array (see query()).  qdesc may be self.stored(idx) or a Packed.
        mask=ScanMask(...): as for query(); the pending list keeps the mask's table alive until query_wait().
        matches=inlier_px: followed by the [nq, K] match array (see query()), valid after query_wait() like the rest.
        among=ScanLists(...): as for query(); the lists are read before this returns."""
        kw, _dev, _nq = self._query_kw(qdesc, epochs, mask, among)
        r = calls.query(lib(), self.h, lb=lb, ub=ub, ranked=ranked, detail=detail, matches=matches, wait=False, keep=self._held(qdesc, mask), **kw)
        return _ret(r.res, r.rank, r.detail, r.match)

    def query_wait(self):
        _chk(lib().cc_db_query_wait(self.h), "cc_db_query_wait")
        self._pending = []

    def add_packed(self, hot, feat, ts, seeds):
        """hot / feat: torch uint8 CUDA [n, HOT_BYTES] / [n, FEAT_BYTES] as produced by Context.pack (possibly gathered from
        other ranks).  Same effect as add_scans on the full descriptors."""
        import torch
        ts = np.ascontiguousarray(ts, np.float64)
        seeds = np.ascontiguousarray(seeds, np.int32)
        n = hot.shape[0]
        assert hot.is_cuda and feat.is_cuda and hot.is_contiguous() and feat.is_contiguous() and feat.shape[0] == n
        assert len(ts) == n and len(seeds) == n
        stream = torch.cuda.current_stream(hot.device).cuda_stream
        _chk(lib().cc_db_add_packed(self.h, hot.data_ptr(), feat.data_ptr(), n, ts.ctypes.data, seeds.ctypes.data, stream),
             "cc_db_add_packed")

    def check_hints(self, qdesc, hints, lb=None, ub=None, max_fine_opt=10, ranked=None, detail=False, matches=None):
        """CandidateManager driven by explicit hints (checkCandWithHint in the given order, tidyUpCandidates, fineOptimize).
        qdesc: torch uint8 CUDA [DESC_BYTES] of the query scan; hints: array of L.hint_dt (cand_gidx = DB index).
        Returns (cc_query_result_t record, per-hint L.hint_score_dt array); with ranked=K followed by (cands [1, K], counts [1]),
        and with detail=True by the [1, K] detail array, with matches=inlier_px by the [1, K] match array (see query())."""
        import torch
        qdesc = qdesc.reshape(-1)
        assert qdesc.is_cuda and qdesc.is_contiguous() and qdesc.numel() == DESC_BYTES
        r = calls.check_hints(lib(), self.h, qdesc.data_ptr(), hints, lb, ub, max_fine_opt, torch.cuda.current_stream(qdesc.device).cuda_stream,
                              ranked, detail, matches)
        return _ret(r.res[0], r.scores, r.rank, r.detail, r.match)

    def _verify(self, qdesc, cands, max_fine_opt, want_hints=False, **kw):
        """what verify() and verify_submit() share: the tensor checks, the stream, the device's hint lists, the call
        -> (calls.verify's record, the hint tensors or None)"""
        import torch
        skw, dev, stream = self._source(qdesc, rows=True)
        cands = calls.cand_table(cands)
        d_h = d_n = None
        if want_hints:
            d_h = torch.zeros((max(len(cands), 1), L.HINT_MAX, L.hint_dt.itemsize), dtype=torch.uint8, device=dev)
            d_n = torch.zeros(max(len(cands), 1), dtype=torch.int32, device=dev)
            kw.update(hints=d_h.data_ptr(), n_hints=d_n.data_ptr())
        r = calls.verify(lib(), self.h, cands, max_fine_opt=self.cfg.max_fine_opt if max_fine_opt is None else max_fine_opt, stream=stream,
                         **skw, **kw)
        return r, d_h, d_n

    def verify(self, qdesc, cands, qidx=None, levels=(1, 2, 3, 4), max_key_dist_sq=1000.0, lb=None, ub=None, max_fine_opt=None,
               want_hints=False, allow_flagged=False, ranked=None, detail=False, matches=None):
        """Score candidates the caller proposes, in one batch (cc_db_verify_batch).  qdesc: torch uint8 CUDA [n_desc, DESC_BYTES]
        -- or self.stored(idx) / Packed(hot, feat, idx): item i is record idx[i] (or qidx[i] of a source without idx), read from
        the packed records (cc_db_verify_submit_packed + the wait); an item may name a stored scan among its own candidates;
        cands: int array [n, <= 8] padded with -1, or a list of lists of DB indices; item i is descriptor qidx[i] (None: i)
        against cands[i].  The hint list of an item is generated on the device: every (candidate, level, candidate anchor,
        query anchor) whose keys are non-zero and at most max_key_dist_sq apart (float("inf"): no bound), candidate outermost.
        max_fine_opt: None = the database's.  Returns the cc_query_result_t array (cand_gidx is a DB index; n_knn_hits the number
        of hints), plus a list of L.hint_dt arrays, one per item, when want_hints is set.  allow_flagged: as for query().
        ranked=K: followed by (cands [n, K] of L.ranked_cand_dt, counts [n]) -- every refined candidate of an item, best first
        (cc_db_verify_submit_ranked), instead of one item per (query, candidate) pair.  Like query(ranked=K) it is the submit
        followed by the wait, so a large batch is chunked by the streamed rule (whole chunks), not one chunk per lane.
        detail=True (with ranked=K): followed by the [n, K] detail array as well (see query()).
        matches=inlier_px (with ranked=K): followed by the [n, K] match array as well (see query(); cc_db_verify_submit_matched)."""
        r, d_h, d_n = self._verify(qdesc, cands, max_fine_opt, want_hints, qidx=qidx, levels=levels, max_key_dist_sq=max_key_dist_sq, lb=lb, ub=ub,
                                   ranked=ranked, detail=detail, matches=matches, tolerate=(CC_ECAPACITY,) if allow_flagged else ())
        hints = None
        if want_hints:
            cnt = d_n.cpu().numpy()
            allh = d_h.cpu().numpy().view(L.hint_dt).reshape(-1, L.HINT_MAX)
            hints = [allh[i, :cnt[i]].copy() for i in range(len(r.res))]
        return _ret(r.res, hints, r.rank, r.detail, r.match)

    def verify_submit(self, qdesc, cands, qidx=None, levels=(1, 2, 3, 4), max_key_dist_sq=1000.0, lb=None, ub=None, max_fine_opt=None,
                      ranked=None, detail=False, matches=None):
        """Asynchronous form of verify(): queues the batch and returns the result array, which is only valid after query_wait()
        (cc_db_verify_submit; verify and query chunks share the lanes and are collected together).  ranked=K: returns
        (results, (cands [n, K], counts [n])), with detail=True followed by the [n, K] detail array.  qdesc may be self.stored(idx)
        or a Packed, as for verify().  matches=inlier_px: followed by the [n, K] match array."""
        r = self._verify(qdesc, cands, max_fine_opt, qidx=qidx, levels=levels, max_key_dist_sq=max_key_dist_sq, lb=lb, ub=ub,
                         ranked=ranked, detail=detail, matches=matches, wait=False, keep=self._held(qdesc))[0]
        return _ret(r.res, r.rank, r.detail, r.match)

    def _pose(self, qdesc, q, gidx, tf, **kw):
        """what score_poses() and score_poses_submit() share: the tensor checks, the stream, the call"""
        skw, _dev, stream = self._source(qdesc, rows=True)
        return calls.pose(lib(), self.h, q, gidx, tf, stream=stream, **skw, **kw)

    def score_poses(self, qdesc, q, gidx, tf, refine=True, min_corr=None, tries=None, curvature=False, allow_flagged=False):
        """Score, probe and refine relative poses the caller believes in, in one batch (cc_db_pose_batch: the reference's
        ConstellCorrelation::initProblem / tryProblem / calcCorrelation).  qdesc: torch uint8 CUDA [n_desc, DESC_BYTES], or
        self.stored() / Packed(hot, feat) -- q then names packed records (cc_db_pose_submit_packed + the wait); item i
        is descriptor q[i] (tgt) against database scan gidx[i] (src) at T_init = tf[i] = (x, y, theta) in BEV pixels / radians.
        refine: run the L-BFGS refinement on the items with pairs whose initial correlation is not below min_corr (None: the
        shipped lb.correlation, 0.3; -inf: every item that has pairs).  tries [n, T, 3], T <= L.POSE_TRY_MAX: further poses per
        item, evaluated over the pair set of T_init.  curvature: Hessian and gradient of -correlation at the returned pose.
        Returns (res [n] of L.pose_result_dt, try_corr [n, T] or None, curv [n] of L.pose_curv_dt or None); a refined row
        carries L.PF_REFINED in flags.  allow_flagged: as for query()."""
        r = self._pose(qdesc, q, gidx, tf, refine=refine, min_corr=min_corr, tries=tries, curvature=curvature,
                       tolerate=(CC_ECAPACITY,) if allow_flagged else ())
        return r.res, r.try_corr, r.curv

    def score_poses_submit(self, qdesc, q, gidx, tf, refine=True, min_corr=None, tries=None, curvature=False):
        """Asynchronous form of score_poses(): queues the batch and returns the same tuple, whose arrays are only valid after
        query_wait() (cc_db_pose_submit; pose chunks share the lanes with query and verify chunks and are collected together)."""
        r = self._pose(qdesc, q, gidx, tf, refine=refine, min_corr=min_corr, tries=tries, curvature=curvature, wait=False,
                       keep=self._held(qdesc))
        return r.res, r.try_corr, r.curv

    def debug_passes(self, cap=1152):
        """Constellations of the last check_hints call that passed all gates: numpy array of L.pass_dbg_dt."""
        out = np.zeros(cap, L.pass_dbg_dt)
        n = C.c_int()
        _chk(lib().cc_db_debug_passes(self.h, out.ctypes.data, cap, C.byref(n)), "cc_db_debug_passes")
        return out[:n.value]

    def debug_cands(self, cap=1152):
        """Every candidate of the last check_hints call as the merge left it, in first-appearance order: numpy array of
        L.cand_dbg_dt (cc_db_debug_cands, include/cont2_amd_cands.h)."""
        out = np.zeros(cap, L.cand_dbg_dt)
        n = C.c_int()
        _chk(lib().cc_db_debug_cands(self.h, out.ctypes.data, cap, C.byref(n)), "cc_db_debug_cands")
        return out[:n.value]

    def debug_key_view(self, layer):
        """The sorted key view of query layer `layer` as the last append left it (cc_db_debug_key_view, include/cont2_amd_keyview.h):
        (keys [11, n] -- ten rows of key entries and the |key|^2 row --, key ids [n], activation epochs [n]) in the view's order."""
        n = C.c_int32()
        z = np.zeros(L.KEY_DIM + 1, np.float32)
        rc = lib().cc_db_debug_key_view(self.h, int(layer), 0, z.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(n))  # cap 0: the size
        if rc != CC_ECAPACITY:
            _chk(rc, "cc_db_debug_key_view")
        cap = max(n.value, 1)
        keys, sid, sact = np.zeros((L.KEY_DIM + 1, cap), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        _chk(lib().cc_db_debug_key_view(self.h, int(layer), cap, keys.ctypes.data, sid.ctypes.data, sact.ctypes.data, C.byref(n)), "cc_db_debug_key_view")
        return keys[:, :n.value], sid[:n.value], sact[:n.value]

    def set_lanes(self, n):
        """1 = query chunks one after the other, 2 (default) = two 256-query chunks in flight on internal streams."""
        _chk(lib().cc_db_set_lanes(self.h, int(n)), "cc_db_set_lanes")

    def set_dynamic_thres(self, on):
        """The reference's DYNAMIC_THRES=1 build: True raises the bars from check to check (up to the ub thresholds) for every
        query submitted after the call; False (the default) keeps them constant."""
        _chk(lib().cc_db_set_dynamic_thres(self.h, 1 if on else 0), "cc_db_set_dynamic_thres")

    def bucket_state(self):
        sizes = np.zeros((3, 6), np.int32)
        ranges = np.zeros((3, 7), np.float32)
        _chk(lib().cc_db_bucket_state(self.h, sizes.ctypes.data, ranges.ctypes.data), "cc_db_bucket_state")
        return sizes, ranges
