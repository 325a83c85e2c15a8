"""The marshalling of the scoring flows of include/cont2_amd.h -- query, verify, check-hints, pose -- free of torch: one function
per flow prepares the host buffers, chooses the entry point, builds its argument tuple, calls it and (in the synchronous forms)
waits.  Every function takes the bound library (abi.bind) and the database handle; device memory arrives as integer addresses
or None, host arrays as numpy arrays, the stream as an integer or None.  Database (the package) and the CPU-harness drivers of
the test suite both sit on top of it; no caller needs the C argument order of an entry point.

wait=True is the synchronous form of the flow, wait=False leaves the batch in flight until cc_db_query_wait.  A submit may fail
with some of its chunks queued, and the library goes on writing into their buffers until the wait: a caller of a wait=False form
hands in `keep`, a list it holds until its wait, and the flow appends its buffers to it before the entry point is called.  Which
entry point runs is behaviour (a synchronous *_batch cuts one chunk per lane, a submit + wait whole chunks):
  query    descriptors: cc_db_query_batch (wait) / cc_db_query_submit; ranked: cc_db_query_submit_ranked[_detail];
           a record source: cc_db_query_submit_packed; a mask, either kind of query: cc_db_query_submit_masked;
           per-query lists of scans (include/cont2_amd_lists.h), with whatever else the call has: cc_db_query_submit_listed
  verify   descriptors: cc_db_verify_batch (wait) / cc_db_verify_submit; ranked: cc_db_verify_submit_ranked[_detail];
           a record source: cc_db_verify_submit_packed
  hints    cc_db_check_hints[_ranked[_detail]] (synchronous by itself)
  matches  (include/cont2_amd_matches.h) matches=inlier_px beside ranked=K on the three flows above: the flow's one *_matched entry
           point, which takes every other form's arguments (descriptors or a record source, a mask, the detail rows)
  pose     descriptors: cc_db_pose_batch (wait) / cc_db_pose_submit; a record source: cc_db_pose_submit_packed
Beside the scoring flows: ingest_images / scan_ingest_image, the calls of include/cont2_amd_images.h (descriptors from max-height images),
class_filter / range_filter / ingest_points_filtered / scan_ingest_points_filtered, those of include/cont2_amd_filter.h (records
dropped by a label, ring or intensity word of their own), and coord_src / ingest_coords / scan_ingest_coords, those of
include/cont2_amd_coords.h (f64, scaled-i32 and split-stream coordinates read in place)."""
import ctypes as C

import numpy as np

import layouts as L

CC_ECAPACITY = -4


class CCError(RuntimeError):
    rc = 0


def _error(what, rc, msg):
    e = CCError("%s failed (%d): %s" % (what, rc, msg))
    e.rc = rc
    return e


def chk(lib, rc, what, tolerate=()):
    if rc != 0 and rc not in tolerate:
        raise _error(what, rc, lib.cc_last_error().decode())
    return rc


class Out:
    """What a flow hands back: its host outputs by name (None where the form has none) and `keep`, every object the library
    reads or writes until the wait."""

    def __init__(self, keep, **outs):
        self.keep = keep
        self.__dict__.update(outs)


def _a(x):
    """the address of a numpy array or a ctypes structure; None stays NULL"""
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else C.addressof(x)


def _call(lib, db, fn, args, wait, tolerate, keep, held):
    """Call entry point `fn`, with `held` (what it reads and writes) registered in the caller's `keep` list first.  A submit with
    wait set is followed by the wait; a refused submit keeps its own message, and nothing of it may stay in flight."""
    if keep is not None:
        keep.append(held)
    rc = getattr(lib, fn)(*args)
    if not wait or fn.endswith("_batch"):  # left in flight, or synchronous by itself
        return chk(lib, rc, fn, tolerate)
    if rc != 0 and rc not in tolerate:
        msg = lib.cc_last_error().decode()
        lib.cc_db_query_wait(db)
        raise _error(fn, rc, msg)
    return chk(lib, lib.cc_db_query_wait(db), "cc_db_query_wait", tolerate)


def ingest_images(lib, ctx, height, pos_rc, n, min_height=None, out=None, dbg=None, stream=None, host=False, bev=None):
    """Descriptors from n max-height images (include/cont2_amd_images.h).  height / pos_rc / out: addresses (pos_rc may be None) --
    device ones for cc_ingest_images (dbg: the address of a cc_ingest_debug_t or None), host ones for host=True
    (cc_ingest_images_host; bev: the address of the host image output or None).  min_height: None or n host f32 values, copied by
    the library before it returns.  -> the return code (the caller checks it)"""
    mh = None
    if min_height is not None:
        mh = np.ascontiguousarray(np.asarray(min_height, np.float32).reshape(-1))
        if len(mh) != n:
            raise ValueError("min_height must hold one value per image: %d for %d images" % (len(mh), n))
    if host:
        return lib.cc_ingest_images_host(ctx, height, pos_rc, n, _a(mh), out, bev)
    return lib.cc_ingest_images(ctx, height, pos_rc, n, _a(mh), out, dbg, stream)


def scan_ingest_image(lib, ctx, height, pos_rc, min_height, want_bev, out_handle):
    """cc_scan_ingest_image: height / pos_rc host addresses (pos_rc may be None), min_height None or one value; out_handle: a
    ctypes c_void_p that receives the cc_scan.  -> the return code"""
    mh = None if min_height is None else np.asarray([min_height], np.float32)
    return lib.cc_scan_ingest_image(ctx, height, pos_rc, _a(mh), int(bool(want_bev)), C.byref(out_handle))


FILTER_WORDS = {"u8": (L.FILTER_U8, 8), "u16": (L.FILTER_U16, 16), "u32": (L.FILTER_U32, 32)}   # names of the class rule's word types -> (CC_FILTER_*, bits)


def class_filter(offset, dtype, keep=None, drop=None, n_classes=None, shift=0, mask=None, other="keep"):
    """The class rule of include/cont2_amd_filter.h -> (L.PointFilterC, its keep_bits array, which the struct points into): the record's
    word (dtype "u8" | "u16" | "u32" or the numpy dtype) at byte `offset`, class = (word >> shift) & mask (mask None: all ones); kept
    are the classes of `keep`, or all but those of `drop` (exactly one is given); n_classes defaults to the largest class named + 1,
    and a class at or beyond it is kept or dropped as other = "keep" | "drop" says."""
    name = dtype if isinstance(dtype, str) else {1: "u8", 2: "u16", 4: "u32"}.get(np.dtype(dtype).itemsize if np.dtype(dtype).kind == "u" else 0)
    if name not in FILTER_WORDS:
        raise ValueError("unknown class word %r (known: %s)" % (dtype, sorted(FILTER_WORDS)))
    if other not in ("keep", "drop"):
        raise ValueError('other must be "keep" or "drop"')
    if (keep is None) == (drop is None):
        raise ValueError("give exactly one of keep and drop")
    named = [int(v) for v in (keep if keep is not None else drop)]
    if n_classes is None:
        n_classes = max(named) + 1 if named else 1
    n_classes = int(n_classes)
    if not 1 <= n_classes <= L.FILTER_CLASSES_MAX:
        raise ValueError("n_classes must be 1 .. %d" % L.FILTER_CLASSES_MAX)
    bits = L.class_bits(n_classes, keep=None if keep is None else named, drop=None if drop is None else named)
    f = L.PointFilterC(int(offset), FILTER_WORDS[name][0], int(shift), 0xFFFFFFFF if mask is None else int(mask) & 0xFFFFFFFF, n_classes,
                       int(other == "keep"), 0.0, 0.0, bits.ctypes.data)
    return f, bits


def range_filter(offset, lo, hi):
    """The range rule: the record's f32 at byte `offset` is kept iff lo <= v <= hi (a NaN is dropped; lo / hi may be infinite)."""
    return L.PointFilterC(int(offset), L.FILTER_F32, 0, 0, 0, 0, float(lo), float(hi), None), None


def ingest_points_filtered(lib, ctx, points, layout, flt, offsets, tf=None, out=None, dbg=None, stream=None, host=False, bev=None):
    """cc_ingest_points_filtered / (host=True) cc_ingest_points_filtered_host.  points / out: addresses (device, or host with host=True);
    layout: an L.PointLayout or None; flt: an L.PointFilterC (or None: the library refuses it); offsets: int64 [n + 1]; tf: f32 [n, 12]
    or None; dbg: the address of a cc_ingest_debug_t (device form), bev: of the host image output (host form).  -> the return code"""
    n = len(offsets) - 1
    if host:
        return lib.cc_ingest_points_filtered_host(ctx, points, _a(layout), _a(flt), _a(offsets), n, _a(tf), out, bev)
    return lib.cc_ingest_points_filtered(ctx, points, _a(layout), _a(flt), _a(offsets), n, _a(tf), out, dbg, stream)


def scan_ingest_points_filtered(lib, ctx, points, layout, flt, n_points, tf, want_bev, out_handle):
    """cc_scan_ingest_points_filtered: points a host address, tf None or 12 f32; out_handle: a ctypes c_void_p that receives the cc_scan.
    -> the return code"""
    return lib.cc_scan_ingest_points_filtered(ctx, points, _a(layout), _a(flt), int(n_points), _a(tf), int(bool(want_bev)), C.byref(out_handle))


COORD_TYPES = {"float32": L.COORD_F32, "float64": L.COORD_F64, "int32": L.COORD_I32}   # dtype names -> CC_COORD_*


def coord_src(x, y, z, dtype, stride_bytes, scale=None):
    """A cc_coord_src_t (L.CoordSrc) from the addresses of the first point's x, y and z, the element dtype's name ("float32" |
    "float64" | "int32"; anything else is a ValueError) and the stride between points.  scale: 3 values (or one for all three),
    with "int32" only; None there means 1.0."""
    name = str(dtype).replace("torch.", "")
    if name not in COORD_TYPES:
        raise ValueError("coordinates must be float32, float64 or int32, not %s" % name)
    if scale is not None and name != "int32":
        raise ValueError("scale comes with int32 coordinates")
    sc = np.ones(3) if scale is None else np.broadcast_to(np.asarray(scale, np.float64).reshape(-1), (3,))
    return L.CoordSrc(x, y, z, COORD_TYPES[name], int(stride_bytes), (C.c_double * 3)(*[float(v) for v in sc]))


def _origin_tf(origin, tf, n):
    o = None if origin is None else np.ascontiguousarray(np.asarray(origin, np.float64).reshape(-1, 3))
    t = None if tf is None else np.ascontiguousarray(np.asarray(tf, np.float32).reshape(-1, 12))
    if (o is not None and len(o) != n) or (t is not None and len(t) != n):
        raise ValueError("origin must be [n, 3] and tf [n, 12] for the call's n = %d scans" % n)
    return o, t


def ingest_coords(lib, ctx, src, offsets, origin=None, tf=None, out=None, dbg=None, stream=None, host=False, bev=None):
    """cc_ingest_coords / (host=True) cc_ingest_coords_host.  src: an L.CoordSrc (or None: the library refuses it) whose streams
    are device addresses, or host ones with host=True; offsets: int64 [n + 1]; origin: f64 [n, 3] or None; tf: f32 [n, 12] or None;
    out: an address; dbg: the address of a cc_ingest_debug_t (device form), bev: of the host image output (host form).
    -> the return code"""
    n = len(offsets) - 1
    o, t = _origin_tf(origin, tf, n)
    if host:
        return lib.cc_ingest_coords_host(ctx, _a(src), _a(offsets), n, _a(o), _a(t), out, bev)
    return lib.cc_ingest_coords(ctx, _a(src), _a(offsets), n, _a(o), _a(t), out, dbg, stream)


def scan_ingest_coords(lib, ctx, src, n_points, origin, tf, want_bev, out_handle):
    """cc_scan_ingest_coords: src's streams are host addresses, origin None or 3 f64, tf None or 12 f32; out_handle: a ctypes
    c_void_p that receives the cc_scan.  -> the return code"""
    o, t = _origin_tf(origin, tf, 1)
    return lib.cc_scan_ingest_coords(ctx, _a(src), int(n_points), _a(o), _a(t), int(bool(want_bev)), C.byref(out_handle))


def detail_buffer(n, ranked, detail):
    """detail=True: the h_detail buffer of a *_ranked_detail call ([n, ranked] of L.ranked_detail_dt), else None"""
    if not detail:
        return None
    if ranked is None:
        raise ValueError("detail=True needs ranked=K: the detail rows belong to the entries of the ranked list")
    return L.rank_detail_buffer(n, ranked)


def _rank(n, ranked, detail):
    """-> ((cands, counts) or None, cc_rank_out_t or None, detail array or None)"""
    det = detail_buffer(n, ranked, detail)
    if ranked is None:
        return None, None, None
    cands, cnt, ro = L.rank_buffers(n, ranked)
    return (cands, cnt), ro, det


def _match(n, ranked, matches):
    """matches=inlier_px -> (rows [n, ranked] of L.ranked_match_dt, cc_match_out_t), else (None, None)"""
    if matches is None:
        return None, None
    if ranked is None:
        raise ValueError("matches=inlier_px needs ranked=K: the match rows belong to the entries of the ranked list")
    return L.match_buffers(n, ranked, matches)


def _ranked_fn(stem, ro, det):
    """the descriptor form's entry point with a ranked list (and detail), and the arguments it takes after the stream"""
    return stem + "_ranked" + ("_detail" if det is not None else ""), (_a(ro),) + (() if det is None else (_a(det),))


def query(lib, db, epochs, qdesc=None, src=None, idx=None, mask=None, lb=None, ub=None, knn=None, knn_cnt=None, stream=None,
          ranked=None, detail=False, matches=None, wait=True, tolerate=(), keep=None, among=None):
    """qdesc: the descriptors' address, or src: an L.PackedSrc with idx, its record selector (None: query i is record i).
    mask: (bits address, n_rows, row_words, int32 rows [nq]).  among: (int32 idx, int32 off [n_lists + 1], int32 rows [nq]), host
    arrays -- list r is idx[off[r] : off[r + 1]], query i names list rows[i] or -1; not together with mask.
    matches: inlier_px (with ranked).  -> Out(res, rank, detail, match)"""
    epochs = np.ascontiguousarray(epochs, np.int32).reshape(-1)
    nq = len(epochs)
    rk, ro, det = _rank(nq, ranked, detail) if ranked is not None or detail else (None, None, None)
    mt, mo = _match(nq, ranked, matches)
    if lb is None:
        lb, ub = L.default_thresholds()
    if idx is not None:
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        if len(idx) != nq:
            raise ValueError("the source names %d records for %d epochs" % (len(idx), nq))
    cm = None
    if mask is not None:
        bits, n_rows, row_words, rows = mask
        rows = np.ascontiguousarray(rows, np.int32).reshape(-1)
        if len(rows) != nq:
            raise ValueError("the mask names rows for %d queries, the call has %d" % (len(rows), nq))
        cm = L.ScanMaskC(bits, int(n_rows), int(row_words), rows.ctypes.data)
        mask = (rows, cm)
    cl = None
    if among is not None:
        if mask is not None:
            raise ValueError("give the scans that may answer as mask= or as among=, not both")
        l_idx, l_off, l_rows = (np.ascontiguousarray(a, np.int32).reshape(-1) for a in among)
        if len(l_rows) != nq:
            raise ValueError("the lists name rows for %d queries, the call has %d" % (len(l_rows), nq))
        if len(l_off) < 1 or (len(l_off) > 1 and int(l_off[-1]) > len(l_idx)):
            raise ValueError("off must hold n_lists + 1 offsets into idx (%d entries)" % len(l_idx))
        cl = L.ScanListsC(l_idx.ctypes.data, l_off.ctypes.data, len(l_off) - 1, l_rows.ctypes.data)
        among = (l_idx, l_off, l_rows, cl)
    res = np.zeros(nq, L.query_result_dt)
    mid = (nq, epochs.ctypes.data, C.addressof(lb), C.addressof(ub), res.ctypes.data, knn, knn_cnt, stream)
    if cl is not None:
        fn, args = "cc_db_query_submit_listed", (db, None if src is not None else qdesc, _a(src), _a(idx)) + mid + (_a(ro), _a(det), _a(cl), _a(mo))
    elif mo is not None:
        fn, args = "cc_db_query_submit_matched", (db, None if src is not None else qdesc, _a(src), _a(idx)) + mid + (_a(ro), _a(det), _a(cm), _a(mo))
    elif cm is not None:
        fn, args = "cc_db_query_submit_masked", (db, qdesc, _a(src), _a(idx)) + mid + (_a(ro), _a(det), _a(cm))
    elif src is not None:
        fn, args = "cc_db_query_submit_packed", (db, _a(src), _a(idx)) + mid + (_a(ro), _a(det))
    elif ranked is not None:
        fn, tail = _ranked_fn("cc_db_query_submit", ro, det)
        args = (db, qdesc) + mid + tail
    else:
        fn, args = "cc_db_query_batch" if wait else "cc_db_query_submit", (db, qdesc) + mid
    held = (src, idx, epochs, lb, ub, res, rk, ro, det, mask, mt, mo, among)
    _call(lib, db, fn, args, wait, tolerate, keep, held)
    return Out(held, res=res, rank=rk, detail=det, match=mt)


def cand_table(cands):
    """an int array [n, <= VERIFY_CANDS_MAX] padded with -1, or a list of lists -> int32 [n, VERIFY_CANDS_MAX] padded with -1"""
    if isinstance(cands, np.ndarray):
        rows = np.asarray(cands, np.int64).reshape(len(cands), -1)
    else:
        rows = [list(c) for c in cands]
    tab = np.full((len(rows), L.VERIFY_CANDS_MAX), -1, np.int32)
    for i, c in enumerate(rows):
        if len(c) > L.VERIFY_CANDS_MAX:
            if any(int(v) != -1 for v in c[L.VERIFY_CANDS_MAX:]):
                raise ValueError("item %d: more than VERIFY_CANDS_MAX = %d candidates" % (i, L.VERIFY_CANDS_MAX))
            c = c[:L.VERIFY_CANDS_MAX]
        tab[i, :len(c)] = c
    return tab


def level_mask(levels):
    """hint levels 1..4 -> cc_verify_cfg_t.level_mask; None: 0, which the library reads as all four"""
    if levels is None:
        return 0
    mask = 0
    for lv in levels:
        if not 1 <= int(lv) <= 4:
            raise ValueError("hint levels are 1..4")
        mask |= 1 << (int(lv) - 1)
    if mask == 0:
        raise ValueError("no hint level given")
    return mask


def verify(lib, db, cands, qdesc=None, n_desc=0, src=None, idx=None, qidx=None, levels=(1, 2, 3, 4), max_fine_opt=10, max_key_dist_sq=1000.0,
           lb=None, ub=None, hints=None, n_hints=None, stream=None, ranked=None, detail=False, matches=None, wait=True, tolerate=(), keep=None):
    """cands: see cand_table; item i is descriptor (or record) qidx[i] (None: i).  levels: see level_mask.  hints / n_hints: device addresses of the generated hint lists.
    matches: inlier_px (with ranked).  -> Out(res, rank, detail, match)"""
    if lb is None:
        lb, ub = L.default_thresholds()
    if src is not None:
        if idx is not None and qidx is not None:
            raise ValueError("name the records by the source's idx or by qidx, not both")
        qidx = idx if qidx is None else qidx
    tab = cand_table(cands)
    n = len(tab)
    if qidx is not None:
        qidx = np.ascontiguousarray(qidx, np.int32)
        if len(qidx) != n:
            raise ValueError("qidx must name one descriptor per item")
    cfg = L.VerifyCfg(level_mask(levels), int(max_fine_opt), float(max_key_dist_sq), 0)
    rk, ro, det = _rank(n, ranked, detail)
    mt, mo = _match(n, ranked, matches)
    res = np.zeros(n, L.query_result_dt)
    mid = (_a(qidx), _a(tab), n, _a(cfg), _a(lb), _a(ub), _a(res), hints, n_hints, stream)
    if mo is not None:
        fn, args = "cc_db_verify_submit_matched", (db, None if src is not None else qdesc, n_desc, _a(src)) + mid + (_a(ro), _a(det), _a(mo))
    elif src is not None:
        fn, args = "cc_db_verify_submit_packed", (db, _a(src)) + mid + (_a(ro), _a(det))
    elif ranked is not None:
        fn, tail = _ranked_fn("cc_db_verify_submit", ro, det)
        args = (db, qdesc, n_desc) + mid + tail
    else:
        fn, args = "cc_db_verify_batch" if wait else "cc_db_verify_submit", (db, qdesc, n_desc) + mid
    held = (src, qidx, tab, cfg, lb, ub, res, rk, ro, det, mt, mo)
    _call(lib, db, fn, args, wait, tolerate, keep, held)
    return Out(held, res=res, rank=rk, detail=det, match=mt)


def check_hints(lib, db, qdesc, hints, lb=None, ub=None, max_fine_opt=10, stream=None, ranked=None, detail=False, matches=None):
    """qdesc: the address of the query scan's descriptor; hints: array of L.hint_dt.  matches: inlier_px (with ranked).
    -> Out(res [1], scores, rank, detail, match)"""
    rk, ro, det = _rank(1, ranked, detail)
    mt, mo = _match(1, ranked, matches)
    if lb is None:
        lb, ub = L.default_thresholds()
    hints = np.ascontiguousarray(hints, L.hint_dt)
    res = np.zeros(1, L.query_result_dt)
    sc = np.zeros(len(hints), L.hint_score_dt)
    fn, tail = ("cc_db_check_hints", ()) if ranked is None else _ranked_fn("cc_db_check_hints", ro, det)
    if mo is not None:
        fn, tail = "cc_db_check_hints_matched", (_a(ro), _a(det), _a(mo))
    chk(lib, getattr(lib, fn)(db, qdesc, _a(hints), len(hints), _a(lb), _a(ub), int(max_fine_opt), _a(res), _a(sc), stream, *tail), fn)
    return Out((), res=res, scores=sc, rank=rk, detail=det, match=mt)


def pose(lib, db, q, gidx, tf, qdesc=None, n_desc=0, src=None, idx=None, refine=True, min_corr=None, tries=None, curvature=False,
         stream=None, wait=True, tolerate=(), keep=None):
    """Item i: descriptor (or record of src) q[i] against database scan gidx[i] at tf[i].  -> Out(res, try_corr, curv)"""
    if src is not None and idx is not None:
        raise ValueError("score_poses names the records by q: give the source without idx")
    q = np.asarray(q).reshape(-1)
    n = len(q)
    if len(np.asarray(gidx).reshape(-1)) != n or np.asarray(tf).size != 3 * n:
        raise ValueError("q, gidx and tf must name one item each: [n], [n] and [n, 3]")
    items = L.pose_items(q, gidx, tf)
    tr = tc = None
    nt = 0
    if tries is not None:
        tr = np.ascontiguousarray(tries, np.float64)
        if tr.ndim != 3 or tr.shape[0] != n or tr.shape[2] != 3:
            raise ValueError("tries must have shape [n, T, 3]")
        nt = tr.shape[1]
        tc = np.zeros((n, nt), np.float64)
    if min_corr is None:
        min_corr = L.default_thresholds()[0].correlation
    cfg = L.PoseCfg(int(refine), float(min_corr), nt, 0)
    res = np.zeros(n, L.pose_result_dt)
    cv = np.zeros(n, L.pose_curv_dt) if curvature else None
    tail = (_a(items), n, _a(cfg), _a(tr) if nt else None, _a(res), _a(tc) if nt else None, _a(cv), stream)
    if src is not None:
        fn, args = "cc_db_pose_submit_packed", (db, _a(src)) + tail
    else:
        fn, args = "cc_db_pose_batch" if wait else "cc_db_pose_submit", (db, qdesc, n_desc) + tail
    held = (src, items, tr, cfg, res, tc, cv)
    _call(lib, db, fn, args, wait, tolerate, keep, held)
    return Out(held, res=res, try_corr=tc, curv=cv)
