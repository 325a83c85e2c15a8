"""numpy/ctypes mirrors of the POD layouts declared in include/cont2_amd.h.

Kept in one place so the host mirror, the tests and the bench all agree with the C header;
`check_sizes()` asserts the numpy itemsizes against the sizes compiled into the shared libraries.
"""
import ctypes as C
import numpy as np

NLEV, KEY_DIM, NPIV, NDIST = 6, 10, 6, 10
BCI_LAYERS, BCI_MAXPTS, MAXC, MAX_CELLS, NQLEV, KNN_MAX = 4, 40, 320, 22500, 3, 64
KNN_MAX_LARGE = 256  # nnk upper bound; a database with nnk > KNN_MAX returns hits [nq][NQLEV][NPIV][KNN_MAX_LARGE]

contour_dt = np.dtype([
    ("level", "<i2"), ("poi", "<i2", (2,)), ("cell_cnt", "<i2"),
    ("pos_mean", "<f4", (2,)), ("pos_cov", "<f4", (4,)), ("eig_vals", "<f4", (2,)),
    ("eig_vecs", "<f4", (4,)), ("eccen", "<f4"), ("vol3_mean", "<f4"), ("com", "<f4", (2,)),
    ("ecc_feat", "u1"), ("com_feat", "u1"), ("pad_", "u1", (2,))], align=True)
relpt_dt = np.dtype([("level", "i1"), ("seq", "i1"), ("bit_pos", "<i2"), ("r", "<f4"), ("theta", "<f4")], align=True)
bci_dt = np.dtype([
    ("dist_bin", "<u8", (BCI_LAYERS,)), ("piv_seq", "i1"), ("level", "i1"), ("n_pts", "u1"), ("n_segs", "u1"),
    ("segs", "<u2", (BCI_MAXPTS + 2,)), ("pts", relpt_dt, (BCI_MAXPTS,))], align=True)
scan_desc_dt = np.dtype([
    ("n_cont", "<i4", (NLEV,)), ("n_stored", "<i4", (NLEV,)), ("layer_cell_cnt", "<i4", (NLEV,)),
    ("max_bin_val", "<f4"), ("min_bin_val", "<f4"), ("n_pix", "<i4"), ("flags", "<i4"),
    ("keys", "<f4", (NLEV, NPIV, KEY_DIM)), ("bcis", bci_dt, (NLEV, NPIV)),
    ("cont", contour_dt, (NLEV, MAXC))], align=True)
HOT_LEVELS, NDIST = 4, 10
# cc_hot_desc_t: what the query path reads of a scan (levels 1..4): hot.X[l] = desc.X[l + 1]
hot_desc_dt = np.dtype([
    ("n_cont", "<i4", (HOT_LEVELS,)), ("layer_cell_cnt", "<i4", (HOT_LEVELS,)), ("flags", "<i4"), ("pad_", "<i4", (3,)),
    ("keys", "<f4", (HOT_LEVELS, NPIV, KEY_DIM)), ("cont", contour_dt, (HOT_LEVELS, NDIST)),
    ("bcis", bci_dt, (HOT_LEVELS, NPIV))], align=True)
assert hot_desc_dt.itemsize == 18448
knn_hit_dt = np.dtype([("gidx", "<i4"), ("level", "<i2"), ("seq", "<i2"), ("dist_sq", "<f4")], align=True)
query_result_dt = np.dtype([
    ("n_res", "<i4"), ("cand_gidx", "<i4"), ("correlation", "<f8"), ("tf", "<f8", (3,)),
    ("cand_aft_check1", "<i4"), ("cand_aft_check2", "<i4"), ("cand_aft_check3", "<i4"),
    ("n_cand_pose", "<i4"), ("n_cand_tidy", "<i4"), ("n_knn_hits", "<i4"), ("flags", "<i4"), ("pad_", "<i4")], align=True)
# the record before `flags` was added (tests/golden/query_fixture.npz stores it)
query_result_v1_dt = np.dtype([
    ("n_res", "<i4"), ("cand_gidx", "<i4"), ("correlation", "<f8"), ("tf", "<f8", (3,)),
    ("cand_aft_check1", "<i4"), ("cand_aft_check2", "<i4"), ("cand_aft_check3", "<i4"),
    ("n_cand_pose", "<i4"), ("n_cand_tidy", "<i4"), ("n_knn_hits", "<i4")], align=True)

assert contour_dt.itemsize == 76 and relpt_dt.itemsize == 12 and bci_dt.itemsize == 600
assert scan_desc_dt.itemsize == 169048, scan_desc_dt.itemsize
assert knn_hit_dt.itemsize == 12 and query_result_dt.itemsize == 72 and query_result_v1_dt.itemsize == 64, query_result_dt.itemsize
# cc_hint_t / cc_hint_score_t (cc_db_check_hints)
hint_dt = np.dtype([("cand_gidx", "<i4"), ("level", "i1"), ("seq_src", "i1"), ("seq_tgt", "i1"), ("pad", "i1")], align=True)
hint_score_dt = np.dtype([("i_ovlp_sum", "<i4"), ("i_ovlp_max_one", "<i4"), ("i_in_ang_rng", "<i4"), ("i_indiv_sim", "<i4"),
                          ("i_orie_sim", "<i4"), ("passed", "<i4")], align=True)
assert hint_dt.itemsize == 8 and hint_score_dt.itemsize == 24
HINT_MAX = NQLEV * NPIV * KNN_MAX  # CC_HINT_MAX: hints of one cc_db_check_hints call / of one item of cc_db_verify_*
VERIFY_CANDS_MAX = 8               # CC_VERIFY_CANDS_MAX: candidates per item (8 x 4 levels x 6 x 6 anchor pairs = HINT_MAX)
assert VERIFY_CANDS_MAX * 4 * NPIV * NPIV == HINT_MAX
# cc_ranked_cand_t / cc_rank_out_t (the *_ranked entry points): one refined candidate of a query's ranked list
RANK_MAX = 16  # CC_RANK_MAX
ranked_cand_dt = np.dtype([("cand_gidx", "<i4"), ("flags", "<i4"), ("correlation", "<f8"), ("tf", "<f8", (3,))], align=True)
assert ranked_cand_dt.itemsize == 40


class RankOut(C.Structure):  # cc_rank_out_t
    _fields_ = [("h_cands", C.c_void_p), ("h_n", C.c_void_p), ("max_ret", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(RankOut) == 24


def rank_buffers(n, max_ret):
    """(cands [n, max_ret] of ranked_cand_dt, counts [n] int32, RankOut pointing at them) for a *_ranked call of n queries"""
    cands = np.zeros((n, max(int(max_ret), 0)), ranked_cand_dt)
    cnt = np.zeros(n, np.int32)
    return cands, cnt, RankOut(cands.ctypes.data, cnt.ctypes.data, int(max_ret), 0)


# cc_ranked_detail_t (the *_ranked_detail entry points): curvature of f = -correlation at the entry's pose and what the device
# knows about its refinement; hess = (xx, xy, xt, yy, yt, tt)
ranked_detail_dt = np.dtype([("hess", "<f8", (6,)), ("grad", "<f8", (3,)), ("tf_init", "<f8", (3,)), ("corr_init", "<f8"),
                             ("iterations", "<i4"), ("termination", "<i4"), ("n_pairs", "<i4"), ("flags", "<i4")], align=True)
assert ranked_detail_dt.itemsize == 120


def rank_detail_buffer(n, max_ret):
    """[n, max_ret] of ranked_detail_dt: the h_detail argument of a *_ranked_detail call of n queries"""
    return np.zeros((n, max(int(max_ret), 0)), ranked_detail_dt)


def hess_matrix(h6):
    """the symmetric 3 x 3 matrix of a cc_ranked_detail_t.hess (xx, xy, xt, yy, yt, tt)"""
    h = np.asarray(h6, np.float64)
    return np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]])


# cc_ranked_match_t / cc_match_out_t (include/cont2_amd_matches.h): the matched contour pairs behind a ranked entry -- the selected
# proposal's constellation as a 400-bit set (bit (level-1)*100 + seq_src*10 + seq_tgt) and its residuals at the entry's pose
ranked_match_dt = np.dtype([("pairs", "<u8", (7,)), ("n_pairs", "<i4"), ("vote_cnt", "<i4"), ("n_props", "<i4"), ("area_perc", "<f4"),
                            ("res_rms", "<f8"), ("res_max", "<f8"), ("n_inlier", "<i4"), ("flags", "<i4")], align=True)
assert ranked_match_dt.itemsize == 96


class MatchOut(C.Structure):  # cc_match_out_t
    _fields_ = [("h_match", C.c_void_p), ("inlier_px", C.c_double)]


assert C.sizeof(MatchOut) == 16


def match_buffers(n, max_ret, inlier_px):
    """([n, max_ret] of ranked_match_dt, MatchOut pointing at it) for a *_matched call of n queries"""
    rows = np.zeros((n, max(int(max_ret), 0)), ranked_match_dt)
    return rows, MatchOut(rows.ctypes.data, float(inlier_px))


def match_pairs(row):
    """the pairs of one ranked_match_dt record in key order -> int8 [n_pairs, 3] of (level, seq_src, seq_tgt); what cc_match_pairs
    gives in C"""
    words = np.asarray(row["pairs"], np.uint64).reshape(7)
    bits = [w * 64 + b for w in range(7) for b in range(64) if (int(words[w]) >> b) & 1]
    return np.array([(b // 100 + 1, (b % 100) // 10, b % 10) for b in bits], np.int8).reshape(-1, 3)


# caller-given relative poses (cc_db_pose_*): cc_pose_item_t, cc_pose_result_t, cc_pose_curv_t, cc_pose_cfg_t
POSE_TRY_MAX = 8      # CC_POSE_TRY_MAX
PF_REFINED = 0x100    # CC_PF_REFINED
pose_item_dt = np.dtype([("q", "<i4"), ("gidx", "<i4"), ("tf", "<f8", (3,))], align=True)
pose_result_dt = np.dtype([("corr_init", "<f8"), ("correlation", "<f8"), ("tf", "<f8", (3,)), ("n_pairs", "<i4"), ("iterations", "<i4"),
                           ("termination", "<i4"), ("flags", "<i4"), ("pad_", "<i4", (2,))], align=True)
pose_curv_dt = np.dtype([("hess", "<f8", (6,)), ("grad", "<f8", (3,))], align=True)
assert pose_item_dt.itemsize == 32 and pose_result_dt.itemsize == 64 and pose_curv_dt.itemsize == 72


class PoseCfg(C.Structure):  # cc_pose_cfg_t
    _fields_ = [("refine", C.c_int32), ("min_corr", C.c_float), ("n_try", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(PoseCfg) == 16


def pose_items(q, gidx, tf):
    """[n] of pose_item_dt from the descriptor indices, the database scans and the start poses [n, 3]"""
    q = np.asarray(q, np.int32).reshape(-1)
    it = np.zeros(len(q), pose_item_dt)
    it["q"], it["gidx"] = q, np.asarray(gidx, np.int32).reshape(-1)
    it["tf"] = np.asarray(tf, np.float64).reshape(len(q), 3)
    return it


class PackedSrc(C.Structure):  # cc_packed_src_t (the *_submit_packed entry points): both pointers None = the database's own records
    _fields_ = [("d_hot", C.c_void_p), ("d_feat", C.c_void_p), ("n_rec", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(PackedSrc) == 24


class ScanMaskC(C.Structure):  # cc_scan_mask_t (the masked query forms): bit g & 31 of word g >> 5 of a row = scan g may answer
    _fields_ = [("bits", C.c_void_p), ("n_rows", C.c_int32), ("row_words", C.c_int32), ("h_row", C.c_void_p)]


assert C.sizeof(ScanMaskC) == 24 and ScanMaskC.n_rows.offset == 8 and ScanMaskC.row_words.offset == 12 and ScanMaskC.h_row.offset == 16


def pack_mask_rows(allowed, n_db=None, row_words=None):
    """allowed: a bool array [n_rows, n_db] or a list of index arrays (then n_db bounds the indices) -> uint32 [n_rows, row_words],
    bit g & 31 of word g >> 5 of row r set iff scan g is in row r's set; row_words defaults to ceil(n_db / 32), at least 1."""
    if isinstance(allowed, np.ndarray) and allowed.dtype == np.bool_:
        a = np.atleast_2d(allowed)
    else:
        rows = [np.asarray(r, np.int64).reshape(-1) for r in allowed]
        n = int(n_db) if n_db is not None else max([int(r.max()) + 1 for r in rows if len(r)] + [1])
        a = np.zeros((len(rows), n), np.bool_)
        for i, r in enumerate(rows):
            if len(r) and (r.min() < 0 or r.max() >= n):
                raise ValueError("row %d names a scan outside [0, %d)" % (i, n))
            a[i, r] = True
    n = a.shape[1]
    rw = max((n + 31) // 32, 1) if row_words is None else int(row_words)
    if 32 * rw < n:
        raise ValueError("row_words = %d holds fewer than %d scans" % (rw, n))
    pad = np.zeros((a.shape[0], 32 * rw), np.bool_)
    pad[:, :n] = a
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view("<u4").reshape(a.shape[0], rw))


LIST_SCANS_MAX = 1024  # CC_LIST_SCANS_MAX (include/cont2_amd_lists.h)


class ScanListsC(C.Structure):  # cc_scan_lists_t (the listed query forms): list r is h_idx[h_off[r] .. h_off[r + 1]), all host memory
    _fields_ = [("h_idx", C.c_void_p), ("h_off", C.c_void_p), ("n_lists", C.c_int32), ("h_row", C.c_void_p)]


assert C.sizeof(ScanListsC) == 32 and ScanListsC.h_off.offset == 8 and ScanListsC.n_lists.offset == 16 and ScanListsC.h_row.offset == 24


def gate_lists(xy, gates):
    """The scans within each gate's circle as index lists, on the host: cc_mask_gates' f32 expression as written --
    dx = x_g - x_r, dy = y_g - y_r, dx * dx + dy * dy <= rad_r * rad_r and rad_r >= 0; a NaN anywhere sets nothing -- so list r
    holds the set bits of Context.gate_mask's row r.  xy [n_scans, 2], gates [n_rows, 3] of (x, y, radius) -> (idx int32,
    off int32 [n_rows + 1])."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    gates = np.asarray(gates, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = xy[None, :, 0] - gates[:, None, 0]
        dy = xy[None, :, 1] - gates[:, None, 1]
        lhs = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
        rad = gates[:, None, 2]
        inside = (lhs <= (rad * rad).astype(np.float32)) & (rad >= 0)
    r, g = np.nonzero(inside)  # row-major: ascending scans within a row
    off = np.zeros(len(gates) + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=len(gates)), out=off[1:])
    return np.ascontiguousarray(g, np.int32), off


pass_dbg_dt = np.dtype([("hint", "<i4"), ("n_pairs", "<i4"), ("tf", "<f8", (3,)), ("pairs", "<u8", (7,))], align=True)
assert pass_dbg_dt.itemsize == 88
# cc_cand_dbg_t (include/cont2_amd_cands.h): a candidate of the last hint call as the merge left it
cand_dbg_dt = np.dtype([("cand_gidx", "<i4"), ("n_props", "<i4"), ("refined", "<i4"), ("pad_", "<i4"), ("tf_init", "<f8", (3,))], align=True)
assert cand_dbg_dt.itemsize == 40


class ManagerCfg(C.Structure):
    _fields_ = [("lv_grads", C.c_float * NLEV), ("reso_row", C.c_float), ("reso_col", C.c_float),
                ("n_row", C.c_int32), ("n_col", C.c_int32), ("lidar_height", C.c_float), ("blind_sq", C.c_float),
                ("min_cont_key_cnt", C.c_int32), ("min_cont_cell_cnt", C.c_int32), ("piv_firsts", C.c_int32),
                ("dist_firsts", C.c_int32), ("roi_radius", C.c_float), ("min_cell_cov", C.c_int32),
                ("point_sigma", C.c_float), ("com_bias_thres", C.c_float)]


class PointLayout(C.Structure):
    """cc_point_layout_t: where the three consecutive f32 (x, y, z) of a point sit.  (16, 0) KITTI, (12, 0) packed xyz."""
    _fields_ = [("stride_bytes", C.c_int32), ("xyz_offset", C.c_int32)]


SEG_MAX = 32  # CC_SEG_MAX: segments per scan of cc_ingest_segments


class PointSegment(C.Structure):
    """cc_point_segment_t: n_points records at `points` (layout {0, 0} stands for {16, 0}) with an optional row-major 3 x 4 matrix."""
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_int64), ("layout", PointLayout), ("has_tf", C.c_int32), ("pad_", C.c_int32),
                ("tf", C.c_float * 12)]


assert C.sizeof(PointSegment) == 80 and PointSegment.tf.offset == 32


MOTION_KNOTS_MAX = 64          # CC_MOTION_KNOTS_MAX: knot matrices per scan of cc_ingest_points_motion
TIME_F32, TIME_U32 = 0, 1      # CC_TIME_F32 / CC_TIME_U32


class PointMotion(C.Structure):
    """cc_point_motion_t: where a record's 4-byte time word sits, its type, and the number of knot matrices per scan."""
    _fields_ = [("time_offset", C.c_int32), ("time_type", C.c_int32), ("n_knots", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(PointMotion) == 16


FILTER_CLASSES_MAX = 4096                                     # CC_FILTER_CLASSES_MAX (include/cont2_amd_filter.h)
FILTER_U8, FILTER_U16, FILTER_U32, FILTER_F32 = 0, 1, 2, 3    # CC_FILTER_U8 / _U16 / _U32 / _F32


class PointFilterC(C.Structure):
    """cc_point_filter_t: the filter word of a record and the rule that keeps a record (class table or f32 band)."""
    _fields_ = [("offset", C.c_int32), ("type", C.c_int32), ("shift", C.c_int32), ("mask", C.c_uint32), ("n_classes", C.c_int32),
                ("keep_other", C.c_int32), ("lo", C.c_float), ("hi", C.c_float), ("keep_bits", C.c_void_p)]


assert C.sizeof(PointFilterC) == 40 and PointFilterC.lo.offset == 24 and PointFilterC.keep_bits.offset == 32


RIG_SEG_MAX = 16                              # CC_RIG_SEG_MAX (include/cont2_amd_rig.h): segments per scan of cc_ingest_rig
RIG_NONE, RIG_TF, RIG_MOTION = 0, 1, 2        # CC_RIG_NONE / _TF / _MOTION


class RigSegment(C.Structure):
    """cc_rig_segment_t: cc_point_segment_t's records with a mode (none, a matrix, or a time word and a slice of the scan's knot pool)
    and the byte offset of the segment's filter word (-1: not filtered)."""
    _fields_ = [("points", C.c_void_p), ("n_points", C.c_int64), ("layout", PointLayout), ("mode", C.c_int32), ("filter_offset", C.c_int32),
                ("tf", C.c_float * 12), ("time_offset", C.c_int32), ("time_type", C.c_int32), ("t_begin", C.c_float), ("scale", C.c_float),
                ("knot0", C.c_int32), ("n_knots", C.c_int32)]


assert C.sizeof(RigSegment) == 104 and RigSegment.tf.offset == 32 and RigSegment.time_offset.offset == 80


def class_bits(n_classes, keep=None, drop=None):
    """The keep_bits of a class rule: uint32 [(n_classes + 31) // 32] with bit c set iff class c is kept -- the classes of `keep`, or
    all but those of `drop` (exactly one of the two is given; every class named must be below n_classes)."""
    if (keep is None) == (drop is None):
        raise ValueError("give exactly one of keep and drop")
    named = np.asarray(list(keep if keep is not None else drop), np.int64).reshape(-1)
    if named.size and (named.min() < 0 or named.max() >= n_classes):
        raise ValueError("a class outside 0 .. n_classes - 1 = %d" % (n_classes - 1))
    kept = np.zeros(((n_classes + 31) // 32) * 32, bool)
    kept[:n_classes] = keep is None
    kept[named] = keep is not None
    return np.ascontiguousarray(np.packbits(kept, bitorder="little").view(np.uint32))


COORD_F32, COORD_F64, COORD_I32 = 0, 1, 2                     # CC_COORD_F32 / _F64 / _I32 (include/cont2_amd_coords.h)
COORD_BYTES = {COORD_F32: 4, COORD_F64: 8, COORD_I32: 4}


class CoordSrc(C.Structure):
    """cc_coord_src_t: three coordinate streams of one element type and one stride (scale: CC_COORD_I32 only)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("type", C.c_int32), ("stride_bytes", C.c_int32), ("scale", C.c_double * 3)]


assert C.sizeof(CoordSrc) == 56 and CoordSrc.type.offset == 24 and CoordSrc.stride_bytes.offset == 28 and CoordSrc.scale.offset == 32


RANGE_ROWS_MAX, RANGE_COLS_MAX = 128, 4096              # CC_RANGE_ROWS_MAX / CC_RANGE_COLS_MAX
RANGE_U16, RANGE_U32, RANGE_F32 = 0, 1, 2               # CC_RANGE_U16 / _U32 / _F32
RANGE_ROW_MAJOR, RANGE_COL_MAJOR = 0, 1                 # CC_RANGE_ROW_MAJOR / _COL_MAJOR


class RangeModel(C.Structure):
    """cc_range_model_t: a range sensor -- image shape, word type and storage order, the beam origin, the number of knots per scan
    and the host tables (row_tab [H][4]: cos(alt), sin(alt), cos(az_off), sin(az_off); col_cos_sin [W][2]; col_knot [W] or NULL)."""
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("word_type", C.c_int32), ("order", C.c_int32), ("range_scale", C.c_float),
                ("origin_n", C.c_float), ("origin_z", C.c_float), ("n_knots", C.c_int32), ("row_tab", C.c_void_p), ("col_cos_sin", C.c_void_p),
                ("col_knot", C.c_void_p)]


assert C.sizeof(RangeModel) == 56 and RangeModel.range_scale.offset == 16 and RangeModel.n_knots.offset == 28 and RangeModel.row_tab.offset == 32 \
    and RangeModel.col_knot.offset == 48


def range_tables(beam_alt, beam_az_off, col_az):
    """The sensor's angles (radians) -> (row_tab [H, 4], col_cos_sin [W, 2]) f32: computed in f64 and rounded to f32."""
    alt, off, az = (np.asarray(a, np.float64).reshape(-1) for a in (beam_alt, beam_az_off, col_az))
    if alt.shape != off.shape:
        raise ValueError("beam_alt and beam_az_off hold one angle per row")
    return (np.ascontiguousarray(np.stack([np.cos(alt), np.sin(alt), np.cos(off), np.sin(off)], 1).astype(np.float32)),
            np.ascontiguousarray(np.stack([np.cos(az), np.sin(az)], 1).astype(np.float32)))


class SimCfg(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ta_cell_cnt", "tp_cell_cnt", "tp_eigval", "ta_h_bar", "ta_rcom", "tp_rcom")]


class Score(C.Structure):
    _fields_ = [("i_ovlp_sum", C.c_int32), ("i_ovlp_max_one", C.c_int32), ("i_in_ang_rng", C.c_int32),
                ("i_indiv_sim", C.c_int32), ("i_orie_sim", C.c_int32), ("correlation", C.c_float),
                ("area_perc", C.c_float), ("neg_est_dist", C.c_float)]


class DbCfg(C.Structure):
    _fields_ = [("nnk", C.c_int32), ("max_fine_opt", C.c_int32), ("n_q_levels", C.c_int32),
                ("q_levels", C.c_int32 * NQLEV), ("cont_sim", SimCfg), ("max_elapse", C.c_double),
                ("min_elapse", C.c_double)]


class VerifyCfg(C.Structure):  # cc_verify_cfg_t
    _fields_ = [("level_mask", C.c_int32), ("max_fine_opt", C.c_int32), ("max_key_dist_sq", C.c_float), ("pad_", C.c_int32)]


assert C.sizeof(VerifyCfg) == 16


def default_manager_cfg(mulran=False):
    """Shipped values: config/batch_bin_test_config.yaml:27-47 (+ contour.h:32-37)."""
    c = ManagerCfg()
    grads = [1.0, 2.5, 4.0, 5.5, 7.0, 8.5] if mulran else [1.5, 2.0, 2.5, 3.0, 3.5, 4.0]
    for i, g in enumerate(grads):
        c.lv_grads[i] = g
    c.reso_row = c.reso_col = 1.0
    c.n_row = c.n_col = 150
    c.lidar_height, c.blind_sq = 2.0, 9.0
    c.min_cont_key_cnt, c.min_cont_cell_cnt, c.piv_firsts, c.dist_firsts = 9, 3, 6, 10
    c.roi_radius = 10.0
    c.min_cell_cov, c.point_sigma, c.com_bias_thres = 4, 1.0, 0.5
    return c


def default_db_cfg(mulran=False):
    """config/batch_bin_test_config.yaml:6-23."""
    d = DbCfg()
    d.nnk, d.max_fine_opt, d.n_q_levels = 50, 10, 3
    for i, q in enumerate([1, 2, 3]):
        d.q_levels[i] = q
    s = d.cont_sim
    s.ta_cell_cnt, s.tp_cell_cnt, s.tp_eigval = 6.0, 0.2, 0.2
    s.ta_h_bar = 0.75 if mulran else 0.3
    s.ta_rcom, s.tp_rcom = 0.4, 0.25
    d.max_elapse, d.min_elapse = 25.0, 15.0
    return d


def default_thresholds():
    """config/batch_bin_test_config.yaml:69-87."""
    lb, ub = Score(), Score()
    (lb.i_ovlp_sum, lb.i_ovlp_max_one, lb.i_in_ang_rng, lb.i_indiv_sim, lb.i_orie_sim) = (3, 3, 3, 3, 4)
    lb.correlation, lb.area_perc, lb.neg_est_dist = 0.3, 0.03, -5.01
    (ub.i_ovlp_sum, ub.i_ovlp_max_one, ub.i_in_ang_rng, ub.i_indiv_sim, ub.i_orie_sim) = (6, 6, 6, 6, 6)
    ub.correlation, ub.area_perc, ub.neg_est_dist = 0.75, 0.15, -5.0
    return lb, ub
