"""cc_ingest_segments and its siblings on the CPU harness: a scan as an ordered list of point segments, each with its own record
shape and its own 3 x 4 transform, swept in place by the rasteriser.  The specified result is cc_ingest_batch's for the cloud
Q = T_0(segment 0) ++ T_1(segment 1) ++ ... -- so every comparison is against the oracle on the numpy-built Q (bev, pix_rc, labels,
descriptor float_exact) AND, as bytes, against cc_ingest_batch on Q; never against another run of the new code alone."""
import ctypes as C

import numpy as np
import pytest

from parity import compare_desc, terrain_scan
from point_layouts import apply_tf, random_tfs, repack, rigid
from point_segments import SEG_MAX, Segment, Segments, SegmentsApi

LAYOUTS = [(12, 0), (16, 0), (32, 0), (48, 8)]
CHUNK = 4096        # CC_K1_U_DEFAULT * CC_INGEST_BLOCK: the points of one chunk of the sweep
K1_SPLIT = 8        # CC_K1_SPLIT ranges per scan for calls of <= CC_K1_SPLIT_MAX_SCANS = 8 scans


def _offs(clouds):
    return np.concatenate([[0], np.cumsum([len(s) for s in clouds])]).astype(np.int64)


def _check(oracle, api, ctx, segs, desc, dbg):
    """desc / dbg of a segments call against the oracle on Q and, as bytes, against cc_ingest_batch on Q: every scan, every field."""
    assert len(desc) == len(segs.q)
    for i, q in enumerate(segs.q):
        # a point with a NaN x or y is rejected by the library and undefined behaviour in the reference: the oracle gets Q without
        # such points (test_emu_point_layouts._oracle_check); the library gets them
        q = q[~(np.isnan(q[:, 0]) | np.isnan(q[:, 1]))]
        o = oracle.Scan(q)
        ob, opix = o.bev()
        assert np.array_equal(ob, dbg["bev"][i]), "scan %d: bev" % i
        assert np.array_equal(opix, dbg["pix_rc"][i]), "scan %d: pix_rc" % i
        assert np.array_equal(o.labels(), dbg["labels"][i]), "scan %d: labels" % i
        bad = compare_desc(o.desc()[0], desc[i], float_exact=True)
        assert not bad, (i, bad[:10])
    ref, rdbg = api.ingest(ctx, np.concatenate(segs.q, 0), _offs(segs.q), debug=True)
    assert ref.tobytes() == desc.tobytes(), "descriptors differ from cc_ingest_batch on Q"
    for k in ("bev", "pix_rc", "labels"):
        assert rdbg[k].tobytes() == dbg[k].tobytes(), k


def _cut(xyzi, cuts):
    """xyzi cut at the indices `cuts` (kept in order; equal neighbours give an empty part)"""
    e = [0] + list(cuts) + [len(xyzi)]
    return [xyzi[e[i]:e[i + 1]] for i in range(len(e) - 1)]


def _mixed_scans(n_scans, seed=3):
    """1 .. 5 segments per scan; layouts drawn from LAYOUTS within one scan; about half of the segments with a matrix; some bases at
    4 mod 16; empty segments first / in the middle / last in scans 0, 1, 2."""
    rng = np.random.default_rng(seed)
    tfs = random_tfs(5 * n_scans, seed=seed + 1)
    n_seg = [([5, 3, 1] + [2, 4, 5, 1, 3] * 2)[i] for i in range(n_scans)]
    scans, t = [], 0
    for i in range(n_scans):
        pts = terrain_scan(100 + 7 * i + seed, n=3001 + 8 * i, scale=1.2 + 0.1 * (i % 5))
        k = n_seg[i]
        cuts = sorted(int(c) for c in rng.integers(1, len(pts) - 1, k - 1))
        if i == 0:
            cuts[0], cuts[2] = 0, cuts[1]      # segment 0 and segment 2 (a middle one) are empty
        if i == 1:
            cuts[-1] = len(pts)                # the last segment is empty
        parts = _cut(pts, cuts)
        scan = []
        for j, part in enumerate(parts):
            lay = LAYOUTS[(i + j) % 4]
            tf = tfs[t] if (i + j) % 2 == 0 else None
            scan.append((part, lay if (i, j) != (2, 0) else None, tf, 4 if (i + j) % 3 == 0 else 0))
            t += 1
        scans.append(scan)
    assert [len(s) for s in scans] == n_seg and min(n_seg) == 1 and max(n_seg) == 5
    assert len(scans[0][0][0]) == 0 and len(scans[0][2][0]) == 0 and len(scans[1][-1][0]) == 0
    assert len({lay for (_p, lay, _t, _s) in scans[0]}) >= 3
    return scans


@pytest.mark.parametrize("n_scans", [3, 9])  # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
def test_mixed_segments(oracle, n_scans):
    segs = Segments(_mixed_scans(n_scans))
    assert any(b.ctypes.data % 16 == 4 for b in segs.bufs) and any(b.ctypes.data % 16 == 0 for b in segs.bufs)
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    plain = api.ingest_segments(ctx, segs)
    d, dbg = api.ingest_segments(ctx, segs, debug=True)
    assert plain.tobytes() == d.tobytes()
    _check(oracle, api, ctx, segs, d, dbg)


def _cells(cfg, q):
    """cell index (or -1) of every point of q, as cc_point_cell computes it at a power-of-two resolution"""
    x, y = q[:, 0], q[:, 1]
    hr, hc = cfg.n_row // 2, cfg.n_col // 2
    ok = (np.abs(x) <= hr * cfg.reso_row) & (np.abs(y) <= hc * cfg.reso_col) & ~(x * x + y * y < cfg.blind_sq)
    row = np.floor(x / cfg.reso_row).astype(np.int64) + hr
    col = np.floor(y / cfg.reso_col).astype(np.int64) + hc
    return np.where(ok & (row > 0), row * cfg.n_col + col, -1)


def _tied_cells(cfg, a, b):
    """cells whose maximum height (over a ++ b) is reached by a point of a AND by a point of b"""
    ca, cb = _cells(cfg, a), _cells(cfg, b)
    tied = []
    for c in np.intersect1d(ca[ca >= 0], cb[cb >= 0]):
        za, zb = a[ca == c, 2].max(), b[cb == c, 2].max()
        if za == zb:
            tied.append(int(c))
    return tied


def _crowd(seed, n=6001, z0=-1.0):
    rng = np.random.default_rng(seed)
    crowd = np.zeros((n, 4), np.float32)   # a few cells, hundreds of points each, heights on a 6-value lattice
    crowd[:, 0], crowd[:, 1] = rng.uniform(10.0, 16.0, n), rng.uniform(-3.0, 3.0, n)
    crowd[:, 2] = rng.integers(0, 6, n) * 0.5 + z0
    return crowd


@pytest.mark.parametrize("n_rep", [1, 2])  # 6 scans: split sweep + merge kernel; 12 scans: one workgroup per scan
def test_ties_across_segments(oracle, n_rep):
    """Equal heights in one cell, in two segments: the FIRST point of Q owns the cell, so the segment listed first wins; with the
    two segments swapped the owner changes, and both orders equal the oracle on their Q."""
    cfg = oracle.L.default_manager_cfg()
    ties = np.tile(np.array([[10.2, 3.3, 1.0, 0], [10.7, 3.9, 1.0, 0], [10.4, 3.1, 1.0, 0]], np.float32), (30, 1))
    t_a, t_b = ties[:46], ties[46:]          # the second part begins with another point of the cell than the first
    crowd = _crowd(5)
    c_a, c_b = crowd[:3000], crowd[3000:]
    # a tie that exists only AFTER the transform: heights on a binary lattice, the second segment 0.5 lower and lifted by t_z = 0.5
    # (z' = ((0 x + 0 y) + 1 z) + 0.5, exact in f32; x and y pass through a unit matrix unchanged)
    low = _crowd(6, z0=-1.5)
    l_a, l_b = _crowd(7)[:3000], low[3000:]
    lift = rigid(0.0, t=(0.0, 0.0, 0.5), dtype=np.float32).reshape(12)
    l_b_moved = apply_tf(l_b, lift)
    assert np.array_equal(l_b_moved[:, :2], l_b[:, :2]) and np.array_equal(l_b_moved[:, 2], l_b[:, 2] + np.float32(0.5))
    assert len(_tied_cells(cfg, t_a, t_b)) == 1
    assert len(_tied_cells(cfg, c_a, c_b)) >= 10
    assert len(_tied_cells(cfg, l_a, l_b)) == 0 and len(_tied_cells(cfg, l_a, l_b_moved)) >= 10
    pairs = [((t_a, (12, 0), None, 0), (t_b, (32, 0), None, 4)),
             ((c_a, (48, 8), None, 0), (c_b, (12, 0), None, 0)),
             ((l_a, (16, 0), None, 4), (l_b, (32, 0), lift, 0))]
    # a segment of other cells in front of each pair: the tied points' indices within Q are not their indices within their segments
    rng = np.random.default_rng(9)
    pre = np.zeros((700, 4), np.float32)
    pre[:, 0], pre[:, 1], pre[:, 2] = rng.uniform(-40.0, -20.0, 700), rng.uniform(-30.0, 30.0, 700), rng.uniform(-1.0, 3.0, 700)
    npre = len(pre)
    scans = []
    for (a, b) in pairs:
        scans += [[(pre, (16, 0), None, 0), a, b], [(pre, (12, 0), None, 4), b, a]]
    segs = Segments(scans * n_rep)
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=len(scans) * n_rep)
    d, dbg = api.ingest_segments(ctx, segs, debug=True)
    _check(oracle, api, ctx, segs, d, dbg)
    # the owner of a tied cell is the first segment's point: its continuous position is the one of the first point of that segment
    # at the cell's maximum, and it changes when the segments change places
    for k, (a, b) in enumerate(pairs):
        qa, qb = segs.q[2 * k], segs.q[2 * k + 1]
        na = len(a[0])
        changed = 0
        tied = _tied_cells(cfg, qa[npre:npre + na], qa[npre + na:])
        for c in tied:
            for (q, i) in ((qa, 2 * k), (qb, 2 * k + 1)):
                cq = _cells(cfg, q)
                first = np.flatnonzero((cq == c) & (q[:, 2] == q[cq == c, 2].max()))[0]
                exp = np.array([q[first, 0] / np.float32(cfg.reso_row) + np.float32(cfg.n_row // 2) - np.float32(0.5),
                                q[first, 1] / np.float32(cfg.reso_col) + np.float32(cfg.n_col // 2) - np.float32(0.5)], np.float32)
                assert np.array_equal(dbg["pix_rc"][i][c], exp), (k, c)
                assert npre <= first < (npre + na if q is qa else len(q) - na), "the owner lies in the first of the two segments"
            changed += not np.array_equal(dbg["pix_rc"][2 * k][c], dbg["pix_rc"][2 * k + 1][c])
        assert changed >= (1 if k == 0 else 10), (k, changed)


def _boundary_scan(seed, lengths, with_tf=True):
    pts = terrain_scan(seed, n=sum(lengths), scale=1.3)
    parts = _cut(pts, np.cumsum(lengths)[:-1])
    tfs = random_tfs(len(lengths), seed=seed)
    return [(p, LAYOUTS[j % 4], tfs[j] if (with_tf and j % 2) else None, 4 * (j % 2)) for j, p in enumerate(parts)]


@pytest.mark.parametrize("n_scans", [2, 9])
def test_segment_lengths_around_the_sweeps_strides(oracle, n_scans):
    """Segment lengths 1, 11, 4 095, 4 096, 4 097 (the sweep's chunk is 4 096 points), in several orders; on the split path the ends
    of the segments lie inside the ranges of the scan, not at their ends."""
    base = [1, 11, CHUNK - 1, CHUNK, CHUNK + 1]
    orders = [base, base[::-1]] + [list(np.roll(base, r)) for r in range(1, 5)] + [[CHUNK, 1, CHUNK + 1, 11, CHUNK - 1]] * 3
    scans = [_boundary_scan(40 + i, orders[i]) for i in range(n_scans)]
    for lens in orders[:n_scans]:
        total = sum(lens)
        per = (total + K1_SPLIT - 1) // K1_SPLIT
        range_ends = {min(k * per, total) for k in range(1, K1_SPLIT)}
        assert not (set(np.cumsum(lens)[:-1].tolist()) & range_ends), lens   # no segment ends where a range ends
    segs = Segments(scans)
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    d, dbg = api.ingest_segments(ctx, segs, debug=True)
    _check(oracle, api, ctx, segs, d, dbg)


@pytest.mark.parametrize("n_scans", [3, 9])
def test_one_segment_per_scan_is_cc_ingest_points(oracle, n_scans):
    clouds = [terrain_scan(60 + i, n=3001 + 8 * i, scale=1.2) for i in range(n_scans)]
    tfs = random_tfs(n_scans, seed=17)
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    for lay in [(12, 0), (48, 8)]:
        segs = Segments([[(c, lay, tfs[i], 0)] for i, c in enumerate(clouds)])
        d, dbg = api.ingest_segments(ctx, segs, debug=True)
        buf = repack(np.concatenate(clouds, 0), lay[0], lay[1])
        p, pdbg = api.ingest_points(ctx, buf, lay, _offs(clouds), tf=tfs, debug=True)
        assert d.tobytes() == p.tobytes()
        for k in ("bev", "pix_rc", "labels"):
            assert dbg[k].tobytes() == pdbg[k].tobytes(), k
    _check(oracle, api, ctx, segs, d, dbg)
    # ... and without a matrix, with the default layout ({0, 0} stands for {16, 0})
    segs = Segments([[(c, None, None, 0)] for c in clouds])
    assert api.ingest_segments(ctx, segs).tobytes() == api.ingest(ctx, np.concatenate(clouds, 0), _offs(clouds)).tobytes()


def test_host_call_and_per_scan_loop(oracle):
    segs = Segments(_mixed_scans(3, seed=11))
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=3)
    d, dbg = api.ingest_segments(ctx, segs, debug=True)
    _check(oracle, api, ctx, segs, d, dbg)
    dh, bev = api.ingest_segments_host(ctx, segs, want_bev=True)
    assert dh.tobytes() == d.tobytes() and bev.tobytes() == dbg["bev"].tobytes()
    assert api.ingest_segments_host(ctx, segs).tobytes() == d.tobytes()
    for i in range(3):
        ds, b = api.scan_ingest_segments(ctx, segs, i, want_bev=True)
        assert ds.tobytes() == d[i].tobytes() and b.tobytes() == dbg["bev"][i].tobytes(), i
        assert api.scan_ingest_segments(ctx, segs, i).tobytes() == d[i].tobytes(), i


def test_refusals_leave_the_context_usable(oracle):
    s = terrain_scan(3, n=3001)
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=2)
    good = Segments([[(s[:1000], (12, 0), None, 0), (s[1000:], (32, 0), None, 4)]])
    ref = api.ingest(ctx, good.q[0], np.array([0, len(s)], np.int64))
    buf = repack(s, 16, 0)
    many = Segments([[(s[100 * j:100 * (j + 1)], (16, 0), None, 0) for j in range(SEG_MAX + 1)]])
    ten = Segments([[(s[:4], (12, 0), None, 0), (s[4:4], (12, 0), None, 0), (s[4:10], (16, 0), None, 0)]])

    def raw(*entries):
        arr = (Segment * len(entries))()
        for g, (ptr, n, lay) in zip(arr, entries):
            g.points, g.n_points, g.layout.stride_bytes, g.layout.xyz_offset = ptr, n, lay[0], lay[1]
        return arr

    p = buf.ctypes.data
    cases = {
        "no segment": (good.arr, [0, 0]),
        "33 segments": (many.arr, [0, SEG_MAX + 1]),
        "a total of 10 points": (ten.arr, [0, 3]),
        # counts only: the pointers are far from any mapping -- nothing may be read before the check
        "a claimed total of 2^21": (raw((4096, 1 << 20, (16, 0)), (8192, 1 << 20, (16, 0))), [0, 2]),
        "a bad layout in the last segment": (raw((p, 2000, (16, 0)), (p, 1000, (22, 0))), [0, 2]),
        "xyz beyond the record in the last segment": (raw((p, 2000, (16, 0)), (p, 1000, (16, 8))), [0, 2]),
        "a pointer at 2 mod 4": (raw((p, 2000, (16, 0)), (p + 2, 1000, (16, 0))), [0, 2]),
        "NULL with points": (raw((p, 2000, (16, 0)), (None, 1000, (16, 0))), [0, 2]),
        "negative n_points": (raw((p, 2000, (16, 0)), (p, -1, (16, 0))), [0, 2]),
        "the second scan is refused": (raw((p, 2000, (16, 0)), (p, 5, (16, 0))), [0, 1, 2]),
    }
    for what, (arr, scan_segs) in cases.items():
        rc, _, _ = api.ingest_segments_rc(ctx, arr, scan_segs)
        assert rc == -1, what   # CC_EINVAL
        assert api.lib.cc_last_error().decode().startswith("cc_ingest_segments:"), what
        assert api.ingest_segments(ctx, good).tobytes() == ref.tobytes(), what
    # the host calls check the same things
    desc = np.zeros(1, oracle.L.scan_desc_dt)
    seg2 = np.array([0, 2], np.int32)
    arr = raw((p, 2000, (16, 0)), (p + 2, 1000, (16, 0)))
    assert api.lib.cc_ingest_segments_host(ctx, arr, C.c_void_p(seg2.ctypes.data), 1, C.c_void_p(desc.ctypes.data), None) == -1
    sc = C.c_void_p()
    assert api.lib.cc_scan_ingest_segments(ctx, arr, 2, 0, C.byref(sc)) == -1
    assert api.lib.cc_scan_ingest_segments(ctx, many.arr, SEG_MAX + 1, 0, C.byref(sc)) == -1
    assert api.lib.cc_scan_ingest_segments(ctx, good.arr, 0, 0, C.byref(sc)) == -1
    assert api.scan_ingest_segments(ctx, good, 0).tobytes() == ref[0].tobytes()
    # CC_SEG_MAX segments are taken
    full = Segments([[(s[90 * j:90 * (j + 1)], LAYOUTS[j % 4], None, 0) for j in range(SEG_MAX)]])
    d = api.ingest_segments(ctx, full)
    assert d.tobytes() == api.ingest(ctx, full.q[0], np.array([0, 90 * SEG_MAX], np.int64)).tobytes()


def test_call_larger_than_the_context_goes_in_chunks(oracle):
    segs = Segments(_mixed_scans(7, seed=23))
    api = SegmentsApi(oracle.L)
    ctx = api.create(max_batch=3)   # chunks of 3, 3, 1 scans: the segment table is staged per chunk
    d, dbg = api.ingest_segments(ctx, segs, debug=True)
    _check(oracle, api, ctx, segs, d, dbg)


def test_segment_struct_layout(cc):
    """the ctypes mirrors of cc_point_segment_t: 80 bytes, tf at offset 32 (the header carries a static_assert of the same)"""
    for S in (Segment, cc.L.PointSegment):
        assert C.sizeof(S) == 80 and S.tf.offset == 32 and S.n_points.offset == 8 and S.layout.offset == 16 and S.has_tf.offset == 24
    assert cc.L.SEG_MAX == SEG_MAX
