"""cc_ingest_points_motion and its siblings on the CPU harness: a sweep de-skewed by a per-point time word while it is rasterised.
The specified result is cc_ingest_batch's for the numpy-moved points (point_motion.apply_motion) in their original order -- so
every comparison is against the oracle on those points (bev, pix_rc, labels, descriptor float_exact) and, as bytes, against the
calls that exist; never against another run of the new code alone."""
import ctypes as C

import numpy as np
import pytest

from parity import compare_desc, terrain_scan
from point_layouts import apply_tf, border_scan, repack, rigid
from point_motion import (KNOTS_MAX, SWEEP, TIME_F32, TIME_U32, Motion, MotionApi, apply_motion, assert_ties_across_bins, bin_edge_inputs, cells,
                          random_knots, repack_with_time, tie_inputs, time_bins, u32_bits_as_f32)
from point_segments import Segments, SegmentsApi

# (stride, xyz_offset, time_offset, base_shift): 16- and 32-byte records (instances of their own), a time in front of xyz, a
# run-time stride, and a base at 4 mod 16
LAYOUTS = [(16, 0, 12, 0), (32, 0, 16, 0), (48, 8, 4, 0), (20, 0, 12, 0), (16, 0, 12, 4)]
CHUNK = 4096   # CC_K1_U_DEFAULT * CC_INGEST_BLOCK: the points of one chunk of the sweep


def _offs(scans):
    return np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)


def _oracle_check(oracle, moved, desc, dbg):
    for i, s in enumerate(moved):
        s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]   # (test_emu_point_layouts._oracle_check)
        o = oracle.Scan(s)
        ob, opix = o.bev()
        assert np.array_equal(ob, dbg["bev"][i]), "scan %d: bev" % i
        assert np.array_equal(opix, dbg["pix_rc"][i]), "scan %d: pix_rc" % i
        assert np.array_equal(o.labels(), dbg["labels"][i]), "scan %d: labels" % i
        bad = compare_desc(o.desc()[0], desc[i], float_exact=True)
        assert not bad, (i, bad[:10])


def _same(a, b, da=None, db=None):
    assert a.tobytes() == b.tobytes(), "descriptors differ"
    if da is not None:
        for k in ("bev", "pix_rc", "labels"):
            assert da[k].tobytes() == db[k].tobytes(), k


def _scans(n_scans, seed0=2):
    """9 001 + 8 i points: more than two 4 096-point chunks and a ragged tail"""
    return [terrain_scan(seed0 + i, n=9001 + 8 * i, scale=1.2 + 0.1 * (i % 5)) for i in range(n_scans)]


def _times(pattern, n, seed):
    """f32 times in [0, SWEEP) of n points"""
    rng = np.random.default_rng(seed)
    if pattern == "rising":
        return (np.arange(n, dtype=np.float32) * (SWEEP / np.float32(n))).astype(np.float32)
    if pattern == "random":
        return rng.uniform(0.0, float(SWEEP), n).astype(np.float32)
    # constant within runs that end in the middle of a wave (not at a multiple of 64) and in the middle of a chunk
    ends = [37, 100, 1000, CHUNK - 30, CHUNK + 21, 2 * CHUNK + 33, n]
    assert all(e % 64 for e in ends[:-1]) and all(e % CHUNK for e in ends[:-1])
    t = np.zeros(n, np.float32)
    lo = 0
    for e in ends:
        t[lo:e] = np.float32(rng.uniform(0.0, float(SWEEP)))
        lo = e
    return t


def _moved(scans, words, time_type, tb, sc, knots):
    return [apply_motion(s, w, time_type, tb[i], sc[i], knots[i]) for i, (s, w) in enumerate(zip(scans, words))]


@pytest.mark.parametrize("n_scans", [3, 9])  # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
@pytest.mark.parametrize("n_knots", [1, 2, 31, 64])
def test_layouts_and_launch_paths(oracle, n_scans, n_knots):
    scans = _scans(n_scans)
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    api = MotionApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    knots = random_knots(n_scans, n_knots, seed=n_knots)
    # every scan its own t_begin and scale: the bins cover the sweep
    tb = np.linspace(-0.01, 0.01, n_scans).astype(np.float32)
    sc = np.full(n_scans, np.float32(n_knots) / SWEEP, np.float32)
    for pattern in ("rising", "random", "runs"):
        words = [(_times(pattern, len(s), 11 + i) + tb[i]).astype(np.float32).view(np.uint32) for i, s in enumerate(scans)]
        bins = [time_bins(w, TIME_F32, tb[i], sc[i], n_knots) for i, w in enumerate(words)]
        assert all(len(np.unique(b)) >= min(n_knots, 4 if pattern == "runs" else n_knots) for b in bins), pattern
        if pattern == "random" and n_knots > 1:   # every wave mixes bins
            assert min(len(np.unique(bins[0][j:j + 64])) for j in range(0, 9001 - 64, 64)) >= 2
        moved = _moved(scans, words, TIME_F32, tb, sc, knots)
        ref, rdbg = api.ingest(ctx, np.concatenate(moved, 0), offs, debug=True)
        wcat = np.concatenate(words)
        for li, (stride, off, toff, shift) in enumerate(LAYOUTS):
            buf = repack_with_time(cat, wcat, stride, off, toff, base_shift=shift)
            assert buf.ctypes.data % 16 == shift
            mo = (toff, TIME_F32, n_knots)
            plain = api.ingest_motion(ctx, buf, (stride, off), mo, offs, tb, sc, knots)
            d, dbg = api.ingest_motion(ctx, buf, (stride, off), mo, offs, tb, sc, knots, debug=True)
            _same(plain, d)
            _same(ref, d, rdbg, dbg)
            if li == 0:
                _oracle_check(oracle, moved, d, dbg)


def test_bin_edges(oracle):
    """Times exactly on bin boundaries and 1 ulp either side, below t_begin, far above the end, +-inf, NaN, and a scale of 0: all
    follow the formula; bins 0 and K - 1 are reached by clamping and by NaN (asserted in point_motion.bin_edge_inputs)."""
    K = 16
    s = terrain_scan(21, n=9001, scale=1.3)
    w, tb, scale = bin_edge_inputs(len(s), K)
    knots = random_knots(2, K, seed=4)
    tbs, scs = np.array([tb, tb], np.float32), np.array([scale, 0.0], np.float32)   # scan 1: scale 0
    scans, words = [s, s], [w, w]
    moved = _moved(scans, words, TIME_F32, tbs, scs, knots)
    assert np.array_equal(moved[1], apply_tf(s, knots[1][0]))
    api = MotionApi(oracle.L)
    for rep in (1, 5):   # 2 scans: split sweep + merge kernel; 10: one workgroup per scan
        ctx = api.create(max_batch=2 * rep)
        cat, offs = np.concatenate(scans * rep, 0), _offs(scans * rep)
        buf = repack_with_time(cat, np.concatenate(words * rep), 32, 0, 16)
        d, dbg = api.ingest_motion(ctx, buf, (32, 0), (16, TIME_F32, K), offs, np.tile(tbs, rep), np.tile(scs, rep), np.tile(knots, (rep, 1, 1)),
                                   debug=True)
        _oracle_check(oracle, moved * rep, d, dbg)


def test_u32_times(oracle):
    """CC_TIME_U32: a t_begin close to 2^32 (the subtraction wraps) and differences above 2^24 (the conversion rounds)."""
    K = 31
    scans = _scans(3, seed0=41)
    rng = np.random.default_rng(8)
    tbu = np.array([0xFFFFFF00, 0xFFF00000, 12345], np.uint32)
    span = np.array([100_000_000, 99_999_999, 50_000_001], np.uint32)   # ns: far above 2^24
    words, tb, sc = [], np.zeros(3, np.float32), np.zeros(3, np.float32)
    for i, s in enumerate(scans):
        dt = rng.integers(0, int(span[i]), len(s)).astype(np.uint32)
        dt[:200] = np.uint32(span[i]) - rng.integers(1, 5, 200).astype(np.uint32)   # odd differences close to the end: they round
        words.append((tbu[i] + dt).astype(np.uint32))                     # wraps modulo 2^32
        tb[i] = u32_bits_as_f32(tbu[i])
        sc[i] = np.float32(K) / np.float32(span[i])
    assert tb.view(np.uint32).tolist() == tbu.tolist()
    assert (words[0] < tbu[0]).sum() > 8000 and (words[1] < tbu[1]).sum() > 5000, "the time words wrapped past 2^32"
    d0 = (words[0] - tbu[0])
    assert ((d0 > (1 << 24)) & (d0.astype(np.float32).astype(np.int64) != d0.astype(np.int64))).sum() > 1000, "differences that round"
    knots = random_knots(3, K, seed=6)
    moved = _moved(scans, words, TIME_U32, tb, sc, knots)
    assert all(len(np.unique(time_bins(w, TIME_U32, tb[i], sc[i], K))) == K for i, w in enumerate(words))
    api = MotionApi(oracle.L)
    ctx = api.create(max_batch=9)
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    buf = repack_with_time(cat, np.concatenate(words), 16, 0, 12)
    d, dbg = api.ingest_motion(ctx, buf, (16, 0), (12, TIME_U32, K), offs, tb, sc, knots, debug=True)
    _oracle_check(oracle, moved, d, dbg)
    # nine scans: one workgroup per scan, a 48-byte record with the time in front
    buf9 = repack_with_time(np.concatenate([cat] * 3, 0), np.concatenate(words * 3), 48, 8, 4)
    d9, dbg9 = api.ingest_motion(ctx, buf9, (48, 8), (4, TIME_U32, K), _offs(scans * 3), np.tile(tb, 3), np.tile(sc, 3), np.tile(knots, (3, 1, 1)),
                                 debug=True)
    _same(np.tile(d, 3), d9)
    for k in ("bev", "pix_rc", "labels"):
        assert np.concatenate([dbg[k]] * 3).tobytes() == dbg9[k].tobytes(), k


@pytest.mark.parametrize("n_rep", [1, 2])  # 6 scans: split sweep + merge kernel; 12: one workgroup per scan
def test_ties_across_bins(oracle, n_rep):
    """Equal moved heights in one cell from points of different bins: the FIRST point in file order owns the cell, whatever its time."""
    cfg = oracle.L.default_manager_cfg()
    scans, words, tb, sc, knots = tie_inputs(6)
    K = knots.shape[1]
    moved = _moved(scans, words, TIME_F32, tb, sc, knots)
    for s, m in zip(scans, moved):
        assert np.array_equal(m[:, :2], s[:, :2]) and len(np.unique(m[:, 2])) == 6
    assert_ties_across_bins(cfg, moved, words, tb, sc, K)
    scans, words, moved = scans * n_rep, words * n_rep, moved * n_rep
    api = MotionApi(oracle.L)
    ctx = api.create(max_batch=len(scans))
    buf = repack_with_time(np.concatenate(scans, 0), np.concatenate(words), 16, 0, 12)
    d, dbg = api.ingest_motion(ctx, buf, (16, 0), (12, TIME_F32, K), _offs(scans), np.tile(tb, n_rep), np.tile(sc, n_rep), np.tile(knots, (n_rep, 1, 1)),
                               debug=True)
    _oracle_check(oracle, moved, d, dbg)
    # the owner's continuous position is the one of the first point in file order at the cell's maximum
    m, c = moved[0], cells(cfg, moved[0])
    for cell in np.unique(c[c >= 0])[:20]:
        first = np.flatnonzero((c == cell) & (m[:, 2] == m[c == cell, 2].max()))[0]
        exp = np.array([m[first, 0] / np.float32(cfg.reso_row) + np.float32(cfg.n_row // 2) - np.float32(0.5),
                        m[first, 1] / np.float32(cfg.reso_col) + np.float32(cfg.n_col // 2) - np.float32(0.5)], np.float32)
        assert np.array_equal(dbg["pix_rc"][0][cell], exp), cell


@pytest.mark.parametrize("n_scans", [3, 9])
def test_against_the_paths_that_exist(oracle, n_scans):
    scans = _scans(n_scans, seed0=71)
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    api = mapi = _BothApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    rng = np.random.default_rng(3)
    t = rng.uniform(0.0, float(SWEEP), len(cat)).astype(np.float32)
    # K = 1: the bytes of cc_ingest_points with that matrix as h_tf
    k1 = random_knots(n_scans, 1, seed=12)
    tb, sc = np.zeros(n_scans, np.float32), np.full(n_scans, 10.0, np.float32)
    d, dbg = mapi.ingest_motion(ctx, repack_with_time(cat, t.view(np.uint32), 32, 0, 16), (32, 0), (16, TIME_F32, 1), offs, tb, sc, k1, debug=True)
    p, pdbg = api.ingest_points(ctx, repack(cat, 32, 0), (32, 0), offs, tf=k1[:, 0], debug=True)
    _same(p, d, pdbg, dbg)
    # identity knots: the bytes of the plain call
    ident = np.tile(rigid(0.0, dtype=np.float32).reshape(12), (n_scans, 8, 1))
    sc8 = np.full(n_scans, np.float32(8) / SWEEP, np.float32)
    d, dbg = mapi.ingest_motion(ctx, repack_with_time(cat, t.view(np.uint32), 16, 0, 12), (16, 0), (12, TIME_F32, 8), offs, tb, sc8, ident, debug=True)
    p, pdbg = api.ingest(ctx, cat, offs, debug=True)
    _same(p, d, pdbg, dbg)
    # the points sorted by bin, K = 8: the bytes of cc_ingest_segments with 8 segments
    k8 = random_knots(n_scans, 8, seed=13)
    sorted_scans, sorted_t, seg_scans = [], [], []
    for i, s in enumerate(scans):
        ti = t[offs[i]:offs[i + 1]]
        b = time_bins(ti.view(np.uint32), TIME_F32, tb[i], sc8[i], 8)
        order = np.argsort(b, kind="stable")
        s, ti, b = s[order], ti[order], b[order]
        sorted_scans.append(s)
        sorted_t.append(ti)
        seg_scans.append([(s[b == k], (16, 0), k8[i][k], 0) for k in range(8)])
        assert all(len(g[0]) > 100 for g in seg_scans[-1])
    scat, st = np.concatenate(sorted_scans, 0), np.concatenate(sorted_t)
    d, dbg = mapi.ingest_motion(ctx, repack_with_time(scat, st.view(np.uint32), 16, 0, 12), (16, 0), (12, TIME_F32, 8), offs, tb, sc8, k8, debug=True)
    g, gdbg = api.ingest_segments(ctx, Segments(seg_scans), debug=True)
    _same(g, d, gdbg, dbg)


class _BothApi(MotionApi, SegmentsApi):
    pass


def _accepted(cfg, s):
    x, y = s[:, 0], s[:, 1]
    half_r, half_c = cfg.n_row / 2 * cfg.reso_row, cfg.n_col / 2 * cfg.reso_col
    return (np.abs(x) < half_r) & (np.abs(y) < half_c) & (x * x + y * y >= cfg.blind_sq)


@pytest.mark.parametrize("n_scans", [2, 10])
def test_border_and_blind_zone(oracle, n_scans):
    """Knots that move points across the map's border both ways and into the blind disc: only the moved point counts."""
    cfg = oracle.L.default_manager_cfg()
    K = 4
    s = border_scan(7, n=9001)
    rng = np.random.default_rng(2)
    t = rng.uniform(0.0, float(SWEEP), len(s)).astype(np.float32)
    kn = np.stack([rigid(0.3, np.deg2rad(1.0), np.deg2rad(-2.0), (4.0, -3.0, 0.2), np.float32).reshape(12),
                   rigid(-0.2, t=(-5.0, 2.0, 0.0), dtype=np.float32).reshape(12),
                   rigid(0.0, dtype=np.float32).reshape(12),
                   rigid(1.0, t=(3.0, 4.0, -0.1), dtype=np.float32).reshape(12)])
    tb, sc = np.float32(0.0), np.float32(K) / SWEEP
    moved = apply_motion(s, t.view(np.uint32), TIME_F32, tb, sc, kn)
    a0, a1 = _accepted(cfg, s), _accepted(cfg, moved)
    r0, r1 = np.hypot(s[:, 0], s[:, 1]), np.hypot(moved[:, 0], moved[:, 1])
    assert (a0 & ~a1 & (r1 > 10)).sum() > 20 and (~a0 & a1 & (r0 > 10)).sum() > 20 and (a0 & ~a1 & (r1 < 2)).sum() > 5
    scans = [s] * n_scans
    api = MotionApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    buf = repack_with_time(np.concatenate(scans, 0), np.tile(t.view(np.uint32), n_scans), 20, 0, 12)
    d, dbg = api.ingest_motion(ctx, buf, (20, 0), (12, TIME_F32, K), _offs(scans), np.full(n_scans, tb), np.full(n_scans, sc),
                               np.tile(kn, (n_scans, 1, 1)), debug=True)
    _oracle_check(oracle, [moved] * n_scans, d, dbg)


def test_per_scan_call_host_call_and_refusals(oracle):
    K = 31
    scans = _scans(3, seed0=91)
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    rng = np.random.default_rng(5)
    t = rng.uniform(0.0, float(SWEEP), len(cat)).astype(np.float32)
    w = t.view(np.uint32)
    tb, sc = np.zeros(3, np.float32), np.full(3, np.float32(K) / SWEEP, np.float32)
    knots = random_knots(3, K, seed=14)
    moved = [apply_motion(s, w[offs[i]:offs[i + 1]], TIME_F32, tb[i], sc[i], knots[i]) for i, s in enumerate(scans)]
    exp = [oracle.Scan(m).desc()[0] for m in moved]
    api = MotionApi(oracle.L)
    ctx = api.create(max_batch=2)   # the batched calls below go in chunks of 2 + 1 scans
    buf = repack_with_time(cat, w, 48, 8, 4)
    lay, mo = (48, 8), (4, TIME_F32, K)
    ref, rdbg = api.ingest_motion(ctx, buf, lay, mo, offs, tb, sc, knots, debug=True)
    _oracle_check(oracle, moved, ref, rdbg)
    # the per-scan call, on the caller's own buffer
    for i in range(3):
        one = repack_with_time(scans[i], w[offs[i]:offs[i + 1]], 48, 8, 4, base_shift=4 * (i % 4))
        rc, d = api.scan_ingest_motion_rc(ctx, one, lay, mo, len(scans[i]), tb[i], sc[i], knots[i])
        assert rc == 0 and not compare_desc(exp[i], d, float_exact=True)
    # the host call, with a leading scan that is skipped
    rc, dh, bev = api.ingest_motion_host_rc(ctx, buf, lay, mo, offs[1:], tb[1:], sc[1:], knots[1:], want_bev=True)
    assert rc == 0
    for i in range(2):
        assert not compare_desc(exp[i + 1], dh[i], float_exact=True)
        assert np.array_equal(bev[i], rdbg["bev"][i + 1])

    # every refused input returns CC_EINVAL, names its entry point, and a following good call still gives the reference bytes
    bad_sc = sc.copy()
    bad_sc[2] = np.inf
    nan_sc = sc.copy()
    nan_sc[0] = np.nan
    cases = {
        "a layout cc_ingest_points refuses": dict(layout=(22, 0)),
        "time_offset not a multiple of 4": dict(motion=(6, TIME_F32, K)),
        "negative time_offset": dict(motion=(-4, TIME_F32, K)),
        "time word beyond the record": dict(motion=(48, TIME_F32, K)),
        "time word on x": dict(motion=(8, TIME_F32, K)),
        "time word on y": dict(motion=(12, TIME_F32, K)),
        "time word on z": dict(motion=(16, TIME_F32, K)),
        "time_type 2": dict(motion=(4, 2, K)),
        "time_type -1": dict(motion=(4, -1, K)),
        "no knots": dict(motion=(4, TIME_F32, 0)),
        "65 knots": dict(motion=(4, TIME_F32, KNOTS_MAX + 1)),
        "NULL motion": dict(motion=None),
        "NULL h_time": dict(t_begin=None),
        "NULL h_knots": dict(knots=None),
        "an infinite scale": dict(scale=bad_sc),
        "a NaN scale": dict(scale=nan_sc),
    }
    for what, over in cases.items():
        a = dict(layout=lay, motion=mo, t_begin=tb, scale=sc, knots=knots)
        a.update(over)
        rc, _, _ = api.ingest_motion_rc(ctx, buf, a["layout"], a["motion"], offs, a["t_begin"], a["scale"], a["knots"])
        assert rc == -1, what   # CC_EINVAL
        assert api.lib.cc_last_error().decode().startswith("cc_ingest_points_motion:"), what
        rc, _, _ = api.ingest_motion_host_rc(ctx, buf, a["layout"], a["motion"], offs, a["t_begin"], a["scale"], a["knots"])
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_points_motion_host:"), what
        if "scale" not in over:   # (the per-scan call brings one scan's numbers)
            rc, _ = api.scan_ingest_motion_rc(ctx, buf, a["layout"], a["motion"], len(scans[0]), None if a["t_begin"] is None else tb[0], sc[0],
                                              None if a["knots"] is None else knots[0])
            assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_points_motion:"), what
        assert api.ingest_motion(ctx, buf, lay, mo, offs, tb, sc, knots).tobytes() == ref.tobytes(), what
    rc, _ = api.scan_ingest_motion_rc(ctx, buf, lay, mo, len(scans[0]), tb[0], np.float32(np.inf), knots[0])
    assert rc == -1
    # 64 knots and a time word in the record's last 4 bytes are taken; so is a time right behind z
    k64 = random_knots(3, KNOTS_MAX, seed=15)
    sc64 = np.full(3, np.float32(KNOTS_MAX) / SWEEP, np.float32)
    m64 = [apply_motion(s, w[offs[i]:offs[i + 1]], TIME_F32, tb[i], sc64[i], k64[i]) for i, s in enumerate(scans)]
    for (toff, stride, off) in ((44, 48, 8), (20, 48, 8)):
        d = api.ingest_motion(ctx, repack_with_time(cat, w, stride, off, toff), (stride, off), (toff, TIME_F32, KNOTS_MAX), offs, tb, sc64, k64)
        for i in range(3):
            assert not compare_desc(oracle.Scan(m64[i]).desc()[0], d[i], float_exact=True)


def test_motion_struct_layout(cc):
    """the ctypes mirrors of cc_point_motion_t: 16 bytes (the header carries a static_assert of the same)"""
    for S in (Motion, cc.L.PointMotion):
        assert C.sizeof(S) == 16 and S.time_offset.offset == 0 and S.time_type.offset == 4 and S.n_knots.offset == 8
    assert cc.L.MOTION_KNOTS_MAX == KNOTS_MAX and (cc.L.TIME_F32, cc.L.TIME_U32) == (TIME_F32, TIME_U32)


def _pose(yaw, roll, pitch, t):
    return rigid(yaw, roll, pitch, t)


def test_motion_knots(oracle):
    api = MotionApi(oracle.L)
    pb = _pose(0.3, 0.01, -0.02, (5.0, -2.0, 0.1))
    pe = _pose(0.36, 0.03, -0.01, (6.4, -1.7, 0.15))
    ident = rigid(0.0).reshape(12)
    # equal poses give identity knots
    # (to 1e-7: R_b^T R_b in f64 is the identity to ~1e-16, rounded to f32 -- one f32 ulp of 1 is 1.2e-7)
    assert np.abs(api.motion_knots(pb, pb, ref=0.7, K=5) - ident.astype(np.float32)).max() < 1e-7
    for K in (1, 8, 32, 64):
        kn = api.motion_knots(pb, pe, ref=1.0, K=K).reshape(K, 3, 4)
        for k in range(K):   # every knot is orthonormal
            R = kn[k, :, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1.0) < 1e-6
        # with ref = (k + 0.5) / K knot k is the identity
        for k in (0, K // 2, K - 1):
            kk = api.motion_knots(pb, pe, ref=(k + 0.5) / K, K=K)[k]
            assert np.abs(kk.astype(np.float64) - ident).max() < 1e-7, (K, k)
    # the ends: T(0) = pose_begin and T(1) = pose_end (a single knot at s = 0.5 referred to s = 0 and s = 1 composes to the whole motion)
    def mat(m):
        return np.vstack([np.asarray(m, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    a = mat(api.motion_knots(pb, pe, ref=0.0, K=1)[0])   # T(0)^-1 T(.5)
    b = mat(api.motion_knots(pb, pe, ref=1.0, K=1)[0])   # T(1)^-1 T(.5)
    assert np.abs(a @ np.linalg.inv(b) - np.linalg.inv(mat(pb)) @ mat(pe)).max() < 1e-6
    try:
        from scipy.spatial.transform import Rotation, Slerp
    except ImportError:
        return
    K = 32
    slerp = Slerp([0.0, 1.0], Rotation.from_matrix(np.stack([pb[:, :3], pe[:, :3]])))
    kn = api.motion_knots(pb, pe, ref=1.0, K=K).reshape(K, 3, 4)
    for k in range(K):
        s = (k + 0.5) / K
        T = np.vstack([np.concatenate([slerp([s]).as_matrix()[0], ((1 - s) * pb[:, 3] + s * pe[:, 3]).reshape(3, 1)], 1), [0, 0, 0, 1]])
        exp = (np.linalg.inv(mat(pe)) @ T)[:3]
        assert np.abs(kn[k].astype(np.float64) - exp).max() < 1e-6, k
