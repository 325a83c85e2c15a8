"""cc_ingest_points and its siblings on the CPU harness: points in packed-xyz and strided records, an optional per-scan 3 x 4
transform fused into the rasteriser's loads.  Descriptors are compared as bytes with cc_ingest_batch's for the float4 records,
and those with the oracle's (float_exact): the chain is pinned to the oracle, not to the code under test."""
import numpy as np
import pytest

from parity import compare_desc, terrain_scan
from point_layouts import PointsApi, apply_tf, border_scan, random_tfs, repack, rigid

LAYOUTS = [(12, 0), (32, 0), (48, 8), (16, 0)]


def _offs(scans):
    return np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)


def _oracle_check(oracle, scans, desc, dbg, cfg=None):
    for i, s in enumerate(scans):
        # a point with a NaN x or y is rejected by the library (cc_point_cell) and is undefined behaviour in the reference
        # (int(floor(NaN))): the oracle gets the scan without such points -- a rejected point changes nothing, the order stays
        s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]
        o = oracle.Scan(s, cfg=cfg)
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


def _ragged_scans(n_scans, seed0=2, n0=3001):
    """Point counts of 1 mod 4: consecutive 12-byte scans start at residues 0, 12, 8, 4 mod 16, one after the other."""
    return [terrain_scan(seed0 + i, n=n0 + 8 * i, scale=1.2 + 0.1 * (i % 5)) for i in range(n_scans)]


@pytest.mark.parametrize("n_scans", [3, 9])  # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
def test_layouts_give_the_float4_descriptor(oracle, n_scans):
    scans = _ragged_scans(n_scans)
    assert len({int(o) * 12 % 16 for o in _offs(scans)[:-1]}) == min(4, n_scans)
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    offs = _offs(scans)
    cat = np.concatenate(scans, 0)
    ref, rdbg = api.ingest(ctx, cat, offs, debug=True)
    _oracle_check(oracle, scans, ref, rdbg)
    for (stride, off) in LAYOUTS:
        buf = repack(cat, stride, off)
        plain = api.ingest_points(ctx, buf, (stride, off), offs)
        d, dbg = api.ingest_points(ctx, buf, (stride, off), offs, debug=True)
        _same(ref, plain)
        _same(ref, d, rdbg, dbg)
    # the default layout (NULL), and KITTI records that are only 4-byte aligned (the 16-byte loads are not for them)
    _same(ref, api.ingest_points(ctx, repack(cat, 16, 0), None, offs))
    _same(ref, api.ingest_points(ctx, repack(cat, 16, 0, base_shift=4), (16, 0), offs))
    _same(ref, api.ingest_points(ctx, repack(cat, 12, 0, base_shift=8), (12, 0), offs))


def _accepted(cfg, s):
    x, y = s[:, 0], s[:, 1]
    half_r, half_c = cfg.n_row / 2 * cfg.reso_row, cfg.n_col / 2 * cfg.reso_col
    return (np.abs(x) < half_r) & (np.abs(y) < half_c) & (x * x + y * y >= cfg.blind_sq)


@pytest.mark.parametrize("n_scans", [4, 10])
def test_transform_equals_oracle_on_numpy_transformed_points(oracle, n_scans):
    scans = _ragged_scans(n_scans - 2, seed0=31) + [border_scan(7), terrain_scan(44, n=3002, scale=1.4)]
    tfs = random_tfs(n_scans, seed=5)
    tfs[n_scans - 2] = rigid(0.3, np.deg2rad(1.0), np.deg2rad(-2.0), (4.0, -3.0, 0.2), np.float32).reshape(12)
    tfs[n_scans - 1] = rigid(0.0, dtype=np.float32).reshape(12)   # identity, passed explicitly
    moved = [apply_tf(s, m) for s, m in zip(scans, tfs)]
    # the border scan: the transform moves points across the map's border in both directions and into the blind disc
    cfg = oracle.L.default_manager_cfg()
    a0, a1 = _accepted(cfg, scans[-2]), _accepted(cfg, moved[-2])
    r0, r1 = np.hypot(scans[-2][:, 0], scans[-2][:, 1]), np.hypot(moved[-2][:, 0], moved[-2][:, 1])
    assert (a0 & ~a1 & (r1 > 10)).sum() > 20 and (~a0 & a1 & (r0 > 10)).sum() > 20 and (a0 & ~a1 & (r1 < 2)).sum() > 5
    assert np.array_equal(moved[-1][:, :3], scans[-1][:, :3])
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    offs = _offs(scans)
    cat = np.concatenate(scans, 0)
    first = None
    for (stride, off) in LAYOUTS:
        buf = repack(cat, stride, off)
        plain = api.ingest_points(ctx, buf, (stride, off), offs, tf=tfs)
        d, dbg = api.ingest_points(ctx, buf, (stride, off), offs, tf=tfs, debug=True)
        _same(plain, d)
        if first is None:
            _oracle_check(oracle, moved, d, dbg)
            first = (d, dbg)
        else:
            _same(first[0], d, first[1], dbg)
    # identity = the untransformed result
    plain = api.ingest(ctx, scans[-1], np.array([0, len(scans[-1])], np.int64))
    assert plain[0].tobytes() == first[0][-1].tobytes()


def test_edge_inputs(oracle):
    """The edge inputs of test_emu_ingest.py through the new loaders: the minimum size, every point rejected, equal heights
    in one cell (the FIRST point in file order owns the cell: what a re-ordered load would break), NaN coordinates."""
    tiny = np.zeros((11, 4), np.float32)
    far = np.full((40, 4), 1000.0, np.float32)
    ties = np.tile(np.array([[10.2, 3.3, 1.0, 0], [10.7, 3.9, 1.0, 0], [10.4, 3.1, 1.0, 0]], np.float32), (30, 1))
    rng = np.random.default_rng(5)
    crowd = np.zeros((6001, 4), np.float32)   # a few cells, hundreds of points each, heights on a 6-value lattice
    crowd[:, 0], crowd[:, 1] = rng.uniform(10.0, 16.0, 6001), rng.uniform(-3.0, 3.0, 6001)
    crowd[:, 2] = rng.integers(0, 6, 6001) * 0.5 - 1.0
    nans = terrain_scan(7, n=5003, scale=1.2)
    nans[::7, 2] = np.nan
    nans[3::11, 0] = np.nan
    nans[5::13, 1] = np.nan
    scans = [tiny, far, ties, crowd, nans]
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=len(scans))
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    ref, rdbg = api.ingest(ctx, cat, offs, debug=True)
    _oracle_check(oracle, scans, ref, rdbg)
    for (stride, off) in [(12, 0), (48, 8)]:
        d, dbg = api.ingest_points(ctx, repack(cat, stride, off), (stride, off), offs, debug=True)
        _same(ref, d, rdbg, dbg)
    # with a transform that keeps equal heights equal (yaw and a shift: z' = ((0 x + 0 y) + 1 z) + tz)
    tfs = np.stack([rigid(0.4 * i - 1.0, t=(0.5 * i, -0.3 * i, 0.25), dtype=np.float32).reshape(12) for i in range(len(scans))])
    moved = [apply_tf(s, m) for s, m in zip(scans, tfs)]
    assert len(np.unique(moved[3][:, 2])) == 6
    d, dbg = api.ingest_points(ctx, repack(cat, 12, 0), (12, 0), offs, tf=tfs, debug=True)
    _oracle_check(oracle, moved, d, dbg)
    d9, dbg9 = api.ingest_points(ctx, repack(np.concatenate(scans + scans, 0), 12, 0), (12, 0), _offs(scans + scans), tf=np.concatenate([tfs, tfs]),
                                 debug=True)   # ten scans: the one-workgroup-per-scan kernels
    _oracle_check(oracle, moved + moved, d9, dbg9)


def test_per_scan_and_host_calls(oracle):
    scans = _ragged_scans(3, seed0=61)
    tfs = random_tfs(3, seed=9)
    moved = [apply_tf(s, m) for s, m in zip(scans, tfs)]
    exp = [oracle.Scan(s).desc()[0] for s in moved]
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=4)
    # cc_scan_ingest_points: the caller's own buffer, packed xyz + transform
    for i in range(3):
        d = api.scan_ingest_points(ctx, repack(scans[i], 12, 0, base_shift=4 * (i % 4)), (12, 0), len(scans[i]), tf=tfs[i])
        assert not compare_desc(exp[i], d, float_exact=True)
    # cc_scan_ingest_points_batch: staged records of 32 bytes, one transform per scan
    db = api.scan_ingest_points_batch(ctx, [repack(s, 32, 0) for s in scans], (32, 0), tf=tfs)
    for i in range(3):
        assert not compare_desc(exp[i], db[i], float_exact=True)
    # ... and without layout and transform it is cc_scan_ingest_batch
    db = api.scan_ingest_points_batch(ctx, [repack(s, 16, 0) for s in scans], None)
    for i in range(3):
        assert not compare_desc(oracle.Scan(scans[i]).desc()[0], db[i], float_exact=True)
    # cc_ingest_points_host: host records with a leading scan that is skipped (offsets need not start at 0)
    cat = np.concatenate(scans, 0)
    offs = _offs(scans)
    dh, bev = api.ingest_points_host(ctx, repack(cat, 48, 8), (48, 8), offs[1:], tf=tfs[1:], want_bev=True)
    for i in range(2):
        assert not compare_desc(exp[i + 1], dh[i], float_exact=True)
        assert np.array_equal(bev[i], oracle.Scan(moved[i + 1]).bev()[0])


def test_refused_layouts_leave_the_context_usable(oracle):
    s = terrain_scan(3, n=3001)
    offs = np.array([0, len(s)], np.int64)
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=2)
    ref = api.ingest(ctx, s, offs)
    buf = repack(s, 64, 0)
    cases = {"stride not a multiple of 4": ((22, 0), buf.ctypes.data), "offset not a multiple of 4": ((32, 2), buf.ctypes.data),
             "xyz beyond the record": ((16, 8), buf.ctypes.data), "stride below 12": ((8, 0), buf.ctypes.data),
             "negative offset": ((16, -4), buf.ctypes.data), "stride above the cap": ((260, 0), buf.ctypes.data),
             "unaligned base": ((16, 0), buf.ctypes.data + 2)}
    for what, (lay, ptr) in cases.items():
        rc, _, _ = api.ingest_points_rc(ctx, ptr, lay, offs)
        assert rc == -1, what   # CC_EINVAL
        assert api.lib.cc_last_error(), what
        got = api.ingest_points(ctx, repack(s, 12, 0), (12, 0), offs)
        assert got.tobytes() == ref.tobytes(), what
    # the limits on a scan count points: 10 points of 48 bytes are still too few
    rc, _, _ = api.ingest_points_rc(ctx, repack(s[:10], 48, 8), (48, 8), np.array([0, 10], np.int64))
    assert rc == -1
    with pytest.raises(RuntimeError):
        api.scan_ingest_points(ctx, buf, (24, 2), len(s))
    assert api.ingest_points(ctx, repack(s, 256, 244), (256, 244), offs).tobytes() == ref.tobytes()   # the largest record taken


def test_call_larger_than_the_context_goes_in_chunks(oracle):
    """n_scans > max_batch: the call is worked off in chunks of max_batch scans -- the device copy of the transforms is reused per
    chunk and the point base advances by the chunk's first offset times the stride.  Packed xyz, a different transform per scan."""
    scans = _ragged_scans(7, seed0=81, n0=2001)
    tfs = random_tfs(7, seed=13)
    moved = [apply_tf(s, m) for s, m in zip(scans, tfs)]
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=3)   # chunks of 3, 3, 1
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    d, dbg = api.ingest_points(ctx, repack(cat, 12, 0), (12, 0), offs, tf=tfs, debug=True)
    _oracle_check(oracle, moved, d, dbg)
    d2 = api.ingest_points(ctx, repack(cat, 48, 8), (48, 8), offs, tf=tfs)
    _same(d, d2)


def test_errors_name_the_entry_point_that_was_called(oracle):
    s = terrain_scan(3, n=3001)
    api = PointsApi(oracle.L)
    ctx = api.create(max_batch=2)
    rc, _, _ = api.ingest_points_rc(ctx, repack(s[:10], 12, 0), (12, 0), np.array([0, 10], np.int64))
    assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_points:")
    with pytest.raises(RuntimeError, match="cc_scan_ingest_points:"):
        api.scan_ingest_points(ctx, repack(s, 12, 0), (22, 0), len(s))
    # a host buffer need not be aligned: the records are copied to device memory as they are
    buf = np.zeros(len(s) * 12 + 8, np.uint8)
    view = buf[(-buf.ctypes.data) % 4 + 1:][:len(s) * 12]
    view[:] = repack(s, 12, 0)
    assert view.ctypes.data % 4 == 1
    d = api.ingest_points_host(ctx, view, (12, 0), np.array([0, len(s)], np.int64))
    assert not compare_desc(oracle.Scan(s).desc()[0], d[0], float_exact=True)
