"""cc_ingest_ranges and its siblings on the CPU harness: a sensor's range image rasterised in place, de-skewed per column.  The
specified result is cc_ingest_batch's for the numpy restatement of the header's formula (range_images.restate) in pixel storage
order -- so every comparison is against cc_ingest_batch on those points, byte for byte, and against the oracle on them (bev, pix_rc,
labels, descriptor float_exact); never against another run of the new code alone."""
import ctypes as C

import numpy as np
import pytest

import cc_amd
from parity import compare_desc
from point_motion import random_knots
from range_images import (CHUNK, COLS_MAX, KNOTS_MAX, ROWS_MAX, RangeModel, RangesApi, Sensor, assert_shape_exercises_paths, cells, edge_words,
                          first_owner_positions, offsets, restate, restate_all, scene, tables, tie_scene)

# (H, W, order, word, range_scale)
# The first four are the shapes the feature was specified with.  Of those only 20 x 512 has boundaries of the split path's eight parts
# inside a storage row (16 x 601 and 8 x 1203 split into whole rows, 16 x 600 col-major into whole firings), so two more shapes, one per
# storage order, put every boundary inside a row.
SHAPES = [(16, 601, "row", "u32", 0.001), (20, 512, "row", "u16", 0.002), (16, 600, "col", "u16", 0.004), (8, 1203, "row", "f32", 1.0),
          (15, 641, "row", "f32", 1.0), (16, 601, "col", "u32", 0.001)]


def _synth():
    return cc_amd.load().synth


def _oracle_check(oracle, clouds, desc, dbg):
    for i, s in enumerate(clouds):
        s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]   # (rejected by the library, undefined behaviour in the reference)
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


_SCENES = {}


def _scene(oracle, si, n):
    """the shape's sensor (without knots) and n images, computed once"""
    if (si, n) not in _SCENES:
        H, W, order, word, scale = SHAPES[si]
        _SCENES[(si, n)] = scene(_synth(), oracle, H, W, order, word, scale, n=n, seed=si)
    return _SCENES[(si, n)]


def _assert_shapes_exercise_the_paths():
    """every shape has more than two 4 096-pixel chunks and a ragged tail; W is no multiple of 64 in three of the first four; part
    boundaries fall inside rows in 20 x 512 and, all seven of them, in the last two shapes (one per storage order)"""
    inside = [assert_shape_exercises_paths(Sensor(H, W, word, order, scale, np.zeros((H, 4)), np.zeros((W, 2)))) for (H, W, order, word, scale) in SHAPES]
    assert sum(1 for s in SHAPES[:4] if s[1] % 64 != 0) == 3
    assert inside[1] >= 4 and inside[4] == 7 and inside[5] == 7, inside
    assert SHAPES[4][2] == "row" and SHAPES[5][2] == "col"


@pytest.mark.parametrize("n_scans", [3, 9])  # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_shapes_and_launch_paths(oracle, si, n_scans):
    _assert_shapes_exercise_the_paths()
    base, images = _scene(oracle, si, n_scans)
    api = RangesApi(oracle.L)
    ctx = api.create(max_batch=n_scans)
    offs = offsets(n_scans, base)
    for K in ((0, 5, 1, 64) if si == 0 else (0, 5)):
        # the knot of a column: rising with the firing for K = 5 (a wave mostly shares one), scattered for K = 64 (every wave mixes them)
        col_knot = None if K == 0 else ((np.arange(base.W) * K // base.W) if K != 64 else (np.arange(base.W) * 37) % K).astype(np.int32)
        sensor = base.with_(K=K, col_knot=col_knot)
        knots = None if K == 0 else random_knots(n_scans, K, seed=10 + K, max_shift=3.0)
        clouds = restate_all(sensor, images, knots)
        ref, rdbg = api.ingest(ctx, np.concatenate(clouds, 0), offs, debug=True)
        h = api.sensor(ctx, sensor)
        plain = api.ingest_ranges(ctx, h, images, knots)
        d, dbg = api.ingest_ranges(ctx, h, images, knots, debug=True)
        api.sensor_destroy(h)
        _same(plain, d)            # with and without dbg the same descriptor
        _same(ref, d, rdbg, dbg)   # the bytes of cc_ingest_batch on the restated cloud
        if si == 0:
            _oracle_check(oracle, clouds, d, dbg)


@pytest.mark.parametrize("word", ["u16", "u32", "f32"])
def test_no_return_and_edge_words(oracle, word):
    """Integer words 0, 1, 65 535 and u32 words from 2^24 on (the conversion rounds); f32 words -1, -0.0, NaN, +inf, a subnormal: every
    word follows the formula, a rejected pixel counts nowhere; a no-return pixel directly in front of a cell's owner."""
    cfg = oracle.L.default_manager_cfg()
    si = {"u32": 0, "u16": 1, "f32": 4}[word]
    base, images = _scene(oracle, si, 3)
    images = images.copy()
    hw = base.H * base.W
    # scan 0: every third pixel an edge word; scan 1: the scene with a no-return pixel directly in front of cell owners
    ew = edge_words(word, hw)
    images[0][::3] = ew[::3]
    q1 = restate(base, images[1])
    c = cells(cfg, q1)
    owners = []
    for cell in np.unique(c[c >= 0])[:200]:
        m = np.flatnonzero(c == cell)
        f = m[np.argmax(q1[m, 2])]   # (argmax: the first of the maxima)
        if f > 0:
            owners.append(f)
    owners = np.array(owners)
    assert len(owners) > 100
    images[1][owners - 1] = 0
    api = RangesApi(oracle.L)
    for n_rep in (1, 3):   # 3 scans: split sweep + merge kernel; 9: one workgroup per scan
        ims = np.concatenate([images] * n_rep)
        clouds = restate_all(base, ims)
        none0 = np.isnan(clouds[0][:, 0])
        assert none0.sum() > hw // 15
        ctx = api.create(max_batch=len(ims))
        h = api.sensor(ctx, base)
        d, dbg = api.ingest_ranges(ctx, h, ims, debug=True)
        ref, rdbg = api.ingest(ctx, np.concatenate(clouds, 0), offsets(len(ims), base), debug=True)
        _same(ref, d, rdbg, dbg)
        _oracle_check(oracle, clouds[:3], d[:3], {k: v[:3] for k, v in dbg.items()})
        # rejected pixels count nowhere: n_pix, max / min height are those of the accepted points alone
        for i in (0, 1):
            q = clouds[i]
            cc_ = cells(cfg, q)
            acc = cc_ >= 0
            assert int(d[i]["n_pix"]) == len(np.unique(cc_[acc]))
            hts = np.float32(cfg.lidar_height) + q[acc, 2]
            assert d[i]["max_bin_val"] == hts.max() and d[i]["min_bin_val"] == hts.min()
        api.sensor_destroy(h)
    if word == "u32":
        # words of 2^24 .. 2^26 in micrometres (16 - 67 m): most are odd and their conversion rounds; the points land inside the map
        rng = np.random.default_rng(9)
        big = (rng.integers(1 << 24, 1 << 26, (3, hw)).astype(np.uint32) | np.uint32(1))
        big[rng.random((3, hw)) < 0.05] = 0
        assert (big.astype(np.float32).astype(np.int64) != big.astype(np.int64)).mean() > 0.5
        um = base.with_(range_scale=1e-6)
        clouds = restate_all(um, big)
        assert all((cells(cfg, q) >= 0).sum() > 1000 for q in clouds)
        ctx = api.create(max_batch=3)
        h = api.sensor(ctx, um)
        d, dbg = api.ingest_ranges(ctx, h, big, debug=True)
        ref, rdbg = api.ingest(ctx, np.concatenate(clouds, 0), offsets(3, um), debug=True)
        _same(ref, d, rdbg, dbg)
        _oracle_check(oracle, clouds, d, dbg)
        api.sensor_destroy(h)


@pytest.mark.parametrize("order", ["row", "col"])
def test_ties(oracle, order):
    """Equal heights in one cell from pixels of different columns and different knots: the pixel with the smaller storage index owns the cell."""
    cfg = oracle.L.default_manager_cfg()
    sensor, images, knots = tie_scene(cfg, order)
    api = RangesApi(oracle.L)
    for n_rep in (1, 3):   # both launch paths
        ims, kn = np.concatenate([images] * n_rep), np.concatenate([knots] * n_rep)
        clouds = restate_all(sensor, ims, kn)
        ctx = api.create(max_batch=len(ims))
        h = api.sensor(ctx, sensor)
        d, dbg = api.ingest_ranges(ctx, h, ims, kn, debug=True)
        api.sensor_destroy(h)
        ref, rdbg = api.ingest(ctx, np.concatenate(clouds, 0), offsets(len(ims), sensor), debug=True)
        _same(ref, d, rdbg, dbg)
        _oracle_check(oracle, clouds[:3], d[:3], {k: v[:3] for k, v in dbg.items()})
        for i in range(3):
            exp = first_owner_positions(cfg, clouds[i])
            assert len(exp) >= 10
            for cell, rc in exp.items():
                assert np.array_equal(dbg["pix_rc"][i][cell], rc), (i, cell)


def test_per_scan_and_host_calls(oracle):
    K = 5
    base, images = _scene(oracle, 1, 3)
    sensor = base.with_(K=K, col_knot=(np.arange(base.W) * K // base.W).astype(np.int32))
    knots = random_knots(3, K, seed=14, max_shift=3.0)
    api = RangesApi(oracle.L)
    ctx = api.create(max_batch=2)   # the batched calls below go in chunks of 2 + 1 scans
    for s, kn in ((sensor, knots), (base, None)):
        h = api.sensor(ctx, s)
        ref, rdbg = api.ingest_ranges(ctx, h, images, kn, debug=True)
        clouds = restate_all(s, images, kn)
        _oracle_check(oracle, clouds, ref, rdbg)
        for i in range(3):
            rc, d = api.scan_ingest_ranges_rc(ctx, h, images[i], None if kn is None else kn[i])
            assert rc == 0 and not compare_desc(ref[i], d, float_exact=True)
            assert not compare_desc(oracle.Scan(clouds[i][~np.isnan(clouds[i][:, 0])]).desc()[0], d, float_exact=True)
        rc, dh, bev = api.ingest_ranges_host_rc(ctx, h, images, 3, kn, want_bev=True)
        assert rc == 0
        for i in range(3):
            assert not compare_desc(ref[i], dh[i], float_exact=True)
            assert np.array_equal(bev[i], rdbg["bev"][i])
        api.sensor_destroy(h)


def test_validation(oracle):
    """every refused input returns CC_EINVAL and names its entry point; afterwards the context still ingests"""
    base, images = _scene(oracle, 1, 3)
    K = 4
    good = base.with_(K=K, col_knot=(np.arange(base.W) % K).astype(np.int32))
    knots = random_knots(3, K, seed=3)
    api = RangesApi(oracle.L)
    ctx = api.create(max_batch=3)
    h = api.sensor(ctx, good)
    ref = api.ingest_ranges(ctx, h, images, knots)
    _same(ref, api.ingest(ctx, np.concatenate(restate_all(good, images, knots), 0), offsets(3, good)))
    bad_knot_hi, bad_knot_lo = good.col_knot.copy(), good.col_knot.copy()
    bad_knot_hi[7], bad_knot_lo[-1] = K, -1

    def m(**over):
        mod, keep = good.model()
        for k, v in over.items():
            setattr(mod, k, v)
        return mod, keep

    big_cs = np.zeros((COLS_MAX + 1, 2), np.float32)
    big_rows = np.zeros((ROWS_MAX + 1, 4), np.float32)
    models = {
        "no rows": m(n_rows=0),
        "129 rows": m(n_rows=ROWS_MAX + 1, row_tab=big_rows.ctypes.data),
        "no columns": m(n_cols=0),
        "4097 columns": m(n_cols=COLS_MAX + 1, col_cos_sin=big_cs.ctypes.data, col_knot=None),
        "10 pixels": m(n_rows=1, n_cols=10),
        "word_type 3": m(word_type=3),
        "word_type -1": m(word_type=-1),
        "order 2": m(order=2),
        "an infinite range_scale": m(range_scale=float("inf")),
        "a NaN origin_n": m(origin_n=float("nan")),
        "an infinite origin_z": m(origin_z=float("-inf")),
        "K = -1": m(n_knots=-1),
        "K = 65": m(n_knots=KNOTS_MAX + 1),
        "a col_knot of K": m(col_knot=bad_knot_hi.ctypes.data),
        "a negative col_knot": m(col_knot=bad_knot_lo.ctypes.data),
        "a col_knot of 1 with K = 0": m(n_knots=0),
        "NULL row_tab": m(row_tab=None),
        "NULL col_cos_sin": m(col_cos_sin=None),
    }
    for what, (mod, keep) in models.items():
        rc, _ = api.sensor_rc(ctx, model=mod)
        assert rc == -1, what   # CC_EINVAL
        assert api.lib.cc_last_error().decode().startswith("cc_range_sensor_create:"), what
    assert api.lib.cc_range_sensor_create(ctx, None, C.byref(C.c_void_p())) == -1
    # accepted at the limits: 11 pixels, 128 x 4096 (2^19 pixels: with these limits on rows and columns no image reaches the 2^21 a
    # scan's index field ends at), K = 64 and K = 0 with a NULL col_knot
    for mod, keep in (m(n_rows=1, n_cols=11), m(n_rows=128, n_cols=4096, row_tab=big_rows.ctypes.data, col_cos_sin=big_cs.ctypes.data, col_knot=None),
                      m(n_knots=KNOTS_MAX), m(n_knots=0, col_knot=None)):
        rc, hh = api.sensor_rc(ctx, model=mod)
        assert rc == 0, api.lib.cc_last_error()
        api.sensor_destroy(hh)
    # the calls
    ctx2 = api.create(max_batch=3)
    h0 = api.sensor(ctx, base)          # K = 0
    h_other = api.sensor(ctx2, good)    # another context's sensor
    odd = images.ctypes.data + 1        # u16 words at an odd address
    calls = {
        "NULL sensor": dict(h=None),
        "NULL ranges": dict(images=None),
        "NULL h_knots with K = 4": dict(knots=None),
        "h_knots with K = 0": dict(h=h0),
        "a misaligned base": dict(ptr=odd),
        "another context's sensor": dict(h=h_other),
    }
    for what, over in calls.items():
        a = dict(h=h, images=images, knots=knots, ptr=None)
        a.update(over)
        rc, _, _ = api.ingest_ranges_rc(ctx, a["h"], a["images"], 3, a["knots"], ptr=a["ptr"])
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_ranges:"), what
        rc, _, _ = api.ingest_ranges_host_rc(ctx, a["h"], a["images"], 3, a["knots"], ptr=a["ptr"])
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_ranges_host:"), what
        rc, _ = api.scan_ingest_ranges_rc(ctx, a["h"], a["images"], None if a["knots"] is None else a["knots"][0], ptr=a["ptr"])
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_ranges:"), what
        assert api.ingest_ranges(ctx, h, images, knots).tobytes() == ref.tobytes(), what
    for hh in (h, h0, h_other):
        api.sensor_destroy(hh)


def test_range_model_layout(cc):
    """the ctypes mirrors of cc_range_model_t: 56 bytes (the header carries a static_assert of the same)"""
    for S in (RangeModel, cc.L.RangeModel):
        assert C.sizeof(S) == 56 and S.n_rows.offset == 0 and S.order.offset == 12 and S.range_scale.offset == 16 and S.origin_z.offset == 24
        assert S.n_knots.offset == 28 and S.row_tab.offset == 32 and S.col_cos_sin.offset == 40 and S.col_knot.offset == 48
    assert (cc.L.RANGE_ROWS_MAX, cc.L.RANGE_COLS_MAX) == (ROWS_MAX, COLS_MAX)
    assert (cc.L.RANGE_U16, cc.L.RANGE_U32, cc.L.RANGE_F32, cc.L.RANGE_ROW_MAJOR, cc.L.RANGE_COL_MAJOR) == (0, 1, 2, 0, 1)
    for sym in ("cc_range_sensor_create", "cc_range_sensor_destroy", "cc_ingest_ranges", "cc_ingest_ranges_host", "cc_scan_ingest_ranges"):
        assert sym in cc.EXPORTS


def test_python_binding_arguments(cc):
    """range_sensor's argument handling, as far as it goes without a device: names, shapes, the f64 -> f32 tables"""
    alt, off, az = np.deg2rad(np.linspace(10, -10, 8)), np.deg2rad(np.linspace(-1, 1, 8)), np.arange(100) * (2 * np.pi / 100)
    mod, (row_tab, col_cs, knot) = cc._range_model(8, 100, "u32", "col", 0.001, alt, off, az, (0.03, 0.04), np.arange(100) % 3, 3)
    rt, cs = tables(alt, off, az)
    assert np.array_equal(row_tab, rt) and np.array_equal(col_cs, cs) and row_tab.dtype == np.float32
    assert np.array_equal(row_tab[:, 0], np.cos(alt).astype(np.float32))   # f64 first, then rounded
    assert (mod.n_rows, mod.n_cols, mod.word_type, mod.order, mod.n_knots) == (8, 100, 1, 1, 3)
    assert mod.range_scale == np.float32(0.001) and mod.origin_n == np.float32(0.03) and mod.origin_z == np.float32(0.04)
    assert knot.dtype == np.int32 and mod.col_knot == knot.ctypes.data and mod.row_tab == row_tab.ctypes.data
    mod0, keep0 = cc._range_model(8, 100, "u16", "row", 0.002, alt, None, az, (0.0, 0.0), None, 0)
    assert mod0.col_knot is None and np.array_equal(keep0[0][:, 2:], np.tile(np.float32([1, 0]), (8, 1)))
    for bad in (dict(word="u8"), dict(order="z"), dict(alt=alt[:7]), dict(az=az[:99]), dict(knot=np.arange(99)), dict(knot=np.arange(100) * 0.5),
                dict(knot=np.arange(100, dtype=np.int64) << 32)):
        a = dict(word="u16", order="row", alt=alt, az=az, knot=None)
        a.update(bad)
        with pytest.raises(ValueError):
            cc._range_model(8, 100, a["word"], a["order"], 0.002, a["alt"], None, a["az"], (0.0, 0.0), a["knot"], 0)
