"""GPU: a sensor's range image rasterised in place, de-skewed per column (cc_ingest_ranges through Context.range_sensor /
Context.ingest_ranges): full-size images of the synthetic sensor, the largest images the model takes, ties and edge words, and one
end-to-end drive.  Every comparison is against Context.ingest of the numpy restatement (range_images.restate), byte for byte, and
against the CPU oracle on those points."""
import numpy as np
import pytest

from parity import compare_desc
from range_images import (ORIGIN_N, ORIGIN_Z, Sensor, assert_scene, cells, edge_words, first_owner_positions, offsets, procedural_ranges,
                          ranges_from_clouds, restate_all, sweep_knots, synth_sensor, tables, tie_scene, to_order)

pytestmark = pytest.mark.gpu

WORDS = {"u32": 0.001, "u16": 0.002, "f32": 1.0}   # word -> range_scale: mm, 2 mm, metres


def _zeros(cc, n):
    import torch
    return torch.zeros((n, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")


def _ingest_both(cc, ctx, sensor, images, knots):
    """(descriptors, debug outputs) of ingest_ranges -- plain and with the debug outputs, equal bytes -- and of Context.ingest on the
    restated clouds; asserts the two are equal byte for byte.  Returns (descriptors, debug outputs, restated clouds)."""
    import torch
    n = len(images)
    h = _make(cc, ctx, sensor)
    x = torch.from_numpy(np.ascontiguousarray(images).view({"u16": np.int16, "u32": np.int32, "f32": np.float32}[sensor.word])).cuda()
    plain = ctx.ingest_ranges(h, x, knots=knots, out=_zeros(cc, n))
    d, dbg = ctx.ingest_ranges(h, x, knots=knots, out=_zeros(cc, n), debug=True)
    clouds = restate_all(sensor, images, knots)
    ref, rdbg = ctx.ingest(torch.from_numpy(np.concatenate(clouds, 0)).cuda(), offsets(n, sensor), out=_zeros(cc, n), debug=True)
    torch.cuda.synchronize()
    h.close()
    assert torch.equal(plain, d), "with / without debug outputs"
    assert torch.equal(ref, d), "descriptors differ from Context.ingest of the restated cloud"
    for k in dbg:
        assert torch.equal(rdbg[k], dbg[k]), k
    return d, dbg, clouds


def _make(cc, ctx, s):
    """range_images.Sensor -> cc.RangeSensor holding the SAME f32 tables (a test sensor's tables are not always the rounded cos / sin
    of angles at hand -- the tie scene sets one sine to +0.0 -- so the model is filled from the tables, as the C-ABI takes them)"""
    m = cc.L.RangeModel(s.H, s.W, cc.RANGE_WORDS[s.word][0], cc.RANGE_ORDERS[s.order], float(s.range_scale), float(s.origin_n), float(s.origin_z), s.K,
                        s.row_tab.ctypes.data, s.col_cs.ctypes.data, s.col_knot.ctypes.data if s.col_knot is not None else None)
    return cc.RangeSensor(ctx, m, s.word)


def _oracle_report(oracle, clouds, d, dbg, tag, which=None):
    report = []
    for i, s in enumerate(clouds):
        if which is not None and i not in which:
            continue
        s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]   # rejected by the library, undefined behaviour in the reference
        o = oracle.Scan(s)
        ob, opix = o.bev()
        if not np.array_equal(ob, dbg["bev"][i].cpu().numpy()):
            report.append("%s scan %d: bev differs" % (tag, i))
        if not np.array_equal(opix, dbg["pix_rc"][i].cpu().numpy()):
            report.append("%s scan %d: pix_rc differs" % (tag, i))
        if not np.array_equal(o.labels(), dbg["labels"][i].cpu().numpy()):
            report.append("%s scan %d: label images differ" % (tag, i))
        report += ["%s scan %d: %s" % (tag, i, m) for m in compare_desc(o.desc()[0], d[i], float_exact=False)]
    return report


_CLOUDS = {}


def _synth_clouds(cc, n):
    """n full-size 64 x 1 875 scans of the synthetic sensor, beam-major (computed once)"""
    if n not in _CLOUDS:
        xyzi, _, _ = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
        assert xyzi.shape[1] == 64 * 1875
        _CLOUDS[n] = xyzi.cpu().numpy()
    return _CLOUDS[n]


@pytest.mark.parametrize("n_scans", [4, 10])   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
@pytest.mark.parametrize("word", ["u32", "u16", "f32"])
@pytest.mark.parametrize("K", [0, 32, 64])
def test_full_size_images(cc, oracle, n_scans, word, K):
    H, W = 64, 1875
    sensor = synth_sensor(H, W, "row", word, WORDS[word], K)
    images = ranges_from_clouds(_synth_clouds(cc, 10)[:n_scans], word, WORDS[word], seed=3)
    assert_scene(oracle, sensor, images[:1])
    ctx = cc.Context(0, max_batch=n_scans)
    # a sweep motion of 1 - 2 m and 2 - 4 degrees per scan, col_knot = col * K // W
    knots = None if K == 0 else sweep_knots(lambda b, e, ref, k: cc.motion_knots(b, e, ref=ref, K=k), n_scans, K, seed=40 + K)
    assert K == 0 or np.array_equal(sensor.col_knot, np.arange(W) * K // W)
    d, dbg, clouds = _ingest_both(cc, ctx, sensor, images, knots)
    report = _oracle_report(oracle, clouds, cc.desc_to_numpy(d), dbg, "%s K=%d" % (word, K))
    assert not report, "\n".join(report[:40])
    # the host-buffer call
    h = _make(cc, ctx, sensor)
    dh, dn = ctx.ingest_ranges_host(h, images, knots=knots), cc.desc_to_numpy(d)
    h.close()
    for i in range(n_scans):
        assert not compare_desc(dn[i], dh[i], float_exact=True), i
    ctx.close()


@pytest.mark.parametrize("n_scans", [1, 9])   # both launch paths
@pytest.mark.parametrize("shape", [(128, 4095, "row"), (127, 4096, "col")])
def test_largest_images(cc, oracle, n_scans, shape):
    """the index arithmetic at its limits: 524 160 / 520 192 pixels per image, a divisor of 4 095 (multiply-high) and of 127"""
    H, W, order = shape
    K = 32
    rows, alt = procedural_ranges(H, W, n_scans, seed=H)
    row_tab, col_cs = tables(alt, np.deg2rad(np.array([-0.9, -0.3, 0.3, 0.9]))[np.arange(H) % 4], np.arange(W) * (2 * np.pi / W))
    sensor = Sensor(H, W, "u16", order, 0.002, row_tab, col_cs, origin=(ORIGIN_N, ORIGIN_Z), col_knot=(np.arange(W) * K // W).astype(np.int32), K=K)
    images = to_order(rows, H, W, order)
    ctx = cc.Context(0, max_batch=n_scans)
    knots = sweep_knots(lambda b, e, ref, k: cc.motion_knots(b, e, ref=ref, K=k), n_scans, K, seed=H)
    d, dbg, clouds = _ingest_both(cc, ctx, sensor, images, knots)
    report = _oracle_report(oracle, clouds, cc.desc_to_numpy(d), dbg, "%d x %d" % (H, W), which=(0, n_scans - 1))
    assert not report, "\n".join(report[:40])
    dn = cc.desc_to_numpy(d)
    assert int(dn[0]["n_pix"]) >= 300 and all(int(dn[0]["n_cont"][lv]) > 0 for lv in (1, 2, 3))
    ctx.close()


@pytest.mark.parametrize("order,n_rep", [("row", 3), ("col", 1)])   # 9 scans: one workgroup per scan; 3: split sweep + merge kernel
def test_ties(cc, oracle, order, n_rep):
    cfg = cc.L.default_manager_cfg()
    sensor, images, knots = tie_scene(cfg, order)
    images, knots = np.concatenate([images] * n_rep), np.concatenate([knots] * n_rep)
    ctx = cc.Context(0, max_batch=len(images))
    d, dbg, clouds = _ingest_both(cc, ctx, sensor, images, knots)
    report = _oracle_report(oracle, clouds, cc.desc_to_numpy(d), dbg, "ties", which=(0, 1, 2))
    assert not report, "\n".join(report[:40])
    pix = dbg["pix_rc"].cpu().numpy()
    for i in range(3):
        exp = first_owner_positions(cfg, clouds[i])
        assert len(exp) >= 10
        for cell, rc in exp.items():
            assert np.array_equal(pix[i][cell], rc), (i, cell)
    ctx.close()


@pytest.mark.parametrize("word,n_rep", [("u16", 1), ("u32", 3), ("f32", 1)])
def test_edge_words(cc, oracle, word, n_rep):
    cfg = cc.L.default_manager_cfg()
    H, W = 64, 1875
    scale = 1e-6 if word == "u32" else WORDS[word]   # u32: micrometres, so that words of 2^24 .. 2^26 (their conversion rounds) land in the map
    sensor = synth_sensor(H, W, "row", word, scale)
    if word == "u32":
        rng = np.random.default_rng(9)
        images = rng.integers(1 << 24, 1 << 26, (3, H * W)).astype(np.uint32) | np.uint32(1)
        assert (images.astype(np.float32).astype(np.int64) != images.astype(np.int64)).mean() > 0.5
    else:
        images = ranges_from_clouds(_synth_clouds(cc, 10)[:3], word, scale, seed=5)
    images[0][::3] = edge_words(word, H * W)[::3]
    images = np.concatenate([images] * n_rep)
    ctx = cc.Context(0, max_batch=len(images))
    d, dbg, clouds = _ingest_both(cc, ctx, sensor, images, None)
    report = _oracle_report(oracle, clouds, cc.desc_to_numpy(d), dbg, "edge words", which=(0, 1))
    assert not report, "\n".join(report[:40])
    dn = cc.desc_to_numpy(d)
    c0 = cells(cfg, clouds[0])
    assert int(dn[0]["n_pix"]) == len(np.unique(c0[c0 >= 0]))
    ctx.close()


def test_refused_arguments(cc):
    import torch
    ctx, ctx2 = cc.Context(0, max_batch=2), cc.Context(0, max_batch=2)
    alt, az = np.deg2rad(np.linspace(2.0, -24.8, 16)), np.arange(601) * (2 * np.pi / 601)
    good = dict(word="u16", order="row", range_scale=0.002, beam_alt=alt, col_az=az, origin=(0.03, 0.04), col_knot=np.arange(601) % 4, K=4)
    s = ctx.range_sensor(16, 601, **good)
    x = torch.randint(1000, 20000, (2, 16 * 601), dtype=torch.int16, device="cuda")
    kn = np.tile(np.eye(3, 4, dtype=np.float32), (2, 4, 1, 1))
    ref = ctx.ingest_ranges(s, x, knots=kn, out=_zeros(cc, 2))
    for bad in (dict(K=65), dict(col_knot=np.arange(601) % 5), dict(range_scale=np.inf), dict(origin=(np.nan, 0.0))):
        with pytest.raises(cc.CCError):
            ctx.range_sensor(16, 601, **dict(good, **bad))
    with pytest.raises(cc.CCError):
        ctx.range_sensor(1, 10, **dict(good, beam_alt=alt[:1], col_az=az[:10], col_knot=None, K=0))
    for bad in (dict(word="u8"), dict(order="diag"), dict(beam_alt=alt[:15]), dict(col_az=az[:600]), dict(beam_alt=None)):
        with pytest.raises(ValueError):
            ctx.range_sensor(16, 601, **dict(good, **bad))
    with pytest.raises(ValueError):
        ctx.ingest_ranges(s, x, knots=None)                   # a sensor with K = 4 needs knots
    with pytest.raises(ValueError):
        ctx.ingest_ranges(s, x.to(torch.int32), knots=kn)     # u16 words, i32 tensor
    with pytest.raises(ValueError):
        ctx.ingest_ranges(s, x.reshape(-1)[:-1], knots=kn)    # not whole images
    with pytest.raises(ValueError):
        ctx2.ingest_ranges(s, x, knots=kn)                    # another context's sensor
    # u16 words at an odd address (no tensor can hold them: the C call itself), and a NULL h_knots for a sensor with knots
    k1 = np.ascontiguousarray(kn[:1].reshape(1, -1))
    out = _zeros(cc, 1)
    assert cc.lib().cc_ingest_ranges(ctx.h, s.h, x.data_ptr() + 1, 1, k1.ctypes.data, out.data_ptr(), None, None) == -1
    assert cc.lib().cc_last_error().decode().startswith("cc_ingest_ranges:")
    assert cc.lib().cc_ingest_ranges(ctx.h, s.h, x.data_ptr(), 1, None, out.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(ref, ctx.ingest_ranges(s, x, knots=kn, out=_zeros(cc, 2)))
    s.close()
    ctx.close()
    ctx2.close()


def test_drive_of_range_images(cc, oracle):
    """Every scan of a drive is a range image with its own sweep motion: de-skewed at ingest, added and queried.  The descriptors are
    byte-equal to the drive ingested from the restated clouds, so ONE query call stands for both; its results are the oracle's on
    the restated clouds."""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n, K, H, W = 72, 32, 32, 900
    xyzi, poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=H, azim=W)
    sensor = synth_sensor(H, W, "row", "u16", 0.002, K)
    images = ranges_from_clouds(xyzi.cpu().numpy(), "u16", 0.002, seed=8)
    knots = sweep_knots(lambda b, e, ref, k: cc.motion_knots(b, e, ref=ref, K=k), n, K, seed=29)
    assert np.abs(knots.reshape(n, K, 3, 4)[:, 0, :, 3]).max() > 1.0
    clouds = restate_all(sensor, images, knots)
    plain = restate_all(sensor.with_(K=0, col_knot=None), images)
    assert max(np.nanmax(np.abs(a[:, :3] - b[:, :3])) for a, b in zip(clouds, plain)) > 1.0   # the de-skew moves points by metres
    ctx = cc.Context(0, max_batch=n)
    h = _make(cc, ctx, sensor)
    x = torch.from_numpy(images.view(np.int16)).cuda()
    desc = ctx.ingest_ranges(h, x, knots=knots, out=_zeros(cc, n))
    ref = ctx.ingest(torch.from_numpy(np.concatenate(clouds, 0)).cuda(), offsets(n, sensor), out=_zeros(cc, n))
    torch.cuda.synchronize()
    assert torch.equal(desc, ref)
    seeds = np.arange(n, dtype=np.int32)
    db = cc.Database(ctx, dcfg, capacity=n)
    db.add_scans(desc, ts, seeds)
    res = db.query(desc, seeds)
    torch.cuda.synchronize()
    kept = [c[~np.isnan(c[:, 0])] for c in clouds]   # (a NaN point is undefined behaviour in the reference)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in kept])]).astype(np.int64)
    ores, _, odesc = oracle.run_sequence(np.concatenate(kept, 0), offs, ts, seeds, dcfg=dcfg, want_desc=True)
    d = cc.desc_to_numpy(desc)
    for i in range(n):
        bad = compare_desc(odesc[i], d[i], float_exact=False)
        assert not bad, "scan %d: %s" % (i, bad[:5])
    for f in ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy", "n_knn_hits"]:
        assert np.array_equal(ores[f], res[f]), f
    m = ores["n_res"] > 0
    if m.any():
        assert np.abs(ores["correlation"][m] - res["correlation"][m]).max() < 1e-4
        assert np.abs(ores["tf"][m] - res["tf"][m]).max() < 1e-4
    db.close()
    h.close()
    ctx.close()
