"""GPU: a sweep de-skewed by per-point time while it is rasterised (cc_ingest_points_motion through Context.ingest(motion=, t_begin=,
scale=, knots=)), on full-size scans against the CPU oracle on the numpy-moved points, and one end-to-end drive whose raw scans are
skewed by a motion per scan."""
import numpy as np
import pytest

from parity import compare_desc, terrain_scan
from point_layouts import apply_tf, border_scan, inverse, rigid
from point_motion import (SWEEP, TIME_F32, TIME_U32, apply_motion, assert_ties_across_bins, bin_edge_inputs, random_knots, repack_with_time,
                          tie_inputs, time_bins)

pytestmark = pytest.mark.gpu

# (stride, xyz_offset, time_offset, base shift): the 16- and 32-byte instances, a time in front of xyz, a run-time stride, a base at 4 mod 16
LAYOUTS = [(16, 0, 12, 0), (32, 0, 16, 0), (48, 8, 4, 0), (20, 0, 12, 0), (16, 0, 12, 4)]
SWEEP_NS = 100_000_000


def _offs(scans):
    return np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)


def _dev(buf, shift=0):
    """numpy uint8 records -> CUDA tensor whose first byte sits `shift` bytes behind a 16-byte boundary"""
    import torch
    t = torch.empty(len(buf) + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + len(buf)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
    return v


def _ing(cc, ctx, x, offs, **kw):
    """Context.ingest into a zeroed buffer (the kernels never write the entries behind a descriptor's counts)"""
    import torch
    out = torch.zeros((len(offs) - 1, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    return ctx.ingest(x, offs, out=out, **kw)


def _oracle_report(oracle, scans, d, dbg, tag):
    report = []
    for i, s in enumerate(scans):
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


_SCANS = {}


def _full_size_scans(cc, n):
    """One 120 000-point scan, a scan around the map's border and the blind disc, terrain scans of 30 - 60 k points (computed once)"""
    if n not in _SCANS:
        xyzi, _, _ = cc.synth.make_sequence(1, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
        assert xyzi.shape[1] == 120000
        scans = [xyzi[0].cpu().numpy()[:119997], border_scan(7, n=40001), terrain_scan(3)[:59997], terrain_scan(104, n=30001, scale=2.2, quant=0.25)]
        scans += [terrain_scan(200 + i, n=30001 + 4096 * i + 8 * i, scale=1.2 + 0.2 * i) for i in range(n - 4)]
        _SCANS[n] = scans
    return _SCANS[n]


def _az_fraction(s):
    """the azimuth of every point as a fraction of the turn, [0, 1): a spinning sensor's time within the sweep"""
    return ((np.arctan2(s[:, 1].astype(np.float64), s[:, 0].astype(np.float64)) + np.pi) / (2 * np.pi)) % 1.0


def _ingest_all(cc, ctx, cat, wcat, offs, time_type, tb, sc, knots):
    """Every layout, plain and with the debug outputs (equal bytes).  Returns (descriptors, debug outputs) of the first."""
    import torch
    first = None
    for (stride, off, toff, shift) in LAYOUTS:
        x = _dev(repack_with_time(cat, wcat, stride, off, toff), shift)
        kw = dict(layout=(stride, off), motion=(toff, time_type), t_begin=tb, scale=sc, knots=knots)
        plain = _ing(cc, ctx, x, offs, **kw)
        desc, dbg = _ing(cc, ctx, x, offs, debug=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(plain, desc), ((stride, off, toff, shift), "with / without debug outputs")
        if first is None:
            first = (desc.clone(), {k: v.clone() for k, v in dbg.items()})
        else:
            assert torch.equal(first[0], desc), (stride, off, toff, shift)
            for k in dbg:
                assert torch.equal(first[1][k], dbg[k]), (stride, off, toff, shift, k)
    return first


@pytest.mark.parametrize("n_scans", [4, 10])   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
@pytest.mark.parametrize("n_knots", [1, 32, 64])
def test_full_size_scans(cc, oracle, n_scans, n_knots):
    import torch
    scans = _full_size_scans(cc, n_scans)
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    ctx = cc.Context(0, max_batch=n_scans)
    knots = random_knots(n_scans, n_knots, seed=100 + n_knots, max_shift=3.0)
    knots[1, :, :] = random_knots(1, n_knots, seed=7, max_shift=5.0)[0]   # the border scan: points cross the border both ways
    rng = np.random.default_rng(n_knots)
    # f32 times: rising with the azimuth in the first scans (a wave mostly shares a bin), random in the others (every wave mixes bins)
    frac = [_az_fraction(s) if i % 2 == 0 else rng.uniform(0.0, 1.0, len(s)) for i, s in enumerate(scans)]
    tb = np.linspace(-0.02, 0.02, n_scans).astype(np.float32)
    sc = np.full(n_scans, np.float32(n_knots) / SWEEP, np.float32)
    words = [(f.astype(np.float32) * SWEEP + tb[i]).astype(np.float32).view(np.uint32) for i, f in enumerate(frac)]
    moved = [apply_motion(s, w, TIME_F32, tb[i], sc[i], knots[i]) for i, (s, w) in enumerate(zip(scans, words))]
    assert all(len(np.unique(time_bins(w, TIME_F32, tb[i], sc[i], n_knots))) == n_knots for i, w in enumerate(words) if i % 2 or i == 0)
    d, dbg = _ingest_all(cc, ctx, cat, np.concatenate(words), offs, "f32", tb, sc, knots.reshape(n_scans, n_knots, 3, 4))
    report = _oracle_report(oracle, moved, cc.desc_to_numpy(d), dbg, "f32")
    # ... and, as bytes, cc_ingest_batch on the moved points
    ref, rdbg = _ing(cc, ctx, torch.from_numpy(np.concatenate(moved, 0)).cuda(), offs, debug=True)
    assert torch.equal(ref, d)
    for k in dbg:
        assert torch.equal(rdbg[k], dbg[k]), k
    # u32 times in ns, t_begin close to 2^32 in every other scan
    tbu = np.array([0xFFFFFF00 if i % 2 else 1000 + i for i in range(n_scans)], np.uint32)
    scu = np.full(n_scans, np.float32(n_knots) / np.float32(SWEEP_NS), np.float32)
    wordsu = [(tbu[i] + (f * (SWEEP_NS - 1)).astype(np.uint32)).astype(np.uint32) for i, f in enumerate(frac)]
    tbf = tbu.view(np.float32)
    movedu = [apply_motion(s, w, TIME_U32, tbf[i], scu[i], knots[i]) for i, (s, w) in enumerate(zip(scans, wordsu))]
    du, dbgu = _ingest_all(cc, ctx, cat, np.concatenate(wordsu), offs, "u32", tbu, scu, knots)
    report += _oracle_report(oracle, movedu, cc.desc_to_numpy(du), dbgu, "u32")
    assert not report, "\n".join(report[:40])
    # the host-buffer call
    dh, dn = ctx.ingest_host(repack_with_time(cat, np.concatenate(wordsu), 32, 0, 16), offs, layout=(32, 0), motion=(16, "u32"), t_begin=tbu, scale=scu,
                             knots=knots), cc.desc_to_numpy(du)
    for i in range(n_scans):
        assert not compare_desc(dn[i], dh[i], float_exact=True), i
    if n_knots == 32:   # the points sorted by bin: the bytes of ingest_segments with one segment per bin (CC_SEG_MAX = 32)
        seg_scans, sorted_scans, sorted_w = [], [], []
        for i, (s, w) in enumerate(zip(scans, words)):
            b = time_bins(w, TIME_F32, tb[i], sc[i], n_knots)
            order = np.argsort(b, kind="stable")
            s, w, b = s[order], w[order], b[order]
            sorted_scans.append(s)
            sorted_w.append(w)
            seg_scans.append([(_dev(np.ascontiguousarray(s[b == k]).view(np.uint8).reshape(-1)), (16, 0), knots[i][k]) for k in range(n_knots)])
        out = torch.zeros((n_scans, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        g, gdbg = ctx.ingest_segments(seg_scans, out=out, debug=True)
        x = _dev(repack_with_time(np.concatenate(sorted_scans, 0), np.concatenate(sorted_w), 16, 0, 12))
        ds, dbgs = _ing(cc, ctx, x, offs, debug=True, layout=(16, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots)
        torch.cuda.synchronize()
        assert torch.equal(g, ds)
        for k in gdbg:
            assert torch.equal(gdbg[k], dbgs[k]), k
    ctx.close()


@pytest.mark.parametrize("n_rep", [1, 2])   # split sweep + merge kernel; one workgroup per scan
def test_bin_edges_and_ties(cc, oracle, n_rep):
    cfg = cc.L.default_manager_cfg()
    # times on the bin boundaries, 1 ulp either side, outside the sweep, +-inf, NaN; one scan with a scale of 0
    K = 16
    s = terrain_scan(21, n=50003, scale=1.3)
    w, tb, scale = bin_edge_inputs(len(s), K)
    ek = random_knots(2, K, seed=4)
    scans, words = [s, s], [w, w]
    tbs, scs = [tb, tb], [scale, np.float32(0.0)]
    knots = [ek[0], ek[1]]
    # equal moved heights in one cell from points of different bins: K = 4 knots, padded to 16 (the call has one K)
    t_scans, t_words, t_tb, t_sc, t_kn = tie_inputs(3, n0=60001)
    t_moved = [apply_motion(a, b, TIME_F32, t_tb[i], t_sc[i], t_kn[i]) for i, (a, b) in enumerate(zip(t_scans, t_words))]
    assert_ties_across_bins(cfg, t_moved, t_words, t_tb, t_sc, 4)
    pad = np.tile(rigid(0.0, t=(50.0, 50.0, 9.0), dtype=np.float32).reshape(12), (K - 4, 1))   # (never selected: u < 4)
    scans, words = (scans + t_scans) * n_rep + [s], (words + t_words) * n_rep + [w]
    tbs, scs = (tbs + list(t_tb)) * n_rep + [tb], (scs + list(t_sc)) * n_rep + [scale]
    knots = (knots + [np.concatenate([k4, pad]) for k4 in t_kn]) * n_rep + [ek[0]]
    tbs, scs, knots = np.array(tbs, np.float32), np.array(scs, np.float32), np.stack(knots)
    assert len(scans) == (6 if n_rep == 1 else 11)
    moved = [apply_motion(a, b, TIME_F32, tbs[i], scs[i], knots[i]) for i, (a, b) in enumerate(zip(scans, words))]
    assert np.array_equal(moved[1], apply_tf(s, ek[1][0])) and np.array_equal(moved[2], t_moved[0])
    ctx = cc.Context(0, max_batch=len(scans))
    d, dbg = _ingest_all(cc, ctx, np.concatenate(scans, 0), np.concatenate(words), _offs(scans), "f32", tbs, scs, knots)
    report = _oracle_report(oracle, moved, cc.desc_to_numpy(d), dbg, "edges / ties")
    assert not report, "\n".join(report[:40])
    ctx.close()


def test_refused_arguments(cc):
    import torch
    ctx = cc.Context(0, max_batch=2)
    s = terrain_scan(3, n=3001)
    offs = np.array([0, len(s)], np.int64)
    t = np.linspace(0.0, 0.0999, len(s)).astype(np.float32)
    kn = random_knots(1, 8, seed=1)
    x = _dev(repack_with_time(s, t.view(np.uint32), 32, 0, 16))
    good = dict(layout=(32, 0), motion=(16, "f32"), t_begin=[0.0], scale=[80.0], knots=kn)
    ref = _ing(cc, ctx, x, offs, **good)
    moved = apply_motion(s, t.view(np.uint32), TIME_F32, 0.0, 80.0, kn[0])
    assert torch.equal(ref, _ing(cc, ctx, torch.from_numpy(moved).cuda(), offs))
    for bad in (dict(motion=(6, "f32")), dict(motion=(8, "f32")), dict(motion=(32, "f32")), dict(scale=[np.inf]),
                dict(knots=random_knots(1, 65, seed=1))):
        with pytest.raises(cc.CCError):
            ctx.ingest(x, offs, **dict(good, **bad))
    for bad in (dict(knots=None), dict(tf=np.zeros((1, 12), np.float32)), dict(motion=(16, "f64")), dict(motion=None), dict(t_begin=None)):
        with pytest.raises(ValueError):
            ctx.ingest(x, offs, **dict(good, **bad))
    with pytest.raises(ValueError):
        ctx.ingest_host(repack_with_time(s, t.view(np.uint32), 32, 0, 16), offs, **dict(good, tf=np.zeros((1, 12), np.float32)))
    assert torch.equal(ref, _ing(cc, ctx, x, offs, **good))
    ctx.close()


def test_drive_with_a_motion_per_scan(cc, oracle):
    """ingest with motion -> add -> query every scan at its own epoch, against the oracle on the numpy-moved points.  Each raw scan is
    the drive's scan with every point moved by the INVERSE of its bin's knot (f64, rounded to f32); the bins come from the point's
    azimuth, the knots from motion_knots of a per-scan motion of 1 - 2 m and 2 - 4 degrees.  What the library rasterises is the
    original drive up to rounding, so the drive still closes loops -- and the plain ingest of the raw scans gives other descriptors."""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n, K = 72, 32
    xyzi, poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    drive = xyzi.cpu().numpy()
    P = drive.shape[1]
    rng = np.random.default_rng(29)
    knots = np.zeros((n, K, 3, 4), np.float32)
    raw = np.zeros((n, P, 4), np.float32)
    words = np.zeros((n, P), np.uint32)
    tb, sc = np.zeros(n, np.float32), np.full(n, np.float32(K) / SWEEP, np.float32)
    for i in range(n):
        ang, dist, yaw = rng.uniform(-np.pi, np.pi), rng.uniform(1.0, 2.0), np.deg2rad(rng.uniform(2.0, 4.0)) * rng.choice([-1.0, 1.0])
        begin = rigid(yaw, np.deg2rad(rng.uniform(-0.5, 0.5)), np.deg2rad(rng.uniform(-0.5, 0.5)), (dist * np.cos(ang), dist * np.sin(ang), 0.0))
        knots[i] = cc.motion_knots(begin, rigid(0.0), ref=1.0, K=K)   # the scan is referred to the sweep's end
        t = (_az_fraction(drive[i]) * float(SWEEP)).astype(np.float32)
        words[i] = t.view(np.uint32)
        b = time_bins(words[i], TIME_F32, tb[i], sc[i], K)
        for k in range(K):
            inv = inverse(knots[i, k].astype(np.float64))
            m = b == k
            raw[i, m, :3] = (drive[i, m, :3].astype(np.float64) @ inv[:, :3].T + inv[:, 3]).astype(np.float32)
    assert np.abs(knots[:, 0, :, 3]).max() > 1.0 and np.abs(knots[:, K - 1, :, 3]).max() < 0.05   # the motion fades towards the sweep's end
    assert np.abs(raw[:, :, :3] - drive[:, :, :3]).max() > 1.0   # the raw scans are not the drive's
    moved = np.stack([apply_motion(raw[i], words[i], TIME_F32, tb[i], sc[i], knots[i].reshape(K, 12)) for i in range(n)])
    assert np.abs(moved[:, :, :3] - drive[:, :, :3]).max() < 1e-3   # ... and the knots bring it back, up to rounding
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(moved.reshape(-1, 4), offs, ts, seeds, dcfg=dcfg, want_desc=True)
    m = ores["n_res"] > 0
    assert m.sum() >= 3, "the oracle's drive must close loops, or the comparison below shows nothing"
    ctx = cc.Context(0, max_batch=n)
    x = _dev(repack_with_time(raw.reshape(-1, 4), words.reshape(-1), 16, 0, 12))
    desc = ctx.ingest(x, offs, layout=(16, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots)
    db = cc.Database(ctx, dcfg, capacity=n)
    db.add_scans(desc, ts, seeds)
    res = db.query(desc, seeds)
    torch.cuda.synchronize()
    d = cc.desc_to_numpy(desc)
    for i in range(n):
        bad = compare_desc(odesc[i], d[i], float_exact=False)
        assert not bad, "scan %d: %s" % (i, bad[:5])
    for f in ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy", "n_knn_hits"]:
        assert np.array_equal(ores[f], res[f]), f
    assert np.abs(ores["correlation"][m] - res["correlation"][m]).max() < 1e-4
    assert np.abs(ores["tf"][m] - res["tf"][m]).max() < 1e-4
    # without the compensation the raw scans give other descriptors
    plain = cc.desc_to_numpy(ctx.ingest(x, offs, layout=(16, 0)))
    n_diff = sum(1 for i in range(n) if compare_desc(odesc[i], plain[i], float_exact=False))
    assert n_diff >= n // 2, n_diff
    db.close()
    ctx.close()
