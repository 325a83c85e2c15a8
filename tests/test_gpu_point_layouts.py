"""GPU: points in packed-xyz / strided records and the per-scan transform fused into the rasteriser (cc_ingest_points through
Context.ingest(layout=, tf=)), on full-size scans against the CPU oracle, and one end-to-end drive ingested as packed xyz with a
transform per scan."""
import numpy as np
import pytest

from parity import compare_desc, terrain_scan
from point_layouts import apply_tf, border_scan, inverse, random_tfs, repack, rigid

pytestmark = pytest.mark.gpu

LAYOUTS = [(12, 0), (32, 0), (48, 8), (16, 0)]


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
    """Context.ingest into a zeroed buffer: the kernels never write the entries behind n_stored / n_pts / n_segs, so descriptors
    can be compared as bytes only when those start out equal."""
    import torch
    out = torch.zeros((len(offs) - 1, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    return ctx.ingest(x, offs, out=out, **kw)


def _oracle_report(oracle, scans, d, dbg, tag):
    report = []
    for i, s in enumerate(scans):
        s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]   # rejected by the library, undefined behaviour in the reference: see test_emu_point_layouts.py
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


def _full_size_scans(cc, n):
    """A scan around the map's border and the blind disc, n - 3 scans of 120 000 points, two contour-rich terrain scans; 1 mod 4
    points each: 12-byte scans then start at every residue mod 16"""
    xyzi, _, _ = cc.synth.make_sequence(n - 3, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
    assert xyzi.shape[1] == 120000
    scans = [xyzi[i].cpu().numpy()[:119997 - 8 * i] for i in range(n - 3)]
    return [border_scan(7, n=40001)] + scans + [terrain_scan(3)[:59997], terrain_scan(104, n=30001, scale=2.2, quant=0.25)]


def _ingest_all(cc, ctx, cat, offs, tf, ref=None):
    """Every layout (and two misaligned bases): plain and with the debug outputs.  Returns (descriptors, debug outputs) of the first."""
    import torch
    first = None
    for (stride, off), shift in [(l, 0) for l in LAYOUTS] + [((12, 0), 8), ((16, 0), 4)]:
        x = _dev(repack(cat, stride, off), shift)
        plain = _ing(cc, ctx, x, offs, layout=(stride, off), tf=tf)
        desc, dbg = _ing(cc, ctx, x, offs, debug=True, layout=(stride, off), tf=tf)
        torch.cuda.synchronize()
        assert torch.equal(plain, desc), ((stride, off), shift, "with / without debug outputs")
        if first is None:
            first = (desc.clone(), {k: v.clone() for k, v in dbg.items()})
        else:
            assert torch.equal(first[0], desc), ((stride, off), shift)
            for k in dbg:
                assert torch.equal(first[1][k], dbg[k]), ((stride, off), shift, k)
        if ref is not None:
            assert torch.equal(ref, desc), ((stride, off), shift, "differs from cc_ingest_batch")
    return first


@pytest.mark.parametrize("n_scans", [4, 10])   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
def test_layouts_and_transform_full_size(cc, oracle, n_scans):
    import torch
    scans = _full_size_scans(cc, n_scans)
    offs, cat = _offs(scans), np.concatenate(scans, 0)
    assert len({int(o) * 12 % 16 for o in offs[:-1]}) == 4
    ctx = cc.Context(0, max_batch=n_scans)
    # 1. no transform: every layout gives cc_ingest_batch's bytes, and those are the oracle's descriptor
    ref, rdbg = _ing(cc, ctx, torch.from_numpy(cat).cuda(), offs, debug=True)
    rdbg = {k: v.clone() for k, v in rdbg.items()}
    report = _oracle_report(oracle, scans, cc.desc_to_numpy(ref), rdbg, "float4")
    assert not report, "\n".join(report[:40])
    d, dbg = _ingest_all(cc, ctx, cat, offs, None, ref=ref)
    for k in dbg:
        assert torch.equal(rdbg[k], dbg[k]), k
    assert torch.equal(ref, _ing(cc, ctx, _dev(repack(cat, 12, 0)), offs, layout="xyz"))
    assert torch.equal(ref, _ing(cc, ctx, torch.from_numpy(cat).cuda(), offs, layout="xyzi"))
    # 2. a different transform per scan (one moves points across the border and into the blind disc, one is the identity)
    tfs = random_tfs(n_scans, seed=17)
    tfs[0] = rigid(0.3, np.deg2rad(1.0), np.deg2rad(-2.0), (4.0, -3.0, 0.2), np.float32).reshape(12)
    tfs[2] = rigid(0.0, dtype=np.float32).reshape(12)
    moved = [apply_tf(s, m) for s, m in zip(scans, tfs)]
    inside = lambda s: (np.abs(s[:, 0]) < 75) & (np.abs(s[:, 1]) < 75)
    assert (inside(scans[0]) & ~inside(moved[0])).sum() > 20 and (~inside(scans[0]) & inside(moved[0])).sum() > 20
    assert ((np.hypot(scans[0][:, 0], scans[0][:, 1]) > 4) & (np.hypot(moved[0][:, 0], moved[0][:, 1]) < 1.5)).sum() > 5
    d, dbg = _ingest_all(cc, ctx, cat, offs, tfs)
    report = _oracle_report(oracle, moved, cc.desc_to_numpy(d), dbg, "transformed")
    assert not report, "\n".join(report[:40])
    assert torch.equal(d[2], ref[2]), "identity passed explicitly = the untransformed result"
    # ... as [n, 3, 4], and through the host-buffer call
    assert torch.equal(d, _ing(cc, ctx, _dev(repack(cat, 12, 0)), offs, layout="xyz", tf=tfs.reshape(-1, 3, 4)))
    dh, dn = ctx.ingest_host(repack(cat, 32, 0), offs, layout=(32, 0), tf=tfs), cc.desc_to_numpy(d)
    for i in range(n_scans):
        assert not compare_desc(dn[i], dh[i], float_exact=True), i
    ctx.close()


def test_edge_inputs(cc, oracle):
    rng = np.random.default_rng(5)
    tiny = np.zeros((11, 4), np.float32)
    far = np.full((50, 4), 1000.0, np.float32)
    ties = np.tile(np.array([[10.2, 3.3, 1.0, 0], [10.7, 3.9, 1.0, 0], [10.4, 3.1, 1.0, 0]], np.float32), (40, 1))
    crowd = np.zeros((60001, 4), np.float32)   # a few cells, thousands of points each, heights on a 6-value lattice
    crowd[:, 0], crowd[:, 1] = rng.uniform(10.0, 16.0, 60001), rng.uniform(-3.0, 3.0, 60001)
    crowd[:, 2] = rng.integers(0, 6, 60001) * 0.5 - 1.0
    nans = terrain_scan(7, n=50003, scale=1.2)
    nans[::7, 2] = np.nan
    nans[3::11, 0] = np.nan
    nans[5::13, 1] = np.nan
    for scans in ([tiny, far, ties, crowd, nans], [tiny, far, ties, crowd, nans] * 2):
        offs, cat = _offs(scans), np.concatenate(scans, 0)
        ctx = cc.Context(0, max_batch=len(scans))
        d, dbg = _ingest_all(cc, ctx, cat, offs, None)
        report = _oracle_report(oracle, scans, cc.desc_to_numpy(d), dbg, "plain")
        tfs = np.stack([rigid(0.4 * i - 1.0, t=(0.5 * i, -0.3 * i, 0.25), dtype=np.float32).reshape(12) for i in range(len(scans))])
        moved = [apply_tf(s, m) for s, m in zip(scans, tfs)]   # yaw and a shift: equal heights stay equal
        assert len(np.unique(moved[3][:, 2])) == 6
        d, dbg = _ingest_all(cc, ctx, cat, offs, tfs)
        report += _oracle_report(oracle, moved, cc.desc_to_numpy(d), dbg, "transformed")
        assert not report, "\n".join(report[:40])
        ctx.close()


def test_refused_layouts(cc):
    import torch
    ctx = cc.Context(0, max_batch=2)
    s = terrain_scan(3, n=3001)
    offs = np.array([0, len(s)], np.int64)
    ref = _ing(cc, ctx, torch.from_numpy(s).cuda(), offs)
    x = _dev(repack(s, 64, 0))
    for lay in [(22, 0), (32, 2), (16, 8), (8, 0), (260, 0)]:
        with pytest.raises(cc.CCError):
            ctx.ingest(x, offs, layout=lay)
    with pytest.raises(cc.CCError):
        ctx.ingest(_dev(repack(s, 16, 0), 2), offs, layout=(16, 0))
    with pytest.raises(ValueError):
        ctx.ingest(x, offs, layout="xyzrgb")
    with pytest.raises(ValueError):
        ctx.ingest(x, offs, layout=(64, 0), tf=np.zeros((2, 12), np.float32))
    assert torch.equal(ref, _ing(cc, ctx, x, offs, layout=(64, 0)))
    ctx.close()


def test_drive_as_packed_xyz_with_a_transform_per_scan(cc, oracle):
    """ingest (packed xyz + per-scan transform) -> add -> query every scan at its own epoch, against the oracle on the
    numpy-transformed float4 scans.  The raw input is each scan of a synthetic drive moved by the INVERSE of its transform (f64,
    rounded to f32): what the library rasterises is the original drive up to rounding, so the drive still closes loops."""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n = 72
    xyzi, poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    drive = xyzi.cpu().numpy()
    P = drive.shape[1]
    tfs = random_tfs(n, seed=23, max_tilt_deg=3.0, max_shift=2.0)
    raw = np.zeros((n, P, 4), np.float32)
    for i in range(n):
        inv = inverse(tfs[i].astype(np.float64))
        raw[i, :, :3] = (drive[i, :, :3].astype(np.float64) @ inv[:, :3].T + inv[:, 3]).astype(np.float32)
    assert np.abs(raw[:, :, :3] - drive[:, :, :3]).max() > 1.0   # the raw scans are not the drive's
    moved = np.stack([apply_tf(raw[i], tfs[i]) for i in range(n)])
    assert np.abs(moved[:, :, :3] - drive[:, :, :3]).max() < 1e-3   # ... and the transform brings it back, up to rounding
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(moved.reshape(-1, 4), offs, ts, seeds, dcfg=dcfg, want_desc=True)
    m = ores["n_res"] > 0
    assert m.sum() >= 3, "the oracle's drive must close loops, or the comparison below shows nothing"
    ctx = cc.Context(0, max_batch=n)
    desc = ctx.ingest(_dev(repack(raw.reshape(-1, 4), 12, 0), 4), offs, layout="xyz", tf=tfs)
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
    db.close()
    ctx.close()
