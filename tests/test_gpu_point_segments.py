"""GPU: a scan from several point segments, each in its own tensor with its own record shape and transform
(cc_ingest_segments through Context.ingest_segments): full-size scans cut into three "sensors", a submap of four sweeps with their
poses, and one end-to-end drive ingested as segments.  The specified result is ingest()'s for the cloud
Q = T_0(segment 0) ++ T_1(segment 1) ++ ...: every comparison is against the CPU oracle on the numpy-built Q and, as bytes,
against cc_ingest_batch on Q."""
import numpy as np
import pytest

from parity import compare_desc
from point_layouts import apply_tf, inverse, random_tfs, repack, rigid

pytestmark = pytest.mark.gpu

LAYOUTS = [(32, 0), (12, 0), (48, 8), (16, 0)]


def _offs(scans):
    return np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)


def _dev(buf, shift=0):
    """numpy uint8 records -> CUDA tensor of its own whose first byte sits `shift` bytes behind a 16-byte boundary"""
    import torch
    t = torch.empty(len(buf) + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + len(buf)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
    return v


def _to_sensor(xyzi, E):
    """the points of a cloud in the frame of a sensor with extrinsic E (3 x 4, sensor -> base): E^-1 applied in f64, rounded to f32"""
    inv = inverse(np.asarray(E, np.float64))
    out = np.zeros((len(xyzi), 4), np.float32)
    out[:, :3] = (xyzi[:, :3].astype(np.float64) @ inv[:, :3].T + inv[:, 3]).astype(np.float32)
    return out


def _rig(scan, extr, k0=0):
    """One scan cut into len(extr) sensors by the azimuth sector of the point (each part keeps its points in their order), each part
    expressed in its sensor's frame.  Returns (segments for ingest_segments -- own tensor, own layout, the extrinsic as matrix --, Q)."""
    ns = len(extr)
    sector = np.minimum(((np.arctan2(scan[:, 1], scan[:, 0]) + np.pi) / (2 * np.pi / ns)).astype(np.int64), ns - 1)
    segs, q = [], []
    for s in range(ns):
        raw = _to_sensor(scan[sector == s], extr[s])
        lay = LAYOUTS[(k0 + s) % 4]
        segs.append((_dev(repack(raw, lay[0], lay[1]), 4 * ((k0 + s) % 2)), lay, extr[s]))
        q.append(apply_tf(raw, extr[s]))
    return segs, np.concatenate(q, 0)


def _ing(cc, ctx, scans, **kw):
    """into a zeroed buffer: the kernels never write the entries behind n_stored / n_pts / n_segs, so descriptors can be compared as
    bytes only when those start out equal"""
    import torch
    out = torch.zeros((len(scans), cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    return ctx.ingest_segments(scans, out=out, **kw)


def _check(cc, oracle, ctx, scans, Q, tag):
    """plain call = call with debug outputs; those against the oracle on Q (every scan, every output) and, as bytes, against
    cc_ingest_batch on Q"""
    import torch
    plain = _ing(cc, ctx, scans)
    desc, dbg = _ing(cc, ctx, scans, debug=True)
    torch.cuda.synchronize()
    assert torch.equal(plain, desc), tag + ": with / without debug outputs"
    d = cc.desc_to_numpy(desc)
    report = []
    for i, q in enumerate(Q):
        o = oracle.Scan(q)
        ob, opix = o.bev()
        if not np.array_equal(ob, dbg["bev"][i].cpu().numpy()):
            report.append("%s scan %d: bev differs" % (tag, i))
        if not np.array_equal(opix, dbg["pix_rc"][i].cpu().numpy()):
            report.append("%s scan %d: pix_rc differs" % (tag, i))
        if not np.array_equal(o.labels(), dbg["labels"][i].cpu().numpy()):
            report.append("%s scan %d: label images differ" % (tag, i))
        report += ["%s scan %d: %s" % (tag, i, m) for m in compare_desc(o.desc()[0], d[i], float_exact=False)]
    assert not report, "\n".join(report[:40])
    ref = torch.zeros_like(desc)
    ref, rdbg = ctx.ingest(torch.from_numpy(np.concatenate(Q, 0)).cuda(), _offs(Q), out=ref, debug=True)
    torch.cuda.synchronize()
    assert torch.equal(ref, desc), tag + ": differs from cc_ingest_batch on Q"
    for k in dbg:
        assert torch.equal(rdbg[k], dbg[k]), (tag, k)
    return desc


def _extrinsics(seed, n=3):
    """sensor -> base: any yaw, a few degrees of tilt, a lever arm of a metre or two"""
    return random_tfs(n, seed=seed, max_tilt_deg=3.0, max_shift=1.5)


@pytest.mark.parametrize("n_scans", [4, 24])   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
def test_rig_of_three_sensors_full_size(cc, oracle, n_scans):
    xyzi, _, _ = cc.synth.make_sequence(n_scans, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
    assert xyzi.shape[1] == 120000
    clouds = xyzi.cpu().numpy()
    extr = _extrinsics(31)
    scans, Q = [], []
    for i in range(n_scans):
        segs, q = _rig(clouds[i], extr, k0=i)
        assert len(q) == 120000 and min(len(s[0]) for s in segs) > 10000 * 12
        assert np.abs(np.sort(q[:, 2]) - np.sort(clouds[i][:, 2])).max() < 1e-3   # Q is the scan, re-ordered, up to the rounding of two transforms
        scans.append(segs)
        Q.append(q)
    ctx = cc.Context(0, max_batch=n_scans)
    _check(cc, oracle, ctx, scans, Q, "rig")
    ctx.close()


def test_submap_of_four_sweeps(cc, oracle):
    """4 consecutive 30 000-point sweeps, each in its own sensor frame with its pose relative to the last one, into ONE descriptor."""
    n_sub, n_maps = 4, 3
    xyzi, poses, _ = cc.synth.make_sequence(n_sub * n_maps, world=cc.synth.World(loop_len=200.0), device="cuda", start=40, beams=16, azim=1875)
    assert xyzi.shape[1] == 30000
    sweeps = xyzi.cpu().numpy()
    scans, Q = [], []
    for m in range(n_maps):
        ref = poses[m * n_sub + n_sub - 1]
        segs, q = [], []
        for k in range(n_sub):
            x, y, yaw = poses[m * n_sub + k]
            # pose of sweep k in the frame of the submap's last sweep (f64), as the 3 x 4 f32 matrix the rasteriser applies
            c, s = np.cos(-ref[2]), np.sin(-ref[2])
            dx, dy = x - ref[0], y - ref[1]
            T = rigid(yaw - ref[2], t=(c * dx - s * dy, s * dx + c * dy, 0.0), dtype=np.float32).reshape(12)
            lay = LAYOUTS[(m + k) % 4]
            segs.append((_dev(repack(sweeps[m * n_sub + k], lay[0], lay[1])), lay, T if k < n_sub - 1 else None))
            q.append(apply_tf(sweeps[m * n_sub + k], T) if k < n_sub - 1 else sweeps[m * n_sub + k] * np.array([1, 1, 1, 0], np.float32))
        scans.append(segs)
        Q.append(np.concatenate(q, 0))
        assert len(Q[-1]) == 120000
    ctx = cc.Context(0, max_batch=n_maps)
    desc = _check(cc, oracle, ctx, scans, Q, "submap")
    # the submap holds more than its last sweep alone
    d = cc.desc_to_numpy(desc)
    alone = cc.desc_to_numpy(ctx.ingest(xyzi[n_sub - 1].contiguous(), np.array([0, 30000], np.int64)))
    assert d[0]["n_pix"] > alone[0]["n_pix"]
    ctx.close()


def test_drive_ingested_as_segments(cc, oracle):
    """every scan of a drive as the three sensors of a rig -> add -> query at its own epoch, against the oracle's run on the Q clouds"""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n = 72
    xyzi, _, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    drive = xyzi.cpu().numpy()
    P = drive.shape[1]
    extr = _extrinsics(41)
    scans, Q = [], []
    for i in range(n):
        segs, q = _rig(drive[i], extr, k0=i)
        scans.append(segs)
        Q.append(q)
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(np.concatenate(Q, 0), offs, ts, seeds, dcfg=dcfg, want_desc=True)
    m = ores["n_res"] > 0
    assert m.sum() >= 3, "the oracle's drive must close loops, or the comparison below shows nothing"
    ctx = cc.Context(0, max_batch=n)
    desc = ctx.ingest_segments(scans)
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
    # the host-records call gives the descriptors of the device call
    host = ctx.ingest_segments_host([[(p.cpu().numpy(), lay, tf) for (p, lay, tf) in sc] for sc in scans[:3]])
    for i in range(3):
        assert not compare_desc(d[i], host[i], float_exact=True), i
    db.close()
    ctx.close()
