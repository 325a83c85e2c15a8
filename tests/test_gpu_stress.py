"""Real-shaped stress on the GPU (VERDICT r2, weak points 2 and 3): scans with the occupancy and contour counts of real
KITTI scans (4-9 k occupied cells, 100+ contours on a level -- the looping synthetic worlds top out at 2.7 k / 52), every
capacity of the kernels hit on hardware, and a number for what a last-ulp difference of a retrieval key can change.

  * n_act > CC_K2_CACHE (3 072 active cells): the cross-level walk's spill path (k_contours.h);
  * more than CC_MAXC = 320 components on a level -> the exact slow path (cc_k_contours_big), nothing refused;
  * a key RoI with more than CC_KEYS_CAP = 416 cells (roi_radius_ = 12) -> CC_DESC_INEXACT_KEYS;
  * the pair pool of the correlation refinement overflowing -> CC_ECAPACITY from the collecting call;
  * stage B1's 256-pair instance and the 64-pair constellation cap on crowded BCIs, against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RING_DIFF_CAP = 1e-3   # ring components of the keys whose bits may differ from the oracle's (test_gpu_query.py says why)


def _keys_to_the_bit(oracle_scan, od, got):
    """tests/key_reference.py on the oracle's inputs: the oracle's keys pass it, then the device's -- bit for bit except components
    that are provably ambiguous -> (ambiguous components, ring components whose bits differ from the oracle's, non-zero ones)"""
    import key_reference as KR
    from parity import compare_desc
    keys, amb, _ = KR.scan_reference(oracle_scan, od, oracle_scan.cfg)
    KR.check_keys(keys, amb, od["keys"])
    n_amb = KR.check_keys(keys, amb, got["keys"])
    _, n_diff, n_ring = compare_desc(od, got, float_exact=False, ring_count=True)
    return n_amb, n_diff, n_ring


INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy",
              "n_knn_hits"]


def real_shaped_scan(seed, n_cells=7500, pts_per_cell=16, scale=1.5, fmax=0.8):
    """120 000 points over ~7 500 cells: KITTI-like occupancy (4-9 k cells, spatially coherent: the cells where a smooth random
    field is high), heights from a rough random field (tens to 100+ contours per level), point noise inside a cell."""
    rng = np.random.default_rng(seed)
    rr, cc_ = np.meshgrid(np.arange(150), np.arange(150), indexing="ij")
    gx, gy = rr - 75 + 0.5, cc_ - 75 + 0.5
    g = np.zeros((150, 150))
    for _ in range(6):
        f = rng.uniform(0.03, 0.16, 2)
        ph = rng.uniform(0, 6.28, 2)
        g += np.sin(f[0] * gx + ph[0]) * np.sin(f[1] * gy + ph[1])
    g += 0.15 * rng.standard_normal(g.shape)
    cells = np.nonzero(g.ravel() >= np.sort(g.ravel())[-n_cells])[0]
    cx = (cells // 150).astype(np.float64) - 75 + 0.5
    cy = (cells % 150).astype(np.float64) - 75 + 0.5
    xy = np.stack([np.repeat(cx, pts_per_cell), np.repeat(cy, pts_per_cell)], 1) + rng.uniform(-0.49, 0.49, (len(cells) * pts_per_cell, 2))
    z = np.zeros(len(xy))
    for _ in range(14):
        f = rng.uniform(0.05, fmax, 2)
        ph = rng.uniform(0, 6.28, 2)
        z += rng.uniform(0.25, 0.9) * np.sin(f[0] * xy[:, 0] + ph[0]) * np.sin(f[1] * xy[:, 1] + ph[1])
    z = z * scale + rng.normal(0, 0.1, len(z))
    pts = np.zeros((len(xy), 4), np.float32)
    pts[:, :2] = xy
    pts[:, 2] = z
    return pts


def _ingest(cc, scans, mcfg=None):
    import torch
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    x = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans), np.float32)).cuda()
    ctx = cc.Context(0, mcfg, max_batch=8)
    d, dbg = ctx.ingest(x, offs, debug=True)
    torch.cuda.synchronize()
    return ctx, d, dbg


def test_real_shaped_scans_bit_exact(cc, oracle):
    from parity import compare_desc
    scans = [real_shaped_scan(s) for s in range(4)] + [real_shaped_scan(10, n_cells=8900, pts_per_cell=13, scale=2.0),
                                                        real_shaped_scan(11, fmax=1.1)]
    assert all(len(s) > 110000 for s in scans)
    ctx, d, dbg = _ingest(cc, scans)
    got = cc.desc_to_numpy(d)
    lab = dbg["labels"].cpu().numpy()
    most = 0
    tally = np.zeros(3, np.int64)
    for i, s in enumerate(scans):
        o = oracle.Scan(s)
        od = o.desc()[0]
        assert 4000 <= od["n_pix"] <= 9000, od["n_pix"]                 # occupied cells: SURVEY.md 8(d)'s real-scan range
        assert od["layer_cell_cnt"][0] > 3072, od["layer_cell_cnt"]     # active cells beyond CC_K2_CACHE: the spill path of the walk
        assert 50 <= od["n_cont"].max() <= 320 and od["flags"] == 0, od["n_cont"]
        most = max(most, int(od["n_cont"].max()))
        bad = compare_desc(od, got[i], float_exact=False)
        assert not bad, "scan %d: %s" % (i, bad[:5])
        assert np.array_equal(o.labels(), lab[i]), "canonical label images differ (scan %d)" % i
        tally += _keys_to_the_bit(o, od, got[i])        # the mid path (window probing) at real occupancy
    assert most >= 100, most   # 100+ contours on a level somewhere
    print("real-shaped scans: %d ambiguous, %d of %d non-zero ring components differ from the oracle's in their bits" % tuple(tally))
    assert tally[2] > 500 and tally[1] <= RING_DIFF_CAP * tally[2] and tally[0] <= RING_DIFF_CAP * tally[2], tally
    ctx.close()


def _blob_field(n_blobs, height=2.3):
    """n_blobs isolated 3-cell L-shaped blobs at `height` (above the two lowest levels), 3 cells apart"""
    pts = []
    per_row = 45
    for b in range(n_blobs):
        r, c = 4 + 3 * (b // per_row), 4 + 3 * (b % per_row)
        for dr, dc in ((0, 0), (0, 1), (1, 0)):
            x, y = (r + dr) - 75 + 0.5, (c + dc) - 75 + 0.5
            if x * x + y * y < 16:
                continue
            pts.append((x, y, height - 2.0 + 0.001 * (b % 7), 0.0))
    return np.asarray(pts, np.float32)


def test_component_and_key_capacities_are_flagged(cc, oracle):
    from parity import compare_desc
    L = cc.L
    # (a) 400 components on the two lowest levels (rounds 1-4: CC_DESC_INEXACT_COMPONENTS, refused everywhere): the slow path
    #     makes the descriptor exact -- bit for bit the oracle's, labels included --, the host-buffer entry point and the DB
    #     take it, and it can be queried
    blobs = _blob_field(400)
    ctx, d, dbg = _ingest(cc, [blobs, real_shaped_scan(3), _blob_field(700, height=3.2)])
    got = cc.desc_to_numpy(d)
    lab = dbg["labels"].cpu().numpy()
    tally = np.zeros(3, np.int64)
    for i, s in ((0, blobs), (2, _blob_field(700, height=3.2))):
        o = oracle.Scan(s)
        od = o.desc()[0]
        assert od["n_cont"].max() > 320 and od["flags"] == 1            # CC_DESC_TRUNCATED: the 320 largest are stored
        bad = compare_desc(od, got[i], float_exact=False)
        assert not bad, bad[:5]
        assert got["flags"][i] == 1, got["flags"]
        assert np.array_equal(o.labels(), lab[i])
        tally += _keys_to_the_bit(o, od, got[i])                        # the slow path's keys
    print("blob fields: %d ambiguous, %d of %d non-zero ring components differ from the oracle's in their bits" % tuple(tally))
    assert tally[1] <= RING_DIFF_CAP * tally[2] and tally[0] <= RING_DIFF_CAP * tally[2], tally
    assert got["flags"][1] == 0
    hd = ctx.ingest_host(blobs, np.array([0, len(blobs)], np.int64))
    assert not compare_desc(oracle.Scan(blobs).desc()[0], hd[0], float_exact=False)
    db = cc.Database(ctx, capacity=8)
    db.add_scans(d[:2], np.zeros(2), np.zeros(2, np.int32))
    assert len(db) == 2
    db.query(d[:1], np.full(1, 2, np.int32))                            # no CC_QF_QUERY_INEXACT any more: the call does not raise
    db.close()
    ctx.close()
    # (b) roi_radius_ = 12: a key RoI holds up to ~450 cells, more than the kernel's list
    mcfg = L.default_manager_cfg()
    mcfg.roi_radius = 12.0
    dense = real_shaped_scan(5, n_cells=21000, pts_per_cell=5, scale=1.5)
    dense[:, 2] += 1.0   # most cells above lv_grads_[1]
    ctx, d, _ = _ingest(cc, [dense], mcfg)
    got = cc.desc_to_numpy(d)
    assert got["flags"][0] & 4, got["flags"]                            # CC_DESC_INEXACT_KEYS
    ctx.close()


def test_pair_pool_overflow_is_reported(cc, monkeypatch):
    """The pair lists of the refined correlation problems come from a pool; running out of it must be an error
    (CC_ECAPACITY), never a shorter list.  Forced with a 32-pair pool (CC_GMM_POOL_PAIRS, read at cc_db_create) on a scan
    checked against its own copy through explicit hints (no retrieval, no time gating)."""
    L = cc.L
    scan = real_shaped_scan(20)
    ctx, d, _ = _ingest(cc, [scan])
    hints = np.zeros(3, L.hint_dt)
    hints["cand_gidx"], hints["level"], hints["seq_src"], hints["seq_tgt"] = 0, [1, 2, 3], 0, 0
    monkeypatch.setenv("CC_GMM_POOL_PAIRS", "32")
    db = cc.Database(ctx, capacity=8)
    db.add_scans(d[:1], np.zeros(1), np.zeros(1, np.int32))
    with pytest.raises(cc.CCError, match="pool"):
        db.check_hints(d[0], hints)
    monkeypatch.delenv("CC_GMM_POOL_PAIRS")
    # ... and the pool of pair codes cc_k_gmm_init files for the refinement (round 6): 1 024 entries hold one first block
    # (258) in their static half and none of the 1 026-entry blocks a long list goes on with
    monkeypatch.setenv("CC_GMM_POOL_CODES", "1024")
    db3 = cc.Database(ctx, capacity=8)
    db3.add_scans(d[:1], np.zeros(1), np.zeros(1, np.int32))
    with pytest.raises(cc.CCError, match="pool"):
        db3.check_hints(d[0], hints)
    monkeypatch.delenv("CC_GMM_POOL_CODES")
    db3.close()
    db2 = cc.Database(ctx, capacity=8)
    db2.add_scans(d[:1], np.zeros(1), np.zeros(1, np.int32))
    r, sc = db2.check_hints(d[0], hints)
    assert r["n_res"] == 1 and r["flags"] == 0 and r["correlation"] > 0.9 and sc["passed"].all()
    db.close()
    db2.close()
    ctx.close()


def test_crowded_constellations_on_the_gpu(cc, oracle):
    """tests/test_emu_dense_constellations.py's rewrite (every anchor's neighbours crowded into three adjacent distance
    bins: 100+ potential pairs per check with many equal orientation differences) on hardware: B1's 256-pair instance, the
    sort replay on ties, the 64-pair constellation cap."""
    import torch
    from test_emu_dense_constellations import _crowd
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    w = cc.synth.World(loop_len=40.0)
    n = 56
    x, poses, ts = cc.synth.make_sequence(n, world=w, beams=16, azim=450)
    _, _, odesc = oracle.run_sequence(x.numpy().reshape(-1, 4), np.arange(n + 1, dtype=np.int64) * x.shape[1], ts,
                                      np.arange(n, dtype=np.int32), dcfg=dcfg, want_desc=True)
    desc, n_big = _crowd(odesc)
    assert n_big > 100
    odb = oracle.DB(dcfg)
    exp = []
    for i in range(n):
        s = oracle.Scan.from_desc(desc[i], int_id=i)
        exp.append(odb.query(s))
        odb.add_scan(s, ts[i])
        odb.push_and_balance(i, ts[i])
    exp = np.array(exp)
    assert exp["cand_aft_check2"].max() > 20
    dd = torch.from_numpy(np.frombuffer(desc.tobytes(), np.uint8).reshape(n, cc.DESC_BYTES).copy()).cuda()
    ctx = cc.Context(0, max_batch=8)
    db = cc.Database(ctx, cfg=dcfg, capacity=n)
    seeds = np.arange(n, dtype=np.int32)
    db.add_scans(dd, ts, seeds)
    res = db.query(dd, seeds)
    assert (res["flags"] == 0).all()
    for f in INT_FIELDS:
        assert np.array_equal(exp[f], res[f]), f
    m = exp["n_res"] > 0
    assert np.abs(exp["correlation"][m] - res["correlation"][m]).max() < 1e-4 and np.abs(exp["tf"][m] - res["tf"][m]).max() < 1e-4
    db.close()
    ctx.close()


def test_key_ulp_sensitivity(cc, oracle):
    """How much can a last-ulp difference of a retrieval key (device exp / atan2f vs glibc) change?  2 000 full-size scans
    of the looping sparse world are ingested on the GPU; the oracle replays the online loop on the device's descriptors
    twice -- as they are, and with every non-zero key component moved by a random -1 / 0 / +1 ulp.  The number of queries
    whose KNN hit count, match or outcome changes is the bound the parity note in DESIGN.md quotes."""
    n = 2000
    w = cc.synth.World(loop_len=600.0)
    ctx = cc.Context(0, max_batch=128)
    descs = []
    for c0 in range(0, n, 125):
        x, _, _ = cc.synth.make_sequence(125, world=w, device="cuda", start=c0)
        descs.append(cc.desc_to_numpy(ctx.ingest(x.reshape(-1, 4), np.arange(126, dtype=np.int64) * x.shape[1])))
    desc = np.concatenate(descs)
    ctx.close()
    rng = np.random.default_rng(1)
    pert = desc.copy()
    k = pert["keys"].view(np.int32)
    k += np.where(pert["keys"] != 0, rng.integers(-1, 2, k.shape, dtype=np.int32), 0)
    ts = np.arange(n) / 10.0

    def replay(dd):
        odb = oracle.DB()
        out = np.zeros(n, cc.L.query_result_dt)
        for i in range(n):
            s = oracle.Scan.from_desc(dd[i], int_id=i)
            out[i] = odb.query(s)
            odb.add_scan(s, ts[i])
            odb.push_and_balance(i, ts[i])
        return out
    a, b = replay(desc), replay(pert)
    closed = a["n_res"] > 0
    assert closed.sum() > 800
    d_hits = int((a["n_knn_hits"] != b["n_knn_hits"]).sum())
    d_match = int((a["cand_gidx"] != b["cand_gidx"]).sum())
    d_res = int((a["n_res"] != b["n_res"]).sum())
    same = closed & (a["cand_gidx"] == b["cand_gidx"])
    d_corr = float(np.abs(a["correlation"][same] - b["correlation"][same]).max())
    print("key +-1 ulp on %d scans (%d loop closures): n_knn_hits differs on %d queries, the matched scan on %d, a result "
          "appears/disappears on %d; max |d correlation| on unchanged matches %.2e" % (n, int(closed.sum()), d_hits, d_match, d_res, d_corr))
    # a key on the edge of the 50-th neighbour distance or of dist_ub may flip; the evaluation must not notice
    assert d_hits <= n // 50 and d_match <= n // 200 and d_res <= 2 and d_corr < 1e-6
