"""GPU: records dropped by a label, ring, tag or intensity word of their own while they are rasterised (cc_ingest_points_filtered through
Context.ingest(keep=) / ingest_host(keep=)): the cases of tests/point_filter.py against the CPU oracle on the kept records alone and,
as bytes, against cc_ingest_points on the records whose dropped x are NaN; one full-size scan; one end-to-end drive whose scans carry
injected moving clutter.  Scans of 9 001 - 13 000 points: several 4 096-point chunks, and the split path's part boundaries fall inside
the data; 4 scans take the split sweep + merge kernel, 9 one workgroup per scan."""
import numpy as np
import pytest

import point_filter as PF
from k1_instances import manager_cfg
from parity import compare_desc
from point_filter import Case

pytestmark = pytest.mark.gpu
BATCHES = (4, 9)


def _dev(buf, shift=0):
    """numpy uint8 records -> CUDA tensor whose first byte sits `shift` bytes behind a 16-byte boundary"""
    import torch
    t = torch.empty(len(buf) + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + len(buf)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
    return v


class GpuDriver:
    """how point_filter.check_case reaches the library on the device: through the Python API, into zeroed descriptors"""
    float_exact = False

    def __init__(self, cc):
        self.cc = cc

    def context(self, cfg, n):
        return self.cc.Context(0, cfg, max_batch=n)

    def close(self, ctx):
        ctx.close()

    def _ingest(self, ctx, case, buf, **kw):
        import torch
        cc = self.cc
        n = len(case.scans)
        x = _dev(buf, case.base_shift)
        out = torch.zeros((n, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        plain = ctx.ingest(x, case.offs(), out=out, layout=case.layout, tf=case.tfs, **kw).clone()
        out.zero_()
        d, dbg = ctx.ingest(x, case.offs(), out=out, debug=True, layout=case.layout, tf=case.tfs, **kw)
        torch.cuda.synchronize()
        assert torch.equal(plain, d), (case.name, "with / without debug outputs")
        return cc.desc_to_numpy(d), {k: v.cpu().numpy() for k, v in dbg.items()}

    def filtered(self, ctx, case, buf):
        return self._ingest(ctx, case, buf, keep=case.rule.python(self.cc))

    def points(self, ctx, case, buf):
        return self._ingest(ctx, case, buf)


@pytest.fixture(scope="module")
def drv(cc):
    return GpuDriver(cc)


EDGES = {"maxima": PF.case_dropped_maxima, "first of equals": PF.case_first_of_equals, "extremes": PF.case_extremes, "boundaries": PF.case_boundaries}


@pytest.mark.parametrize("reso", ["pow2", "div"])   # resolution 1.0, and 1.5 x 0.75 (an IEEE division per point)
@pytest.mark.parametrize("n_scans", BATCHES)
def test_edges(cc, oracle, drv, n_scans, reso):
    """Cases 1 - 4 in one context: a dropped record that is a cell's maximum, the first of several equal heights, the scan's extremes,
    and records at 4 095 / 4 096 / 8 191 / 8 192 and on both sides of every split-part boundary."""
    cfg = manager_cfg(cc.L, reso)
    ctx = drv.context(cfg, n_scans)
    for edge, make in EDGES.items():
        case = make(4)
        PF.assert_edge(oracle, cfg, case)
        PF.check_case(drv, oracle, cfg, case.repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_everything_kept_and_everything_dropped(cc, oracle, drv, n_scans):
    """Cases 5 and 6: everything kept is cc_ingest_points' bytes (device and host forms); everything dropped, and all but 5, are the
    bytes of cc_ingest_points on the NaN-substituted records."""
    import torch
    cfg = cc.L.default_manager_cfg()
    ctx = drv.context(cfg, n_scans)
    case = PF.case_everything("kept").repeat(n_scans)
    assert all(k.all() for k in case.keep)
    d, dbg = PF.check_case(drv, oracle, cfg, case, ctx)
    p, pdbg = drv.points(ctx, case, case.buffer())
    assert d.tobytes() == p.tobytes() and all(dbg[k].tobytes() == pdbg[k].tobytes() for k in dbg)
    dh = ctx.ingest_host(case.buffer(), case.offs(), layout=case.layout, keep=case.rule.python(cc))
    ph = ctx.ingest_host(case.buffer(), case.offs(), layout=case.layout)
    for i in range(n_scans):
        assert not compare_desc(ph[i], dh[i], float_exact=True), i
    assert dh.tobytes() == p.tobytes()
    for kind, n_kept in (("dropped", 0), ("five", 5)):
        case = PF.case_everything(kind).repeat(n_scans)
        assert all(int(k.sum()) == n_kept for k in case.keep)
        d, _ = PF.check_case(drv, oracle, cfg, case, ctx)
        assert np.all(d["n_pix"] == n_kept)
    torch.cuda.synchronize()
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_layouts(cc, oracle, drv, n_scans):
    """Case 7: {16, 0} with SemanticKITTI's u32 at 12, {32, 0} with a u8 at 17 and a u16 at 18, {48, 8} with the word in front of xyz,
    a base 4 bytes off a 16-byte boundary."""
    cfg = cc.L.default_manager_cfg()
    ctx = drv.context(cfg, n_scans)
    for variant in range(PF.N_LAYOUTS):
        case = PF.case_layout(variant)
        if variant == 0:
            PF.assert_edge(oracle, cfg, case)
        PF.check_case(drv, oracle, cfg, case.repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("half", [0, 1])
def test_shift_mask_and_table_sizes(cc, oracle, drv, half):
    """Case 8: shift / mask combinations, n_classes of 1, 32, 33 and 4 096, classes beyond the table under both keep_other values."""
    cfg = cc.L.default_manager_cfg()
    n_scans = BATCHES[half]
    ctx = drv.context(cfg, n_scans)
    for variant in range(half, PF.N_SHIFT_MASK, 2):
        PF.check_case(drv, oracle, cfg, PF.case_shift_mask(variant).repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("half", [0, 1])
def test_range_rule(cc, oracle, drv, half):
    """Case 9: a band, lo == hi, (-inf, inf), NaN words, -0.0 against lo = 0, an empty band."""
    cfg = cc.L.default_manager_cfg()
    n_scans = BATCHES[1 - half]
    ctx = drv.context(cfg, n_scans)
    for variant in range(half, PF.N_RANGES, 2):
        PF.check_case(drv, oracle, cfg, PF.case_range(variant).repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_range_rule_at_the_division_resolution(cc, oracle, drv, n_scans):
    """the range kind's two instances that divide by the resolution (the class kind's run in test_edges)"""
    cfg = manager_cfg(cc.L, "div")
    PF.check_case(drv, oracle, cfg, PF.case_range(0).repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
def test_with_a_matrix_per_scan(cc, oracle, drv, n_scans):
    """Case 10: with h_tf, the bytes of cc_ingest_points with that matrix on the kept records."""
    cfg = cc.L.default_manager_cfg()
    case = PF.case_with_tf(4)
    PF.assert_edge(oracle, cfg, case)
    case = case.repeat(n_scans)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PF.check_case(drv, oracle, cfg, case, ctx)
    kept = Case(case.name, [s[k] for s, k in zip(case.scans, case.keep)], [w[k] for w, k in zip(case.words, case.keep)], case.rule, case.layout, tfs=case.tfs)
    p, pdbg = drv.points(ctx, kept, kept.buffer())
    assert d.tobytes() == p.tobytes() and all(dbg[k].tobytes() == pdbg[k].tobytes() for k in dbg)
    drv.close(ctx)


def test_host_call_and_chunks(cc, oracle, drv):
    """Case 11 through the Python API: ingest_host(keep=) returns the batch call's descriptors; a context of 2 scans takes 3 in chunks.
    (The per-scan call is the class mirror's: tests/test_hostcpp_point_filter.py runs it on the device.)"""
    cfg = cc.L.default_manager_cfg()
    for case in (PF.case_layout(1, n_scans=3), PF.case_with_tf(3), PF.case_range(0, n_scans=3)):
        ctx = drv.context(cfg, 2)
        ref, _ = PF.check_case(drv, oracle, cfg, case, ctx)
        dh = ctx.ingest_host(case.buffer(), case.offs(), layout=case.layout, tf=case.tfs, keep=case.rule.python(cc))
        assert dh.tobytes() == ref.tobytes(), case.name
        drv.close(ctx)


def test_refused_arguments(cc, drv):
    """Case 12 through the Python API: what the library refuses is a CCError, what the package refuses a ValueError, and the context works afterwards."""
    import torch
    cfg = cc.L.default_manager_cfg()
    case = PF.case_layout(1, n_scans=2)   # {32, 0}, a u8 at 17
    ctx = drv.context(cfg, 2)
    x, offs = _dev(case.buffer()), case.offs()
    good = case.rule.python(cc)
    out = torch.zeros((2, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    ref = ctx.ingest(x, offs, out=out, layout=case.layout, keep=good).clone()
    F = cc.PointFilter
    for bad in (F.classes(32, "u8", keep=[0]), F.classes(17, "u16", keep=[0]), F.classes(8, "u8", keep=[0]), F.classes(17, "u8", keep=[0], shift=8),
                F.classes(20, "u32", keep=[0], shift=32), F.range(18, 0.0, 1.0), F.range(4, 0.0, 1.0), F.range(20, float("nan"), 1.0),
                F.range(20, 0.0, float("nan"))):
        with pytest.raises(cc.CCError):
            ctx.ingest(x, offs, layout=case.layout, keep=bad)
        with pytest.raises(cc.CCError):
            ctx.ingest_host(case.buffer(), offs, layout=case.layout, keep=bad)
    with pytest.raises(cc.CCError):
        ctx.ingest(x, offs, layout=(22, 0), keep=good)
    for kw in (dict(keep=good, motion=(20, "f32"), t_begin=[0.0, 0.0], scale=[1.0, 1.0], knots=np.zeros((2, 1, 12), np.float32)), dict(keep="moving")):
        with pytest.raises(ValueError):
            ctx.ingest(x, offs, layout=case.layout, **kw)
        with pytest.raises(ValueError):
            ctx.ingest_host(case.buffer(), offs, layout=case.layout, **kw)
    out.zero_()
    assert torch.equal(ref, ctx.ingest(x, offs, out=out, layout=case.layout, keep=good))
    drv.close(ctx)


def test_one_full_size_scan(cc, oracle, drv):
    """The suite's one 120 000-point scan, with SemanticKITTI's rule on clustered moving labels, alone (split path) and with 8 short ones."""
    cfg = cc.L.default_manager_cfg()
    xyzi, _, _ = cc.synth.make_sequence(1, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
    big = xyzi[0].cpu().numpy()[:119997]
    rng = np.random.default_rng(77)
    small = PF.case_layout(0, n_scans=8)
    for n_scans in (1, 9):
        scans = [big] + small.scans[:n_scans - 1]
        words = [PF.kitti_labels(rng, big)] + small.words[:n_scans - 1]
        case = Case("full size", scans, words, small.rule)
        assert 0.05 < 1.0 - case.keep[0].mean() < 0.3
        PF.check_case(drv, oracle, cfg, case)


def test_drive_with_moving_clutter(cc, oracle):
    """Case 13: a short drive whose scans carry injected "moving" clutter of classes 252 - 259 -- boxes of points above the ground near
    the sensor, a tenth of each scan, spliced in between the scan's own records -- ingested with the filter, added and queried: the
    query results equal those of the drive ingested from the clean clouds, and the oracle's on the clean clouds.  Without the filter
    the cluttered scans give other descriptors."""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n = 72
    xyzi, poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    clean = xyzi.cpu().numpy()
    P = clean.shape[1]
    Q = P // 10
    rng = np.random.default_rng(31)
    dirty = np.zeros((n, P + Q, 4), np.float32)
    for i in range(n):
        boxes = rng.uniform([-40.0, -40.0], [40.0, 40.0], (6, 2))
        b = rng.integers(0, 6, Q)
        clutter = np.zeros((Q, 4), np.float32)
        clutter[:, :2] = boxes[b] + rng.uniform(-2.0, 2.0, (Q, 2))
        clutter[:, 2] = rng.uniform(0.0, 4.0, Q)
        label = np.concatenate([rng.integers(0, 100, P), rng.integers(252, 260, Q)]).astype(np.uint32) | (rng.integers(1, 2 ** 16, P + Q).astype(np.uint32) << np.uint32(16))
        rec = np.concatenate([clean[i], clutter], 0)
        rec[:, 3] = label.view(np.float32)
        dirty[i] = rec[_splice(rng, P, Q)]
    offs_c = np.arange(n + 1, dtype=np.int64) * P
    offs_d = np.arange(n + 1, dtype=np.int64) * (P + Q)
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(clean.reshape(-1, 4), offs_c, ts, seeds, dcfg=dcfg, want_desc=True)
    m = ores["n_res"] > 0
    assert m.sum() >= 3, "the oracle's drive must close loops, or the comparison below shows nothing"
    ctx = cc.Context(0, max_batch=n)
    keep = cc.PointFilter.classes(12, "u32", drop=PF.MOVING, mask=0xFFFF)
    xd = torch.from_numpy(dirty.reshape(-1, 4)).cuda()
    desc = ctx.ingest(xd, offs_d, keep=keep)
    desc_clean = ctx.ingest(xyzi.reshape(-1, 4), offs_c)
    results = []
    for dsc in (desc, desc_clean):
        db = cc.Database(ctx, dcfg, capacity=n)
        db.add_scans(dsc, ts, seeds)
        results.append(db.query(dsc, seeds))
        torch.cuda.synchronize()
        db.close()
    res, res_clean = results
    for f in res.dtype.names:
        assert np.array_equal(res[f], res_clean[f], equal_nan=res[f].dtype.kind == "f"), f
    d = cc.desc_to_numpy(desc)
    for i in range(n):
        bad = compare_desc(odesc[i], d[i], float_exact=False)
        assert not bad, "scan %d: %s" % (i, bad[:5])
    for f in ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy", "n_knn_hits"]:
        assert np.array_equal(ores[f], res[f]), f
    plain = cc.desc_to_numpy(ctx.ingest(xd, offs_d))
    n_diff = sum(1 for i in range(n) if compare_desc(odesc[i], plain[i], float_exact=False))
    assert n_diff >= n // 2, n_diff
    ctx.close()


def _splice(rng, P, Q):
    """an order of P + Q records that keeps the first P in their order and puts the other Q between them at random places"""
    is_clutter = np.zeros(P + Q, bool)
    is_clutter[rng.choice(P + Q, Q, replace=False)] = True
    order = np.zeros(P + Q, np.int64)
    order[~is_clutter] = np.arange(P)
    order[is_clutter] = P + np.arange(Q)
    return order
