"""GPU: a rig's sensors de-skewed, filtered and joined in one sweep (cc_ingest_rig through Context.ingest_rig / ingest_rig_host): the
cases of tests/point_rig.py against the CPU oracle on the kept, moved points and, as bytes, against cc_ingest_batch on the numpy-built
cloud Q whose dropped x are NaN; one full-size scan of two sensors; one short drive ingested this way, added and queried, against the
same drive ingested from Q.  Scans of 9 001 - 13 000 records: several 4 096-point chunks, and the split path's part boundaries fall
inside the data; 4 scans take the split sweep + merge kernel, 9 one workgroup per scan."""
import numpy as np
import pytest

import point_rig as PR
from k1_instances import manager_cfg
from point_filter import kitti_labels
from point_layouts import rigid
from point_motion import TIME_F32, TIME_U32, u32_bits_as_f32
from point_rig import Case, Motion, Seg

pytestmark = pytest.mark.gpu
BATCHES = (4, 9)


def _dev(buf, shift=0):
    """numpy uint8 records -> CUDA tensor of its own whose first byte sits `shift` bytes behind a 16-byte boundary"""
    import torch
    t = torch.empty(len(buf) + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + len(buf)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
    return v


def _mode(cc, s):
    if s.motion is not None:
        m = s.motion
        tb = np.float32(m.t_begin).reshape(1).view(np.uint32)[0] if m.time_type == TIME_U32 else m.t_begin
        return cc.SegMotion(m.time_offset, "u32" if m.time_type == TIME_U32 else "f32", tb, m.scale, m.knot0, m.n_knots)
    return s.tf


def py_scans(cc, case, device=True):
    """the case as Context.ingest_rig / ingest_rig_host take it: every segment's records in a tensor (array) of its own"""
    return [[((_dev(s.buffer(), s.shift) if device else s.buffer()) if len(s) else None, s.layout, _mode(cc, s), None if s.flt is None else s.flt[0]) for s in sc]
            for sc in case.scans]


class GpuDriver:
    """how point_rig.check_case reaches the library on the device: through the Python API, into zeroed descriptors"""
    float_exact = False

    def __init__(self, cc):
        self.cc = cc

    def context(self, cfg, n):
        return self.cc.Context(0, cfg, max_batch=n)

    def close(self, ctx):
        ctx.close()

    def _twice(self, call, n, name):
        import torch
        out = torch.zeros((n, self.cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        plain = call(out=out).clone()
        out.zero_()
        d, dbg = call(out=out, debug=True)
        torch.cuda.synchronize()
        assert torch.equal(plain, d), (name, "with / without debug outputs")
        return self.cc.desc_to_numpy(d), {k: v.cpu().numpy() for k, v in dbg.items()}

    def rig(self, ctx, case):
        scans = py_scans(self.cc, case)
        keep = None if case.rule is None else case.rule.python(self.cc)
        return self._twice(lambda **kw: ctx.ingest_rig(scans, knots=case.pools, keep=keep, **kw), len(case.scans), case.name)

    def batch(self, ctx, clouds):
        import torch
        offs = np.concatenate([[0], np.cumsum([len(q) for q in clouds])]).astype(np.int64)
        x = torch.from_numpy(np.concatenate(clouds, 0)).cuda()
        return self._twice(lambda **kw: ctx.ingest(x, offs, **kw), len(clouds), "cc_ingest_batch")


@pytest.fixture(scope="module")
def drv(cc):
    return GpuDriver(cc)


EDGES = {"boundaries": PR.case_boundaries, "ties dropped": lambda: PR.case_ties(True), "ties": lambda: PR.case_ties(False), "empties": PR.case_empties}


@pytest.mark.parametrize("reso", ["pow2", "div"])   # resolution 1.0, and 1.5 x 0.75 (an IEEE division per point)
@pytest.mark.parametrize("n_scans", BATCHES)
def test_edges(cc, oracle, drv, n_scans, reso):
    """In one context: segment boundaries at every chunk and split-part boundary with a dropped record and a change of slice on both
    sides; ties across segments with and without the earlier record dropped; empty segments and a segment all dropped."""
    cfg = manager_cfg(cc.L, reso)
    ctx = drv.context(cfg, n_scans)
    for edge, make in EDGES.items():
        case = make()
        PR.assert_edge(oracle, cfg, case)
        PR.check_case(drv, oracle, cfg, case.repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_slices_and_limits(cc, oracle, drv, n_scans):
    """Times beyond a slice's end clamp to ITS last knot (a clamp to the pool's size puts hundreds of records into other cells); scans
    whose records are all dropped; CC_RIG_SEG_MAX segments on a pool of 64."""
    cfg = cc.L.default_manager_cfg()
    ctx = drv.context(cfg, n_scans)
    case = PR.case_slices()
    PR.assert_slices(cfg, case)
    PR.check_case(drv, oracle, cfg, case.repeat(n_scans), ctx)
    d, _ = PR.check_case(drv, oracle, cfg, PR.case_all_dropped().repeat(n_scans), ctx)
    assert np.all(d["n_pix"] == 0) and np.all(d["n_cont"] == 0)
    case = PR.case_max_segments()
    assert all(len(sc) == cc.L.RIG_SEG_MAX for sc in case.scans) and case.n_pool() == 64
    PR.check_case(drv, oracle, cfg, case.repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_mixed_scan(cc, oracle, drv, n_scans):
    """none, tf, f32-time and u32-time segments, five record shapes, the filter word at another offset per segment, one unfiltered
    segment; u8 / u16 / u32 class words and the range rule."""
    for kind in PR.MIXED_KINDS:
        cfg = manager_cfg(cc.L, "div" if kind == "u16" else "pow2")
        PR.check_case(drv, oracle, cfg, PR.case_mixed(kind).repeat(n_scans))


def _same(a, b):
    (d, dbg), (e, ebg) = a, b
    assert d.tobytes() == e.tobytes(), "descriptors differ"
    for k in dbg:
        assert dbg[k].tobytes() == ebg[k].tobytes(), k


def _packed(case):
    """one-segment scans as one record buffer with offsets"""
    return np.concatenate([sc[0].buffer() for sc in case.scans]), np.concatenate([[0], np.cumsum([len(sc[0]) for sc in case.scans])]).astype(np.int64)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_equivalences(cc, oracle, drv, n_scans):
    """As bytes against the existing calls: only none / tf segments and no rule = cc_ingest_segments; one motion segment with knot0 0 =
    cc_ingest_points_motion; one tf segment with a rule = cc_ingest_points_filtered."""
    cfg = cc.L.default_manager_cfg()
    ctx = drv.context(cfg, n_scans)
    mixed = PR.case_mixed("u32")
    case = Case("no motion, no rule", [[Seg(s.xyzi, s.layout, s.shift, tf=s.tf if s.motion is None else PR.shift_knots(1, 5)[0]) for s in sc] for sc in mixed.scans]).repeat(n_scans)
    segs = [[(t, lay, mode) for (t, lay, mode, _k) in sc] for sc in py_scans(cc, case)]
    _same(PR.check_case(drv, oracle, cfg, case, ctx), drv._twice(lambda **kw: ctx.ingest_segments(segs, **kw), n_scans, "cc_ingest_segments"))

    sl = PR.case_slices()
    case = Case("one motion segment", [[Seg(sc[0].xyzi, (32, 0), motion=Motion(28, TIME_F32, 2.0, 16 / 0.1, 0, 16, sc[0].motion.words))] for sc in sl.scans], sl.pools[:, :16]).repeat(n_scans)
    buf, offs = _packed(case)
    x = _dev(buf)
    _same(PR.check_case(drv, oracle, cfg, case, ctx),
          drv._twice(lambda **kw: ctx.ingest(x, offs, layout=(32, 0), motion=(28, "f32"), t_begin=np.full(n_scans, 2.0, np.float32), scale=np.full(n_scans, 160.0, np.float32),
                                             knots=case.pools, **kw), n_scans, "cc_ingest_points_motion"))

    m8 = PR.case_mixed("u8")
    tfs = PR.shift_knots(4, 9)
    case = Case("one tf segment", [[Seg(sc[1].xyzi, (32, 0), tf=tfs[i], flt=sc[1].flt, fill=3)] for i, sc in enumerate(m8.scans)], None, m8.rule).repeat(n_scans)
    buf, offs = _packed(case)
    x = _dev(buf)
    keep = cc.PointFilter.classes(17, "u8", drop=range(200, 208), n_classes=208, mask=0xFF)
    _same(PR.check_case(drv, oracle, cfg, case, ctx),
          drv._twice(lambda **kw: ctx.ingest(x, offs, layout=(32, 0), tf=np.stack([tfs[i % 4] for i in range(n_scans)]), keep=keep, **kw), n_scans, "cc_ingest_points_filtered"))
    drv.close(ctx)


def test_host_form_and_chunks(cc, oracle, drv):
    """ingest_rig_host returns the device form's descriptors; 3 scans go through a context of 2 in chunks.  (The per-scan form is the class
    mirror's and the CPU harness': tests/test_emu_point_rig.py.)"""
    cfg = cc.L.default_manager_cfg()
    for case in (PR.case_mixed("u16", n_scans=3), PR.case_empties(n_scans=3), PR.case_mixed("range", n_scans=3)):
        ctx = drv.context(cfg, 2)
        ref, _ = PR.check_case(drv, oracle, cfg, case, ctx)
        dh = ctx.ingest_rig_host(py_scans(cc, case, device=False), knots=case.pools, keep=case.rule.python(cc))
        assert dh.tobytes() == ref.tobytes(), case.name
        drv.close(ctx)


def test_refused_arguments(cc, drv):
    """What the library refuses is a CCError, what the package refuses a ValueError, and the context works afterwards.  A sample of the
    refusals: the checks are host code shared by the device, host and per-scan forms, and the whole list runs against all three entry
    points on the CPU harness (tests/test_emu_point_rig.py::test_refusals)."""
    import torch
    cfg = cc.L.default_manager_cfg()
    case = PR.case_mixed("u16", n_scans=2)
    ctx = drv.context(cfg, 2)
    scans, keep = py_scans(cc, case), case.rule.python(cc)
    out = torch.zeros((2, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    ref = ctx.ingest_rig(scans, knots=case.pools, keep=keep, out=out).clone()

    def with_seg(k, **over):
        sc = [list(s) for s in scans[0]]
        for name, v in over.items():
            sc[k][{"layout": 1, "mode": 2, "keep_offset": 3}[name]] = v
        return [[tuple(s) for s in sc], scans[1]]

    M = cc.SegMotion
    bad = [dict(scans=with_seg(2, mode=M(16, "f32", 5.0, 240.0, 0, 24))),            # the time word on z
           dict(scans=with_seg(2, mode=M(4, "f32", 5.0, 240.0, 9, 24))),             # a slice outside the pool
           dict(scans=with_seg(2, mode=M(4, "f32", 5.0, float("inf"), 0, 24))),      # an infinite scale
           dict(scans=with_seg(1, keep_offset=6)),                                    # the filter word on y
           dict(scans=with_seg(3, keep_offset=20)),                                   # ... beyond the record
           dict(scans=with_seg(1, keep_offset=17)),                                   # a u16 at an odd offset
           dict(scans=[scans[0] * 4, scans[1]]),                                      # 20 segments
           dict(knots=None), dict(keep=None)]
    for kw in bad:
        args = dict(scans=scans, knots=case.pools, keep=keep)
        args.update(kw)
        with pytest.raises(cc.CCError):
            ctx.ingest_rig(args["scans"], knots=args["knots"], keep=args["keep"])
    with pytest.raises(cc.CCError):
        ctx.ingest_rig_host(py_scans(cc, case, device=False), knots=None, keep=keep)
    for kw in (dict(keep="moving"), dict(knots=np.zeros((2, 7), np.float32)), dict(knots=np.zeros((3, 12), np.float32))):
        args = dict(knots=case.pools, keep=keep)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.ingest_rig(scans, **args)
    with pytest.raises(ValueError):
        cc.SegMotion(4, "f64", 0.0, 1.0, 0, 1)
    out.zero_()
    assert torch.equal(ref, ctx.ingest_rig(scans, knots=case.pools, keep=keep, out=out))
    drv.close(ctx)


def _two_sensors(scan, rng, share=0.07):
    """a scan cut into two sensors' sweeps: the first half as {32, 0} records (f32 time at 12, label at 16) on the slice [0, 16), the second
    as {48, 8} records (u32 time at 4, label at 0) on [16, 32); times run with the records' order over a 0.1 s sweep, a little past its ends"""
    h = len(scan) // 2
    lab = kitti_labels(rng, scan, share=share, high=False)
    ta = (np.linspace(-0.002, 0.103, h) + 7.0).astype(np.float32)
    tb = (np.uint64(4286000000) + np.linspace(0, 1.02e8, len(scan) - h).astype(np.uint64)).astype(np.uint32)   # wraps past 2^32 inside the sweep
    return [Seg(scan[:h], (32, 0), motion=Motion(12, TIME_F32, 7.0, 160.0, 0, 16, ta.view(np.uint32)), flt=(16, lab[:h])),
            Seg(scan[h:], (48, 8), motion=Motion(4, TIME_U32, u32_bits_as_f32(4286000000), 16 / 1e8, 16, 16, tb), flt=(0, lab[h:]))]


def _sweep_knots(rng, n_knots=32):
    """small rigid motions around two extrinsics: what a de-skew at 15 m/s and 0.5 rad/s brings"""
    ext =[(0.0, (1.2, 0.0, 0.0)), (0.02, (-0.8, 0.3, 0.1))]
    return np.stack([rigid(ext[k // 16][0] + 0.003 * (k % 16), t=(ext[k // 16][1][0] + 0.09 * (k % 16), ext[k // 16][1][1], ext[k // 16][1][2]), dtype=np.float32).reshape(12)
                     for k in range(n_knots)])


def test_one_full_size_scan(cc, oracle, drv):
    """Two sensors of 60 000 points, 16 knots each, SemanticKITTI's rule: alone (split path) and with 8 short scans."""
    cfg = cc.L.default_manager_cfg()
    xyzi, _, _ = cc.synth.make_sequence(1, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
    big = xyzi[0].cpu().numpy()[:120000]
    assert len(big) == 120000
    rng = np.random.default_rng(78)
    small = PR.case_max_segments(n_scans=4)   # 16 segments on a pool of 64: the full-size scan's pool is padded to it
    pool = np.concatenate([_sweep_knots(rng), np.zeros((32, 12), np.float32)])
    for n_scans in (1, 9):
        idx = [i % 4 for i in range(n_scans - 1)]
        case = Case("full size", [_two_sensors(big, rng)] + [small.scans[i] for i in idx], np.stack([pool] + [small.pools[i] for i in idx]), small.rule)
        assert len(case.scans[0][0]) == 60000 and 0.04 < 1.0 - case.keep(0).mean() < 0.3
        PR.check_case(drv, oracle, cfg, case)


def test_drive_of_two_sensors(cc, oracle):
    """A short drive whose every scan comes as two sensors' sweeps with time words and labels, ingested by ingest_rig, added and queried:
    the descriptors and the query results equal those of the same drive ingested from the numpy-built Q, and loops are closed."""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n = 72
    xyzi, _poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    clouds = xyzi.cpu().numpy()
    rng = np.random.default_rng(33)
    pool = _sweep_knots(rng)
    case = Case("drive", [_two_sensors(clouds[i], rng, share=0.03) for i in range(n)], np.stack([pool] * n), PR.drop_classes(0, PR.U32, mask=0xFFFF))
    PR.assert_keeps(case, at_least=1000)
    qs = [case.q(i) for i in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=n)
    out = torch.zeros((n, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    desc = ctx.ingest_rig(py_scans(cc, case), knots=case.pools, keep=case.rule.python(cc), out=out)
    desc_q = ctx.ingest(torch.from_numpy(np.concatenate(qs, 0)).cuda(), offs, out=torch.zeros_like(out))
    torch.cuda.synchronize()
    assert torch.equal(desc, desc_q)
    results = []
    for dsc in (desc, desc_q):
        db = cc.Database(ctx, dcfg, capacity=n)
        db.add_scans(dsc, ts, seeds)
        results.append(db.query(dsc, seeds))
        torch.cuda.synchronize()
        db.close()
    res, res_q = results
    for f in res.dtype.names:
        assert np.array_equal(res[f], res_q[f], equal_nan=res[f].dtype.kind == "f"), f
    assert (res["n_res"] > 0).sum() >= 3, "the drive must close loops, or the comparison shows nothing"
    ctx.close()
