"""GPU: f64, scaled-i32 and split-stream coordinates converted while they are rasterised (cc_ingest_coords through
Context.ingest_coords / ingest_coords_host): the cases of tests/point_coords.py against the CPU oracle on the specified f32 points p
and, as bytes, against cc_ingest_points on the packed p; one full-size scan; one end-to-end drive ingested as local f32 clouds and as
f64 world coordinates.  Scans of 9 001 - 13 000 points: several 4 096-point chunks, and the split path's part boundaries fall inside
the data; 4 scans take the split sweep + merge kernel, 9 one workgroup per scan."""
import numpy as np
import pytest

import point_coords as PC
from k1_instances import manager_cfg
from parity import compare_desc
from point_coords import F32, F64, I32, Case

pytestmark = pytest.mark.gpu
BATCHES = (4, 9)


def _dev(buf, shift=0):
    """numpy uint8 bytes -> CUDA tensor whose first byte sits `shift` bytes behind a 16-byte boundary"""
    import torch
    t = torch.empty(len(buf) + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + len(buf)]
    v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
    return v


def _streams(case, bufs, streams, stride, n):
    """the case's three streams as 1-D strided CUDA tensors of its dtype (views of the uploaded bytes: nothing is repacked)"""
    import torch
    dt = {F32: torch.float32, F64: torch.float64, I32: torch.int32}[case.type]
    elem = np.dtype(PC.DTYPES[case.type]).itemsize
    dev = [_dev(b, case.place.base_shift) for b in bufs]
    out = tuple(dev[b][o:o + (n - 1) * stride + elem].view(dt)[::stride // elem] for b, o in streams)
    assert all(len(t) == n and t.stride(0) * elem == stride for t in out)
    return out


class GpuDriver:
    """how point_coords.check_case reaches the library on the device: through the Python API, into zeroed descriptors"""
    float_exact = False

    def __init__(self, cc):
        self.cc = cc

    def context(self, cfg, n):
        return self.cc.Context(0, cfg, max_batch=n)

    def close(self, ctx):
        ctx.close()

    def _twice(self, case, call):
        import torch
        cc = self.cc
        out = torch.zeros((len(case.raws), cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        plain = call(out=out).clone()
        out.zero_()
        d, dbg = call(out=out, debug=True)
        torch.cuda.synchronize()
        assert torch.equal(plain, d), (case.name, "with / without debug outputs")
        return cc.desc_to_numpy(d), {k: v.cpu().numpy() for k, v in dbg.items()}

    def coords(self, ctx, case):
        bufs, streams, stride = case.build()
        xyz = _streams(case, bufs, streams, stride, int(case.offs()[-1]))
        return self._twice(case, lambda **kw: ctx.ingest_coords(xyz, case.offs(), origin=case.origins, scale=case.scale, tf=case.tfs, **kw))

    def points(self, ctx, case):
        x = _dev(case.packed())
        return self._twice(case, lambda **kw: ctx.ingest(x, case.offs(), layout=(12, 0), tf=case.tfs, **kw))


@pytest.fixture(scope="module")
def drv(cc):
    return GpuDriver(cc)


@pytest.mark.parametrize("reso", ["pow2", "div"])   # resolution 1.0, and 1.5 x 0.75 (an IEEE division per point)
@pytest.mark.parametrize("n_scans", BATCHES)
def test_georeferenced_rounding_and_boundaries(cc, oracle, drv, n_scans, reso):
    """Cases 1, 2 and 5 in one context: georeferenced f64 with an origin per scan; D halfway between two f32 and an f64 ulp beside
    it, at cell borders, the map's edge and the blind disc, and i32 triples a fused multiply-add rounds differently; the records at
    4 095 / 4 096 / 8 191 / 8 192 and on both sides of every split-part boundary, each the owner of a cell."""
    cfg = manager_cfg(cc.L, reso)
    dflt = cc.L.default_manager_cfg()
    ctx = drv.context(cfg, n_scans)
    geo = PC.case_georef(4)
    PC.assert_georef_edge(oracle, cfg, geo)
    PC.check_case(drv, oracle, cfg, geo.repeat(n_scans), ctx)
    for case, wrong in ((PC.case_rounding_f64(4), (PC.wrong_truncated, PC.wrong_f32_subtraction)), (PC.case_rounding_f64(4, with_origin=False), (PC.wrong_truncated,)),
                        (PC.case_rounding_i32(4), (PC.wrong_truncated, PC.wrong_f32_subtraction, PC.wrong_fused))):
        for fn in wrong:
            PC.assert_variant_matters(case, dflt, fn, fn.__name__)
        PC.check_case(drv, oracle, cfg, case.repeat(n_scans), ctx)
    bnd = PC.case_boundaries(4)
    PC.assert_boundary_edge(oracle, cfg, bnd)
    PC.check_case(drv, oracle, cfg, bnd.repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("half", [0, 1])
def test_types_and_streams(cc, oracle, drv, half):
    """Case 3: f64 / f32 / i32 as columns and as records with x, y, z apart and out of order, strides up to 256, bases 8 and 4 bytes
    off a 16-byte boundary, NaN patterns and random bytes between the streams."""
    cfg = cc.L.default_manager_cfg()
    n_scans = BATCHES[half]
    ctx = drv.context(cfg, n_scans)
    for variant in range(half, PC.N_TYPES, 2):
        PC.check_case(drv, oracle, cfg, PC.case_types(variant).repeat(n_scans), ctx)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_every_type_at_the_division_resolution(cc, oracle, drv, n_scans):
    """the f32 and i32 instances that divide by the resolution (f64's run in the first test): with the tests above all 12 sweep and 3
    merge instances"""
    cfg = manager_cfg(cc.L, "div")
    ctx = drv.context(cfg, n_scans)
    for variant in (2, 6, 0):   # f32, i32, f64 columns
        PC.check_case(drv, oracle, cfg, PC.case_types(variant).repeat(n_scans), ctx)
    drv.close(ctx)


def test_special_values(cc, oracle, drv):
    """Case 4: NaN, +-inf, +-1e300, -0.0; INT32_MIN / INT32_MAX"""
    cfg = cc.L.default_manager_cfg()
    for type, n_scans in ((F64, 4), (I32, 9)):
        case = PC.case_special(type)
        PC.assert_special_edge(case)
        d, _ = PC.check_case(drv, oracle, cfg, case.repeat(n_scans))
        assert np.all(d["n_pix"] > 200)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_with_a_matrix_per_scan(cc, oracle, drv, n_scans):
    """Case 6: with h_tf, the bytes of cc_ingest_points {12, 0} with that matrix on p."""
    PC.check_case(drv, oracle, cc.L.default_manager_cfg(), PC.case_with_tf(4).repeat(n_scans))


def test_identity(cc, oracle, drv):
    """Case 7: F32, consecutive, no origin: the bytes of cc_ingest_points with the same layout, device and host forms."""
    import torch
    cfg = cc.L.default_manager_cfg()
    ctx = drv.context(cfg, 4)
    for layout in ((12, 0), (16, 0), (32, 4)):
        case = PC.case_identity(layout)
        d, dbg = PC.check_case(drv, oracle, cfg, case, ctx)
        bufs, streams, stride = case.build()
        out = torch.zeros((4, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        p, pdbg = ctx.ingest(_dev(bufs[0]), case.offs(), out=out, debug=True, layout=layout)
        torch.cuda.synchronize()
        assert cc.desc_to_numpy(p).tobytes() == d.tobytes() and all(dbg[k].tobytes() == pdbg[k].cpu().numpy().tobytes() for k in dbg)
        rec = bufs[0].view(np.float32).reshape(-1, layout[0] // 4)
        dh = ctx.ingest_coords_host(rec[:, layout[1] // 4:layout[1] // 4 + 3], case.offs())
        ph = ctx.ingest_host(bufs[0], case.offs(), layout=layout)
        for i in range(4):
            assert not compare_desc(ph[i], dh[i], float_exact=True), i
        assert dh.tobytes() == d.tobytes()
    drv.close(ctx)


def test_host_form_and_chunks(cc, oracle, drv):
    """Case 8: a context of 2 scans takes 5 with five origins and matrices in chunks; ingest_coords_host on one record array and on
    three arrays, each of exactly the spanned size in front of an inaccessible page, returns the device call's bytes."""
    cfg = cc.L.default_manager_cfg()
    for variant in (1, 0, 4):   # f64 records of 32 B with x, y, z at 0, 16, 8; f64 columns; i32 records of 20 B
        c = PC.case_types(variant, n_scans=5)
        case = Case(c.name, c.raws, c.type, c.place, c.scale, c.origins, PC.random_tfs(5, seed=3, max_tilt_deg=2.0, max_shift=3.0))
        assert len({tuple(o) for o in case.origins}) == 5
        ctx = drv.context(cfg, 2)
        ref, _ = PC.check_case(drv, oracle, cfg, case, ctx)
        bufs, streams, stride = case.build(exact=True, alloc=PC.guarded)
        n, dt = int(case.offs()[-1]), PC.DTYPES[case.type]
        elem = np.dtype(dt).itemsize
        cols = tuple(bufs[b][o:o + (n - 1) * stride + elem].view(dt)[::stride // elem] for b, o in streams)
        dh = ctx.ingest_coords_host(cols, case.offs(), origin=case.origins, scale=case.scale, tf=case.tfs)
        assert dh.tobytes() == ref.tobytes(), case.name
        drv.close(ctx)


def test_tensor_forms(cc, oracle, drv):
    """The shapes Context.ingest_coords takes without a copy -- a float64 [N, 3], a view t[:, 2:5] of a wider tensor, a transposed
    [3, N].T, three separately allocated columns -- give the same bytes, those check_case holds against the oracle."""
    import torch
    cfg = cc.L.default_manager_cfg()
    case = PC.case_georef(4)
    ctx = drv.context(cfg, 4)
    ref, _ = PC.check_case(drv, oracle, cfg, case, ctx)
    X = torch.from_numpy(np.concatenate(case.raws, 0)).cuda()
    wide = torch.full((len(X), 7), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 2:5] = X
    soa = X.t().contiguous()
    forms = {"[N, 3]": X, "t[:, 2:5]": wide[:, 2:5], "[3, N].T": soa.t(), "three columns": tuple(X[:, k].clone() for k in range(3))}
    assert not forms["t[:, 2:5]"].is_contiguous() and not forms["[3, N].T"].is_contiguous()
    for name, xyz in forms.items():
        out = torch.zeros((4, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        d = cc.desc_to_numpy(ctx.ingest_coords(xyz, case.offs(), origin=case.origins, out=out))
        assert d.tobytes() == ref.tobytes(), name
    drv.close(ctx)


def test_refused_arguments(cc, drv):
    """Case 10 through the Python API: what the library refuses is a CCError, what the package refuses a ValueError, and the context
    works afterwards."""
    import torch
    cfg = cc.L.default_manager_cfg()
    case = PC.case_georef(2, sizes=[9001, 9500])
    ctx = drv.context(cfg, 2)
    X = torch.from_numpy(np.concatenate(case.raws, 0)).cuda()
    offs, O = case.offs(), case.origins
    out = torch.zeros((2, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    ref = ctx.ingest_coords(X, offs, origin=O, out=out).clone()
    wide = torch.zeros((len(X), 40), dtype=torch.float64, device="cuda")
    bad_origin = O.copy()
    bad_origin[1, 2] = np.inf
    refused = [
        dict(xyz=wide[:, :3], origin=O),   # a stride of 320 bytes
        dict(xyz=X, origin=bad_origin),
        dict(xyz=X.to(torch.int32), origin=O, scale=[0.001, float("nan"), 0.001]),
        dict(xyz=X, origin=O, offsets=np.array([0, 10, 9001], np.int64)),
    ]
    for kw in refused:
        with pytest.raises(cc.CCError):
            ctx.ingest_coords(kw["xyz"], kw.get("offsets", offs), origin=kw["origin"], scale=kw.get("scale"))
    with pytest.raises(cc.CCError):
        ctx.ingest_coords_host(np.concatenate(case.raws, 0), offs, origin=bad_origin)
    for xyz, kw in ((X.to(torch.float16), {}), (X.to(torch.int64), {}), (X, dict(scale=[1.0, 1.0, 1.0])), (X[:, :2], {}), ((X[:, 0], X[:, 1]), {}),
                    ((X[:, 0], X[:, 1], X[::2, 2]), {})):
        with pytest.raises(ValueError):
            ctx.ingest_coords(xyz, offs, **kw)
    with pytest.raises(ValueError):
        ctx.ingest_coords_host(np.zeros((int(offs[-1]), 3), np.float16), offs)
    out.zero_()
    assert torch.equal(ref, ctx.ingest_coords(X, offs, origin=O, out=out))
    drv.close(ctx)


def test_one_full_size_scan(cc, oracle, drv):
    """Case 11: 119 997 points, f64, georeferenced: alone (split path) and with 8 short ones."""
    cfg = cc.L.default_manager_cfg()
    xyzi, _, _ = cc.synth.make_sequence(1, world=cc.synth.World(loop_len=200.0), device="cuda", start=11)
    big = PC.quantised(xyzi[0].cpu().numpy()[:119997])
    small = PC.case_georef(8)
    O = PC.geo_origins(9, seed=91)
    for n_scans in (1, 9):
        local = [big] + [r - small.origins[i] for i, r in enumerate(small.raws[:n_scans - 1])]
        case = Case("full size", [q + O[i] for i, q in enumerate(local)], F64, PC.Place.records(24, (0, 8, 16)), origins=O[:n_scans])
        assert case.p()[0][:, :3].astype(np.float64).tobytes() == big.tobytes()
        PC.check_case(drv, oracle, cfg, case)


def test_drive_in_world_coordinates(cc, oracle):
    """Case 12: 72 scans of a drive, quantised to 2^-10 m, ingested once as local f32 clouds and once as f64 world coordinates (local +
    the pose's translation, with UTM-sized offsets) with origin = that translation: the descriptors are equal byte for byte, the query
    results field for field, and equal to the oracle's on the integer fields."""
    import torch
    L = cc.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    n = 72
    xyzi, poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    local = np.round(xyzi.cpu().numpy().astype(np.float64) * PC.Q10) / PC.Q10 + 0.0
    local[..., 3] = 0.0
    P = local.shape[1]
    trans = np.concatenate([np.asarray(poses, np.float64)[:, :2], np.zeros((n, 1))], 1)   # the pose's translation (x, y; the trajectory is planar)
    O = np.round((trans + np.array([448000.0, 5412000.0, 300.0])) * PC.Q10) / PC.Q10
    assert len({tuple(o) for o in O}) > n // 2
    world = local[..., :3] + O[:, None, :]
    f32 = np.ascontiguousarray(local.astype(np.float32))
    assert f32.astype(np.float64).tobytes() == local.tobytes()
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(f32.reshape(-1, 4), offs, ts, seeds, dcfg=dcfg, want_desc=True)
    assert (ores["n_res"] > 0).sum() >= 3, "the oracle's drive must close loops, or the comparison below shows nothing"
    ctx = cc.Context(0, max_batch=n)
    out = [torch.zeros((n, cc.DESC_BYTES), dtype=torch.uint8, device="cuda") for _ in range(2)]
    desc_local = ctx.ingest(torch.from_numpy(f32.reshape(-1, 4)).cuda(), offs, out=out[0])
    desc_world = ctx.ingest_coords(torch.from_numpy(world.reshape(-1, 3)).cuda(), offs, origin=O, out=out[1])
    torch.cuda.synchronize()
    assert torch.equal(desc_local, desc_world)
    results = []
    for dsc in (desc_world, desc_local):
        db = cc.Database(ctx, dcfg, capacity=n)
        db.add_scans(dsc, ts, seeds)
        results.append(db.query(dsc, seeds))
        torch.cuda.synchronize()
        db.close()
    res, res_local = results
    for f in res.dtype.names:
        assert np.array_equal(res[f], res_local[f], equal_nan=res[f].dtype.kind == "f"), f
    d = cc.desc_to_numpy(desc_world)
    for i in range(n):
        bad = compare_desc(odesc[i], d[i], float_exact=False)
        assert not bad, "scan %d: %s" % (i, bad[:5])
    for f in ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy", "n_knn_hits"]:
        assert np.array_equal(ores[f], res[f]), f
    ctx.close()
