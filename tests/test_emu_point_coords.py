"""cc_ingest_coords and its siblings (include/cont2_amd_coords.h) on the CPU harness: f64, scaled-i32 and split-stream coordinates
converted while they are rasterised.  The specified result is cc_ingest_points' for the packed f32 points p = (float)((double)v
[* scale] - origin) -- so every case is held against the oracle on p (bev, pix_rc, label images, descriptor float_exact) and, as
bytes, against cc_ingest_points on the packed p (point_coords.check_case); never against another run of the new code alone.
The harness' workgroups have 256 threads: a chunk is 1 024 points there, and a call of <= 8 scans takes the split path."""
import ctypes as C

import numpy as np
import pytest

import point_coords as PC
from k1_instances import manager_cfg
from parity import compare_desc
from point_coords import F32, F64, I32, Case, CoordSrc, Place

CHUNK = 1024
BATCHES = (4, 9)   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan


@pytest.fixture(scope="module")
def drv(oracle):
    return PC.EmuDriver(oracle.L)


@pytest.mark.parametrize("reso", ["pow2", "div"])   # resolution 1.0, and 1.5 x 0.75 (an IEEE division per point)
@pytest.mark.parametrize("n_scans", BATCHES)
def test_georeferenced_f64(oracle, drv, n_scans, reso):
    """Case 1: f64 [N, 3] world coordinates near (448 000, 5 412 000, 300) with an origin per scan."""
    cfg = manager_cfg(oracle.L, reso)
    case = PC.case_georef(4)
    PC.assert_georef_edge(oracle, cfg, case)
    PC.check_case(drv, oracle, cfg, case.repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("kind", ["f64 origin", "f64", "i32"])
def test_rounding(oracle, drv, kind, n_scans):
    """Case 2: D exactly halfway between two f32 and one f64 ulp beside it, within an f32 ulp of cell borders, the map's edge and the
    blind disc; i32 triples that a fused multiply-add rounds differently.  Truncation, an f32 subtraction and the fused form each
    change at least 50 points' bits and move at least 5 points to another cell."""
    cfg = oracle.L.default_manager_cfg()
    case = {"f64 origin": lambda: PC.case_rounding_f64(4), "f64": lambda: PC.case_rounding_f64(4, with_origin=False), "i32": lambda: PC.case_rounding_i32(4)}[kind]()
    PC.assert_variant_matters(case, cfg, PC.wrong_truncated, "truncation")
    if kind != "f64":
        PC.assert_variant_matters(case, cfg, PC.wrong_f32_subtraction, "the subtraction in f32")
    if kind == "i32":
        PC.assert_variant_matters(case, cfg, PC.wrong_fused, "the fused form")
    PC.check_case(drv, oracle, cfg, case.repeat(n_scans))


@pytest.mark.parametrize("variant", range(PC.N_TYPES))
def test_types_and_streams(oracle, drv, variant):
    """Case 3: f64 / f32 / i32 as columns and as records with x, y, z apart and out of order, strides up to 256, bases 8 and 4 bytes
    off a 16-byte boundary, NaN patterns and random bytes between the streams."""
    cfg = oracle.L.default_manager_cfg()
    PC.check_case(drv, oracle, cfg, PC.case_types(variant).repeat(9 if variant % 2 else 4))


@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("variant", [0, 2, 6])   # f64, f32 and i32 columns
def test_every_type_at_the_division_resolution(oracle, drv, variant, n_scans):
    """the instances that divide by the resolution, per type and per path (the others run in test_types_and_streams)"""
    cfg = manager_cfg(oracle.L, "div")
    PC.check_case(drv, oracle, cfg, PC.case_types(variant).repeat(n_scans))


@pytest.mark.parametrize("type", [F64, I32])
def test_special_values(oracle, drv, type):
    """Case 4: NaN, +-inf, +-1e300 (overflow to +-inf), -0.0; INT32_MIN / INT32_MAX: rejected like any point cc_point_cell rejects, and
    n_pix is the oracle's on the rest."""
    cfg = oracle.L.default_manager_cfg()
    case = PC.case_special(type)
    PC.assert_special_edge(case)
    d, _ = PC.check_case(drv, oracle, cfg, case.repeat(4 if type == F64 else 9))
    assert np.all(d["n_pix"] > 200)


@pytest.mark.parametrize("reso", ["pow2", "div"])
@pytest.mark.parametrize("n_scans", BATCHES)
def test_boundaries(oracle, drv, n_scans, reso):
    """Case 5: the records on both sides of every chunk and split-part boundary own a cell each."""
    cfg = manager_cfg(oracle.L, reso)
    case = PC.case_boundaries(4, chunk=CHUNK)
    PC.assert_boundary_edge(oracle, cfg, case, CHUNK)
    PC.check_case(drv, oracle, cfg, case.repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
def test_with_a_matrix_per_scan(oracle, drv, n_scans):
    """Case 6: with h_tf, the bytes of cc_ingest_points {12, 0} with that matrix on p."""
    cfg = oracle.L.default_manager_cfg()
    PC.check_case(drv, oracle, cfg, PC.case_with_tf(4).repeat(n_scans))


@pytest.mark.parametrize("layout", [(12, 0), (16, 0), (32, 4)])
def test_identity(oracle, drv, layout):
    """Case 7: F32, consecutive, no origin: the bytes of cc_ingest_points with the same layout, device and host forms."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    case = PC.case_identity(layout)
    ctx = drv.context(cfg, 4)
    d, dbg = PC.check_case(drv, oracle, cfg, case, ctx)
    bufs, streams, stride = case.build()
    assert [o for _, o in streams] == [layout[1], layout[1] + 4, layout[1] + 8] and stride == layout[0]
    p, pdbg = api.ingest_points(ctx, bufs[0], layout, case.offs(), debug=True)
    assert p.tobytes() == d.tobytes() and all(np.asarray(dbg[k]).tobytes() == np.asarray(pdbg[k]).tobytes() for k in dbg)
    rc, dh, bev = api.ingest_coords_host_rc(ctx, api.src(bufs, streams, stride, F32), case.offs(), want_bev=True)
    ph, pbev = api.ingest_points_host(ctx, bufs[0], layout, case.offs(), want_bev=True)
    assert rc == 0 and bev.tobytes() == pbev.tobytes() == pdbg["bev"].tobytes()
    for i in range(4):
        assert not compare_desc(ph[i], dh[i], float_exact=True), i
    assert dh.tobytes() == p.tobytes()
    drv.close(ctx)


def _five(kind):
    c = PC.case_types({"records": 1, "columns": 0, "i32": 4}[kind], n_scans=5)
    return Case(c.name, c.raws, c.type, c.place, c.scale, c.origins, PC.random_tfs(5, seed=3, max_tilt_deg=2.0, max_shift=3.0))


@pytest.mark.parametrize("kind", ["records", "columns", "i32"])
def test_host_form_and_chunks(oracle, drv, kind):
    """Case 8: a context of 2 scans takes 5 in chunks -- a scan of the third chunk gets ITS origin and matrix; the host form on one
    record array and on three arrays returns the device call's bytes from buffers of EXACTLY the spanned size, each in front of an
    inaccessible page."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    case = _five(kind)
    assert len({tuple(o) for o in case.origins}) == 5
    ctx = drv.context(cfg, 2)
    ref, rdbg = PC.check_case(drv, oracle, cfg, case, ctx)
    bufs, streams, stride = case.build(exact=True, alloc=PC.guarded)
    assert len(bufs) == (3 if kind == "columns" else 1)
    rc, dh, bev = api.ingest_coords_host_rc(ctx, api.src(bufs, streams, stride, case.type, case.scale), case.offs(), case.origins, case.tfs, want_bev=True)
    assert rc == 0, api.lib.cc_last_error()
    assert dh.tobytes() == ref.tobytes() and bev.tobytes() == np.asarray(rdbg["bev"]).tobytes()
    # a leading scan that is skipped: the copy begins at the second scan's first point
    offs = case.offs()
    rc, dh, _ = api.ingest_coords_host_rc(ctx, api.src(bufs, streams, stride, case.type, case.scale), offs[1:], case.origins[1:], case.tfs[1:])
    assert rc == 0 and dh.tobytes() == ref[1:].tobytes()
    drv.close(ctx)


@pytest.mark.parametrize("kind", ["records", "columns", "i32"])
def test_per_scan_call(oracle, drv, kind):
    """Case 9 on the harness: cc_scan_ingest_coords returns the batch call's descriptor, from exactly-spanned guarded buffers."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    case = _five(kind)
    ctx = drv.context(cfg, 5)
    ref, _ = PC.check_case(drv, oracle, cfg, case, ctx)
    for i in (0, 3):
        one = Case(case.name, [case.raws[i]], case.type, case.place, case.scale, case.origins[i:i + 1], case.tfs[i:i + 1])
        bufs, streams, stride = one.build(exact=True, alloc=PC.guarded)
        rc, d = api.scan_ingest_coords_rc(ctx, api.src(bufs, streams, stride, case.type, case.scale), len(case.raws[i]), case.origins[i], case.tfs[i])
        assert rc == 0, api.lib.cc_last_error()
        assert not compare_desc(ref[i], d, float_exact=True), (kind, i)
        assert d.tobytes() == ref[i].tobytes()
    drv.close(ctx)


def test_refusals(oracle, drv):
    """Case 10: every refused input returns CC_EINVAL, names its entry point, and a following good call still gives the reference bytes."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    case = PC.case_types(1, n_scans=2)   # f64 records of 32 B
    ctx = drv.context(cfg, 2)
    bufs, streams, stride = case.build()
    offs, O = case.offs(), case.origins
    good = api.src(bufs, streams, stride, F64)
    rc, ref, _ = api.ingest_coords_rc(ctx, good, offs, O)
    assert rc == 0
    nan, inf = float("nan"), float("inf")

    def src(**over):
        s = CoordSrc(good.x, good.y, good.z, good.type, good.stride_bytes, (C.c_double * 3)(1.0, 1.0, 1.0))
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def origin(i, v):
        o = O.copy()
        o.reshape(-1)[i] = v
        return o

    cases = {
        "a NULL src": (None, O, offs),
        "a NULL x": (src(x=None), O, offs),
        "a NULL y": (src(y=None), O, offs),
        "a NULL z": (src(z=None), O, offs),
        "type 3": (src(type=3), O, offs),
        "type -1": (src(type=-1), O, offs),
        "an f64 stride of 28": (src(stride_bytes=28), O, offs),
        "an f64 stride of 4": (src(stride_bytes=4), O, offs),
        "an f64 stride of 0": (src(stride_bytes=0), O, offs),
        "a negative stride": (src(stride_bytes=-32), O, offs),
        "an f32 stride of 6": (src(type=F32, stride_bytes=6), O, offs),
        "an i32 stride of 2": (src(type=I32, stride_bytes=2), O, offs),
        "a stride of 264": (src(stride_bytes=PC.STRIDE_MAX + 8), O, offs),
        "an f64 x 4 bytes off": (src(x=good.x + 4), O, offs),
        "an f64 z 4 bytes off": (src(z=good.z + 4), O, offs),
        "an f32 y 2 bytes off": (src(type=F32, y=good.y + 2), O, offs),
        "an i32 x 1 byte off": (src(type=I32, x=good.x + 1), O, offs),
        "a NaN scale": (src(type=I32, scale=(C.c_double * 3)(0.001, nan, 0.001)), O, offs),
        "an infinite scale": (src(type=I32, scale=(C.c_double * 3)(0.001, 0.001, -inf)), O, offs),
        "a NaN origin": (good, origin(1, nan), offs),
        "an infinite origin in the second scan": (good, origin(5, inf), offs),
        "a scan of 10 points": (good, O, np.array([0, 10, 5000], np.int64)),
        "a scan of 2^21 points": (good, O, np.array([0, 5000, 5000 + 2 ** 21], np.int64)),
    }
    for what, (s, o, of) in cases.items():
        rc, _, _ = api.ingest_coords_rc(ctx, s, of, o)
        assert rc == -1, what   # CC_EINVAL
        assert api.lib.cc_last_error().decode().startswith("cc_ingest_coords:"), what
        rc, _, _ = api.ingest_coords_host_rc(ctx, s, of, o)
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_coords_host:"), what
        rc, _ = api.scan_ingest_coords_rc(ctx, s, int(of[1] - of[0]) if "2^21" not in what else 2 ** 21, None if o is None else o[1 if "second" in what else 0])
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_coords:"), what
        rc, d, _ = api.ingest_coords_rc(ctx, good, offs, O)
        assert rc == 0 and d.tobytes() == ref.tobytes(), what
    # not read: the scales of an f32 / f64 source
    rc, d, _ = api.ingest_coords_rc(ctx, src(scale=(C.c_double * 3)(nan, inf, -1.0)), offs, O)
    assert rc == 0 and d.tobytes() == ref.tobytes()
    # taken: the largest stride, an element in the record's last bytes, 11 points
    c = PC.case_types(7, n_scans=2)
    PC.check_case(drv, oracle, cfg, c, ctx)
    rc, d, _ = api.ingest_coords_rc(ctx, good, np.array([0, 11, 5000], np.int64), O)
    assert rc == 0
    drv.close(ctx)


def test_struct_mirrors(cc):
    """the ctypes mirrors of cc_coord_src_t: 56 bytes (the header carries a static_assert of the same)"""
    for S in (CoordSrc, cc.L.CoordSrc):
        assert C.sizeof(S) == 56 and S.y.offset == 8 and S.z.offset == 16 and S.type.offset == 24 and S.stride_bytes.offset == 28 and S.scale.offset == 32
    assert (cc.L.COORD_F32, cc.L.COORD_F64, cc.L.COORD_I32) == (F32, F64, I32)
    assert Place is not None
