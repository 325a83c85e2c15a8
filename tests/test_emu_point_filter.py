"""cc_ingest_points_filtered and its siblings (include/cont2_amd_filter.h) on the CPU harness: records dropped by a label, ring, tag or
intensity word of their own while they are rasterised.  The specified result is cc_ingest_points' for the kept records alone -- so
every case is held against the oracle on those records (bev, pix_rc, label images, descriptor float_exact) and, as bytes, against
cc_ingest_points on the records whose dropped x are NaN (point_filter.check_case); never against another run of the new code alone.
The harness' workgroups have 256 threads: a chunk is 1 024 points there, and a call of <= 8 scans takes the split path."""
import ctypes as C

import numpy as np
import pytest

import point_filter as PF
from k1_instances import manager_cfg
from parity import compare_desc
from point_filter import F32, U8, U16, U32, Case, Filter, Rule

CHUNK = 1024
BATCHES = (4, 9)   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan


@pytest.fixture(scope="module")
def drv(oracle):
    return PF.EmuDriver(oracle.L)


def _same(a, b, da=None, db=None):
    assert a.tobytes() == b.tobytes(), "descriptors differ"
    if da is not None:
        for k in ("bev", "pix_rc", "labels"):
            assert da[k].tobytes() == db[k].tobytes(), k


def _compacted(drv, ctx, case, d, dbg):
    """the bytes of cc_ingest_points on the kept records alone (every scan keeps more than 10)"""
    kept = [s[k] for s, k in zip(case.scans, case.keep)]
    words = [w[k] for w, k in zip(case.words, case.keep)]
    extra = [[(o, a[k]) for o, a in e] for e, k in zip(case.extra, case.keep)]
    c = Case(case.name, kept, words, case.rule, case.layout, case.base_shift, case.tfs, extra, case.fill)
    p, pdbg = drv.points(ctx, c, c.buffer())
    _same(p, d, pdbg, dbg)


EDGES = {"maxima": PF.case_dropped_maxima, "first of equals": PF.case_first_of_equals, "extremes": PF.case_extremes,
         "boundaries": lambda n: PF.case_boundaries(n, chunk=CHUNK)}


@pytest.mark.parametrize("reso", ["pow2", "div"])   # resolution 1.0, and 1.5 x 0.75 (an IEEE division per point)
@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(oracle, drv, edge, n_scans, reso):
    """Cases 1 - 4: a dropped record that is a cell's maximum, the first of several equal heights, the scan's extremes, and records on
    both sides of every chunk and split-part boundary."""
    cfg = manager_cfg(oracle.L, reso)
    case = EDGES[edge](4)
    PF.assert_edge(oracle, cfg, case)
    case = case.repeat(n_scans)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PF.check_case(drv, oracle, cfg, case, ctx)
    _compacted(drv, ctx, case, d, dbg)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_everything_kept(oracle, drv, n_scans):
    """Case 5: the bytes of cc_ingest_points on the same call, device and host forms."""
    cfg = oracle.L.default_manager_cfg()
    case = PF.case_everything("kept").repeat(n_scans)
    assert all(k.all() for k in case.keep)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PF.check_case(drv, oracle, cfg, case, ctx)
    buf = case.buffer()
    p, pdbg = drv.api.ingest_points(ctx, buf, case.layout, case.offs(), debug=True)
    _same(p, d, pdbg, dbg)
    f, _bits = case.rule.c()
    rc, dh, bev = drv.api.ingest_filtered_host_rc(ctx, buf, case.layout, f, case.offs(), want_bev=True)
    ph, pbev = drv.api.ingest_points_host(ctx, buf, case.layout, case.offs(), want_bev=True)
    assert rc == 0 and bev.tobytes() == pbev.tobytes() == pdbg["bev"].tobytes()
    # cc_ingest_points_host leaves what lies behind a descriptor's counts as its allocation had it: everything a descriptor defines
    # is compared with it, and the bytes with the device call's (the filtered host call zeroes its descriptors first)
    for i in range(n_scans):
        assert not compare_desc(ph[i], dh[i], float_exact=True), i
    assert dh.tobytes() == p.tobytes()
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("kind", ["dropped", "five"])
def test_everything_dropped(oracle, drv, kind, n_scans):
    """Case 6: every record dropped, and all but 5: the bytes of cc_ingest_points on the NaN-substituted records -- a valid, empty scan
    (the limits on a scan count records, not kept points)."""
    cfg = oracle.L.default_manager_cfg()
    case = PF.case_everything(kind).repeat(n_scans)
    assert all(int(k.sum()) == (0 if kind == "dropped" else 5) for k in case.keep)
    d, dbg = PF.check_case(drv, oracle, cfg, case)
    if kind == "dropped":
        assert np.all(d["n_pix"] == 0) and np.all(d["max_bin_val"] == -1000.0) and np.all(d["min_bin_val"] == 1000.0) and np.all(d["n_cont"] == 0)
    else:
        assert np.all(d["n_pix"] == 5) and np.all(d["max_bin_val"] < 100.0)


@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("variant", range(PF.N_LAYOUTS))
def test_layouts(oracle, drv, variant, n_scans):
    """Case 7: {16, 0} with SemanticKITTI's u32 at 12 (an instance id in the high bits), {32, 0} with a u8 at 17 and a u16 at 18,
    {48, 8} with the word in front of xyz, a base 4 bytes off a 16-byte boundary."""
    cfg = oracle.L.default_manager_cfg()
    case = PF.case_layout(variant)
    if variant == 0:
        PF.assert_edge(oracle, cfg, case)
        assert all(((w >> 16) != 0).mean() > 0.99 for w in case.words)
    assert all(0.02 < 1.0 - k.mean() < 0.6 for k in case.keep)
    PF.check_case(drv, oracle, cfg, case.repeat(n_scans))


@pytest.mark.parametrize("variant", range(PF.N_SHIFT_MASK))
def test_shift_mask_and_table_sizes(oracle, drv, variant):
    """Case 8: shift / mask combinations, n_classes of 1, 32, 33 and 4 096, classes beyond the table under both keep_other values;
    the bytes around a u8 / u16 word are random, and a mask wider than the word must not let them reach the class."""
    cfg = oracle.L.default_manager_cfg()
    case = PF.case_shift_mask(variant)
    PF.check_case(drv, oracle, cfg, case.repeat(9 if variant % 2 else 4))


@pytest.mark.parametrize("variant", range(PF.N_RANGES))
def test_range_rule(oracle, drv, variant):
    """Case 9: a band, lo == hi, (-inf, inf), NaN words, -0.0 against lo = 0 (and +0.0 against hi = -0.0), an empty band."""
    cfg = oracle.L.default_manager_cfg()
    case = PF.case_range(variant)
    PF.check_case(drv, oracle, cfg, case.repeat(4 if variant % 2 else 9))


@pytest.mark.parametrize("n_scans", BATCHES)
def test_range_rule_at_the_division_resolution(oracle, drv, n_scans):
    """the range kind's two instances that divide by the resolution (the class kind's run in test_edges)"""
    cfg = manager_cfg(oracle.L, "div")
    PF.check_case(drv, oracle, cfg, PF.case_range(0).repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
def test_with_a_matrix_per_scan(oracle, drv, n_scans):
    """Case 10: with h_tf, the bytes of cc_ingest_points with that matrix on the kept records; the filter looks at the record."""
    cfg = oracle.L.default_manager_cfg()
    case = PF.case_with_tf(4)
    PF.assert_edge(oracle, cfg, case)
    case = case.repeat(n_scans)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PF.check_case(drv, oracle, cfg, case, ctx)
    _compacted(drv, ctx, case, d, dbg)
    drv.close(ctx)


def test_per_scan_call_and_host_call(oracle, drv):
    """Case 11: the per-scan call and the _host call return the batch call's descriptors; a context of 2 scans takes 3 in chunks."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    for case in (PF.case_layout(1, n_scans=3), PF.case_with_tf(3), PF.case_range(0, n_scans=3)):
        ctx = drv.context(cfg, 2)   # the batch call goes in chunks of 2 + 1 scans
        ref, rdbg = PF.check_case(drv, oracle, cfg, case, ctx)
        f, _bits = case.rule.c()
        offs, buf = case.offs(), case.buffer()
        stride = case.layout[0]
        for i in range(3):
            one = np.ascontiguousarray(buf[offs[i] * stride:offs[i + 1] * stride])
            rc, d = api.scan_ingest_filtered_rc(ctx, one, case.layout, f, len(case.scans[i]), None if case.tfs is None else case.tfs[i])
            assert rc == 0 and not compare_desc(ref[i], d, float_exact=True), (case.name, i)
        # the host call, with a leading scan that is skipped
        rc, dh, bev = api.ingest_filtered_host_rc(ctx, buf, case.layout, f, offs[1:], None if case.tfs is None else case.tfs[1:], want_bev=True)
        assert rc == 0
        for i in range(2):
            assert not compare_desc(ref[i + 1], dh[i], float_exact=True), (case.name, i)
            assert np.array_equal(bev[i], rdbg["bev"][i + 1])
        assert dh.tobytes() == ref[1:].tobytes(), case.name   # (class and range rule: the host form zeroes its descriptors first)
        drv.close(ctx)


def test_refusals(oracle, drv):
    """Case 12: every refused input returns CC_EINVAL, names its entry point, and a following good call still gives the reference bytes."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    case = PF.case_layout(1, n_scans=2)   # {32, 0}, a u8 at 17
    ctx = drv.context(cfg, 2)
    offs, buf, lay = case.offs(), case.buffer(), case.layout
    good, bits = case.rule.c()
    rc, ref, _ = api.ingest_filtered_rc(ctx, buf, lay, good, offs)
    assert rc == 0
    nan = float("nan")

    def flt(**over):
        f = Filter(good.offset, good.type, good.shift, good.mask, good.n_classes, good.keep_other, 0.0, 0.0, good.keep_bits)
        for k, v in over.items():
            setattr(f, k, v)
        return f

    cases = {
        "a layout cc_ingest_points refuses": (dict(), (22, 0)),
        "a NULL filter": (None, lay),
        "type 4": (dict(type=4), lay),
        "type -1": (dict(type=-1), lay),
        "a negative offset": (dict(offset=-1), lay),
        "a u16 at an odd offset": (dict(type=U16, offset=17), lay),
        "a u32 at 18": (dict(type=U32, offset=18), lay),
        "an f32 at 18": (dict(type=F32, offset=18), lay),
        "a u8 beyond the record": (dict(offset=32), lay),
        "a u16 beyond the record": (dict(type=U16, offset=32), lay),
        "a u32 beyond the record": (dict(type=U32, offset=32), lay),
        "a u8 on x": (dict(offset=0), lay),
        "a u8 on z's last byte": (dict(offset=11), lay),
        "a u16 on y": (dict(type=U16, offset=6), lay),
        "a u32 on z": (dict(type=U32, offset=8), lay),
        "an f32 on x": (dict(type=F32, offset=0), lay),
        "a u8 shifted by 8": (dict(shift=8), lay),
        "a u16 shifted by 16": (dict(type=U16, offset=18, shift=16), lay),
        "a u32 shifted by 32": (dict(type=U32, offset=20, shift=32), lay),
        "a negative shift": (dict(shift=-1), lay),
        "no classes": (dict(n_classes=0), lay),
        "4 097 classes": (dict(n_classes=PF.CLASSES_MAX + 1), lay),
        "NULL keep_bits": (dict(keep_bits=None), lay),
        "a NaN lo": (dict(type=F32, offset=20, lo=nan, hi=1.0), lay),
        "a NaN hi": (dict(type=F32, offset=20, lo=0.0, hi=nan), lay),
    }
    for what, (over, layout) in cases.items():
        f = None if over is None else flt(**over)
        rc, _, _ = api.ingest_filtered_rc(ctx, buf, layout, f, offs)
        assert rc == -1, what   # CC_EINVAL
        assert api.lib.cc_last_error().decode().startswith("cc_ingest_points_filtered:"), what
        rc, _, _ = api.ingest_filtered_host_rc(ctx, buf, layout, f, offs)
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_points_filtered_host:"), what
        rc, _ = api.scan_ingest_filtered_rc(ctx, buf, layout, f, len(case.scans[0]))
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_points_filtered:"), what
        rc, d, _ = api.ingest_filtered_rc(ctx, buf, lay, good, offs)
        assert rc == 0 and d.tobytes() == ref.tobytes(), what
    # a misaligned device base, as cc_ingest_points refuses it
    rc, _, _ = api.ingest_filtered_rc(ctx, buf[2:], lay, good, np.array([0, 100], np.int64))
    assert rc == -1 and "4-byte aligned" in api.lib.cc_last_error().decode()
    # a scan of <= 10 records is refused however many are kept; 11 records of which none is kept are a valid, empty scan
    rc, _, _ = api.ingest_filtered_rc(ctx, buf, lay, good, np.array([0, 10], np.int64))
    assert rc == -1 and "<= 10 points" in api.lib.cc_last_error().decode()
    none = Rule(17, U8, kept=[False], keep_other=0)
    fn, _b = none.c()
    rc, d, _ = api.ingest_filtered_rc(ctx, buf, lay, fn, np.array([0, 11], np.int64))
    assert rc == 0 and d["n_pix"][0] == 0
    # taken: the record's last byte, the last two bytes, a word right behind z, the fields of the other rule holding rubbish
    words = case.words
    for (typ, off, shift) in ((U8, 31, 7), (U16, 30, 15), (U32, 28, 31), (U32, 12, 0), (U8, 12, 0)):
        w = [np.random.default_rng(off).integers(0, 2 ** 32, len(s), dtype=np.uint64).astype(PF.DTYPES[typ]) for s in case.scans]
        c = Case("taken", case.scans, w, Rule(off, typ, shift, 0xFFFFFFFF, [True], 0), layout=lay, fill=1)
        PF.check_case(drv, oracle, cfg, c, ctx)
    band = Case("taken", case.scans, [np.random.default_rng(3).uniform(0, 1, len(s)).astype(np.float32) for s in case.scans], Rule(28, F32, lo=0.2, hi=np.inf), layout=lay)
    fb, _ = band.rule.c()
    fb.shift, fb.n_classes, fb.mask, fb.keep_bits = 99, -5, 0, None   # not read by the range rule
    rc, d, _ = api.ingest_filtered_rc(ctx, band.buffer(), lay, fb, offs)
    assert rc == 0 and d.tobytes() == PF.check_case(drv, oracle, cfg, band, ctx)[0].tobytes()
    good2 = flt(lo=nan, hi=nan)   # not read by the class rule
    rc, d, _ = api.ingest_filtered_rc(ctx, buf, lay, good2, offs)
    assert rc == 0 and d.tobytes() == ref.tobytes()
    assert words is case.words and bits is not None
    drv.close(ctx)


def test_filter_struct(cc):
    """the ctypes mirrors of cc_point_filter_t: 40 bytes (the header carries a static_assert of the same)"""
    for S in (Filter, cc.L.PointFilterC):
        assert C.sizeof(S) == 40 and S.mask.offset == 12 and S.lo.offset == 24 and S.hi.offset == 28 and S.keep_bits.offset == 32
    assert cc.L.FILTER_CLASSES_MAX == PF.CLASSES_MAX and (cc.L.FILTER_U8, cc.L.FILTER_U16, cc.L.FILTER_U32, cc.L.FILTER_F32) == (U8, U16, U32, F32)
