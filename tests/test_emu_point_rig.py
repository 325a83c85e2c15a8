"""cc_ingest_rig and its siblings (include/cont2_amd_rig.h) on the CPU harness: a scan made of segments, each moved by its own mode (none,
a matrix, its time words and a slice of the scan's knot pool) and filtered by a word of its own place, in one sweep.  Every case is held
against the oracle on the kept, moved points (bev, pix_rc, label images, descriptor float_exact) and, as bytes, against cc_ingest_batch
on the numpy-built cloud Q whose dropped x are NaN (point_rig.check_case); never against another run of the new code alone.
The harness' workgroups have 256 threads: a chunk is 1 024 points there, and a call of <= 8 scans takes the split path."""
import ctypes as C

import numpy as np
import pytest

import point_rig as PR
from k1_instances import manager_cfg
from parity import compare_desc
from point_filter import F32, U8, U16, U32, FilterApi, Rule
from point_motion import TIME_F32, MotionApi
from point_rig import Case, Motion, RigSegment, Seg
from point_segments import Segments, SegmentsApi

CHUNK = 1024
BATCHES = (4, 9)   # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan


@pytest.fixture(scope="module")
def drv(oracle):
    return PR.EmuDriver(oracle.L)


EDGES = {"boundaries": lambda: PR.case_boundaries(chunk=CHUNK), "ties dropped": lambda: PR.case_ties(True), "ties": lambda: PR.case_ties(False),
         "empties": PR.case_empties}


@pytest.mark.parametrize("reso", ["pow2", "div"])   # resolution 1.0, and 1.5 x 0.75 (an IEEE division per point)
@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("edge", list(EDGES))
def test_edges(oracle, drv, edge, n_scans, reso):
    """Segment boundaries at every chunk and split-part boundary with a dropped record and a change of slice on both sides; ties across
    segments with and without the earlier record dropped; empty segments first, in the middle and last, and a segment all dropped."""
    cfg = manager_cfg(oracle.L, reso)
    case = EDGES[edge]()
    PR.assert_edge(oracle, cfg, case)
    PR.check_case(drv, oracle, cfg, case.repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
def test_slices(oracle, drv, n_scans):
    """Times beyond a slice's end clamp to ITS last knot, times before t_begin and NaN go to its first: the case's own assertion shows
    that a clamp to the pool's size would put hundreds of records into other cells."""
    cfg = oracle.L.default_manager_cfg()
    case = PR.case_slices()
    PR.assert_slices(cfg, case)
    PR.check_case(drv, oracle, cfg, case.repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
@pytest.mark.parametrize("kind", PR.MIXED_KINDS)
def test_mixed_scan(oracle, drv, kind, n_scans):
    """none, tf, f32-time and u32-time segments, five record shapes, the filter word at another offset per segment, one unfiltered
    segment; u8 / u16 / u32 class words and the range rule."""
    cfg = manager_cfg(oracle.L, "div" if kind == "u16" else "pow2")
    PR.check_case(drv, oracle, cfg, PR.case_mixed(kind).repeat(n_scans))


@pytest.mark.parametrize("n_scans", BATCHES)
def test_everything_dropped_and_max_segments(oracle, drv, n_scans):
    cfg = oracle.L.default_manager_cfg()
    d, _ = PR.check_case(drv, oracle, cfg, PR.case_all_dropped().repeat(n_scans))
    assert np.all(d["n_pix"] == 0) and np.all(d["max_bin_val"] == -1000.0) and np.all(d["min_bin_val"] == 1000.0) and np.all(d["n_cont"] == 0)
    case = PR.case_max_segments()
    assert all(len(sc) == PR.RIG_SEG_MAX for sc in case.scans) and case.n_pool() == 64
    PR.check_case(drv, oracle, cfg, case.repeat(n_scans))


# ---- equivalences, as bytes against the existing calls ----
def _same(a, b, da, db):
    assert a.tobytes() == b.tobytes(), "descriptors differ"
    for k in ("bev", "pix_rc", "labels"):
        assert da[k].tobytes() == db[k].tobytes(), k


@pytest.mark.parametrize("n_scans", BATCHES)
def test_equals_ingest_segments(oracle, drv, n_scans):
    """only none / tf segments and no rule: cc_ingest_segments' bytes"""
    cfg = oracle.L.default_manager_cfg()
    mixed = PR.case_mixed("u32")
    scans = [[Seg(s.xyzi, s.layout, s.shift, tf=s.tf if s.motion is None else PR.shift_knots(1, 5)[0]) for s in sc] for sc in mixed.scans]
    case = Case("no motion, no rule", scans).repeat(n_scans)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PR.check_case(drv, oracle, cfg, case, ctx)
    api = SegmentsApi(oracle.L)
    api._cfg = cfg
    segs = Segments([[(s.xyzi, s.layout, s.tf, s.shift) for s in sc] for sc in case.scans])
    sd, sdbg = api.ingest_segments(ctx, segs, debug=True)
    _same(d, sd, dbg, sdbg)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_equals_ingest_points_motion(oracle, drv, n_scans):
    """one motion segment with knot0 0: cc_ingest_points_motion's bytes"""
    cfg = oracle.L.default_manager_cfg()
    sl = PR.case_slices()
    scans = [[Seg(sc[0].xyzi, (32, 0), motion=Motion(28, TIME_F32, 2.0, 16 / 0.1, 0, 16, sc[0].motion.words))] for sc in sl.scans]
    case = Case("one motion segment", scans, sl.pools[:, :16]).repeat(n_scans)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PR.check_case(drv, oracle, cfg, case, ctx)
    api = MotionApi(oracle.L)
    api._cfg = cfg
    buf = np.concatenate([sc[0].buffer() for sc in case.scans])
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in case.scans])]).astype(np.int64)
    md, mdbg = api.ingest_motion(ctx, buf, (32, 0), (28, TIME_F32, 16), offs, np.full(n_scans, 2.0, np.float32), np.full(n_scans, 16 / 0.1, np.float32), case.pools, debug=True)
    _same(d, md, dbg, mdbg)
    drv.close(ctx)


@pytest.mark.parametrize("n_scans", BATCHES)
def test_equals_ingest_points_filtered(oracle, drv, n_scans):
    """one tf segment with a rule: cc_ingest_points_filtered's bytes"""
    cfg = oracle.L.default_manager_cfg()
    mixed = PR.case_mixed("u8")
    tfs = PR.shift_knots(4, 9)
    scans = [[Seg(sc[1].xyzi, (32, 0), tf=tfs[i], flt=sc[1].flt, fill=3)] for i, sc in enumerate(mixed.scans)]
    case = Case("one tf segment", scans, None, mixed.rule).repeat(n_scans)
    ctx = drv.context(cfg, n_scans)
    d, dbg = PR.check_case(drv, oracle, cfg, case, ctx)
    api = FilterApi(oracle.L)
    api._cfg = cfg
    buf = np.concatenate([sc[0].buffer() for sc in case.scans])
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in case.scans])]).astype(np.int64)
    f, _bits = Rule(17, U8, 0, 0xFF, mixed.rule.kept, mixed.rule.keep_other).c()
    rc, fd, fdbg = api.ingest_filtered_rc(ctx, buf, (32, 0), f, offs, np.stack([tfs[i % 4] for i in range(n_scans)]), debug=True)
    assert rc == 0
    _same(d, fd, dbg, fdbg)
    drv.close(ctx)


def test_host_form_per_scan_form_and_chunks(oracle, drv):
    """The host and per-scan forms return the device form's descriptors; 3 scans go through a context of 2 in chunks."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    for case in (PR.case_mixed("u16", n_scans=3), PR.case_empties(n_scans=3), PR.case_mixed("range", n_scans=3)):
        ctx = drv.context(cfg, 2)
        ref, rdbg = PR.check_case(drv, oracle, cfg, case, ctx)
        arr, scan_segs, _held = case.table()
        f, _bits = PR.c_rule(case)
        for i in range(3):
            rc, d = api.scan_ingest_rig_rc(ctx, arr, int(scan_segs[i]), int(scan_segs[i + 1] - scan_segs[i]), case.pools[i], f)
            assert rc == 0 and not compare_desc(ref[i], d, float_exact=True), (case.name, i)
        rc, dh, bev = api.ingest_rig_host_rc(ctx, arr, scan_segs[1:], case.pools[1:], f, want_bev=True)   # with a leading scan that is skipped
        assert rc == 0 and dh.tobytes() == ref[1:].tobytes(), case.name
        assert np.array_equal(bev, rdbg["bev"][1:])
        drv.close(ctx)


def test_refusals(oracle, drv):
    """Every refused input returns CC_EINVAL from all three entry points, names the entry point, queues nothing, and a good call afterwards
    gives the reference bytes."""
    cfg = oracle.L.default_manager_cfg()
    api = drv.api
    case = PR.case_mixed("u16", n_scans=2)
    ctx = drv.context(cfg, 2)
    arr, scan_segs, _held = case.table()
    good, _bits = PR.c_rule(case)
    rc, ref, _ = api.ingest_rig_rc(ctx, arr, scan_segs, case.pools, good)
    assert rc == 0
    n_seg = len(arr)

    def table(k, **over):
        """a copy of the table with fields of segment k replaced"""
        a = (RigSegment * n_seg)()
        C.memmove(a, arr, C.sizeof(arr))
        for name, v in over.items():
            if name == "layout":
                a[k].layout.stride_bytes, a[k].layout.xyz_offset = v
            else:
                setattr(a[k], name, v)
        return a

    def rule(**over):
        f = type(good)(good.offset, good.type, good.shift, good.mask, good.n_classes, good.keep_other, 0.0, 0.0, good.keep_bits)
        for name, v in over.items():
            setattr(f, name, v)
        return f

    many = np.array([0, PR.RIG_SEG_MAX + 1], np.int32)
    big = (RigSegment * (PR.RIG_SEG_MAX + 1))()
    for k in range(PR.RIG_SEG_MAX + 1):
        C.memmove(C.addressof(big[k]), C.addressof(arr[4]), C.sizeof(RigSegment))
    nan = float("nan")
    # segments of the case: 0 none {16, 0} u16 at 14; 1 tf {32, 0} u16 at 18; 2 f32 time at 4, {48, 8}, u16 at 2; 3 u32 time at 12, {20, 0}, u16 at 18; 4 tf, unfiltered
    refused = {
        # what cc_ingest_segments refuses
        "a stride that is no multiple of 4": dict(tab=table(1, layout=(30, 0))),
        "xyz beyond the record": dict(tab=table(1, layout=(32, 24))),
        "a negative n_points": dict(tab=table(0, n_points=-1)),
        "2^21 points": dict(tab=table(0, n_points=1 << 21)),
        "a NULL pointer with points": dict(tab=table(0, points=None)),
        "a misaligned pointer": dict(tab=table(0, points=arr[0].points + 2)),
        "no segments": dict(segs=np.array([0, 0, n_seg], np.int32)),
        "more than CC_RIG_SEG_MAX segments": dict(tab=big, segs=many, n=1),
        "a scan of 10 records": dict(tab=table(0, n_points=10), segs=np.array([0, 1, 2], np.int32), n=1),
        # what cc_ingest_points_motion refuses
        "a time word on z": dict(tab=table(2, time_offset=16)),
        "a time word at an odd offset": dict(tab=table(2, time_offset=2)),
        "a time word beyond the record": dict(tab=table(2, time_offset=48)),
        "a negative time offset": dict(tab=table(2, time_offset=-4)),
        "a time type 2": dict(tab=table(2, time_type=2)),
        "no knots": dict(tab=table(2, n_knots=0)),
        "65 knots": dict(tab=table(2, n_knots=65)),
        "an infinite scale": dict(tab=table(3, scale=float("inf"))),
        "a NaN scale": dict(tab=table(3, scale=nan)),
        # the rig's own
        "mode 3": dict(tab=table(1, mode=3)),
        "mode -1": dict(tab=table(1, mode=-1)),
        "a slice beyond the pool": dict(tab=table(3, knot0=25)),
        "a slice longer than the pool": dict(tab=table(2, n_knots=33)),
        "a negative knot0": dict(tab=table(2, knot0=-1)),
        "a motion segment without a pool": dict(pools=None),
        "a pool of 0": dict(n_pool=0),
        "a pool of 65": dict(n_pool=65),
        "a filter offset of -2": dict(tab=table(1, filter_offset=-2)),
        "a filtered segment without a rule": dict(flt=None),
        # what cc_ingest_points_filtered refuses, against the segment's own layout
        "a filter word on x": dict(tab=table(0, filter_offset=0)),
        "a filter word on z's last bytes": dict(tab=table(2, filter_offset=18)),
        "a filter word on y (a record with room elsewhere)": dict(tab=table(1, filter_offset=6)),
        "a u16 at an odd offset": dict(tab=table(1, filter_offset=17)),
        "a filter word beyond the record": dict(tab=table(0, filter_offset=16)),
        "a filter word beyond a 20-byte record": dict(tab=table(3, filter_offset=20)),
        "type 4": dict(flt=rule(type=4)),
        "a u16 shifted by 16": dict(flt=rule(shift=16)),
        "a negative shift": dict(flt=rule(shift=-1)),
        "no classes": dict(flt=rule(n_classes=0)),
        "4 097 classes": dict(flt=rule(n_classes=4097)),
        "NULL keep_bits": dict(flt=rule(keep_bits=None)),
        "a u32 word where only a u16 fits in front of the time": dict(flt=rule(type=U32)),
        "a NaN lo": dict(flt=rule(type=F32, lo=nan, hi=1.0)),
    }
    for what, kw in refused.items():
        tab, segs, pools, flt, n_pool = kw.get("tab", arr), kw.get("segs", scan_segs), kw.get("pools", case.pools), kw.get("flt", good), kw.get("n_pool")
        rc, _, _ = api.ingest_rig_rc(ctx, tab, segs, pools, flt, n_pool=n_pool)
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_rig:"), (what, rc, api.lib.cc_last_error())
        rc, _, _ = api.ingest_rig_host_rc(ctx, tab, segs, pools, flt, n_pool=n_pool)
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_rig_host:"), (what, rc, api.lib.cc_last_error())
        s0, ns = int(segs[0]), int(segs[1] - segs[0])
        rc, _ = api.scan_ingest_rig_rc(ctx, tab, s0, ns, None if pools is None else pools[0], flt, n_pool=n_pool)
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_rig:"), (what, rc, api.lib.cc_last_error())
        rc, d, _ = api.ingest_rig_rc(ctx, arr, scan_segs, case.pools, good)
        assert rc == 0 and d.tobytes() == ref.tobytes(), what
    # NULL arguments
    assert api.lib.cc_ingest_rig(ctx, None, C.c_void_p(scan_segs.ctypes.data), 2, None, 0, None, C.c_void_p(ref.ctypes.data), None, None) == -1
    assert api.lib.cc_ingest_rig(ctx, arr, None, 2, None, 0, None, C.c_void_p(ref.ctypes.data), None, None) == -1
    # taken: a rule that no segment uses; a pool without a motion segment; the rule's own offset holding rubbish
    plain = Case("plain", [[Seg(s.xyzi, s.layout, s.shift, tf=s.tf) for s in sc if s.motion is None] for sc in case.scans])
    a2, s2, _h2 = plain.table()
    rc, d0, _ = api.ingest_rig_rc(ctx, a2, s2, None, None)
    rc1, d1, _ = api.ingest_rig_rc(ctx, a2, s2, case.pools, rule(offset=-77))
    assert rc == 0 and rc1 == 0 and d0.tobytes() == d1.tobytes()
    rc, d, _ = api.ingest_rig_rc(ctx, arr, scan_segs, case.pools, rule(offset=12345, lo=nan, hi=nan))
    assert rc == 0 and d.tobytes() == ref.tobytes()
    drv.close(ctx)


def test_rig_struct(cc):
    """the ctypes mirrors of cc_rig_segment_t: 104 bytes (the header carries a static_assert of the same)"""
    for S in (RigSegment, cc.L.RigSegment):
        assert C.sizeof(S) == 104 and S.mode.offset == 24 and S.filter_offset.offset == 28 and S.tf.offset == 32 and S.time_offset.offset == 80
        assert S.t_begin.offset == 88 and S.knot0.offset == 96 and S.n_knots.offset == 100
    assert cc.L.RIG_SEG_MAX == PR.RIG_SEG_MAX and (cc.L.RIG_NONE, cc.L.RIG_TF, cc.L.RIG_MOTION) == (PR.NONE, PR.TF, PR.MOTION)
