"""Which C function each form of the scoring flows calls, with how many arguments and which pointers NULL (calls.py), on a
recording fake in the place of the library: no built library, no GPU.  The rows are the dispatch table of calls.py's docstring;
the entry point decides how a batch is chunked, so it is behaviour."""
import ctypes as C

import numpy as np
import pytest

CC_EINVAL, CC_ECAPACITY = -1, -4
DB, QD, STREAM, KNN, CNT, HINTS, NHINTS, BITS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000
WAIT = "cc_db_query_wait"


class FakeLib:
    """attribute lookup gives a callable that records (symbol, args) and returns 0, or what `rcs` holds for the symbol"""

    def __init__(self, **rcs):
        self.log, self.rcs = [], rcs

    def __getattr__(self, name):
        def fn(*args):
            self.log.append((name, args))
            return b"the canned message" if name == "cc_last_error" else self.rcs.get(name, 0)
        return fn

    def names(self):
        return [n for n, _a in self.log]


@pytest.fixture(scope="module")
def calls(cc):
    return cc.calls


def nulls(args):
    return {i for i, a in enumerate(args) if a is None}


def src(cc):
    return cc.L.PackedSrc(0x9000, 0xA000, 4, 0)


def mask():
    return (BITS, 1, 1, np.zeros(2, np.int32))


def run_query(calls, lib, wait, **kw):
    return calls.query(lib, DB, [5, 6], stream=STREAM, wait=wait, **kw)


def run_verify(calls, lib, wait, **kw):
    return calls.verify(lib, DB, [[1, 2], [3]], stream=STREAM, wait=wait, **kw)


def run_pose(calls, lib, wait, **kw):
    return calls.pose(lib, DB, [0, 1], [2, 3], np.zeros((2, 3)), stream=STREAM, wait=wait, **kw)


# (flow, keywords, wait) -> (symbol, argument count, NULL positions, the wait follows)
def rows(cc):
    s, qd, vd = src(cc), dict(qdesc=QD), dict(qdesc=QD, n_desc=2)
    knn, hints = dict(knn=KNN, knn_cnt=CNT), dict(hints=HINTS, n_hints=NHINTS)
    return [
        # query(): descriptors [db, qdesc, nq, epochs, lb, ub, res, knn, cnt, stream, (rank, (detail))]
        (run_query, dict(qd, **knn), True, "cc_db_query_batch", 10, set(), False),
        (run_query, dict(qd), True, "cc_db_query_batch", 10, {7, 8}, False),
        (run_query, dict(qd, ranked=3, **knn), True, "cc_db_query_submit_ranked", 11, set(), True),
        (run_query, dict(qd, ranked=3, detail=True), True, "cc_db_query_submit_ranked_detail", 12, {7, 8}, True),
        # a source [db, src, rec, nq, epochs, lb, ub, res, knn, cnt, stream, rank, detail]
        (run_query, dict(src=s), True, "cc_db_query_submit_packed", 13, {2, 8, 9, 11, 12}, True),
        (run_query, dict(src=s, idx=[1, 0], ranked=2, detail=True, **knn), True, "cc_db_query_submit_packed", 13, set(), True),
        (run_query, dict(src=s, ranked=2), True, "cc_db_query_submit_packed", 13, {2, 8, 9, 12}, True),
        # a mask [db, qdesc, src, rec, nq, epochs, lb, ub, res, knn, cnt, stream, rank, detail, mask]: d_qdesc or src, never both
        (run_query, dict(qd, mask=mask()), True, "cc_db_query_submit_masked", 15, {2, 3, 9, 10, 12, 13}, True),
        (run_query, dict(src=s, idx=[1, 0], mask=mask(), ranked=2, detail=True, **knn), True, "cc_db_query_submit_masked", 15, {1}, True),
        # query_submit(): no hit lists
        (run_query, dict(qd), False, "cc_db_query_submit", 10, {7, 8}, False),
        (run_query, dict(qd, ranked=3), False, "cc_db_query_submit_ranked", 11, {7, 8}, False),
        (run_query, dict(qd, ranked=3, detail=True), False, "cc_db_query_submit_ranked_detail", 12, {7, 8}, False),
        (run_query, dict(src=s), False, "cc_db_query_submit_packed", 13, {2, 8, 9, 11, 12}, False),
        (run_query, dict(qd, mask=mask()), False, "cc_db_query_submit_masked", 15, {2, 3, 9, 10, 12, 13}, False),
        (run_query, dict(src=s, mask=mask()), False, "cc_db_query_submit_masked", 15, {1, 3, 9, 10, 12, 13}, False),
        # verify(): descriptors [db, qdesc, n_desc, qidx, cands, n, cfg, lb, ub, res, hints, n_hints, stream, (rank, (detail))]
        (run_verify, dict(vd, **hints), True, "cc_db_verify_batch", 13, {3}, False),
        (run_verify, dict(vd, qidx=[1, 0], ranked=4, **hints), True, "cc_db_verify_submit_ranked", 14, set(), True),
        (run_verify, dict(vd, ranked=4, detail=True), True, "cc_db_verify_submit_ranked_detail", 15, {3, 10, 11}, True),
        # a source [db, src, qidx, cands, n, cfg, lb, ub, res, hints, n_hints, stream, rank, detail]
        (run_verify, dict(src=s, idx=[1, 0]), True, "cc_db_verify_submit_packed", 14, {9, 10, 12, 13}, True),
        (run_verify, dict(src=s, qidx=[1, 0], ranked=2, detail=True, **hints), True, "cc_db_verify_submit_packed", 14, set(), True),
        # verify_submit(): d_hints and d_n_hints NULL
        (run_verify, dict(vd), False, "cc_db_verify_submit", 13, {3, 10, 11}, False),
        (run_verify, dict(vd, ranked=4), False, "cc_db_verify_submit_ranked", 14, {3, 10, 11}, False),
        (run_verify, dict(vd, ranked=4, detail=True), False, "cc_db_verify_submit_ranked_detail", 15, {3, 10, 11}, False),
        (run_verify, dict(src=s), False, "cc_db_verify_submit_packed", 14, {2, 9, 10, 12, 13}, False),
        # score_poses(): descriptors [db, qdesc, n_desc, items, n, cfg, tries, res, try_corr, curv, stream]
        (run_pose, dict(vd), True, "cc_db_pose_batch", 11, {6, 8, 9}, False),
        (run_pose, dict(vd, tries=np.zeros((2, 3, 3)), curvature=True), True, "cc_db_pose_batch", 11, set(), False),
        # a source [db, src, items, n, cfg, tries, res, try_corr, curv, stream]
        (run_pose, dict(src=s), True, "cc_db_pose_submit_packed", 10, {5, 7, 8}, True),
        # score_poses_submit()
        (run_pose, dict(vd, curvature=True), False, "cc_db_pose_submit", 11, {6, 8}, False),
        (run_pose, dict(src=s, tries=np.zeros((2, 1, 3))), False, "cc_db_pose_submit_packed", 10, {8}, False),
    ]


def test_every_row_of_the_dispatch_table(cc, calls):
    for flow, kw, wait, symbol, n_args, null_at, waits in rows(cc):
        lib = FakeLib()
        out = flow(calls, lib, wait, **kw)
        what = (flow.__name__, sorted(kw), wait)
        assert lib.names() == [symbol] + ([WAIT] if waits else []), what
        args = lib.log[0][1]
        assert len(args) == n_args and nulls(args) == null_at, (what, nulls(args))
        assert args[0] == DB and STREAM in args and all(a is None or isinstance(a, int) for a in args), what
        if waits:
            assert lib.log[1][1] == (DB,), what
        assert len(out.res) == 2 and out.keep, what


def test_query_arguments_are_the_buffers_handed_back(cc, calls):
    """the addresses in the tuple are those of the record's arrays; the structs the library reads are kept"""
    L, lib = cc.L, FakeLib()
    r = run_query(calls, lib, False, src=src(cc), idx=[3, 1], mask=mask(), ranked=2, detail=True)
    a = lib.log[0][1]
    assert a[1] is None and a[4] == 2 and a[8] == r.res.ctypes.data and a[13] == r.detail.ctypes.data
    ro = C.cast(a[12], C.POINTER(L.RankOut)).contents
    assert (ro.h_cands, ro.h_n, ro.max_ret) == (r.rank[0].ctypes.data, r.rank[1].ctypes.data, 2)
    m = C.cast(a[14], C.POINTER(L.ScanMaskC)).contents
    assert (m.bits, m.n_rows, m.row_words) == (BITS, 1, 1) and np.ctypeslib.as_array(C.cast(m.h_row, C.POINTER(C.c_int32)), (2,)).tolist() == [0, 0]
    assert np.ctypeslib.as_array(C.cast(a[3], C.POINTER(C.c_int32)), (2,)).tolist() == [3, 1]
    assert np.ctypeslib.as_array(C.cast(a[5], C.POINTER(C.c_int32)), (2,)).tolist() == [5, 6]
    assert r.rank[0].shape == (2, 2) and r.detail.shape == (2, 2)


def test_check_hints_rows(cc, calls):
    """[db, qdesc, hints, n, lb, ub, max_fine_opt, res, scores, stream, (rank, (detail))], one query, never a wait"""
    hints = np.zeros(5, cc.L.hint_dt)
    for kw, symbol, n_args in ((dict(), "cc_db_check_hints", 10), (dict(ranked=3), "cc_db_check_hints_ranked", 11),
                               (dict(ranked=3, detail=True), "cc_db_check_hints_ranked_detail", 12)):
        lib = FakeLib()
        r = calls.check_hints(lib, DB, QD, hints, max_fine_opt=7, stream=STREAM, **kw)
        assert lib.names() == [symbol]
        a = lib.log[0][1]
        assert len(a) == n_args and nulls(a) == set() and a[:2] == (DB, QD) and (a[3], a[6], a[9]) == (5, 7, STREAM)
        assert len(r.res) == 1 and len(r.scores) == 5 and (r.rank is None) == ("ranked" not in kw) and (r.detail is None) == ("detail" not in kw)


def test_a_refused_submit_keeps_its_message(cc, calls):
    """the submit returns CC_EINVAL: the message is read first, then the wait drains the lanes, then the exception carries the
    submit's label, code and message"""
    for flow, kw, symbol in ((run_query, dict(qdesc=QD, ranked=2), "cc_db_query_submit_ranked"),
                             (run_query, dict(src=src(cc)), "cc_db_query_submit_packed"),
                             (run_verify, dict(src=src(cc)), "cc_db_verify_submit_packed"),
                             (run_pose, dict(src=src(cc)), "cc_db_pose_submit_packed")):
        lib = FakeLib(**{symbol: CC_EINVAL})
        with pytest.raises(cc.CCError) as e:
            flow(calls, lib, True, **kw)
        assert lib.names() == [symbol, "cc_last_error", WAIT]
        assert e.value.rc == CC_EINVAL and str(e.value) == "%s failed (%d): the canned message" % (symbol, CC_EINVAL)
    # the synchronous batch call and a submit left in flight: no wait
    for wait, symbol in ((True, "cc_db_query_batch"), (False, "cc_db_query_submit")):
        lib = FakeLib(**{symbol: CC_EINVAL})
        with pytest.raises(cc.CCError, match="%s failed" % symbol):
            run_query(calls, lib, wait, qdesc=QD)
        assert lib.names() == [symbol, "cc_last_error"]


def test_a_failed_submit_leaves_its_buffers_with_the_caller(cc, calls):
    """A wait=False submit that returns an error may have queued some of its chunks (a lane's earlier chunk reporting
    CC_ECAPACITY, an allocation failing at chunk k): the library writes their results until the wait.  The flow has put every
    buffer of the call into the caller's `keep` list before the entry point ran, and that is where the library's pointers lead."""
    for flow, kw, symbol, res_at in ((run_query, dict(qdesc=QD, ranked=2, detail=True), "cc_db_query_submit_ranked_detail", 6),
                                     (run_query, dict(src=src(cc), mask=mask()), "cc_db_query_submit_masked", 8),
                                     (run_verify, dict(qdesc=QD, n_desc=2, ranked=2), "cc_db_verify_submit_ranked", 9),
                                     (run_verify, dict(src=src(cc)), "cc_db_verify_submit_packed", 8),
                                     (run_pose, dict(qdesc=QD, n_desc=2, curvature=True), "cc_db_pose_submit", 7),
                                     (run_pose, dict(src=src(cc)), "cc_db_pose_submit_packed", 6)):
        lib, keep = FakeLib(**{symbol: CC_ECAPACITY}), []
        with pytest.raises(cc.CCError) as e:
            flow(calls, lib, False, keep=keep, **kw)
        assert e.value.rc == CC_ECAPACITY and lib.names() == [symbol, "cc_last_error"]  # no wait: the caller's query_wait drains
        assert len(keep) == 1
        arrays = [x for x in keep[0] if isinstance(x, np.ndarray)] + [y for x in keep[0] if isinstance(x, tuple) for y in x if isinstance(y, np.ndarray)]
        assert lib.log[0][1][res_at] in [x.ctypes.data for x in arrays], symbol
        held = {x.ctypes.data for x in arrays} | {C.addressof(x) for x in keep[0] if isinstance(x, C.Structure)}
        held |= {C.addressof(y) for x in keep[0] if isinstance(x, tuple) for y in x if isinstance(y, C.Structure)}
        host = [a for i, a in enumerate(lib.log[0][1]) if isinstance(a, int) and a > 0xFFFF]  # every address the flow made itself
        assert host and set(host) <= held, symbol
    lib, keep = FakeLib(), []  # and a submit that succeeds registers the same way; the record's keep is that entry
    r = run_query(calls, lib, False, qdesc=QD, keep=keep)
    assert keep == [r.keep]


def test_capacity_is_tolerated_only_when_allowed(cc, calls):
    """the wait returns CC_ECAPACITY (every result delivered, some flagged): an error without allow_flagged's tolerance, the
    results with it; the same on the synchronous batch call"""
    for flow, kw, failing in ((run_query, dict(qdesc=QD, ranked=2), WAIT), (run_verify, dict(src=src(cc)), WAIT),
                              (run_pose, dict(src=src(cc)), WAIT), (run_query, dict(qdesc=QD), "cc_db_query_batch"),
                              (run_verify, dict(qdesc=QD, n_desc=2), "cc_db_verify_batch"), (run_pose, dict(qdesc=QD, n_desc=2), "cc_db_pose_batch")):
        lib = FakeLib(**{failing: CC_ECAPACITY})
        with pytest.raises(cc.CCError) as e:
            flow(calls, lib, True, **kw)
        assert e.value.rc == CC_ECAPACITY and str(e.value).startswith("%s failed (-4)" % failing)
        lib = FakeLib(**{failing: CC_ECAPACITY})
        r = flow(calls, lib, True, tolerate=(CC_ECAPACITY,), **kw)
        assert len(r.res) == 2 and lib.names()[-1] == failing and "cc_last_error" not in lib.names()


def test_refusals_before_the_library_is_called(cc, calls):
    lib, s = FakeLib(), src(cc)
    bad = [
        (ValueError, "detail=True needs ranked=K", lambda: run_query(calls, lib, True, qdesc=QD, detail=True)),
        (ValueError, "detail=True needs ranked=K", lambda: run_verify(calls, lib, True, qdesc=QD, n_desc=2, detail=True)),
        (ValueError, "detail=True needs ranked=K", lambda: calls.check_hints(lib, DB, QD, np.zeros(1, cc.L.hint_dt), detail=True)),
        (ValueError, "the source names 3 records for 2 epochs", lambda: run_query(calls, lib, True, src=s, idx=[0, 1, 2])),
        (ValueError, "the mask names rows for 3 queries, the call has 2", lambda: run_query(calls, lib, True, qdesc=QD, mask=(BITS, 1, 1, np.zeros(3, np.int32)))),
        (ValueError, "not both", lambda: run_verify(calls, lib, True, src=s, idx=[0, 1], qidx=[0, 1])),
        (ValueError, "qidx must name one descriptor per item", lambda: run_verify(calls, lib, True, qdesc=QD, n_desc=2, qidx=[0])),
        (ValueError, "hint levels are 1..4", lambda: run_verify(calls, lib, True, qdesc=QD, n_desc=2, levels=(0,))),
        (ValueError, "no hint level given", lambda: run_verify(calls, lib, True, qdesc=QD, n_desc=2, levels=())),
        (ValueError, "item 1: more than VERIFY_CANDS_MAX = 8 candidates", lambda: calls.verify(lib, DB, [[1], list(range(9))], qdesc=QD, n_desc=2)),
        (ValueError, "give the source without idx", lambda: run_pose(calls, lib, True, src=s, idx=[0, 1])),
        (ValueError, "tries must have shape", lambda: run_pose(calls, lib, True, qdesc=QD, n_desc=2, tries=np.zeros((2, 3)))),
        (ValueError, "must name one item each", lambda: calls.pose(lib, DB, [0, 1], [2], np.zeros((2, 3)), qdesc=QD, n_desc=2)),
    ]
    for exc, text, call in bad:
        with pytest.raises(exc, match=text):
            call()
    assert lib.log == []
    tab = calls.cand_table(np.array([[1, 2, -1, -1, -1, -1, -1, -1, -1, -1]]))  # padding beyond the eighth column is no candidate
    assert tab.shape == (1, 8) and tab[0].tolist() == [1, 2, -1, -1, -1, -1, -1, -1]
    assert calls.level_mask((1, 3)) == 5 and calls.level_mask((1, 2, 3, 4)) == 15
    assert calls.level_mask(None) == 0  # cc_verify_cfg_t: 0 stands for all four levels


def test_verify_and_pose_configs(cc, calls):
    """cc_verify_cfg_t and cc_pose_cfg_t as the call's keywords give them; the candidate table and the items"""
    L, lib = cc.L, FakeLib()
    kept = run_verify(calls, lib, False, qdesc=QD, n_desc=2, levels=(2, 4), max_fine_opt=6, max_key_dist_sq=50.0)
    a = lib.log[0][1]
    cfg = C.cast(a[6], C.POINTER(L.VerifyCfg)).contents
    assert bytes(cfg) == bytes(L.VerifyCfg(10, 6, 50.0, 0)) and (a[2], a[5]) == (2, 2)
    assert np.ctypeslib.as_array(C.cast(a[4], C.POINTER(C.c_int32)), (2, 8)).tolist() == [[1, 2] + [-1] * 6, [3] + [-1] * 7] and kept.keep
    lib = FakeLib()
    r = run_pose(calls, lib, False, qdesc=QD, n_desc=2, refine=False, min_corr=0.5, tries=np.zeros((2, 3, 3)))
    a = lib.log[0][1]
    assert bytes(C.cast(a[5], C.POINTER(L.PoseCfg)).contents) == bytes(L.PoseCfg(0, 0.5, 3, 0)) and a[4] == 2
    assert r.try_corr.shape == (2, 3) and r.curv is None and a[8] == r.try_corr.ctypes.data
    lib = FakeLib()
    kept = run_pose(calls, lib, False, qdesc=QD, n_desc=2)  # min_corr None: the shipped lb.correlation
    assert bytes(C.cast(lib.log[0][1][5], C.POINTER(L.PoseCfg)).contents) == bytes(L.PoseCfg(1, L.default_thresholds()[0].correlation, 0, 0))
    assert kept.keep
