"""cc_db_verify_* (batched verification of caller-proposed candidates; hint lists generated on the device by
cc_k_hints_expand) on the CPU harness: against the oracle's hint flow on the demo's hint list, against cc_db_check_hints item
by item (memcmp), under dynamic thresholds, every refusal, and the streamed form."""
import ctypes as C

import numpy as np

import dyn_oracle
import emu_api
from test_dyn_thres_oracle import short_loop_drive
from test_emu_hints import INT_FIELDS, _demo_hints

CMAX = 8  # CC_VERIFY_CANDS_MAX
_drive = {}


def drive(cc, oracle):
    """The world of test_emu_hints.py::_run (64 scans of the looping world, delays 1.5 / 2.5), computed once per session."""
    if not _drive:
        _drive["v"] = short_loop_drive(cc, oracle)
    return _drive["v"]


class Verify:
    """ctypes helper around EmuApi(...).lib for the three verify entry points ("device" pointers are host pointers there)."""

    def __init__(self, L, desc, ts, seeds, dcfg):
        self.L = L
        self.api = emu_api.EmuApi(L)
        self.lib = self.api.lib
        self.ctx = self.api.create(max_batch=8)
        self.db = self.api.db_create(self.ctx, dcfg, cap=len(desc))
        self.api.db_add(self.db, desc, ts, seeds)
        self.keep = []

    table = staticmethod(emu_api.calls.cand_table)

    def raw(self, fn, qdesc, n_desc, qidx, tab, n, cfg, lb, ub, res, hints=None, cnt=None, host=False):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)  # noqa: E731
        b = lambda s: None if s is None else C.cast(C.byref(s), C.c_void_p)  # noqa: E731
        if host:
            return self.lib.cc_db_verify_batch_host(self.db, p(qdesc), n_desc, p(qidx), p(tab), n, b(cfg), b(lb), b(ub), p(res))
        return getattr(self.lib, fn)(self.db, p(qdesc), n_desc, p(qidx), p(tab), n, b(cfg), b(lb), b(ub), p(res), p(hints), p(cnt), None)

    def run(self, qdesc, cands, qidx=None, mask=0, mfo=10, bound=1000.0, lb=None, ub=None, submit=False, host=False):
        """-> (results, list of hint arrays per item); with submit the results are valid after api.db_query_wait"""
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        n = len(cands)
        hints = np.zeros((max(n, 1), L.HINT_MAX), L.hint_dt)
        cnt = np.zeros(max(n, 1), np.int32)
        self.keep.append((qdesc, hints, cnt))
        if host:
            if lb is None:
                lb, ub = L.default_thresholds()
            tab = self.table(cands)
            qi = None if qidx is None else np.ascontiguousarray(qidx, np.int32)
            res = np.zeros(n, L.query_result_dt)
            self.api.chk(self.raw(None, qdesc, len(qdesc), qi, tab, n, L.VerifyCfg(mask, mfo, bound, 0), lb, ub, res, host=True), "cc_db_verify")
        else:
            r = emu_api.calls.verify(self.lib, self.db, cands, qdesc=qdesc.ctypes.data, n_desc=len(qdesc), qidx=qidx, levels=emu_api.levels_of(mask),
                                     max_fine_opt=mfo, max_key_dist_sq=bound, lb=lb, ub=ub, hints=hints.ctypes.data, n_hints=cnt.ctypes.data, wait=not submit, keep=self.keep)
            res = r.res
        return res, [hints[i, :cnt[i]] for i in range(n)]


def _expected_hints(L, desc, q, cands, levels=(1, 2, 3, 4)):
    h = _demo_hints(L, desc, q, cands, levels)
    out = np.zeros(len(h), L.hint_dt)
    if len(h):
        out["cand_gidx"] = np.array(cands)[h[:, 0]]
        out["level"], out["seq_src"], out["seq_tgt"] = h[:, 1], h[:, 2], h[:, 3]
    return h, out


def _cand_list(c, n_scans):
    """[c, c-1, c+1, 3] as ONE item.  An item may not name a scan twice or a scan outside the database (CC_EINVAL), so where the
    pattern does (the drive's second closed query has c = 0: c-1 is no scan, and test_emu_hints.py's max(c-1, 0) repeats c) the
    entry is left out; the oracle gets the same list."""
    out = []
    for g in (c, c - 1, c + 1, 3):
        if 0 <= g < n_scans and g not in out:
            out.append(g)
    return out


def _assert_bound_is_not_marginal(L, desc, q, cands, bound=1000.0):
    """no anchor pair of the inputs has a key distance within a relative 1e-4 of the bound (f64): summation order cannot decide
    which hints exist"""
    for c in cands:
        k1 = desc["keys"][c][1:5].astype(np.float64).reshape(4, L.NPIV, 1, L.KEY_DIM)
        k2 = desc["keys"][q][1:5].astype(np.float64).reshape(4, 1, L.NPIV, L.KEY_DIM)
        d = ((k1 - k2) ** 2).sum(-1)
        assert not (np.abs(d - bound) <= 1e-4 * bound).any(), (q, c)


def test_oracle_parity(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    L = oracle.L
    v = Verify(L, desc, ts, seeds, dcfg)
    hit = np.nonzero(ores["n_res"] > 0)[0]
    assert len(hit) >= 2
    n_full = 0
    for qi in hit[:2]:
        c = int(ores["cand_gidx"][qi])
        cands = _cand_list(c, len(desc))
        assert len(cands) >= 3
        _assert_bound_is_not_marginal(L, desc, qi, cands)
        hints, exp_h = _expected_hints(L, desc, qi, cands)
        assert len(hints) > 30
        oscans = [oracle.Scan.from_desc(desc[g], int_id=int(g)) for g in cands]
        otgt = oracle.Scan.from_desc(desc[qi], int_id=int(qi))
        for mfo in (5, 1):
            eres, _ = oracle.check_hints(otgt, oscans, hints, sim=dcfg.cont_sim, max_fine_opt=mfo)
            res, got_h = v.run(desc[qi:qi + 1], [cands], mfo=mfo)
            res = res[0]
            assert got_h[0].tobytes() == exp_h.tobytes(), (qi, len(got_h[0]), len(exp_h))
            for f in INT_FIELDS:
                exp = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[int(eres[f])]
                assert exp == res[f], (qi, f, exp, res[f])
            assert res["n_knn_hits"] == len(hints)
            if eres["n_res"]:
                assert abs(eres["correlation"] - res["correlation"]) < 1e-6
                assert np.abs(eres["tf"] - res["tf"]).max() < 1e-6
            n_full += int(res["cand_aft_check3"] > 0 and res["n_res"] == 1)
    assert n_full > 0, "no item reached the merge and the correlation"


def _items(n_scans, ores):
    """>= 12 items: lists of 1, 4 and 8 candidates, an empty list, descriptors shared through qidx"""
    hit = np.nonzero(ores["n_res"] > 0)[0]
    q0, q1 = int(hit[0]), int(hit[1])
    c0, c1 = int(ores["cand_gidx"][q0]), int(ores["cand_gidx"][q1])
    rng = np.random.default_rng(11)
    qs = [q0, q1, 50, 63]  # the batch's descriptors
    items = [(0, [c0]), (0, [c0 + 1]), (1, _cand_list(c1, n_scans) + [5]), (1, [c1]), (2, []),
             (0, [c0, c0 + 1, c0 + 2, max(c0 - 1, 0), 3, 40, 41, 62]), (3, [int(x) for x in rng.choice(n_scans, 8, replace=False)]),
             (2, [int(x) for x in rng.choice(n_scans, 4, replace=False)]), (3, [63]), (1, [int(x) for x in rng.choice(n_scans, 8, replace=False)]),
             (2, [c0, c1]), (0, [c1, c0]), (3, [c1, 2, c0, 7])]
    return qs, items


def test_batch_shape_memcmp_with_check_hints(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    L = oracle.L
    v = Verify(L, desc, ts, seeds, dcfg)
    qs, items = _items(len(desc), ores)
    assert len(items) >= 12 and {len(c) for _, c in items} >= {0, 1, 4, 8}
    qdesc = np.ascontiguousarray(desc[qs])
    qidx = [k for k, _ in items]
    cands = [c for _, c in items]
    before = v.api.db_query(v.db, desc[40:], seeds[40:])
    n_res = 0
    for mask, bound, levels in ((0, 1000.0, (1, 2, 3, 4)), (0b0110, 1000.0, (2, 3)), (0, float("inf"), (1, 2, 3, 4))):
        res, hl = v.run(qdesc, cands, qidx=qidx, mask=mask, mfo=5, bound=bound)
        for i, (k, c) in enumerate(items):
            if bound == 1000.0:  # the list itself: the demo's loop
                _, exp_h = _expected_hints(L, desc, qs[k], c, levels)
                assert hl[i].tobytes() == exp_h.tobytes(), (i, mask)
            else:  # no bound: every pair of existing anchors
                exp = [(g, lv, a, b) for g in c for lv in levels for a in range(L.NPIV) for b in range(L.NPIV)
                       if desc["keys"][g][lv][a].sum() != 0 and desc["keys"][qs[k]][lv][b].sum() != 0]
                got = [(int(h["cand_gidx"]), int(h["level"]), int(h["seq_src"]), int(h["seq_tgt"])) for h in hl[i]]
                assert got == exp, (i, len(got), len(exp))
            one, _ = v.api.check_hints(v.db, qdesc[k:k + 1], hl[i], max_fine_opt=5)
            assert res[i].tobytes() == one.tobytes(), (i, mask, bound, res[i], one)
            assert res[i]["n_knn_hits"] == len(hl[i])
            if len(c) == 0 or len(hl[i]) == 0:
                assert res[i]["n_res"] == 0
            n_res += int(res[i]["n_res"])
        # the host-descriptor form gives the same bytes
        res_h, _ = v.run(qdesc, cands, qidx=qidx, mask=mask, mfo=5, bound=bound, host=True)
        assert res_h.tobytes() == res.tobytes()
    assert n_res >= 3
    # identity (no qidx): item i reads descriptor i
    res_i, hl_i = v.run(qdesc, [items[0][1], items[3][1], items[4][1], items[8][1]], mfo=5)
    for i, k in enumerate((0, 3, 4, 8)):
        ref, _ = v.run(qdesc, [items[k][1]], qidx=[i], mfo=5)
        assert res_i[i].tobytes() == ref[0].tobytes()
    after = v.api.db_query(v.db, desc[40:], seeds[40:])
    assert before.tobytes() == after.tobytes()


def test_dynamic_thresholds(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    L = oracle.L
    v = Verify(L, desc, ts, seeds, dcfg)
    assert v.lib.cc_db_set_dynamic_thres(v.db, 1) == 0
    qi = int(np.nonzero(ores["n_res"] > 0)[0][0])
    c = int(ores["cand_gidx"][qi])
    cands = _cand_list(c, len(desc))
    _assert_bound_is_not_marginal(L, desc, qi, cands)
    hints, exp_h = _expected_hints(L, desc, qi, cands)
    eres, _ = dyn_oracle.check_hints(desc, qi, cands, hints, dcfg.cont_sim, max_fine_opt=5, dyn=1)
    res, hl = v.run(desc[qi:qi + 1], [cands], mfo=5)
    assert hl[0].tobytes() == exp_h.tobytes()
    for f in INT_FIELDS:
        exp = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[int(eres[f])]
        assert exp == res[0][f], (f, exp, res[0][f])
    if eres["n_res"]:
        assert abs(eres["correlation"] - res[0]["correlation"]) < 1e-6 and np.abs(eres["tf"] - res[0]["tf"]).max() < 1e-6
    one, _ = v.api.check_hints(v.db, desc[qi:qi + 1], hl[0], max_fine_opt=5)
    assert one.tobytes() == res[0].tobytes()


def test_validation(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    L = oracle.L
    v = Verify(L, desc, ts, seeds, dcfg)
    n_db = len(desc)
    lb, ub = L.default_thresholds()
    qdesc = np.ascontiguousarray(desc[60:62])
    ref = v.api.db_query(v.db, desc[56:], seeds[56:])
    res = np.zeros(2, L.query_result_dt)
    ok_tab = Verify.table([[3, 4], [5]])
    ok_cfg = L.VerifyCfg(0, 5, 1000.0, 0)
    EINVAL = -1

    def call(fn="cc_db_verify_batch", qd=qdesc, n_desc=2, qidx=None, tab=ok_tab, n=2, cfg=ok_cfg, lb_=lb, ub_=ub, res_=res, host=False):
        return v.raw(fn, qd, n_desc, qidx, tab, n, cfg, lb_, ub_, res_, host=host)

    assert call() == 0  # the well-formed call the bad ones are variations of
    bad_ub = L.Score.from_buffer_copy(bytes(ub))
    bad_ub.i_ovlp_sum = lb.i_ovlp_sum
    cases = {
        "null descriptors": dict(qd=None),
        "null candidates": dict(tab=None),
        "null cfg": dict(cfg=None),
        "null lb": dict(lb_=None),
        "null ub": dict(ub_=None),
        "null results": dict(res_=None),
        "n < 0": dict(n=-1),
        "identity needs n == n_desc": dict(n=1),
        "qidx below 0": dict(qidx=np.array([0, -1], np.int32)),
        "qidx beyond n_desc": dict(qidx=np.array([2, 0], np.int32)),
        "candidate beyond the DB": dict(tab=Verify.table([[3, n_db], [5]])),
        "candidate below -1": dict(tab=Verify.table([[3, -2], [5]])),
        "candidate twice": dict(tab=Verify.table([[3, 4, 3], [5]])),
        "entry after the first -1": dict(tab=Verify.table([[3, -1, 4], [5]])),
        "max_fine_opt 0": dict(cfg=L.VerifyCfg(0, 0, 1000.0, 0)),
        "level_mask 16": dict(cfg=L.VerifyCfg(16, 5, 1000.0, 0)),
        "level_mask -1": dict(cfg=L.VerifyCfg(-1, 5, 1000.0, 0)),
        "bound NaN": dict(cfg=L.VerifyCfg(0, 5, float("nan"), 0)),
        "bound negative": dict(cfg=L.VerifyCfg(0, 5, -1.0, 0)),
        "lb not below ub": dict(ub_=bad_ub),
    }
    for what, kw in cases.items():
        for fn, host in (("cc_db_verify_batch", False), ("cc_db_verify_submit", False), ("cc_db_verify_batch", True)):
            assert call(fn=fn, host=host, **kw) == EINVAL, (what, fn, host)
        got = v.api.db_query(v.db, desc[56:], seeds[56:])
        assert got.tobytes() == ref.tobytes(), what
    # a refused call leaves a chunk in flight untouched: it is still collected by the wait, with the right answer
    sync, _ = v.run(qdesc, [[3, 4], [5]], mfo=5)
    pend, _ = v.run(qdesc, [[3, 4], [5]], mfo=5, submit=True)
    assert call(cfg=L.VerifyCfg(16, 5, 1000.0, 0), fn="cc_db_verify_submit") == EINVAL
    v.api.db_query_wait(v.db)
    assert pend.tobytes() == sync.tobytes()


def test_streaming(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    L = oracle.L
    v = Verify(L, desc, ts, seeds, dcfg)
    qs, items = _items(len(desc), ores)
    qdesc = np.ascontiguousarray(desc[qs])
    b1, b2 = items[:7], items[7:]
    s1, h1 = v.run(qdesc, [c for _, c in b1], qidx=[k for k, _ in b1], mfo=5)
    s2, h2 = v.run(qdesc, [c for _, c in b2], qidx=[k for k, _ in b2], mfo=3, mask=0b0011)
    sq = v.api.db_query(v.db, desc[58:], seeds[58:])
    a1, g1 = v.run(qdesc, [c for _, c in b1], qidx=[k for k, _ in b1], mfo=5, submit=True)
    aq, keep = v.api.db_query_submit(v.db, desc[58:], seeds[58:])  # a query batch between the two: the lanes are shared
    a2, g2 = v.run(qdesc, [c for _, c in b2], qidx=[k for k, _ in b2], mfo=3, mask=0b0011, submit=True)
    v.api.db_query_wait(v.db)
    assert a1.tobytes() == s1.tobytes() and a2.tobytes() == s2.tobytes() and aq.tobytes() == sq.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(h1 + h2, g1 + g2))
