"""cc_db_query_submit_packed / cc_db_verify_submit_packed / cc_db_pose_submit_packed on the CPU harness: the query of every
scoring flow taken from packed records (a caller's cc_pack_scans arrays) or from the database's own rows instead of from
descriptors.  The yardstick is the descriptor form of the same call on the descriptors the records were packed from: every
output is compared by tobytes().  The drive is the 64-scan looping world of test_dyn_thres_oracle.py (31 loop closures)."""
import numpy as np
import pytest

import packed_emu as P
from test_emu_verify import drive

INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy",
              "n_knn_hits"]
N = 64
_state = {}


def world(cc, oracle, lanes=2):
    """the drive, a two-lane database holding it, and its packed records (once per session)"""
    if "w" not in _state:
        desc, ts, seeds, dcfg, ores = drive(cc, oracle)
        e = P.PackedEmu(oracle.L, dcfg, cap=N, lanes=lanes)
        e.add(desc, ts, seeds)
        _state["w"] = (e, desc, e.pack(desc), ores)
    return _state["w"]


def not_empty(out, n_hit=4, n_ranked=None):
    """equality of empty answers must not pass a comparing test: asserted on the descriptor path's outputs"""
    assert (out["res"]["n_res"] > 0).sum() >= n_hit, out["res"]["n_res"]
    if n_ranked is not None:
        assert (out["rank_n"] >= 2).sum() >= n_ranked, out["rank_n"]


def cycled(n):
    return (np.arange(n) % N).astype(np.int32)


# ---- 1: replay from the database ----
def test_replay_from_the_database(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    ep = np.arange(N, dtype=np.int32)
    a = e.query(desc, None, ep)
    not_empty(a, 31)
    b = e.query(e.src(), ep, ep)
    P.same_bytes(a, b)
    for f in INT_FIELDS:
        assert np.array_equal(ores[f], b["res"][f]), f
    m = ores["n_res"] > 0
    assert np.abs(ores["correlation"][m] - b["res"]["correlation"][m]).max() < 1e-4
    assert np.abs(ores["tf"][m] - b["res"]["tf"][m]).max() < 1e-4
    # record i without a selector (h_rec NULL)
    P.same_bytes(a, e.query(e.src(), None, ep))


# ---- 2: caller arrays ----
def test_caller_arrays(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    ep = np.arange(N, dtype=np.int32)
    a = e.query(desc, None, ep)
    not_empty(a)
    P.same_bytes(a, e.query(e.src(packed), None, ep))
    rng = np.random.RandomState(5)
    idx = np.concatenate([[0, 1, 63, 1, 63, 0], rng.permutation(N), rng.randint(0, N, 20)]).astype(np.int32)
    a = e.query(desc, idx, idx)
    not_empty(a)
    P.same_bytes(a, e.query(e.src(packed), idx, idx))
    # later epochs: a stored scan may find itself
    late = np.full(len(idx), N, np.int32)
    a = e.query(desc, idx, late)
    not_empty(a)
    P.same_bytes(a, e.query(e.src(packed), idx, late))


def test_source_of_one_record(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    hit = np.nonzero(ores["n_res"] > 0)[0]
    for g in hit[:4]:   # (each an odd or even row of the big arrays: here it is row 0 of its own)
        one = e.pack(desc[g:g + 1])
        ep = np.array([g, g, N], np.int32)
        a = e.query(desc[g:g + 1], [0, 0, 0], ep)
        assert a["res"]["n_res"][0] > 0
        P.same_bytes(a, e.query(e.src(one), [0, 0, 0], ep))


# ---- 3: chunk shapes ----
@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_chunk_shapes(cc, oracle, n):
    """1 and 64: zero-copy chunks (the kernel brings the epoch records and reads the selector from pinned memory); 65: the first
    size with the copies; 130: cut into 128 + 2 over the two lanes"""
    e, desc, packed, ores = world(cc, oracle)
    hit = np.nonzero(ores["n_res"] > 0)[0]
    rec = cycled(n) if n > 1 else hit[:1].astype(np.int32)
    a = e.query(desc, rec, rec)
    not_empty(a, 4 if n > 1 else 1)
    P.same_bytes(a, e.query(e.src(packed), rec, rec))
    P.same_bytes(a, e.query(e.src(), rec, rec))


@pytest.mark.parametrize("n", [40, 130])
def test_packed_and_descriptor_chunks_alternate_on_a_lane(cc, oracle, n):
    """Each lane takes a descriptor chunk with loop closures, then a packed chunk, then a descriptor chunk again: the list heads
    and pass counters the previous chunk left behind are cleared by whichever prep kernel runs next."""
    e, desc, packed, ores = world(cc, oracle)
    rec = cycled(n)
    quiet = np.zeros(n, np.int32)   # epoch 0: nothing to find -- the answers must not inherit the previous chunk's counters
    ref = e.query(desc, rec, rec)
    ref0 = e.query(desc, rec, quiet)
    not_empty(ref)
    assert not ref0["res"]["n_res"].any()
    outs = []
    for k in range(2):
        outs.append((ref, e.query(desc, rec, rec, wait=False)))
    for k in range(2):
        outs.append((ref0, e.query(e.src(packed), rec, quiet, wait=False)))
    for k in range(2):
        outs.append((ref, e.query(e.src(), rec, rec, wait=False)))
    for k in range(2):
        outs.append((ref0, e.query(desc, rec, quiet, wait=False)))
    for k in range(2):
        outs.append((ref, e.query(e.src(packed), rec, rec, wait=False)))
    e.wait()
    for want, got in outs:
        P.same_bytes(want, got)


# ---- 4: modes ----
def test_ranked_detail(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    rec = cycled(70)
    a = e.query(desc, rec, rec, ranked=16, detail=True)
    not_empty(a, 4, 2)
    P.same_bytes(a, e.query(e.src(packed), rec, rec, ranked=16, detail=True))
    P.same_bytes(a, e.query(e.src(), rec, rec, ranked=16, detail=True))
    a = e.query(desc, rec, rec, ranked=3)
    not_empty(a, 4, 2)
    P.same_bytes(a, e.query(e.src(), rec, rec, ranked=3))


def test_knn_outputs(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    rec = cycled(70)
    a = e.query(desc, rec, rec, want_knn=True)
    not_empty(a)
    assert a["knn_cnt"].any()
    P.same_bytes(a, e.query(e.src(packed), rec, rec, want_knn=True))
    P.same_bytes(a, e.query(e.src(), rec, rec, want_knn=True))


def test_dynamic_thresholds(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    e = P.PackedEmu(oracle.L, dcfg, cap=N, lanes=2, dyn=True)
    e.add(desc, ts, seeds)
    ep = np.arange(N, dtype=np.int32)
    a = e.query(desc, None, ep, ranked=16, detail=True)
    not_empty(a, 4, 2)
    P.same_bytes(a, e.query(e.src(), ep, ep, ranked=16, detail=True))
    P.same_bytes(a, e.query(e.src(e.pack(desc)), ep, ep, ranked=16, detail=True))
    e.close()


def test_large_k_database(cc, oracle):
    """nnk_ = 128: the _l instances of the chain, lanes of 256 items, hit rows of 256"""
    desc, ts, seeds, dcfg0, ores = drive(cc, oracle)
    L = oracle.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse, dcfg.nnk = dcfg0.max_elapse, dcfg0.min_elapse, 128
    e = P.PackedEmu(L, dcfg, cap=N, lanes=2)
    assert e.lib.cc_db_knn_stride(e.db) == L.KNN_MAX_LARGE
    e.add(desc, ts, seeds)
    rec = cycled(70)
    a = e.query(desc, rec, rec, want_knn=True)
    not_empty(a)
    P.same_bytes(a, e.query(e.src(), rec, rec, want_knn=True))
    P.same_bytes(a, e.query(e.src(e.pack(desc)), rec, rec, want_knn=True))
    e.close()


# ---- 5: verify ----
def verify_items(res):
    """per closed query: itself, its answer and the neighbours of both, up to 8 candidates (q is among its own candidates)"""
    qidx, cands = [], []
    for q in np.nonzero(res["n_res"] > 0)[0][:12]:
        c = int(res["cand_gidx"][q])
        lst = []
        for g in (int(q), c, c + 1, c - 1, int(q) - 1, c + 2, 3, c - 2):
            if 0 <= g < N and g not in lst:
                lst.append(g)
        qidx.append(int(q))
        cands.append(lst)
    return np.asarray(qidx, np.int32), cands


def test_verify(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    qidx, cands = verify_items(ores)
    assert len(qidx) >= 8 and max(len(c) for c in cands) == 8
    a = e.verify(desc, qidx, cands)
    not_empty(a)
    assert (a["hint_cnt"] > 0).sum() >= 4
    P.same_bytes(a, e.verify(e.src(), qidx, cands))
    P.same_bytes(a, e.verify(e.src(packed), qidx, cands))
    a = e.verify(desc, qidx, cands, ranked=8, detail=True)
    not_empty(a, 4, 2)
    P.same_bytes(a, e.verify(e.src(), qidx, cands, ranked=8, detail=True))
    a = e.verify(desc, qidx, cands, ranked=8)
    P.same_bytes(a, e.verify(e.src(packed), qidx, cands, ranked=8))
    # without a selector item i reads record i
    lists = [[(i + 1) % N, i] for i in range(10)]
    a = e.verify(desc[:10], None, lists)
    P.same_bytes(a, e.verify(e.src(), None, lists))


# ---- 6: pose ----
def pose_items(res):
    hit = np.nonzero(res["n_res"] > 0)[0][:10]
    q = np.concatenate([hit, hit[:3], [7]]).astype(np.int32)
    g = np.concatenate([res["cand_gidx"][hit], res["cand_gidx"][hit[:3]], [7]]).astype(np.int32)
    tf = np.concatenate([res["tf"][hit] + np.array([0.4, -0.3, 0.01]), res["tf"][hit[:3]], np.zeros((1, 3))])
    st = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0.01]], np.float64)
    return q, g, tf, tf[:, None, :] + st[None]


def test_pose(cc, oracle):
    e, desc, packed, ores = world(cc, oracle)
    q, g, tf, tries = pose_items(ores)
    a = e.pose(desc, q, g, tf, tries=tries, curvature=True, min_corr=float("-inf"))
    assert (a["res"]["n_pairs"] > 0).sum() >= 4 and (a["res"]["flags"] & oracle.L.PF_REFINED).sum() >= 4
    assert a["res"]["n_pairs"][-1] > 0, "a scan against itself at tf = 0"
    P.same_bytes(a, e.pose(e.src(), q, g, tf, tries=tries, curvature=True, min_corr=float("-inf")))
    P.same_bytes(a, e.pose(e.src(packed), q, g, tf, tries=tries, curvature=True, min_corr=float("-inf")))
    a = e.pose(desc, q, g, tf)
    P.same_bytes(a, e.pose(e.src(), q, g, tf))
    big = cycled(70) % len(q)
    a = e.pose(desc, q[big], g[big], tf[big], tries=tries[big])
    P.same_bytes(a, e.pose(e.src(packed), q[big], g[big], tf[big], tries=tries[big]))


# ---- 7: interleaving with appends ----
def test_stored_queries_in_flight_across_an_append(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    e = P.PackedEmu(oracle.L, dcfg, cap=N, lanes=2)
    e.add(desc[:40], ts[:40], seeds[:40])
    ep = np.arange(40, dtype=np.int32)
    fly = e.query(e.src(), ep, ep, ranked=4, wait=False)
    e.api.db_add_prepared(e.db, desc[40:], ts[40:], seeds[40:])
    e.wait()
    assert e.lib.cc_db_size(e.db) == N
    after = e.query(e.src(), ep, ep, ranked=4)
    not_empty(after, 4, 2)
    P.same_bytes(after, fly)
    P.same_bytes(after, e.query(desc, ep, ep, ranked=4))
    e.close()


# ---- 8: refusals ----
def test_refusals(cc, oracle):
    desc, ts, seeds, dcfg, ores = drive(cc, oracle)
    L = oracle.L
    e = P.PackedEmu(L, dcfg, cap=N, lanes=2)
    e.add(desc[:40], ts[:40], seeds[:40])
    packed = e.pack(desc[:40])
    off8 = e.pack(desc[:4], off=8)
    ep = np.arange(40, dtype=np.int32)
    ref = e.query(desc[:40], None, ep)
    not_empty(ref)
    fly = e.query(e.src(), ep, ep, wait=False)   # a chunk submitted before the refusals still delivers
    hot, feat = packed
    one = np.array([0], np.int32)
    vt = [[1, 2]]
    ok = e.src(packed)
    bad_src = [("one array NULL (feat)", L.PackedSrc(hot.ctypes.data, None, 40, 0)), ("one array NULL (hot)", L.PackedSrc(None, feat.ctypes.data, 40, 0)),
               ("n_rec 0", L.PackedSrc(hot.ctypes.data, feat.ctypes.data, 0, 0)), ("n_rec -3", L.PackedSrc(hot.ctypes.data, feat.ctypes.data, -3, 0)),
               ("misaligned bases", e.src(off8)), ("misaligned hot", L.PackedSrc(off8[0].ctypes.data, feat.ctypes.data, 4, 0)),
               ("misaligned feat", L.PackedSrc(hot.ctypes.data, off8[1].ctypes.data, 4, 0))]
    bad_idx = [("index -1", ok, -1), ("index n_rec", ok, 40), ("stored index == cc_db_size", e.src(), 40), ("stored index -1", e.src(), -1)]

    def refused(rc, what):
        assert rc == P.CC_EINVAL, (what, rc)
        assert e.lib.cc_last_error(), what

    for what, s in bad_src:
        refused(e.query(s, one, one, raw_rc=True), ("query", what))
        refused(e.verify(s, one, vt, raw_rc=True), ("verify", what))
        refused(e.pose(s, one, one, np.zeros((1, 3)), raw_rc=True), ("pose", what))
    for what, s, i in bad_idx:
        r = np.array([0, i], np.int32)
        refused(e.query(s, r, [1, 1], raw_rc=True), ("query", what))
        refused(e.verify(s, r, [[1], [2]], raw_rc=True), ("verify", what))
        refused(e.pose(s, r, [1, 1], np.zeros((2, 3)), raw_rc=True), ("pose", what))
    # a NULL source; without a selector query i is record i: more queries than records
    lb, ub = L.default_thresholds()
    res = np.zeros(1, L.query_result_dt)
    refused(e.lib.cc_db_query_submit_packed(e.db, None, P._p(one), 1, P._p(one), P._b(lb), P._b(ub), P._p(res), None, None, None, None, None), "NULL source")
    vcfg, tab = L.VerifyCfg(0, 10, 1000.0, 0), P.PackedEmu.table(vt)
    refused(e.lib.cc_db_verify_submit_packed(e.db, None, P._p(one), P._p(tab), 1, P._b(vcfg), P._b(lb), P._b(ub), P._p(res), None, None, None, None, None),
            "NULL source, verify")
    pcfg, items, pres = L.PoseCfg(1, 0.3, 0, 0), L.pose_items([0], [1], np.zeros((1, 3))), np.zeros(1, L.pose_result_dt)
    refused(e.lib.cc_db_pose_submit_packed(e.db, None, P._p(items), 1, P._b(pcfg), None, P._p(pres), None, None, None), "NULL source, pose")
    refused(e.query(e.src(e.pack(desc[:2])), None, [1, 1, 1], raw_rc=True), "three queries of a two-record source")
    # h_detail without rank
    det = L.rank_detail_buffer(1, 4)
    refused(e.lib.cc_db_query_submit_packed(e.db, P._b(ok), P._p(one), 1, P._p(one), P._b(lb), P._b(ub), P._p(res), None, None, None, None, P._p(det)),
            "h_detail without rank")
    refused(e.lib.cc_db_verify_submit_packed(e.db, P._b(ok), P._p(one), P._p(tab), 1, P._b(vcfg), P._b(lb), P._b(ub), P._p(res), None, None, None, None, P._p(det)),
            "h_detail without rank, verify")
    # what the descriptor form refuses: an epoch beyond the database, a candidate outside it, a non-finite pose
    refused(e.query(ok, one, [41], raw_rc=True), "epoch")
    refused(e.verify(ok, one, [[40]], raw_rc=True), "candidate")
    refused(e.pose(ok, one, one, np.array([[np.nan, 0, 0]]), raw_rc=True), "pose")
    assert not res.tobytes().strip(b"\0") and not pres.tobytes().strip(b"\0")
    e.wait()
    P.same_bytes(ref, fly)
    P.same_bytes(ref, e.query(ok, ep, ep))   # the handle is still usable
    e.close()


# ---- 9: the class mirror ----
def mirror_outcome(stdout):
    t = stdout.strip().splitlines()[-1].split()
    assert t[0] == "done", stdout[-500:]
    return dict(n=int(t[1]), closed=int(t[3]), lists=int(t[5]), verified=int(t[7]), posed=int(t[9]), bad=[int(x) for x in t[11:15]])


def test_mirror_stored_methods(cc, tmp_path):
    """ContourDB::queryStored(i, i) hands out what queryRangedKNN answered for scan i during the drive; verifyStored and
    scorePosesStored what verifyCandidates and scorePoses do on the scan's ContourManager (tests/stored_mirror_check.cpp)"""
    import os
    import subprocess

    import emu_api
    from test_mirror_read_ahead import _build, _lists
    exe = _build(tmp_path, "stored_mirror_check.cpp", "stored_mirror_check", gpu=False)
    lst, pos = _lists(cc, tmp_path, 64, 16, 450, 1.0)
    env = dict(os.environ, CC_DB_READ_AHEAD="0", CC_EVAL_AHEAD="4", CC_EVAL_INGEST_BATCH="1", **emu_api.SMALL_GRIDS)
    r = subprocess.run([exe, str(pos), str(lst)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
    o = mirror_outcome(r.stdout)
    assert o["n"] == 64 and o["closed"] >= 4 and o["lists"] >= 2 and o["verified"] == 4 and o["posed"] >= 2, o
    assert o["bad"] == [0, 0, 0, 0], o
