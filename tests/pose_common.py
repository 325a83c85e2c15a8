"""TEST INFRASTRUCTURE shared by test_emu_pose.py / test_gpu_pose.py: the checks of the caller-given-pose entry points
(cc_db_pose_submit / cc_db_pose_batch / cc_db_pose_batch_host) against the CPU oracle, written once over a small back-end
interface (the CPU harness through ctypes, the MI355X through the Python package).

Reference values, src = the database scan's descriptor, tgt = the query's:
  oracle.gmm(src, tgt, tf_init)         -> corr_init, corr_opt, tf_opt, (iterations, termination, n_eval)
  oracle.gmm_eval(src, tgt, tf_init, p) -> cost, gradient, (ac_src, ac_tgt) at p over the pair set of tf_init

Bars:
  TOL (1e-6, ranked_common)   corr_init, correlation, tf against the oracle: what the hint, verify and ranked tests use
  TRY_BAR 1e-10               try_corr against -cost / sqrt(ac_src ac_tgt): both sides are f64 sums of <~ 2 000 terms of <~ 1e-2 after
                              normalisation; reassociation moves them by ~1e-13, a dropped or repeated pair by >= 1e-6
  INIT_BAR 1e-12              the try at T_init against corr_init (not bit for bit: cc_k_gmm_init sums over 16 or 64 lanes by chunk)
  SAME_BAR 1e-9               the same problem through another chunk composition or another flow (pose against verify)
  the curvature bars of ranked_detail_common.check_entry

cc_ranked_cand_t.correlation is the f32 rounding of the refined correlation (fineOptimize keeps correlation_ as a float), a pose
row's correlation is the f64 value: agree() compares the f64 value with the nearest f64 that rounds to the entry's f32."""
import ctypes as C
import os

import numpy as np

import ranked_detail_common as RD
from ranked_common import TOL

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [(0, 1), (0, 2), (1, 0), (3, 4), (3, 5), (4, 3)]   # (query descriptor, database scan) on the seven recorded scans
TRY_BAR, INIT_BAR, SAME_BAR = 1e-10, 1e-12, 1e-9
WRAP_BAR = 1e-14   # atan2(sin t, cos t) on the device against numpy's: a few ulp of pi
EINVAL = -1
NINF = float("-inf")
CLASS_NAMES = ("0", "1..96", "97..256", "257..1280", "> 1280")


def fixture_desc(L):
    fx = np.load(os.path.join(HERE, "golden", "ranked_detail_scans.npz"))["desc"]
    return np.frombuffer(fx.tobytes(), L.scan_desc_dt).copy()


def pair_class(n):
    n = int(n)
    return 0 if n == 0 else 1 if n <= 96 else 2 if n <= 256 else 3 if n <= 1280 else 4


def wrap(a):
    return np.arctan2(np.sin(a), np.cos(a))


def tf_diff(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    d[..., 2] = wrap(d[..., 2])
    return np.abs(d)


def f32_gap(x64, x32):
    """distance from x64 to the f64 interval that rounds to the f32 value x32 (0 inside it)"""
    x32 = np.float32(x32)
    half = 0.5 * float(np.spacing(x32))
    return max(0.0, abs(float(x64) - float(x32)) - half)


class Back:
    """what a back end provides: L, desc [7] (numpy), verify_d, pose, query, query_submit, wait, raw, last_error"""


def scans(oracle, B, i):
    return RD.scan_of(oracle, B.desc, i, "pose-fixture")


def verify_entries(B):
    """every entry of verify(..., ranked=8, detail=True) over PAIRS: list of (q, entry, detail); cached on the back end"""
    if not hasattr(B, "_ventries"):
        qidx = sorted(set(q for q, _ in PAIRS))
        lists = [[g for q2, g in PAIRS if q2 == q] for q in qidx]
        res, c, n, det = B.verify_d(lists, qidx, 8)
        out = []
        for i, q in enumerate(qidx):
            for k in range(int(n[i])):
                out.append((q, c[i][k].copy(), det[i][k].copy()))
        B._ventries = out
    return B._ventries


def start_items(B):
    """The item set of tests 1-3 and 5 (cached): per pair the verify flow's tf_init; that pose shifted by (+-0.5 px, +-0.5 px,
    +-0.01 rad); poses pushed away along x until the pair count has fallen through every class (found with refine = 0 calls over
    a ladder of 4 px steps on the two pairs with the longest lists); a pose 1e4 px away (no pairs); and item 0 once more."""
    if hasattr(B, "_items"):
        return B._items
    L = B.L
    tf0 = {}
    for q, e, d in verify_entries(B):
        tf0.setdefault((q, int(e["cand_gidx"])), np.array(d["tf_init"], np.float64))
    missing = [p for p in PAIRS if p not in tf0]
    assert not missing, ("the verify flow lists no entry for", missing)
    rows, kind = [], []
    for p in PAIRS:
        rows.append((p[0], p[1], tf0[p]))
        kind.append("verify")
    signs = [(1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1), (1, 1, -1), (-1, -1, 1)]
    for p, s in zip(PAIRS, signs):
        rows.append((p[0], p[1], tf0[p] + np.array(s) * np.array([0.5, 0.5, 0.01])))
        kind.append("shifted")
    seen = set()
    for p in (PAIRS[0], PAIRS[3]):
        dx = np.arange(1, 31) * 4.0
        lad = [(p[0], p[1], tf0[p] + np.array([x, 0.0, 0.0])) for x in dx]
        r, _, _ = B.pose(L.pose_items(*zip(*lad)), refine=0, min_corr=NINF)
        npairs = r["n_pairs"]
        print("ladder", p, "n_pairs", npairs.tolist())
        for j in range(len(lad)):
            c = pair_class(npairs[j])
            if c and (p, c) not in seen:   # the first step of this pair in each class it passes through
                seen.add((p, c))
                rows.append(lad[j])
                kind.append("ladder")
    rows.append((PAIRS[0][0], PAIRS[0][1], tf0[PAIRS[0]] + np.array([1e4, 0.0, 0.0])))
    kind.append("far")
    rows.append(rows[0])
    kind.append("repeat")
    B._items = (L.pose_items(*zip(*rows)), kind)
    return B._items


def refined_run(B):
    """run A (cached): every item that has pairs refined (min_corr = -inf), with curvature"""
    if not hasattr(B, "_runA"):
        items, _ = start_items(B)
        B._runA = B.pose(items, refine=1, min_corr=NINF, curv=True)
    return B._runA


def oracle_runs(oracle, B):
    if not hasattr(B, "_oracle"):
        items, _ = start_items(B)
        B._oracle = [oracle.gmm(scans(oracle, B, it["gidx"]), scans(oracle, B, it["q"]), it["tf"]) for it in items]
    return B._oracle


# ---- test 1 -------------------------------------------------------------------------------------------------------------
def check_against_oracle(B, oracle):
    items, kind = start_items(B)
    res, _, _ = refined_run(B)
    refs = oracle_runs(oracle, B)
    classes = sorted(set(pair_class(n) for n in res["n_pairs"]))
    print("n_pairs", res["n_pairs"].tolist(), "classes", [CLASS_NAMES[c] for c in classes])
    assert classes == [0, 1, 2, 3, 4], ("the items do not cover the five pair-count classes", res["n_pairs"].tolist())
    mx = {"corr_init": 0.0, "corr": 0.0, "tf": 0.0}
    n_ls_fail = n_full = 0
    for i, (it, r, (ci, co, tf, st)) in enumerate(zip(items, res, refs)):
        what = (i, kind[i], int(it["q"]), int(it["gidx"]), int(r["n_pairs"]))
        mx["corr_init"] = max(mx["corr_init"], abs(ci - r["corr_init"]))
        assert abs(ci - r["corr_init"]) < TOL, (what, ci, r["corr_init"])
        refined = bool(r["flags"] & B.L.PF_REFINED)
        assert refined == (r["n_pairs"] > 0), what
        if not refined:
            assert r["correlation"].tobytes() == r["corr_init"].tobytes() and r["iterations"] == 0 and r["termination"] == 0, what
            assert tf_diff(r["tf"], it["tf"]).max() <= WRAP_BAR, what
            continue
        assert r["correlation"] >= r["corr_init"] - 1e-12, (what, r["correlation"], r["corr_init"])
        if int(st[1]) < 0:   # the oracle's own line search fails from this start: corr_init only
            n_ls_fail += 1
            print("line search fails in the oracle:", what, "oracle", st.tolist(), "device", int(r["iterations"]), int(r["termination"]))
            continue
        n_full += 1
        mx["corr"] = max(mx["corr"], abs(co - r["correlation"]))
        mx["tf"] = max(mx["tf"], float(tf_diff(tf, r["tf"]).max()))
        assert abs(co - r["correlation"]) < TOL, (what, co, r["correlation"])
        assert tf_diff(tf, r["tf"]).max() < TOL, (what, tf, r["tf"])
        assert (int(st[0]), int(st[1])) == (int(r["iterations"]), int(r["termination"])), (what, st, r["iterations"], r["termination"])
    print("test 1: %d items, %d compared in full, %d starts from which the oracle's line search fails; max |corr_init| %.2e |corr| %.2e |tf| %.2e"
          % (len(items), n_full, n_ls_fail, mx["corr_init"], mx["corr"], mx["tf"]))
    assert n_full >= 12


# ---- test 2 -------------------------------------------------------------------------------------------------------------
def try_poses(B):
    """[n, 8, 3]: T_init, the refined pose of test 1, a +-1 px / +-0.01 rad stencil around it"""
    items, _ = start_items(B)
    res, _, _ = refined_run(B)
    st = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.01], [0, 0, -0.01]], np.float64)
    t = np.zeros((len(items), 8, 3))
    t[:, 0] = items["tf"]
    t[:, 1] = res["tf"]
    t[:, 2:] = res["tf"][:, None, :] + st[None]
    return t


def check_tries(B, oracle):
    items, kind = start_items(B)
    t8 = try_poses(B)
    mx = {"try": 0.0, "init": 0.0}
    r8, c8, _ = B.pose(items, refine=1, min_corr=NINF, tries=t8)
    r0, c0, v0 = B.pose(items, refine=0, min_corr=NINF, tries=t8, curv=True)
    B._run0 = (r0, c0, v0)
    assert c8.tobytes() == c0.tobytes(), "the try values depend on whether the items were refined"
    outs = {8: c8}
    for nt in (1, 3):
        _, outs[nt], _ = B.pose(items, refine=0, min_corr=NINF, tries=np.ascontiguousarray(t8[:, :nt]))
        assert outs[nt].shape == (len(items), nt)
    for i, it in enumerate(items):
        src, tgt = scans(oracle, B, it["gidx"]), scans(oracle, B, it["q"])
        ref = []
        for t in range(8):
            cost, _, ac = oracle.gmm_eval(src, tgt, it["tf"], t8[i, t])
            ref.append(-cost / np.sqrt(ac[0] * ac[1]))
        for nt, c in outs.items():
            for t in range(nt):
                if r0[i]["n_pairs"] == 0:
                    assert c[i, t] == 0.0, (i, nt, t, c[i, t])
                    continue
                mx["try"] = max(mx["try"], abs(c[i, t] - ref[t]))
                assert abs(c[i, t] - ref[t]) < TRY_BAR, (i, kind[i], nt, t, c[i, t], ref[t])
            mx["init"] = max(mx["init"], abs(c[i, 0] - r0[i]["corr_init"]))
            assert abs(c[i, 0] - r0[i]["corr_init"]) < INIT_BAR, (i, nt, c[i, 0], r0[i]["corr_init"])
    print("test 2: %d items x (1, 3, 8) tries; max |try - oracle| %.2e, max |try(T_init) - corr_init| %.2e" % (len(items), mx["try"], mx["init"]))


# ---- test 3 -------------------------------------------------------------------------------------------------------------
def as_detail(it, r, cv):
    """(entry dict, cc_ranked_detail_t-shaped dict) of a pose row, as ranked_detail_common.check_entry reads them"""
    e = {"cand_gidx": int(it["gidx"]), "correlation": float(r["correlation"]), "tf": np.array(r["tf"])}
    d = {"tf_init": np.array(it["tf"]), "corr_init": float(r["corr_init"]), "iterations": int(r["iterations"]), "termination": int(r["termination"]),
         "n_pairs": int(r["n_pairs"]), "hess": np.array(cv["hess"]), "grad": np.array(cv["grad"])}
    return e, d


def check_curv_only(oracle, src, tgt, tf_init, p, cv, what, stats):
    """check_entry's curvature comparisons (its bars, its reference) at a pose the refinement did not produce"""
    _, g0, ac = oracle.gmm_eval(src, tgt, tf_init, p)
    nrm = np.sqrt(ac[0] * ac[1])
    G = lambda x: oracle.gmm_eval(src, tgt, tf_init, x)[1] / nrm  # noqa: E731
    H = RD.mat(cv["hess"])
    gerr = np.abs(g0 / nrm - cv["grad"]) / np.sqrt(np.abs(np.diag(H)))
    H2 = RD.ref_hessian(G, p, RD.STEPS / 2)
    agree = RD.scaled(RD.ref_hessian(G, p, RD.STEPS) - H2, H2)
    herr = RD.scaled(H - H2, H2)
    stats["grad"].append(float(gerr.max()))
    stats["ref_agree"].append(agree)
    stats["hess"].append(herr)
    print("%s: grad %.2e (x sqrt Hkk) ref-agree %.2e hess %.2e" % (what, gerr.max(), agree, herr))
    assert (gerr < RD.GRAD_BAR).all(), (what, "grad", g0 / nrm, cv["grad"], gerr)
    assert agree < RD.REF_AGREE, (what, agree)
    assert herr < RD.HESS_BAR, (what, "hess", H, H2, herr)


def check_curvature(B, oracle):
    items, kind = start_items(B)
    res, _, cv = refined_run(B)
    refs = oracle_runs(oracle, B)
    st = RD.new_stats()
    done = set()
    for i, it in enumerate(items):   # refined items of the three list classes (16-lane, in between, long), verify starts first
        c = min(pair_class(res[i]["n_pairs"]), 3)
        if c == 0 or c in done or int(refs[i][3][1]) < 0 or kind[i] == "repeat":
            continue
        done.add(c)
        e, d = as_detail(it, res[i], cv[i])
        RD.check_entry(oracle, scans(oracle, B, it["gidx"]), scans(oracle, B, it["q"]), e, d, ("pose", i, kind[i]), st)
    assert done == {1, 2, 3}, done
    # an item that was not refined: curvature at T_init
    if not hasattr(B, "_run0"):
        B._run0 = B.pose(items, refine=0, min_corr=NINF, tries=try_poses(B), curv=True)
    r0, _, v0 = B._run0
    assert not (r0["flags"] & B.L.PF_REFINED).any()
    for i in (1, 9):
        it = items[i]
        assert r0[i]["n_pairs"] > 0
        check_curv_only(oracle, scans(oracle, B, it["gidx"]), scans(oracle, B, it["q"]), it["tf"], np.array(it["tf"]), v0[i], ("unrefined", i), st)
    far = kind.index("far")
    assert not cv[far]["hess"].any() and not cv[far]["grad"].any() and not v0[far]["hess"].any(), "a problem without pairs: zeros"
    st["corr_init"] = st["corr_init"] or [0.0]
    st["corr"] = st["corr"] or [0.0]
    st["tf"] = st["tf"] or [0.0]
    RD.report(st, "test 3")


# ---- test 4 -------------------------------------------------------------------------------------------------------------
def agree(B, it_q, e, d, r, cv, what, mx):
    """a pose row against a ranked entry and its detail row of the same problem"""
    mx["corr"] = max(mx["corr"], f32_gap(r["correlation"], e["correlation"]))
    mx["tf"] = max(mx["tf"], float(tf_diff(r["tf"], e["tf"]).max()))
    mx["corr_init"] = max(mx["corr_init"], abs(r["corr_init"] - d["corr_init"]))
    assert r["flags"] & B.L.PF_REFINED, what
    assert f32_gap(r["correlation"], e["correlation"]) <= SAME_BAR, (what, r["correlation"], e["correlation"])
    assert tf_diff(r["tf"], e["tf"]).max() <= SAME_BAR, (what, r["tf"], e["tf"])
    assert abs(r["corr_init"] - d["corr_init"]) <= INIT_BAR, (what, r["corr_init"], d["corr_init"])
    assert (int(r["n_pairs"]), int(r["iterations"]), int(r["termination"])) == (int(d["n_pairs"]), int(d["iterations"]), int(d["termination"])), (what, r, d)
    assert (int(r["flags"]) & ~B.L.PF_REFINED) == int(e["flags"]), what
    H = RD.mat(d["hess"])
    herr = RD.scaled(RD.mat(cv["hess"]) - H, H)
    mx["hess"] = max(mx["hess"], herr)
    assert herr <= SAME_BAR, (what, cv["hess"], d["hess"], herr)


def check_agreement(B, oracle):
    ents = verify_entries(B)
    items = B.L.pose_items([q for q, _, _ in ents], [int(e["cand_gidx"]) for _, e, _ in ents], [d["tf_init"] for _, _, d in ents])
    res, _, cv = B.pose(items, refine=1, min_corr=NINF, curv=True)
    mx = {"corr": 0.0, "tf": 0.0, "corr_init": 0.0, "hess": 0.0}
    for i, (q, e, d) in enumerate(ents):
        agree(B, q, e, d, res[i], cv[i], ("verify entry", i, q, int(e["cand_gidx"])), mx)
    print("test 4: %d entries; max |corr| %.2e (beyond the f32 rounding of the entry) |tf| %.2e |corr_init| %.2e hess %.2e (scaled)"
          % (len(ents), mx["corr"], mx["tf"], mx["corr_init"], mx["hess"]))
    assert len(ents) >= len(PAIRS)


# ---- test 5 -------------------------------------------------------------------------------------------------------------
def rows_close(a, b, what, bar=SAME_BAR):
    for f in ("n_pairs", "iterations", "termination", "flags"):
        assert np.array_equal(a[f], b[f]), (what, f, a[f], b[f])
    for f in ("corr_init", "correlation"):
        assert np.abs(a[f] - b[f]).max() <= bar, (what, f)
    assert tf_diff(a["tf"], b["tf"]).max() <= bar, what


def check_gating(B, oracle):
    L = B.L
    items, kind = start_items(B)
    resA, _, _ = refined_run(B)
    # refine = 0
    r0, _, _ = B.pose(items, refine=0, min_corr=NINF)
    assert r0["correlation"].tobytes() == r0["corr_init"].tobytes() and not (r0["flags"] & L.PF_REFINED).any()
    assert not r0["iterations"].any() and not r0["termination"].any()
    assert np.array_equal(r0["tf"][:, :2], items["tf"][:, :2]) and np.abs(r0["tf"][:, 2] - wrap(items["tf"][:, 2])).max() <= WRAP_BAR
    assert np.abs(r0["corr_init"] - resA["corr_init"]).max() <= INIT_BAR
    # min_corr = 0.3
    r3, _, _ = B.pose(items, refine=1, min_corr=0.3)
    want = (r3["corr_init"].astype(np.float32) >= np.float32(0.3)) & (r3["n_pairs"] > 0)
    got = (r3["flags"] & L.PF_REFINED) != 0
    assert np.array_equal(want, got), (r3["corr_init"], got)
    assert want.any() and not want.all(), "the bar should separate the items"
    rows_close(r3[want], resA[want], "min_corr 0.3: the refined rows")
    nr = r3[~want]
    assert nr["correlation"].tobytes() == nr["corr_init"].tobytes() and not nr["iterations"].any()
    # the shipped default through the submit form
    rs, _, _ = B.pose(items, refine=1, min_corr=0.3, submit=True)
    assert rs.tobytes() == r3.tobytes(), "submit + wait against the synchronous call"
    # items sharing one descriptor / repeating a pair
    rep = kind.index("repeat")
    assert resA[rep].tobytes() == resA[0].tobytes()
    # 70 items (above the zero-copy limit) against the same content as 3 items
    cheap = [i for i in np.argsort(resA["n_pairs"]) if resA[i]["n_pairs"] > 0][:2] + [kind.index("far")]
    t3 = items[cheap]
    tries = try_poses(B)[cheap][:, :2]
    a, ta, ca = B.pose(t3, refine=1, min_corr=NINF, tries=tries, curv=True)
    big = np.arange(70) % 3
    b, tb, cb = B.pose(t3[big], refine=1, min_corr=NINF, tries=np.ascontiguousarray(tries[big]), curv=True)
    rows_close(b, a[big], "70 items against 3")
    assert np.abs(tb - ta[big]).max() <= SAME_BAR
    for f in ("hess", "grad"):
        assert np.allclose(cb[f], ca[f][big], rtol=1e-9, atol=1e-12), f
    # pose chunks interleaved with a query chunk in flight
    qs = np.arange(len(B.desc), dtype=np.int32)
    alone = B.query(qs)
    pend = B.query_submit(qs)
    rp, _, _ = B.pose(t3, refine=1, min_corr=NINF, submit="no-wait")
    B.wait()
    assert pend.tobytes() == alone.tobytes(), "a pose chunk disturbed a query chunk in flight"
    rows_close(rp, a, "pose rows behind a query chunk")


# ---- test 6 -------------------------------------------------------------------------------------------------------------
def check_refusals(B, kinds):
    """every refusal returns CC_EINVAL with a message, writes nothing and leaves a query chunk in flight collectable"""
    L = B.L
    items, _ = start_items(B)
    it = items[:2].copy()
    n_desc, size = len(B.desc), len(B.desc)
    good_cfg = L.PoseCfg(1, 0.3, 0, 0)
    tr = np.zeros((2, 1, 3))
    qs = np.arange(n_desc, dtype=np.int32)
    alone = B.query(qs)
    pend = B.query_submit(qs)

    def bad(field, i, v):
        x = it.copy()
        if field == "tf":
            x["tf"][i[0], i[1]] = v
        else:
            x[field][i] = v
        return x

    badtr = tr.copy()
    badtr[1, 0, 2] = np.inf
    cases = [
        ("db NULL", dict(db=False)), ("qdesc NULL", dict(qdesc=False)), ("items NULL", dict(items=None)), ("cfg NULL", dict(cfg=None)),
        ("res NULL", dict(res=False)), ("n < 0", dict(n=-1)),
        ("q < 0", dict(items=bad("q", 1, -1))), ("q >= n_desc", dict(items=bad("q", 0, n_desc))),
        ("gidx < 0", dict(items=bad("gidx", 0, -1))), ("gidx >= size", dict(items=bad("gidx", 1, size))),
        ("tf NaN", dict(items=bad("tf", (0, 0), np.nan))), ("tf inf", dict(items=bad("tf", (1, 2), np.inf))), ("tf -inf", dict(items=bad("tf", (1, 1), -np.inf))),
        ("try inf", dict(cfg=L.PoseCfg(1, 0.3, 1, 0), tries=badtr, tc=True)),
        ("refine 2", dict(cfg=L.PoseCfg(2, 0.3, 0, 0))), ("refine -1", dict(cfg=L.PoseCfg(-1, 0.3, 0, 0))),
        ("min_corr NaN", dict(cfg=L.PoseCfg(1, float("nan"), 0, 0))),
        ("n_try -1", dict(cfg=L.PoseCfg(1, 0.3, -1, 0))), ("n_try 9", dict(cfg=L.PoseCfg(1, 0.3, L.POSE_TRY_MAX + 1, 0), tries=np.zeros((2, 9, 3)), tc=True)),
        ("h_try NULL", dict(cfg=L.PoseCfg(1, 0.3, 1, 0), tries=None, tc=True)), ("h_try_corr NULL", dict(cfg=L.PoseCfg(1, 0.3, 1, 0), tries=tr, tc=False)),
    ]
    for fn in kinds:
        for name, kw in cases:
            args = dict(db=True, qdesc=True, items=it, n=2, cfg=good_cfg, tries=None, res=True, tc=False)
            args.update(kw)
            rc, res, tc = B.raw(fn, **args)
            assert rc == EINVAL, (fn, name, rc)
            assert B.last_error(), (fn, name)
            assert not res.tobytes().strip(b"\0") and not tc.tobytes().strip(b"\0"), (fn, name, "a refused call wrote an answer")
        rc, _, _ = B.raw(fn, db=True, qdesc=True, items=it, n=0, cfg=good_cfg, tries=None, res=True, tc=False)
        assert rc == 0, (fn, "n == 0 is CC_OK", rc)
    B.wait()
    assert pend.tobytes() == alone.tobytes(), "the query chunk submitted before the refusals"
    r, _, _ = B.pose(it, refine=1, min_corr=NINF)
    rows_close(r, refined_run(B)[0][:2], "the handle after the refusals")


def check_abi(cc):
    """sizes and offsets of the four records against the compiled header"""
    import subprocess
    import tempfile
    L = cc.L
    root = os.path.dirname(HERE)
    fields = [("cc_pose_item_t", L.pose_item_dt, ("q", "gidx", "tf")),
              ("cc_pose_result_t", L.pose_result_dt, ("corr_init", "correlation", "tf", "n_pairs", "iterations", "termination", "flags", "pad_")),
              ("cc_pose_curv_t", L.pose_curv_dt, ("hess", "grad"))]
    exprs = []
    for t, _, fs in fields:
        exprs += ["sizeof(%s)" % t] + ["offsetof(%s, %s)" % (t, f) for f in fs]
    exprs += ["sizeof(cc_pose_cfg_t)", "offsetof(cc_pose_cfg_t, refine)", "offsetof(cc_pose_cfg_t, min_corr)", "offsetof(cc_pose_cfg_t, n_try)",
              "(size_t)CC_POSE_TRY_MAX", "(size_t)CC_PF_REFINED"]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "cont2_amd.h"\nint main(void) { printf("' + "%zu " * len(exprs) + '\\n", ' + ", ".join(exprs) +
           "); return 0; }\n")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(td, "t")]).split()]
    want = []
    for _, dt, fs in fields:
        want += [dt.itemsize] + [dt.fields[f][1] for f in fs]
    want += [C.sizeof(L.PoseCfg), L.PoseCfg.refine.offset, L.PoseCfg.min_corr.offset, L.PoseCfg.n_try.offset, L.POSE_TRY_MAX, L.PF_REFINED]
    assert got == want, (got, want)
    assert (L.pose_item_dt.itemsize, L.pose_result_dt.itemsize, L.pose_curv_dt.itemsize, C.sizeof(L.PoseCfg)) == (32, 64, 72, 16)
