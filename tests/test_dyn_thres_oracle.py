"""The CPU oracle of the reference's DYNAMIC_THRES=1 build (tests/dyn_thres_oracle.cpp): with the switch off it is the
static oracle; with it on, an independent numpy restatement of the bar rules reproduces its per-hint scores; and the
short loop drive tells the two modes apart (so the device tests that use it can)."""
import numpy as np

import dyn_oracle
from test_emu_hints import _demo_hints

INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy",
              "n_knn_hits"]


def short_loop_drive(cc, oracle):
    """64 scans of the looping world, DB delays 2.5 / 1.5 s (test_emu_query.py's drive): descriptors, stamps, seeds, config."""
    L = oracle.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    w = cc.synth.World(loop_len=40.0)
    n = 64
    x, poses, ts = cc.synth.make_sequence(n, world=w, beams=16, azim=450)
    xs = x.numpy().reshape(-1, 4)
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(xs, offs, ts, seeds, dcfg=dcfg, want_desc=True)
    return odesc, np.asarray(ts), seeds, dcfg, ores


def _differs(a, b):
    return (a["cand_aft_check2"] != b["cand_aft_check2"]) | (a["cand_aft_check3"] != b["cand_aft_check3"]) | \
           (a["n_cand_tidy"] != b["n_cand_tidy"]) | (a["cand_gidx"] != b["cand_gidx"])


def test_static_mode_is_the_oracle(cc, oracle):
    desc, ts, seeds, dcfg, ores = short_loop_drive(cc, oracle)
    r0 = dyn_oracle.run_sequence(desc, ts, seeds, dcfg, dyn=0)
    for f in INT_FIELDS:
        assert np.array_equal(r0[f], ores[f]), f
    m = ores["n_res"] > 0
    assert np.array_equal(r0["correlation"][m], ores["correlation"][m]) and np.array_equal(r0["tf"][m], ores["tf"][m])


def test_drive_tells_the_modes_apart(cc, oracle):
    desc, ts, seeds, dcfg, ores = short_loop_drive(cc, oracle)
    r1 = dyn_oracle.run_sequence(desc, ts, seeds, dcfg, dyn=1)
    assert int(_differs(r1, ores).sum()) >= 3
    assert (r1["cand_aft_check3"] <= ores["cand_aft_check3"]).all()  # (n_cand_tidy may move either way: other proposals)


def _numpy_replay(full, lb, ub):
    """Rules 1-2 from the full per-hint scores under the initial bars: the bars, partial scores, passed flags and counts."""
    names = ("i_ovlp_sum", "i_ovlp_max_one", "i_in_ang_rng", "i_indiv_sim", "i_orie_sim")
    B = np.array([getattr(lb, f) for f in names])
    U = np.array([getattr(ub, f) for f in names])
    out = np.zeros_like(full)
    c2 = c3 = 0
    for i, (s0, s1, s2, s3, s4, _) in enumerate(full):
        anchor = s0 > 0 or s1 > 0  # (a hint that fails the anchor test returns all zeros)
        pc = s0 >= B[0] and s1 >= B[1]
        st2 = pc and s2 >= B[2]
        p3 = st2 and s3 >= B[3] and s4 >= B[4]
        out[i] = (s0, s1, s2 if pc else 0, s3 if st2 else 0, s4 if st2 and s3 >= B[3] else 0, int(p3))
        c2 += int(anchor and st2)
        c3 += int(p3)
        if p3:
            B = np.minimum(np.maximum(B, s4), U)
    return out, c2, c3


def test_numpy_restatement_of_the_check_bars(cc, oracle):
    desc, ts, seeds, dcfg, ores = short_loop_drive(cc, oracle)
    L = oracle.L
    lb, ub = L.default_thresholds()
    hit = np.nonzero(ores["n_res"] > 0)[0]
    n_raised = 0
    for qi in hit[:3]:
        c = int(ores["cand_gidx"][qi])
        cands = [c, max(c - 1, 0), c + 1, 3]
        hints = _demo_hints(L, desc, qi, cands)
        for seed in (None, 1, 2):
            h = hints if seed is None else hints[np.random.default_rng(seed).permutation(len(hints))]
            _, full = dyn_oracle.check_hints(desc, qi, cands, h, dcfg.cont_sim, dyn=0)
            res, got = dyn_oracle.check_hints(desc, qi, cands, h, dcfg.cont_sim, dyn=1)
            exp, c2, c3 = _numpy_replay(full, lb, ub)
            assert np.array_equal(got, exp), (qi, seed)
            assert (res["cand_aft_check2"], res["cand_aft_check3"]) == (c2, c3)
            n_raised += int((got != full).any())
    assert n_raised > 0, "no hint order where the raised bars changed a score"
