"""cc_db_set_dynamic_thres (the reference's DYNAMIC_THRES=1 build) on the CPU harness: the device query path and hint flow
in dynamic mode vs the dynamic CPU oracle (tests/dyn_thres_oracle.cpp), mode 0 vs the static oracle, per-submit modes."""
import numpy as np

import dyn_oracle
import emu_api
from test_dyn_thres_oracle import INT_FIELDS, short_loop_drive
from test_emu_hints import _demo_hints


def _set_dyn(api, db, on):
    return api.lib.cc_db_set_dynamic_thres(db, on)


def _same(exp, got, what):
    for f in INT_FIELDS:
        assert exp[f] == got[f], (what, f, exp[f], got[f])
    if exp["n_res"]:
        assert abs(exp["correlation"] - got["correlation"]) < 1e-6, what
        assert np.abs(exp["tf"] - got["tf"]).max() < 1e-6, what


def _emu_db(oracle, desc, ts, seeds, dcfg):
    api = emu_api.EmuApi(oracle.L)
    ctx = api.create(max_batch=8)
    db = api.db_create(ctx, dcfg, cap=len(desc))
    api.db_add(db, desc, ts, seeds)
    return api, db


def _pick(ores, dres, n):
    """queries where the two modes differ first, then loop closures, then a plain one"""
    diff = np.nonzero((ores["cand_aft_check3"] != dres["cand_aft_check3"]) | (ores["n_cand_tidy"] != dres["n_cand_tidy"]) |
                      (ores["cand_gidx"] != dres["cand_gidx"]))[0]
    hit = np.nonzero(dres["n_res"] > 0)[0]
    return np.unique(np.concatenate([diff[:3], hit[-2:], [n - 1]])).astype(np.int32), len(diff)


def test_query_path_short_loop(cc, oracle):
    desc, ts, seeds, dcfg, ores = short_loop_drive(cc, oracle)
    dres = dyn_oracle.run_sequence(desc, ts, seeds, dcfg, dyn=1)
    qs, n_diff = _pick(ores, dres, len(desc))
    assert n_diff >= 3
    api, db = _emu_db(oracle, desc, ts, seeds, dcfg)
    assert _set_dyn(api, db, 1) == 0
    got = api.db_query(db, desc[qs], qs)
    for k, qi in enumerate(qs):
        _same(dres[qi], got[k], ("dyn", int(qi)))
    # mode 0 on the same DB: the static answers again
    assert _set_dyn(api, db, 0) == 0
    got0 = api.db_query(db, desc[qs], qs)
    for k, qi in enumerate(qs):
        _same(ores[qi], got0[k], ("static", int(qi)))
    # the mode is taken per submit: two batches in flight, one of each mode, collected by one wait
    assert _set_dyn(api, db, 1) == 0
    r1, k1 = api.db_query_submit(db, desc[qs], qs)
    assert _set_dyn(api, db, 0) == 0
    r2, k2 = api.db_query_submit(db, desc[qs], qs)
    api.db_query_wait(db)
    for k, qi in enumerate(qs):
        _same(dres[qi], r1[k], ("submit dyn", int(qi)))
        _same(ores[qi], r2[k], ("submit static", int(qi)))


def test_argument_validation(oracle):
    api = emu_api.EmuApi(oracle.L)
    ctx = api.create(max_batch=2)
    db = api.db_create(ctx, cap=4)
    EINVAL = -1  # CC_EINVAL
    assert _set_dyn(api, db, 2) == EINVAL
    assert _set_dyn(api, db, -1) == EINVAL
    assert _set_dyn(api, None, 1) == EINVAL
    assert _set_dyn(api, db, 1) == 0 and _set_dyn(api, db, 0) == 0


def _variant(cc, oracle, nnk, qlv, thr, sim):
    L = oracle.L
    d = L.default_db_cfg()
    d.max_elapse, d.min_elapse = 2.5, 1.5
    d.nnk, d.n_q_levels = nnk, len(qlv)
    for i, v in enumerate(qlv):
        d.q_levels[i] = v
    for k, v in sim.items():
        setattr(d.cont_sim, k, v)
    lb, ub = L.default_thresholds()
    for k, v in thr.items():
        setattr(lb, k, v)
    w = cc.synth.World(loop_len=40.0)
    n = 64
    x, poses, ts = cc.synth.make_sequence(n, world=w, beams=16, azim=450)
    xs = x.numpy().reshape(-1, 4)
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    ores, _, desc = oracle.run_sequence(xs, offs, ts, seeds, dcfg=d, lb=lb, ub=ub, want_desc=True)
    dres = dyn_oracle.run_sequence(desc, ts, seeds, d, lb=lb, ub=ub, dyn=1)
    qs, n_diff = _pick(ores, dres, n)
    api, db = _emu_db(oracle, desc, ts, seeds, d)
    assert _set_dyn(api, db, 1) == 0
    got = api.db_query(db, desc[qs], qs, lb=lb, ub=ub)
    for k, qi in enumerate(qs):
        _same(dres[qi], got[k], int(qi))
    return n_diff


def test_variant_nnk8_two_levels(cc, oracle):
    _variant(cc, oracle, 8, (2, 3), {}, {})


def test_variant_relaxed_bars(cc, oracle):
    n_diff = _variant(cc, oracle, 64, (1, 2, 3), dict(i_ovlp_sum=2, i_ovlp_max_one=2, i_in_ang_rng=2, i_indiv_sim=2, i_orie_sim=3,
                                                     correlation=0.1, area_perc=0.01, neg_est_dist=-8.0),
                      dict(ta_cell_cnt=12.0, tp_cell_cnt=0.4, tp_eigval=0.4, ta_h_bar=0.6, ta_rcom=0.8, tp_rcom=0.5))
    assert n_diff >= 1


def test_hint_flow(cc, oracle):
    desc, ts, seeds, dcfg, ores = short_loop_drive(cc, oracle)
    L = oracle.L
    api, db = _emu_db(oracle, desc, ts, seeds, dcfg)
    assert _set_dyn(api, db, 1) == 0
    hit = np.nonzero(ores["n_res"] > 0)[0]
    n_changed = 0
    for qi in hit[:2]:
        c = int(ores["cand_gidx"][qi])
        cands = [c, max(c - 1, 0), c + 1, 3]
        hints = _demo_hints(L, desc, qi, cands)
        for seed in (None, 5):
            hs = hints if seed is None else hints[np.random.default_rng(seed).permutation(len(hints))]
            eres, esc = dyn_oracle.check_hints(desc, qi, cands, hs, dcfg.cont_sim, max_fine_opt=5, dyn=1)
            _, ssc = dyn_oracle.check_hints(desc, qi, cands, hs, dcfg.cont_sim, max_fine_opt=5, dyn=0)
            h = np.zeros(len(hs), L.hint_dt)
            h["cand_gidx"] = np.array(cands)[hs[:, 0]]
            h["level"], h["seq_src"], h["seq_tgt"] = hs[:, 1], hs[:, 2], hs[:, 3]
            res, sc = api.check_hints(db, desc[qi:qi + 1], h, max_fine_opt=5)
            got = np.stack([sc[f] for f in ("i_ovlp_sum", "i_ovlp_max_one", "i_in_ang_rng", "i_indiv_sim", "i_orie_sim", "passed")], 1)
            bad = np.nonzero((got != esc).any(1))[0]
            assert len(bad) == 0, (qi, bad[:5], got[bad[:5]], esc[bad[:5]])
            for f in INT_FIELDS:
                exp = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[int(eres[f])]
                assert exp == res[f], (qi, f, exp, res[f])
            if eres["n_res"]:
                assert abs(eres["correlation"] - res["correlation"]) < 1e-6
                assert np.abs(eres["tf"] - res["tf"]).max() < 1e-6
            n_changed += int((esc != ssc).any())
    assert n_changed > 0
