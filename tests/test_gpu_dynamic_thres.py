"""cc_db_set_dynamic_thres (the reference's DYNAMIC_THRES=1 build) on the MI355X vs the dynamic CPU oracle
(tests/dyn_thres_oracle.cpp) replaying the driver loop from the device's own descriptors: every integer of every query
result equal, correlation and pose within 1e-4."""
import numpy as np
import pytest

import dyn_oracle
from test_dyn_thres_oracle import INT_FIELDS

pytestmark = pytest.mark.gpu


def _compare(exp, got, what):
    bad = []
    for i in range(len(exp)):
        for f in INT_FIELDS:
            if exp[f][i] != got[f][i]:
                bad.append("%s query %d: %s oracle=%d got=%d" % (what, i, f, exp[f][i], got[f][i]))
        if exp["n_res"][i]:
            if abs(exp["correlation"][i] - got["correlation"][i]) > 1e-4 or np.abs(exp["tf"][i] - got["tf"][i]).max() > 1e-4:
                bad.append("%s query %d: correlation / pose %g %s vs %g %s" % (what, i, exp["correlation"][i], exp["tf"][i],
                                                                              got["correlation"][i], got["tf"][i]))
    assert not bad, "%d mismatches\n" % len(bad) + "\n".join(bad[:40])


def _drive(cc, oracle, xyzi, ts, dcfg=None, min_diff=1):
    import torch
    L = oracle.L
    dcfg = dcfg or L.default_db_cfg()
    n, P = xyzi.shape[0], xyzi.shape[1]
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=128)
    desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
    db = cc.Database(ctx, dcfg, capacity=n + 8)
    db.add_scans(desc, ts, seeds)
    db.set_dynamic_thres(True)
    res = db.query(desc, seeds)
    db.set_dynamic_thres(False)
    res0 = db.query(desc, seeds)
    torch.cuda.synchronize()
    d = cc.desc_to_numpy(desc)
    exp = dyn_oracle.run_sequence(d, np.asarray(ts), seeds, dcfg, dyn=1)
    exp0 = dyn_oracle.run_sequence(d, np.asarray(ts), seeds, dcfg, dyn=0)
    _compare(exp, res, "dynamic")
    _compare(exp0, res0, "static")
    n_diff = int(((exp["cand_aft_check3"] != exp0["cand_aft_check3"]) | (exp["n_cand_tidy"] != exp0["n_cand_tidy"]) |
                  (exp["cand_gidx"] != exp0["cand_gidx"])).sum())
    print("%d queries, %d loop closures (static %d), %d differ between the modes" % (n, int((res["n_res"] > 0).sum()),
                                                                                   int((res0["n_res"] > 0).sum()), n_diff))
    assert n_diff >= min_diff
    db.close()
    ctx.close()
    return exp, res


def test_loop_sequence(cc, oracle):
    w = cc.synth.World(loop_len=200.0)
    xyzi, poses, ts = cc.synth.make_sequence(300, world=w, device="cuda")
    _drive(cc, oracle, xyzi, ts, min_diff=3)


def test_kitti_shaped(cc, oracle):
    w = cc.synth.World(kitti=True)
    idx = np.concatenate([np.arange(1484, 1584), np.arange(2667, 2787)])
    xyzi, poses, ts = cc.synth.make_sequence(0, world=w, device="cuda", indices=idx)
    _drive(cc, oracle, xyzi, ts)


def test_dense_world(cc, oracle):
    w = cc.synth.World(dense=True, loop_len=150.0)
    xyzi, poses, ts = cc.synth.make_sequence(330, world=w, device="cuda")  # (the loop closes after ~150 scans)
    _drive(cc, oracle, xyzi, ts)


def test_online_loop_four_lanes(cc, oracle):
    """cc_db_add_scans_prepare -> cc_db_add_scans -> cc_db_query_submit per sub-batch, four lanes, dynamic mode."""
    import torch
    L = oracle.L
    w = cc.synth.World(loop_len=200.0)
    n = 256
    xyzi, poses, ts = cc.synth.make_sequence(n, world=w, device="cuda")
    P = xyzi.shape[1]
    offs = np.arange(n + 1, dtype=np.int64) * P
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=128)
    desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
    db = cc.Database(ctx, capacity=n + 8)
    db.set_lanes(4)
    db.set_dynamic_thres(True)
    outs = []
    for b0 in range(0, n, 32):
        sub = desc[b0:b0 + 32].contiguous()
        db.add_scans_prepare(sub)
        db.add_scans(sub, ts[b0:b0 + 32], seeds[b0:b0 + 32])
        outs.append(db.query_submit(sub, seeds[b0:b0 + 32]))
    db.query_wait()
    torch.cuda.synchronize()
    res = np.concatenate(outs)
    exp = dyn_oracle.run_sequence(cc.desc_to_numpy(desc), np.asarray(ts), seeds, L.default_db_cfg(), dyn=1)
    # a query of a sub-batch sees its own epoch (seeds = epochs): the sub-batch's own scans are not yet searchable
    _compare(exp, res, "online")
    db.close()
    ctx.close()


def test_hint_flow(cc, oracle):
    import torch
    from test_emu_hints import _demo_hints
    L = oracle.L
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5
    w = cc.synth.World(loop_len=40.0)
    n = 64
    xyzi, poses, ts = cc.synth.make_sequence(n, world=w, device="cuda", beams=16, azim=450)
    offs = np.arange(n + 1, dtype=np.int64) * xyzi.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=n)
    desc = ctx.ingest(xyzi.reshape(-1, 4), offs)
    db = cc.Database(ctx, dcfg, capacity=n)
    db.add_scans(desc, ts, seeds)
    db.set_dynamic_thres(True)
    d = cc.desc_to_numpy(desc)
    exp = dyn_oracle.run_sequence(d, np.asarray(ts), seeds, dcfg, dyn=1)
    hit = np.nonzero(exp["n_res"] > 0)[0]
    assert len(hit) >= 2
    for qi in hit[:2]:
        c = int(exp["cand_gidx"][qi])
        cands = [c, max(c - 1, 0), c + 1, 3]
        hints = _demo_hints(L, d, qi, cands)
        hs = hints[np.random.default_rng(3).permutation(len(hints))]
        eres, esc = dyn_oracle.check_hints(d, qi, cands, hs, dcfg.cont_sim, max_fine_opt=5, dyn=1)
        h = np.zeros(len(hs), L.hint_dt)
        h["cand_gidx"] = np.array(cands)[hs[:, 0]]
        h["level"], h["seq_src"], h["seq_tgt"] = hs[:, 1], hs[:, 2], hs[:, 3]
        res, sc = db.check_hints(desc[qi:qi + 1].contiguous(), h, max_fine_opt=5)
        torch.cuda.synchronize()
        got = np.stack([sc[f] for f in ("i_ovlp_sum", "i_ovlp_max_one", "i_in_ang_rng", "i_indiv_sim", "i_orie_sim", "passed")], 1)
        assert np.array_equal(got, esc), qi
        for f in INT_FIELDS:
            e = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[int(eres[f])]
            assert e == res[f], (qi, f, e, res[f])
        if eres["n_res"]:
            assert abs(eres["correlation"] - res["correlation"]) < 1e-4 and np.abs(eres["tf"] - res["tf"]).max() < 1e-4
    db.close()
    ctx.close()


def _compare_outcome():
    import importlib.util
    import os
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "contour-context_amd", "tools", "compare_outcome.py")
    spec = importlib.util.spec_from_file_location("cc_compare_outcome", p)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_online_replay_4096_kitti_outcome(cc, oracle, tmp_path):
    """A 4 096-scan online replay of the KITTI-shaped drive in dynamic mode (sub-batches of 256: ingest -> cc_db_add_scans ->
    cc_db_query_submit at each scan's own epoch, nothing collected in between): every result against the dynamic oracle's
    replay of the driver loop on the device's descriptors, and the two outcome files row by row (tools/compare_outcome.py,
    max-F1 / arg-max / TP count included)."""
    import torch
    from test_gpu_query import _outcome_and_pr, _write_eval_files
    L = oracle.L
    n, sub = 4096, 256
    w = cc.synth.World(kitti=True)
    ctx = cc.Context(0, max_batch=sub)
    db = cc.Database(ctx, capacity=n)
    db.set_dynamic_thres(True)
    parts, descs, poses, ts_all = [], [], [], []
    for k in range(n // sub):
        x, p, ts = cc.synth.make_sequence(sub, world=w, device="cuda", start=k * sub)
        idx = np.arange(k * sub, (k + 1) * sub, dtype=np.int32)
        desc = ctx.ingest(x.reshape(-1, 4), np.arange(sub + 1, dtype=np.int64) * x.shape[1])
        db.add_scans(desc, ts, idx)
        parts.append(db.query_submit(desc, idx))
        descs.append(cc.desc_to_numpy(desc).copy())
        poses.append(p)
        ts_all.append(np.asarray(ts))
        del x
    db.query_wait()
    torch.cuda.synchronize()
    res = np.concatenate(parts)
    d, poses, ts_all = np.concatenate(descs), np.concatenate(poses), np.concatenate(ts_all)
    exp = dyn_oracle.run_sequence(d, ts_all, np.arange(n, dtype=np.int32), L.default_db_cfg(), dyn=1)
    _compare(exp, res, "kitti 4096")
    pos, lst = _write_eval_files(tmp_path, poses, ts_all)
    f_o, pr_o, _ = _outcome_and_pr(cc, tmp_path, "dyn-oracle", pos, lst, exp)
    f_g, pr_g, _ = _outcome_and_pr(cc, tmp_path, "dyn-hip", pos, lst, res)
    r = _compare_outcome().compare(f_g, f_o, pos, tol_corr=1e-4, tol_pose=1e-4)
    assert r["ok"], r["details"]
    st = dyn_oracle.run_sequence(d, ts_all, np.arange(n, dtype=np.int32), L.default_db_cfg(), dyn=0)
    _, pr_s, _ = _outcome_and_pr(cc, tmp_path, "static-oracle", pos, lst, st)
    print("kitti online replay, dynamic mode: %d scans, %d loop closures, max-F1 %.6f at %.6f, %d TP (static mode: %d loop closures, "
          "max-F1 %.6f); %d queries differ between the modes"
          % (n, int((res["n_res"] > 0).sum()), pr_g["max_f1"], pr_g["sim_thres"], pr_g["tp_count"], int((st["n_res"] > 0).sum()),
             pr_s["max_f1"], int(((st["cand_aft_check3"] != exp["cand_aft_check3"]) | (st["cand_gidx"] != exp["cand_gidx"])).sum())))
    db.close()
    ctx.close()


def test_batch_bin_test_driver_dynamic(cc, oracle, tmp_path):
    """The drop-in offline driver (hostcpp/examples/batch_bin_test.cpp) built with -DDYNAMIC_THRES=1: its outcome file equals
    the one the dynamic oracle's replay of the same list gives (tools/compare_outcome.py)."""
    import os
    import subprocess
    from test_gpu_query import _outcome_and_pr, _write_eval_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "contour-context_amd")
    exe = str(tmp_path / "batch_bin_test_dyn")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-DDYNAMIC_THRES=1", os.path.join(pkg, "hostcpp", "examples", "batch_bin_test.cpp"),
                           "-I", os.path.join(pkg, "hostcpp"), "-I", os.path.join(root, "include"), "-L", pkg, "-lcont2_amd",
                           "-Wl,-rpath," + pkg, "-L/opt/rocm/lib", "-lamdhip64", "-o", exe])
    w = cc.synth.World(loop_len=40.0)
    n = 96
    x, poses, ts = cc.synth.make_sequence(n, world=w, beams=32, azim=900, device="cuda")
    ts = ts * 4.0  # 0.4 s per scan: a 40-scan lap takes 16 s, past the evaluator's 15 s exclusion window
    xs = x.cpu().numpy()
    drv = tmp_path / "drv"
    drv.mkdir()
    lst, pos = drv / "scans.txt", drv / "poses.txt"
    with open(lst, "w") as f, open(pos, "w") as g:
        for i in range(n):
            p = drv / ("%06d.bin" % i)
            xs[i].astype(np.float32).tofile(p)
            f.write("%.6f %d %s\n" % (ts[i], i, p))
            c, s_ = np.cos(poses[i, 2]), np.sin(poses[i, 2])
            g.write("%.6f %.9f %.9f 0 %.9f %.9f %.9f 0 %.9f 0 0 1 0\n" % (ts[i], c, -s_, poses[i, 0], s_, c, poses[i, 1]))
    cfg = open(os.path.join(pkg, "hostcpp", "examples", "batch_bin_test_config.yaml")).read()
    cfg = cfg.replace("/path/to/ts-sens_pose-kitti08.txt", str(pos)).replace("/path/to/ts-lidar_bins-kitti08.txt", str(lst))
    cfg = cfg.replace("/path/to/outcome-kitti08.txt", str(drv / "outcome.txt"))
    cfg = cfg.replace("max_elapse_: 25.0", "max_elapse_: 10.0").replace("min_elapse_: 15.0", "min_elapse_: 6.0")
    (drv / "cfg.yaml").write_text(cfg)
    subprocess.check_output([exe, str(drv / "cfg.yaml")], text=True)
    dcfg = cc.L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 10.0, 6.0
    P = xs.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    ores, _, odesc = oracle.run_sequence(xs.reshape(-1, 4), np.arange(n + 1, dtype=np.int64) * P, ts, seeds, dcfg=dcfg, want_desc=True)
    exp = dyn_oracle.run_sequence(odesc, np.asarray(ts), seeds, dcfg, dyn=1)
    n_diff = int(((exp["cand_aft_check3"] != ores["cand_aft_check3"]) | (exp["cand_gidx"] != ores["cand_gidx"]) |
                  (exp["n_cand_tidy"] != ores["n_cand_tidy"])).sum())
    assert (exp["n_res"] > 0).sum() > 10 and n_diff >= 3
    ev = tmp_path / "ev"
    ev.mkdir()
    epos, elst = _write_eval_files(ev, poses, ts)
    f_o, pr_o, _ = _outcome_and_pr(cc, ev, "dyn-oracle", epos, elst, exp)
    r = _compare_outcome().compare(str(drv / "outcome.txt"), f_o, epos, tol_corr=1e-4, tol_pose=1e-4)
    assert r["ok"], r["details"]
