"""Randomised parity campaign of the dynamic-threshold mode ON THE GPU (not collected by pytest; run by hand on the GPU box):
    python tests/fuzz_gpu_dynamic_thres.py <seed0> <n_iter>
Per drive: a random world (loop, dense, KITTI-shaped), DB configuration and bars -- the upper bars drawn close to the lower
ones, so that they are reached mid-window -- the device in dynamic mode (one batched query of every scan at its own epoch,
or the online loop on 1-4 lanes) against the dynamic CPU oracle (tests/dyn_thres_oracle.cpp) replaying the driver loop on the
device's descriptors: every integer of every result, correlation and pose within 1e-4.  Then the hint flow for two loop
closures in random hint orders: per-hint scores, passed flags and the result."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE]
import cc_amd  # noqa: E402
import dyn_oracle  # noqa: E402
import oracle_py as oracle  # noqa: E402
from test_emu_hints import _demo_hints  # noqa: E402

INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy", "n_knn_hits"]
SCORES = ("i_ovlp_sum", "i_ovlp_max_one", "i_in_ang_rng", "i_indiv_sim", "i_orie_sim", "passed")


def one(cc, seed):
    import torch
    L = oracle.L
    rng = np.random.default_rng(seed)
    d = L.default_db_cfg()
    d.min_elapse = float(rng.uniform(0.8, 2.0))
    d.max_elapse = d.min_elapse + float(rng.uniform(0.5, 1.5))
    d.nnk = int(rng.choice([10, 30, 50, 64]))
    d.max_fine_opt = int(rng.choice([2, 5, 10]))
    qlv = [(1, 2, 3), (2, 3), (2, 3, 4)][int(rng.integers(3))]
    d.n_q_levels = len(qlv)
    for i, v in enumerate(qlv):
        d.q_levels[i] = v
    lb, ub = L.default_thresholds()
    if rng.random() < 0.6:
        lb.i_ovlp_sum, lb.i_ovlp_max_one, lb.i_in_ang_rng, lb.i_indiv_sim, lb.i_orie_sim = [int(v) for v in rng.integers(2, 5, 5)]
        lb.correlation = float(rng.uniform(0.1, 0.5))
    if rng.random() < 0.6:  # upper bars a few steps above the lower ones
        for f in ("i_ovlp_sum", "i_ovlp_max_one", "i_in_ang_rng", "i_indiv_sim", "i_orie_sim"):
            setattr(ub, f, getattr(lb, f) + int(rng.integers(1, 6)))
        ub.correlation = lb.correlation + float(rng.uniform(0.05, 0.4))
        ub.area_perc = lb.area_perc + float(rng.uniform(0.01, 0.2))
        ub.neg_est_dist = lb.neg_est_dist + float(rng.uniform(0.5, 8.0))
    kind = int(rng.integers(3))
    world = cc.synth.World(loop_len=float(rng.uniform(24, 36)), dense=(kind == 1), seed=int(rng.integers(1 << 20))) if kind < 2 else \
        cc.synth.World(kitti=True, seed=int(rng.integers(1 << 20)), block=float(rng.uniform(36, 50)), tile=300.0)
    n = int(rng.integers(56, 84))
    full = seed % 3 == 0
    x, poses, ts = cc.synth.make_sequence(n, world=world, device="cuda", step=(1.0 if kind < 2 else 3.0),
                                          **({} if full else dict(beams=16, azim=450)))
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    seeds = np.arange(n, dtype=np.int32)
    ctx = cc.Context(0, max_batch=512)
    desc = ctx.ingest(x.reshape(-1, 4), offs)
    db = cc.Database(ctx, cfg=d, capacity=n)
    db.set_dynamic_thres(True)
    online = seed % 3 == 1
    if not online:
        db.add_scans(desc, ts, seeds)
        res = db.query(desc, seeds, lb=lb, ub=ub, allow_flagged=True)
    else:
        sub = int(rng.choice([1, 5, 16, 37]))
        db.set_lanes(int(rng.choice([1, 2, 4])))
        parts = []
        for a0 in range(0, n, sub):
            a1 = min(a0 + sub, n)
            blk = desc[a0:a1].contiguous()
            db.add_scans(blk, ts[a0:a1], seeds[a0:a1])
            try:
                parts.append(db.query_submit(blk, seeds[a0:a1], lb=lb, ub=ub))
            except cc.CCError as e:
                if e.rc != cc.CC_ECAPACITY:
                    raise
        try:
            db.query_wait()
        except cc.CCError as e:
            if e.rc != cc.CC_ECAPACITY:
                raise
        res = np.concatenate(parts)
    torch.cuda.synchronize()
    dn = cc.desc_to_numpy(desc)
    exp = dyn_oracle.run_sequence(dn, np.asarray(ts), seeds, d, lb=lb, ub=ub, dyn=1)
    st = dyn_oracle.run_sequence(dn, np.asarray(ts), seeds, d, lb=lb, ub=ub, dyn=0)
    bad = 0
    for i in range(n):
        if dn["flags"][i] or res["flags"][i]:
            continue  # a capacity was met and reported: not a parity case
        for f in INT_FIELDS:
            if exp[f][i] != res[f][i]:
                print("  MISMATCH seed %d scan %d field %s: oracle %s kernels %s" % (seed, i, f, exp[f][i], res[f][i]))
                bad += 1
        if exp["n_res"][i] and res["n_res"][i]:
            e = max(abs(exp["correlation"][i] - res["correlation"][i]), float(np.abs(exp["tf"][i] - res["tf"][i]).max()))
            if e > 1e-4:
                print("  MISMATCH seed %d scan %d float error %.3g" % (seed, i, e))
                bad += 1
    n_diff = int(((exp["cand_aft_check3"] != st["cand_aft_check3"]) | (exp["cand_gidx"] != st["cand_gidx"]) |
                  (exp["n_cand_tidy"] != st["n_cand_tidy"])).sum())
    # hint flow: two loop closures, random hint orders
    n_hint = 0
    for qi in np.nonzero(exp["n_res"] > 0)[0][:2]:
        c = int(exp["cand_gidx"][qi])
        cands = sorted({c, max(c - 1, 0), min(c + 1, int(qi) - 1), int(rng.integers(0, max(int(qi), 1)))})
        hints = _demo_hints(L, dn, qi, cands)
        if len(hints) == 0:
            continue
        hs = hints[rng.permutation(len(hints))]
        eres, esc = dyn_oracle.check_hints(dn, qi, cands, hs, d.cont_sim, lb=lb, ub=ub, max_fine_opt=d.max_fine_opt, dyn=1)
        h = np.zeros(len(hs), L.hint_dt)
        h["cand_gidx"] = np.array(cands)[hs[:, 0]]
        h["level"], h["seq_src"], h["seq_tgt"] = hs[:, 1], hs[:, 2], hs[:, 3]
        try:
            r, sc = db.check_hints(desc[qi:qi + 1].contiguous(), h, lb=lb, ub=ub, max_fine_opt=d.max_fine_opt)
        except cc.CCError as e:
            if e.rc != cc.CC_ECAPACITY:
                raise
            continue
        got = np.stack([sc[f] for f in SCORES], 1)
        nb = int((got != esc).any(1).sum())
        for f in INT_FIELDS:
            e = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[int(eres[f])]
            nb += int(e != r[f])
        if eres["n_res"] and (abs(eres["correlation"] - r["correlation"]) > 1e-4 or np.abs(eres["tf"] - r["tf"]).max() > 1e-4):
            nb += 1
        if nb:
            print("  MISMATCH seed %d hint flow query %d: %d" % (seed, qi, nb))
        bad += nb
        n_hint += len(hs)
    print("seed %d kind %d %s %s n %d nnk %d qlv %s ub-near %s hits %d flagged %d modes-differ %d hints %d: %s" % (
        seed, kind, "full" if full else "16x450", "online" if online else "batch", n, d.nnk, qlv, ub.i_orie_sim - lb.i_orie_sim <= 5,
        int((exp["n_res"] > 0).sum()), int((dn["flags"] != 0).sum() + (res["flags"] != 0).sum()), n_diff, n_hint,
        "ok" if not bad else "%d MISMATCHES" % bad), flush=True)
    db.close()
    ctx.close()
    return bad == 0, n_diff > 0


if __name__ == "__main__":
    s0, n_it = int(sys.argv[1]), int(sys.argv[2])
    cc = cc_amd.load()
    oracle.lib()
    n_ok = n_bad = n_differ = 0
    for s in range(s0, s0 + n_it):
        ok, differ = one(cc, s)
        n_ok += ok
        n_bad += not ok
        n_differ += differ
    print("dynamic-threshold campaign: %d drives, %d differ from the oracle, %d where the two modes give different answers" % (n_it, n_bad, n_differ))
