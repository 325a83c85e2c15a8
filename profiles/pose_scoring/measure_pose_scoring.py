"""What scoring caller-given poses costs: cc_db_pose_batch over 1 024 items, four variants (refine = 0; refine = 1; refine = 1 with
curvature; refine = 1 with eight try poses), next to a cc_db_verify_batch over the SAME (query, candidate) pairs, one candidate
per item -- whose chain runs the same cc_k_gmm_init / cc_k_gmm_refine on the same problems behind its checks and merge.
Setting of DESIGN.md section 3.6: 130 full-size scans on a 100 m loop, a database of scans 0..99, the queries 100..129 against
the neighbours of their place on the first lap; the items cycle over the entries the verify flow (ranked = 8, detail) accepts,
tf_init = the detail row's.  Variants alternated in one process, WARM warm-up and REPS timed repetitions each; per repetition
the host wall time of the synchronous call and the stage slots of cc_db_profile_read (summed over the call's chunks: a
synchronous call of 1 024 items is two chunks of 512 on two lanes).  The oracle's time for the same gmm calls on one core is
printed as context.  cc_k_pose_eval alone: rocprofv3 --kernel-trace --stats -- python this_script.py - 2 1
usage: python profiles/pose_scoring/measure_pose_scoring.py [out.jsonl|-] [REPS] [WARM]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import cc_amd  # noqa: E402


def main():
    import torch
    cc = cc_amd.load()
    L = cc.L
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 and sys.argv[1] != "-" else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    n, n_db, n_items = 130, 100, 1024
    xyzi, poses, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=100.0), device="cuda")
    ctx = cc.Context(0, max_batch=128)
    desc = ctx.ingest(xyzi.reshape(-1, 4), np.arange(n + 1, dtype=np.int64) * xyzi.shape[1])
    db = cc.Database(ctx, capacity=n)
    db.add_scans(desc[:n_db], np.asarray(ts)[:n_db], np.arange(n_db, dtype=np.int32))
    qs = np.arange(n_db, n, dtype=np.int32)
    lists = [[q - 100, q - 99] + ([q - 101] if q > 100 else []) for q in qs]
    res, (c, cnt), det = db.verify(desc, lists, qidx=qs, ranked=8, detail=True)
    ents = [(int(qs[i]), int(c[i][k]["cand_gidx"]), det[i][k]["tf_init"].copy(), int(det[i][k]["n_pairs"])) for i in range(len(qs)) for k in range(int(cnt[i]))]
    assert ents, "the verify flow accepts nothing"
    pick = [ents[i % len(ents)] for i in range(n_items)]
    q = np.array([e[0] for e in pick], np.int32)
    g = np.array([e[1] for e in pick], np.int32)
    tf = np.array([e[2] for e in pick])
    rng = np.random.default_rng(3)
    tries = tf[:, None, :] + rng.uniform(-1, 1, (n_items, 8, 3)) * np.array([1.0, 1.0, 0.01])
    lib = cc.lib()
    assert lib.cc_db_profile_enable(db.h, 1) == 0

    def slots():
        ms = (C.c_double * 5)()
        k = C.c_int()
        assert lib.cc_db_profile_read(db.h, ms, C.byref(k)) == 0
        return list(ms), k.value

    variants = {
        "pose_refine0": lambda: db.score_poses(desc, q, g, tf, refine=False),
        "pose_refine1": lambda: db.score_poses(desc, q, g, tf, refine=True),
        "pose_refine1_curv": lambda: db.score_poses(desc, q, g, tf, refine=True, curvature=True),
        "pose_refine1_try8": lambda: db.score_poses(desc, q, g, tf, refine=True, tries=tries),
        "verify_same_pairs": lambda: db.verify(desc, [[int(x)] for x in g], qidx=q),
    }
    rows = {k: [] for k in variants}
    last = {}
    for rep in range(-warm, reps):
        for name, fn in variants.items():
            slots()
            t0 = time.perf_counter()
            last[name] = fn()
            wall = (time.perf_counter() - t0) * 1e3
            ms, k = slots()
            if rep < 0:
                continue
            rec = {"variant": name, "rep": rep, "items": k, "wall_ms": wall, "slot0_ms": ms[0], "slot1_ms": ms[1], "slot2_ms": ms[2], "k5_ms": ms[3], "out_ms": ms[4]}
            rows[name].append(rec)
            line = json.dumps(rec)
            print(line)
            if out:
                out.write(line + "\n")
    r1 = last["pose_refine1"][0]
    vr = last["verify_same_pairs"]
    same = (vr["n_res"] > 0) & ((r1["flags"] & L.PF_REFINED) != 0)
    summ = {"summary": True, "items": n_items, "distinct_entries": len(ents), "reps": reps, "warm": warm,
            "n_pairs_min_median_max": [int(r1["n_pairs"].min()), float(np.median(r1["n_pairs"])), int(r1["n_pairs"].max())],
            "refined_items": int(((r1["flags"] & L.PF_REFINED) != 0).sum()), "iterations_mean": float(r1["iterations"][r1["iterations"] > 0].mean()),
            "verify_items_with_a_result": int((vr["n_res"] > 0).sum()),
            "max_abs_corr_pose_minus_verify": float(np.abs(r1["correlation"][same] - vr["correlation"][same]).max()) if same.any() else None}
    for name in variants:
        for f in ("wall_ms", "slot0_ms", "k5_ms", "out_ms"):
            v = sorted(r[f] for r in rows[name])
            summ["%s_%s_median_min_max" % (name, f)] = [v[len(v) // 2], v[0], v[-1]]
    # the oracle on one core, the same 1 024 gmm calls (context, not a target)
    try:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_py as O
        hd = cc.desc_to_numpy(desc)
        sc = {i: O.Scan.from_desc(hd[i], int_id=int(i)) for i in set(q.tolist()) | set(g.tolist())}
        t0 = time.perf_counter()
        for i in range(n_items):
            O.gmm(sc[int(g[i])], sc[int(q[i])], tf[i])
        summ["oracle_gmm_1024_calls_s"] = time.perf_counter() - t0
    except Exception as e:  # the oracle is test infrastructure: the measurement stands without it
        summ["oracle_gmm_1024_calls_s"] = "unavailable: %s" % e
    line = json.dumps(summ)
    print(line)
    if out:
        out.write(line + "\n")
        out.close()
    torch.cuda.synchronize()
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
