"""What the per-candidate detail costs: the query chain with `ranked=16, detail=True` (cc_k_gmm_hess behind the refinement,
cc_k_final_rd, the detail rows' copy) against the `ranked=16` chain of the SAME process, in the setting of
profiles/ranked_results/measure_ranked.py: a KITTI-shaped 5 000-scan database (synth.World(kitti=True), scans 0-4 999), the last
1 024 scans queried at their own epochs, cc_db_profile_enable / cc_db_profile_read, REPS x 1 024 queries per variant after a
warm-up batch each, the two variants alternated.  Both go through query_submit + query_wait (one chunk of 1 024 on one lane).
The profile's K5 slot (gmm_ms) ends behind cc_k_gmm_hess, so it carries the new kernel; cc_k_gmm_hess alone comes from a
kernel trace of this script (rocprofv3 --kernel-trace --stats -- python ... , REPS=2).
usage: python profiles/ranked_detail/measure_ranked_detail.py [out.jsonl] [REPS]   one JSON line per timed batch + a summary"""
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
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_db, nq, K = 5000, 1024, 16
    w = cc.synth.World(kitti=True)
    ctx = cc.Context(0, max_batch=256)
    db = cc.Database(ctx, capacity=n_db + 16)
    ts = np.arange(n_db, dtype=np.float64) / 10.0
    seeds = np.arange(n_db, dtype=np.int32)
    qdesc = torch.empty((nq, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    for c0 in range(0, n_db, 128):
        c1 = min(c0 + 128, n_db)
        xyzi, _, _ = cc.synth.make_sequence(0, world=w, device="cuda", indices=np.arange(c0, c1))
        d = ctx.ingest(xyzi.reshape(-1, 4), np.arange(c1 - c0 + 1, dtype=np.int64) * xyzi.shape[1])
        db.add_scans(d, ts[c0:c1], seeds[c0:c1])
        lo = max(c0, n_db - nq)
        if c1 > lo:
            qdesc[lo - (n_db - nq):c1 - (n_db - nq)] = d[lo - c0:]
    torch.cuda.synchronize()
    epochs = np.arange(n_db - nq, n_db, dtype=np.int32)
    lib = cc.lib()
    assert lib.cc_db_profile_enable(db.h, 1) == 0

    def batch(detail):
        t0 = time.perf_counter()
        r = db.query_submit(qdesc, epochs, ranked=K, detail=detail)
        db.query_wait()
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 5)()
        n = C.c_int()
        assert lib.cc_db_profile_read(db.h, ms, C.byref(n)) == 0
        return r, wall, list(ms), n.value

    (ref, (rc0, rn0)), _, _, _ = batch(False)          # warm-up, one batch per variant
    (res, (cands, cnt), det), _, _, _ = batch(True)
    assert res.tobytes() == ref.tobytes() and cands.tobytes() == rc0.tobytes() and np.array_equal(cnt, rn0)
    rows = {False: [], True: []}
    for rep in range(reps):
        for detail in (False, True):
            _, wall, ms, n = batch(detail)
            rec = {"variant": "ranked16_detail" if detail else "ranked16", "rep": rep, "queries": n, "wall_ms": wall, "knn_ms": ms[0],
                   "check_ms": ms[1], "merge_ms": ms[2], "gmm_ms": ms[3], "final_ms": ms[4], "chain_ms": sum(ms)}
            rows[detail].append(rec)
            line = json.dumps(rec)
            print(line)
            if out:
                out.write(line + "\n")
    listed = np.concatenate([det[i][:cnt[i]] for i in range(nq)]) if cnt.sum() else det[:0].reshape(-1)
    # the refined problems of the chunk are a superset of the listed entries (max_fine_opt refined, max_ret listed: 10 <= 16, so all)
    summ = {"summary": True, "db_scans": n_db, "queries_per_batch": nq, "max_ret": K, "reps": reps,
            "queries_with_a_result": int((ref["n_res"] > 0).sum()), "listed_entries": int(cnt.sum()),
            "listed_pairs_total": int(listed["n_pairs"].sum()), "listed_pairs_median": float(np.median(listed["n_pairs"])) if len(listed) else 0.0,
            "listed_pairs_max": int(listed["n_pairs"].max()) if len(listed) else 0,
            "iterations_mean": float(listed["iterations"].mean()) if len(listed) else 0.0,
            "terminations": {str(k): int((listed["termination"] == k).sum()) for k in np.unique(listed["termination"])} if len(listed) else {},
            "detail_bytes_per_chunk": nq * K * 120}
    if len(listed):
        ev = np.array([np.linalg.eigvalsh(cc.L.hess_matrix(h))[[0, 2]] for h in listed["hess"]])
        summ["min_eig_min_median"] = [float(ev[:, 0].min()), float(np.median(ev[:, 0]))]
        summ["condition_median_max"] = [float(np.median(ev[:, 1] / ev[:, 0])), float((ev[:, 1] / ev[:, 0]).max())]
    for detail, name in ((False, "ranked16"), (True, "ranked16_detail")):
        for f in ("gmm_ms", "final_ms", "chain_ms", "wall_ms"):
            v = sorted(r[f] for r in rows[detail])
            summ["%s_%s_median" % (name, f)] = v[len(v) // 2]
            summ["%s_%s_min_max" % (name, f)] = [v[0], v[-1]]
    line = json.dumps(summ)
    print(line)
    if out:
        out.write(line + "\n")
        out.close()
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
