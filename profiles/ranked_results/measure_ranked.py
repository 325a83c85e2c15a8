"""What the ranked list costs: the query chain with `ranked=16` (cc_k_final_r + the list copy) against the plain chain
(cc_k_final) of the SAME process, in the setting of DESIGN.md section 3.5's cost paragraph: a KITTI-shaped 5 000-scan database
(synth.World(kitti=True), scans 0-4 999), the last 1 024 scans queried at their own epochs, cc_db_profile_enable /
cc_db_profile_read, 5 x 1 024 queries per variant after a warm-up batch each, the two variants alternated.  Both variants go
through query_submit + query_wait (one chunk of 1 024 on one lane), so the chains differ in K6 and the copy only.
usage: python profiles/ranked_results/measure_ranked.py [out.jsonl]     prints / writes one JSON line per timed batch + a summary"""
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
    n_db, nq, reps, K = 5000, 1024, 5, 16
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

    def batch(ranked):
        t0 = time.perf_counter()
        r = db.query_submit(qdesc, epochs, ranked=K if ranked else None)
        db.query_wait()
        wall = (time.perf_counter() - t0) * 1e3
        ms = (C.c_double * 5)()
        n = C.c_int()
        assert lib.cc_db_profile_read(db.h, ms, C.byref(n)) == 0
        return r, wall, list(ms), n.value

    ref, _, _, _ = batch(False)          # warm-up, one batch per variant
    (res, (cands, cnt)), _, _, _ = batch(True)
    assert res.tobytes() == ref.tobytes()
    rows = {False: [], True: []}
    for rep in range(reps):
        for ranked in (False, True):
            _, wall, ms, n = batch(ranked)
            rec = {"variant": "ranked16" if ranked else "plain", "rep": rep, "queries": n, "wall_ms": wall, "knn_ms": ms[0], "check_ms": ms[1],
                   "merge_ms": ms[2], "gmm_ms": ms[3], "final_ms": ms[4], "chain_ms": sum(ms)}
            rows[ranked].append(rec)
            line = json.dumps(rec)
            print(line)
            if out:
                out.write(line + "\n")
    summ = {"summary": True, "db_scans": n_db, "queries_per_batch": nq, "max_ret": K,
            "queries_with_a_result": int((ref["n_res"] > 0).sum()), "listed_entries": int(cnt.sum()),
            "queries_with_2_or_more_entries": int((cnt >= 2).sum()), "list_bytes_per_chunk": nq * K * 40}
    for ranked, name in ((False, "plain"), (True, "ranked16")):
        for f in ("final_ms", "chain_ms", "wall_ms"):
            v = sorted(r[f] for r in rows[ranked])
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
