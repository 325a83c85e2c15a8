"""K3's stage time of a listed query against the masked walk on the same sets, on the bench's KITTI-shaped database (tuning aid,
needs the GPU).

usage: listed_knn_time.py [--tree ROOT] [--db-scans 5000] [--batch 1024] [--reps 10] [--variant V]

One chunk of `batch` queries at a time on one lane, CC_KNN_MODE=0, the retrieval's time read from cc_db_profile_read (device
events around the stage), median of `reps` chunks after 3 warm-ups; beside it the host's time for submit + wait of the chunk
(everything behind the retrieval included) and, for the listed forms, the bytes the chunk stages (8 per query + 16 per listed
scan).  ONE variant per process:
  unmasked          no restriction
  masked_gates_db   row i: the scans within --radius of database scan 4 i's position (Context.gate_mask), the masked walk
  listed_gates_db   the same sets as lists (ScanLists.from_gates)
  listed_N          list i: the N scans around database scan 4 i in adding order (N = 16, 64, 256, 1024, ...)
--tree: another checkout (with its library built) to load the package from; a tree without the listed form runs the first two.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--db-scans", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--radius", type=float, default=30.0)
    ap.add_argument("--variant", default="listed_gates_db")
    args = ap.parse_args()
    os.environ["CC_KNN_MODE"] = "0"
    sys.path.insert(0, args.tree)
    import torch
    import cc_amd
    cc = cc_amd.load()
    dev = torch.device("cuda", 0)
    wld = cc.synth.World(kitti=True)
    n_db, B, v = args.db_scans, args.batch, args.variant
    ctx = cc.Context(0, max_batch=256)
    db = cc.Database(ctx, capacity=n_db + 16)
    xy_db = np.zeros((n_db, 2), np.float32)
    P = None
    for c0 in range(0, n_db, 256):
        c1 = min(c0 + 256, n_db)
        x, poses, _ = cc.synth.make_sequence(c1 - c0, world=wld, device=dev, start=c0)
        P = x.shape[1]
        d = ctx.ingest(x.reshape(-1, 4), np.arange(c1 - c0 + 1, dtype=np.int64) * P)
        db.add_scans(d, np.arange(c0, c1) / 10.0, np.arange(c0, c1, dtype=np.int32))
        xy_db[c0:c1] = np.asarray(poses)[:, :2]
    qd = torch.empty((B, cc.DESC_BYTES), dtype=torch.uint8, device=dev)
    for c0 in range(0, B, 256):
        c1 = min(c0 + 256, B)
        x, _, _ = cc.synth.make_sequence(c1 - c0, world=wld, device=dev, start=n_db + c0)
        qd[c0:c1] = ctx.ingest(x.reshape(-1, 4), np.arange(c1 - c0 + 1, dtype=np.int64) * P)
    epochs = np.full(B, n_db, np.int32)
    db.set_lanes(1)
    cc.lib().cc_db_profile_enable(db.h, 1)
    ms5, nq = (C.c_double * 5)(), C.c_int()
    centre = (np.arange(B) * 4) % n_db
    gates = np.concatenate([xy_db[centre], np.full((B, 1), args.radius, np.float32)], 1).astype(np.float32)
    out = {"variant": v, "db_scans": n_db, "batch": B, "reps": args.reps, "tree": os.path.abspath(args.tree)}
    kw = {}
    if v == "masked_gates_db":
        bits = ctx.gate_mask(torch.from_numpy(xy_db).to(dev), torch.from_numpy(gates).to(dev))
        torch.cuda.synchronize()
        kw["mask"] = cc.ScanMask(bits, np.arange(B))
        out["scans_per_set_mean"] = float(np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little").sum(1).mean())
        out["table_bytes"] = int(bits.numel() * 4)
    elif v.startswith("listed_"):
        if v == "listed_gates_db":
            sl = cc.ScanLists.from_gates(xy_db, gates)
        else:
            n = int(v.split("_")[1])
            lo = np.clip(centre - n // 2, 0, n_db - n)
            sl = cc.ScanLists.from_lists([np.arange(a, a + n) for a in lo])
        kw["among"] = sl
        out["scans_per_set_mean"] = float(np.diff(sl.off).mean())
        out["staged_bytes_per_chunk"] = int(8 * B + 16 * len(sl.idx))
    elif v != "unmasked":
        raise SystemExit("unknown variant %r" % v)
    k3, wall = [], []
    res = None
    for r in range(3 + args.reps):
        cc.lib().cc_db_profile_read(db.h, ms5, C.byref(nq))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = db.query_submit(qd, epochs, **kw)
        db.query_wait()
        t1 = time.perf_counter()
        cc.lib().cc_db_profile_read(db.h, ms5, C.byref(nq))
        assert nq.value == B, nq.value
        if r >= 3:
            k3.append(ms5[0])
            wall.append((t1 - t0) * 1e3)
    k3, wall = np.array(k3), np.array(wall)
    out.update(k3_ms_per_chunk_median=float(np.median(k3)), k3_min=float(k3.min()), k3_max=float(k3.max()),
               submit_wait_ms_median=float(np.median(wall)), submit_wait_min=float(wall.min()), submit_wait_max=float(wall.max()),
               knn_hits_per_query=float(res["n_knn_hits"].mean()), queries_with_an_answer=int((res["n_res"] > 0).sum()))
    print(json.dumps(out))
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
