"""K3's stage time with and without a scan mask, on the bench's KITTI-shaped database (tuning aid, needs the GPU).

usage: masked_knn_time.py [--tree ROOT] [--db-scans 5000] [--batch 1024] [--reps 10] [--variants unmasked,ones,gates]

One chunk of `batch` queries at a time on one lane, CC_KNN_MODE=0 (the walk), the retrieval's time read from
cc_db_profile_read (device events around the stage).  Variants: unmasked | ones (a row of all ones per query: the price of the
test) | gates (a cc_mask_gates row per query, 30 m around the query's own position: on this drive, whose queries go on into new
streets, all but the first rows are empty) | gates_db (row i: 30 m around database scan 4 i's position -- rows of a few dozen
scans that have nothing to do with the query) -- and the time of cc_k_mask_gates itself.
--tree: another checkout (with its library built) to load the package from: a tree without masks runs `unmasked` alone.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--db-scans", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--radius", type=float, default=30.0)
    ap.add_argument("--variants", default="unmasked,ones,gates")
    args = ap.parse_args()
    os.environ["CC_KNN_MODE"] = "0"
    sys.path.insert(0, args.tree)
    import torch
    import cc_amd
    cc = cc_amd.load()
    L = cc.L
    dev = torch.device("cuda", 0)
    wld = cc.synth.World(kitti=True)
    n_db, B = args.db_scans, args.batch
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
    xy_q = np.zeros((B, 2), np.float32)
    for c0 in range(0, B, 256):
        c1 = min(c0 + 256, B)
        x, poses, _ = cc.synth.make_sequence(c1 - c0, world=wld, device=dev, start=n_db + c0)
        qd[c0:c1] = ctx.ingest(x.reshape(-1, 4), np.arange(c1 - c0 + 1, dtype=np.int64) * P)
        xy_q[c0:c1] = np.asarray(poses)[:, :2]
    epochs = np.full(B, n_db, np.int32)
    db.set_lanes(1)
    cc.lib().cc_db_profile_enable(db.h, 1)
    ms5, nq = (C.c_double * 5)(), C.c_int()

    def k3(mask):
        kw = {} if mask is None else {"mask": mask}
        out = []
        for r in range(3 + args.reps):
            cc.lib().cc_db_profile_read(db.h, ms5, C.byref(nq))
            res = db.query(qd, epochs, **kw)
            torch.cuda.synchronize()
            cc.lib().cc_db_profile_read(db.h, ms5, C.byref(nq))
            assert nq.value == B, nq.value
            if r >= 3:
                out.append(ms5[0])
        out = np.array(out)
        return {"k3_ms_per_chunk_median": float(np.median(out)), "min": float(out.min()), "max": float(out.max()),
                "knn_hits_per_query": float(res["n_knn_hits"].mean()), "queries_with_an_answer": int((res["n_res"] > 0).sum())}

    out = {"db_scans": n_db, "batch": B, "reps": args.reps, "tree": os.path.abspath(args.tree)}
    rw = (n_db + 31) // 32
    for v in args.variants.split(","):
        if v == "unmasked":
            out[v] = k3(None)
        elif v == "ones":
            bits = torch.full((B, rw), -1, dtype=torch.int32, device=dev)
            out[v] = k3(cc.ScanMask(bits, np.arange(B)))
        elif v in ("gates", "gates_db"):
            a_db, a_q = xy_db, (xy_q if v == "gates" else xy_db[(np.arange(B) * 4) % n_db])
            t_xy = torch.from_numpy(a_db).to(dev)
            gates = torch.from_numpy(np.concatenate([a_q, np.full((B, 1), args.radius, np.float32)], 1)).to(dev)
            bits = ctx.gate_mask(t_xy, gates)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tg = []
            for r in range(23):
                e0.record()
                bits = ctx.gate_mask(t_xy, gates)
                e1.record()
                torch.cuda.synchronize()
                if r >= 3:
                    tg.append(e0.elapsed_time(e1))
            allowed = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little").sum(1)
            out[v] = k3(cc.ScanMask(bits, np.arange(B)))
            out[v]["allowed_scans_per_row_mean"] = float(allowed.mean())
            out[v]["rows_without_a_scan"] = int((allowed == 0).sum())
            out["mask_gates_ms"] = {"rows": B, "scans": n_db, "median": float(np.median(tg)), "min": float(min(tg)), "max": float(max(tg))}
    print(json.dumps(out))
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
