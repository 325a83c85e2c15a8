"""Chunk timings of the ranked query call with and without matches: the bench's KITTI-shaped 5 000-scan
database, chunks of 1 024 queries, ranked=16; per chunk the K4b (merge) and tail (final) stage times from the library's stage
events (cc_db_profile_read) and the host's submit + wait.  Median, min and max of --chunks chunks after --warmup warm-up chunks.

usage: measure_matches.py [--root TREE] [--matches INLIER_PX] [--chunks 10] [--warmup 3] [--label NAME]
  --root     the tree whose package and built library are measured (default: this one); the parent commit's tree, built, for
             the parent's figures -- the script uses nothing the parent's package lacks unless --matches is given
One JSON line per run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--matches", type=float, default=None)
ap.add_argument("--chunks", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--db-scans", type=int, default=5000)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch  # noqa: E402
import cc_amd  # noqa: E402

cc = cc_amd.load()
dev = torch.device("cuda", 0)
B, n_db = 1024, args.db_scans
beams, azim = 64, 1875
P = beams * azim
wld = cc.synth.World(kitti=True)
ctx = cc.Context(0, max_batch=256)
HB, FB = cc.packed_sizes()
hot_db = torch.zeros((n_db, HB), dtype=torch.uint8, device=dev)
feat_db = torch.zeros((n_db, FB), dtype=torch.uint8, device=dev)
CH = 128
tmp = torch.empty((CH, cc.DESC_BYTES), dtype=torch.uint8, device=dev)
for c0 in range(0, n_db, CH):
    c1 = min(c0 + CH, n_db)
    xyzi, _, _ = cc.synth.make_sequence(0, world=wld, device=dev, indices=np.arange(c0, c1), beams=beams, azim=azim)
    d = ctx.ingest(xyzi.reshape(-1, 4), np.arange(c1 - c0 + 1, dtype=np.int64) * P, out=tmp[:c1 - c0])
    h, f = ctx.pack(d)
    hot_db[c0:c1], feat_db[c0:c1] = h, f
db = cc.Database(ctx, capacity=n_db + 16)
db.set_lanes(1)   # one chunk at a time: a chunk's stage times are its own
db.add_packed(hot_db, feat_db, np.arange(n_db, dtype=np.float64) / 10.0, np.arange(n_db, dtype=np.int32))
n_chunks = args.warmup + args.chunks
qd = []
for s in range(n_chunks):   # every chunk its own 1 024 scans, their descriptors resident before the timed calls
    out = torch.empty((B, cc.DESC_BYTES), dtype=torch.uint8, device=dev)
    for c0 in range(0, B, CH):
        xyzi, _, _ = cc.synth.make_sequence(CH, world=wld, device=dev, start=n_db + s * B + c0, beams=beams, azim=azim)
        ctx.ingest(xyzi.reshape(-1, 4), np.arange(CH + 1, dtype=np.int64) * P, out=out[c0:c0 + CH])
    qd.append(out)
torch.cuda.synchronize()
epochs = np.full(B, n_db, np.int32)
cc.lib().cc_db_profile_enable(db.h, 1)
ms5, nq = (C.c_double * 5)(), C.c_int()
cc.lib().cc_db_profile_read(db.h, ms5, C.byref(nq))
rows = []
kw = {} if args.matches is None else {"matches": args.matches}
entries = pairs = 0
for s in range(n_chunks):
    t0 = time.perf_counter()
    r = db.query_submit(qd[s], epochs, ranked=16, **kw)
    db.query_wait()
    host_ms = (time.perf_counter() - t0) * 1e3
    cc.lib().cc_db_profile_read(db.h, ms5, C.byref(nq))
    assert nq.value == B, nq.value
    rows.append((ms5[2], ms5[4], host_ms, sum(ms5)))
    if s >= args.warmup:
        entries += int(r[1][1].sum())
        if args.matches is not None:
            pairs += int(r[2]["n_pairs"].sum())
a = np.array(rows[args.warmup:])


def stat(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


print(json.dumps({"label": args.label, "matches": args.matches, "chunks": args.chunks, "warmup": args.warmup, "queries_per_chunk": B, "db_scans": n_db,
                  "k4b_merge_ms": stat(a[:, 0]), "tail_final_ms": stat(a[:, 1]), "host_submit_wait_ms": stat(a[:, 2]), "all_stages_ms": stat(a[:, 3]),
                  "ranked_entries": entries, "matched_pairs": pairs,
                  "match_bytes_per_chunk": B * 16 * 96 if args.matches is not None else 0}))
