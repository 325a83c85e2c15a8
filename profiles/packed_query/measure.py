"""The query flow from descriptors, from packed records and from the database's own rows, on one MI355X: the KITTI-shaped
5 000-scan database of bench.py, 1 024 queries per submit -- 1 024 scans OF the database, spread over it, queried at the last
epoch, so that the three variants ask the same questions:
  A  query_submit(desc) + wait          cc_k_pack_hot + cc_k_gmm_prep build the chunk's records from 169 KB descriptors
  B  query_submit(cc.Packed(...)) + wait  cc_k_prep_packed copies them from the caller's cc_pack_scans arrays
  C  query_submit(db.stored(...)) + wait  ... from the database's rows
The variants alternate in one process, --repeats times each after two warm-up rounds; wall times are host clocks around submit +
wait (which ends in a stream synchronise).  The answers of B and C must be A's bytes.

  wall times:    python profiles/packed_query/measure.py                                 -> one JSON line
  kernel times:  rocprofv3 --kernel-trace --output-format csv -d DIR -o r -- python profiles/packed_query/measure.py --repeats 3
                 python profiles/packed_query/measure.py --kernels DIR                   -> the prep kernels' launches of 1 024 items
The copy moves 1 024 x 59 448 B in and as many out (121.7 MB); its floor is that over the 6.3 TB/s a streaming copy achieves."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
N_DB, NQ = 5000, 1024
REC_BYTES = 18448 + 41000
FLOOR_MS = 2 * NQ * REC_BYTES / 6.3e12 * 1e3
PREP = ("cc_k_pack_hot", "cc_k_gmm_prep", "cc_k_prep_packed")


def drive(repeats):
    import torch
    import cc_amd
    cc = cc_amd.load()
    wld = cc.synth.World(kitti=True)
    mk = dict(beams=64, azim=1875)
    P = 64 * 1875
    ctx = cc.Context(0, max_batch=256)
    HB, FB = cc.packed_sizes()
    assert HB + FB == REC_BYTES
    hot_db = torch.empty((N_DB, HB), dtype=torch.uint8, device="cuda")
    feat_db = torch.empty((N_DB, FB), dtype=torch.uint8, device="cuda")
    q_idx = (np.arange(NQ) * (N_DB // NQ)).astype(np.int32)   # the queries: every fourth scan of the database
    qdesc = torch.empty((NQ, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    tmp = torch.empty((128, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    pos = {int(g): k for k, g in enumerate(q_idx)}
    for c0 in range(0, N_DB, 128):
        c1 = min(c0 + 128, N_DB)
        xyzi, _, _ = cc.synth.make_sequence(0, world=wld, device="cuda", indices=np.arange(c0, c1), **mk)
        d = ctx.ingest(xyzi.reshape(-1, 4), np.arange(c1 - c0 + 1, dtype=np.int64) * P, out=tmp[:c1 - c0])
        h, f = ctx.pack(d)
        hot_db[c0:c1], feat_db[c0:c1] = h, f
        for g in range(c0, c1):
            if g in pos:
                qdesc[pos[g]].copy_(d[g - c0])
    db = cc.Database(ctx, capacity=N_DB + 16)
    db.add_packed(hot_db, feat_db, np.arange(N_DB, dtype=np.float64) / 10.0, np.arange(N_DB, dtype=np.int32))
    qhot, qfeat = ctx.pack(qdesc)
    torch.cuda.synchronize()
    epochs = np.full(NQ, N_DB, np.int32)
    variants = {"A_desc": lambda: db.query_submit(qdesc, epochs), "B_packed": lambda: db.query_submit(cc.Packed(qhot, qfeat), epochs),
                "C_stored": lambda: db.query_submit(db.stored(q_idx), epochs)}
    wall = {k: [] for k in variants}
    out = {}
    for r in range(2 + repeats):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            db.query_wait()
            t1 = time.perf_counter()
            if r >= 2:
                wall[k].append((t1 - t0) * 1e3)
            out[k] = res.copy()
    assert out["B_packed"].tobytes() == out["A_desc"].tobytes() and out["C_stored"].tobytes() == out["A_desc"].tobytes(), "the variants answer differently"
    # the descriptor side's prep stage alone: cc_pack_scans launches exactly cc_k_pack_hot + cc_k_gmm_prep on the 1 024 descriptors
    ev = []
    for r in range(2 + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.pack(qdesc)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    pack_ms = [a.elapsed_time(b) for a, b in ev[2:]]
    line = {"what": "1 024 queries per submit against the KITTI-shaped 5 000-scan database, submit + wait, ms", "repeats": repeats,
            "loop_closures": int((out["A_desc"]["n_res"] > 0).sum()), "copy_floor_ms_at_6.3TBps": FLOOR_MS,
            "pack_scans_1024_event_ms": {"median": float(np.median(pack_ms)), "min": min(pack_ms), "max": max(pack_ms)}}
    for k, v in wall.items():
        line[k] = {"median": float(np.median(v)), "min": min(v), "max": max(v), "all": [round(x, 4) for x in v]}
    top_a = line["A_desc"]["max"]
    line["bar"] = {k: bool(line[k]["median"] <= top_a) for k in ("B_packed", "C_stored")}
    print(json.dumps(line), flush=True)
    db.close()
    ctx.close()


def kernels(d):
    """the prep kernels' launches over 1 024 items in a rocprofv3 kernel trace: count, median / min / max duration in microseconds"""
    rows = [r for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)) for r in csv.DictReader(open(f))]
    out = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        k = next((p for p in PREP if name.startswith(p)), None)
        if k is None:
            continue
        grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"])
        wg = int(r["Workgroup_Size_X"]) if "Workgroup_Size_X" in r else int(r["Workgroup_Size"])
        items = grid // wg // (8 if k == "cc_k_prep_packed" else 1)
        if items != NQ:
            continue
        out.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for k, v in out.items():
        line = {"kernel": k, "items": NQ, "launches": len(v), "median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)}
        if k == "cc_k_prep_packed":
            line["floor_us"] = FLOOR_MS * 1e3
            line["fraction_of_floor_rate"] = FLOOR_MS * 1e3 / line["median_us"]
            line["TB_per_s"] = 2 * NQ * REC_BYTES / (line["median_us"] * 1e-6) / 1e12
        print(json.dumps(line))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
        kernels(sys.argv[2])
    else:
        drive(int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 7)
