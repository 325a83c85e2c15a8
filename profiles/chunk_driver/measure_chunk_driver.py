"""The launch chains of every chunked submit, to compare two builds of the library: a 40-scan database, two lanes, and one call of
each form with 3 items (one chunk that writes its results through pinned memory) and with 70 (a copied chunk of 64 and a small one
of 6): plain, ranked and ranked-detail query, verify, ranked verify, poses with tries and curvature, poses without refinement, a
hint check -- then the query forms again with the dynamic thresholds on.  Prints one line per call with a digest of what it
returned, so two builds can be compared by their answers as well.

  drive:    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv json -d DIR -o r -- \\
                python profiles/chunk_driver/measure_chunk_driver.py            (CC_AMD_LIB=<other build> for the other side)
  extract:  python profiles/chunk_driver/measure_chunk_driver.py --lists DIR > lists.txt
            per hardware queue (numbered in the order they first appear) the ordered (kernel, grid, workgroup) of its launches,
            then the ordered (direction, bytes) of the copies.  The runtime runs most of the chains' copies (pinned host memory on
            one side) as blit kernels: those are the __amd_rocclr_copyBuffer rows of the queue lists, their grid set by the
            size; the copy rows are the transfers it handed to a copy engine (bytes: from the JSON records, the CSV has none)."""
import csv
import glob
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def flat(x):
    """the arrays of a call's return value, in order"""
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in flat(y)]
    return [x]


def drive():
    import torch
    import cc_amd
    cc = cc_amd.load()
    L = cc.L
    n_db, n_q = 40, 70
    dcfg = L.default_db_cfg()
    dcfg.max_elapse, dcfg.min_elapse = 2.5, 1.5  # a short loop and a short delay: revisits within a few dozen scans
    xyzi, poses, ts = cc.synth.make_sequence(n_db + n_q, world=cc.synth.World(loop_len=40.0), device="cuda", beams=32, azim=900)
    ctx = cc.Context(0, max_batch=n_db + n_q)
    desc = ctx.ingest(xyzi.reshape(-1, 4), np.arange(n_db + n_q + 1, dtype=np.int64) * xyzi.shape[1])
    db = cc.Database(ctx, dcfg, capacity=n_db)
    db.set_lanes(2)
    db.add_scans(desc[:n_db], np.asarray(ts)[:n_db], np.arange(n_db, dtype=np.int32))
    torch.cuda.synchronize()

    def say(name, n, out):
        print("%-28s n=%-3d %s" % (name, n, digest(*flat(out))), flush=True)

    def queries(tag):
        for n in (3, 70):
            q, ep = desc[n_db:n_db + n], np.full(n, n_db, np.int32)
            say(tag + "query", n, db.query(q, ep))
            say(tag + "query_ranked", n, db.query(q, ep, ranked=8))
            say(tag + "query_ranked_detail", n, db.query(q, ep, ranked=8, detail=True))

    queries("")
    hints = None
    for n in (3, 70):
        qs = np.arange(n_db, n_db + n, dtype=np.int32)
        lists = [[int(q) % n_db, (int(q) + 1) % n_db] for q in qs]
        res, hl = db.verify(desc, lists, qidx=qs, want_hints=True)
        say("verify", n, res)
        if hints is None:
            hints = next(((int(qs[i]), h) for i, h in enumerate(hl) if len(h)), None)
        say("verify_ranked", n, db.verify(desc, lists, qidx=qs, ranked=8))
        g = np.array([l[0] for l in lists], np.int32)
        tf = np.zeros((n, 3))
        tries = tf[:, None, :] + np.linspace(-1.0, 1.0, 4)[None, :, None] * np.array([1.0, 1.0, 0.01])
        say("pose_tries_curvature", n, db.score_poses(desc, qs, g, tf, refine=True, min_corr=float("-inf"), tries=tries, curvature=True))
        say("pose_no_refine", n, db.score_poses(desc, qs, g, tf, refine=False))
    assert hints is not None, "no verify item of the drive has a hint: nothing to run the hint check on"
    say("check_hints", 1, db.check_hints(desc[hints[0]], hints[1]))
    db.set_dynamic_thres(True)
    queries("dyn_")
    torch.cuda.synchronize()
    db.close()
    ctx.close()


def lists(d):
    def rows(pat):
        fs = sorted(glob.glob(os.path.join(d, "**", pat), recursive=True))
        return [r for f in fs for r in csv.DictReader(open(f))]

    def dims(r, k):
        return "x".join(r[k + s] for s in ("_X", "_Y", "_Z")) if k + "_X" in r else r[k]

    per_q, order = {}, []
    for r in sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"])):
        q = (r.get("Agent_Id"), r.get("Queue_Id"))
        if q not in per_q:
            per_q[q] = []
            order.append(q)
        name = r["Kernel_Name"]
        per_q[q].append("%s grid %s wg %s" % (name.split("(")[0] if "cc_k_" in name else name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size")))
    for i, q in enumerate(order):
        print("== queue %d: %d launches" % (i, len(per_q[q])))
        print("\n".join(per_q[q]))
    cp = sorted(rows("*memory_copy_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))

    def find(x, key):  # the lists under `key`, wherever the JSON keeps them
        if isinstance(x, dict):
            return [v for k, v in x.items() if k == key and isinstance(v, list)] + [f for v in x.values() for f in find(v, key)]
        return [f for v in x for f in find(v, key)] if isinstance(x, list) else []

    recs = [c for f in sorted(glob.glob(os.path.join(d, "**", "*results.json"), recursive=True)) for l in find(json.load(open(f)), "memory_copy") for c in l]
    recs.sort(key=lambda c: int(c.get("start_timestamp", 0)))
    print("== copies: %d" % len(cp))
    for i, r in enumerate(cp):
        print("%s %s" % (r.get("Direction", "?"), recs[i].get("bytes", "?") if len(recs) == len(cp) else "?"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--lists":
        lists(sys.argv[2])
    else:
        drive()
