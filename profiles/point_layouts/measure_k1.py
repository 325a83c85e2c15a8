"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident 120 000-point scans, per point layout / transform; variants alternated."""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
from point_layouts import random_tfs
cc = cc_amd.load()
N, REPS = 1024, 7
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
assert P == 120000
x16 = xyzi.reshape(-1, 4).contiguous()
x12 = x16[:, :3].contiguous()
x32 = torch.full((N * P, 8), float("nan"), dtype=torch.float32, device="cuda")
x32[:, :3] = x12
offs = np.arange(N + 1, dtype=np.int64) * P
tfs = random_tfs(N, seed=3, max_tilt_deg=3.0, max_shift=2.0)
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
variants = [("float4 (cc_ingest_batch)", lambda: ctx.ingest(x16, offs, out=out)),
            ("{16,0}+tf", lambda: ctx.ingest(x16, offs, out=out, layout=(16, 0), tf=tfs)),
            ("{12,0}", lambda: ctx.ingest(x12, offs, out=out, layout=(12, 0))),
            ("{12,0}+tf", lambda: ctx.ingest(x12, offs, out=out, layout=(12, 0), tf=tfs)),
            ("{32,0}", lambda: ctx.ingest(x32, offs, out=out, layout=(32, 0)))]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
cc.lib().cc_profile_enable(ctx.h, 1)
ms, nl = (C.c_double * 2)(), C.c_int()
rows = {k: [] for k, _ in variants}
with open("k1_layouts.jsonl", "w") as fo:
    for r in range(REPS):
        for k, f in variants:
            f()
            cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
            rows[k].append(ms[0])
            line = json.dumps({"rep": r, "variant": k, "k1_ms": round(ms[0], 4), "k2_ms": round(ms[1], 4), "launches": nl.value, "scans": N, "points": P})
            fo.write(line + "\n")
            print(line, flush=True)
    for k, v in rows.items():
        line = json.dumps({"variant": k, "k1_ms_mean": round(float(np.mean(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v)})
        fo.write(line + "\n")
        print(line, flush=True)
