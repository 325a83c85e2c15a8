"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident 120 000-point KITTI-world scans, quantised to 2^-10 m and shifted
into a georeferenced frame (an origin per scan near (448 000, 5 412 000, 300)): the typed-coordinate sweep (cc_ingest_coords) on
f64 [N, 3], f64 columns, scaled-i32 12-byte records and f32 columns, next to cc_ingest_points on the packed f32 xyz and next to what
such a caller did before -- a torch pass (X - O[scan of point]).float() into a packed buffer (timed with events), followed by
cc_ingest_points.  Every input is 1.5 - 3 GB, streamed once per call: none is cache-resident.  Every instance warmed up, variants
alternated, 7 repeats.
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
cc = cc_amd.load()
N, REPS = 1024, 7
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_coords_kitti_world.jsonl")
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
assert P == 120000
local = (torch.round(xyzi[:, :, :3].double() * 1024.0) / 1024.0 + 0.0).contiguous()            # [N, P, 3] f64 on the 2^-10 lattice
del xyzi
g = torch.Generator(device="cuda").manual_seed(5)
O = torch.tensor([448000.0, 5412000.0, 300.0], dtype=torch.float64, device="cuda") + \
    torch.round(torch.rand((N, 3), device="cuda", generator=g, dtype=torch.float64) * 1000.0 * 1024.0) / 1024.0 - 500.0
O_host = O.cpu().numpy()
x_f32 = local.float().reshape(-1, 3).contiguous()                                                # A: packed f32 xyz, 12 B per point
assert bool((x_f32.double() == local.reshape(-1, 3)).all())
x_f64 = (local + O[:, None, :]).reshape(-1, 3).contiguous()                                      # B: f64 [N * P, 3], 24 B per point
cols_f64 = tuple(x_f64[:, k].contiguous() for k in range(3))                                     # C: three f64 columns
file_off = torch.tensor([448000.0, 5412000.0, 0.0], dtype=torch.float64, device="cuda")
las_origin = O - file_off                                                                        # D: LAS -- the call's origin folds the file offset in
x_i32 = torch.round((local + las_origin[:, None, :]) / 0.001).to(torch.int32).reshape(-1, 3).contiguous()
las_origin_host = las_origin.cpu().numpy()
cols_f32 = tuple(x_f32[:, k].contiguous() for k in range(3))                                     # E: three f32 columns
del local
offs = np.arange(N + 1, dtype=np.int64) * P
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms = [0.0]
packed = torch.empty((N * P, 3), dtype=torch.float32, device="cuda")


def pass_then_points():
    """what a caller does today: subtract the scan's origin in f64, narrow, write a packed f32 copy; then cc_ingest_points"""
    ev[0].record()
    packed.view(N, P, 3).copy_(x_f64.view(N, P, 3) - O[:, None, :])   # (the f64 difference is a temporary of its own: 2.9 GB written and read again)
    ev[1].record()
    ctx.ingest(packed, offs, out=out, layout=(12, 0))
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])


variants = [("A cc_ingest_points on packed f32 xyz {12,0}", lambda: ctx.ingest(x_f32, offs, out=out, layout=(12, 0))),
            ("B f64 [N,3] with an origin per scan", lambda: ctx.ingest_coords(x_f64, offs, origin=O_host, out=out)),
            ("C f64 columns with an origin per scan", lambda: ctx.ingest_coords(cols_f64, offs, origin=O_host, out=out)),
            ("D i32 12-byte records, scale 0.001, origin", lambda: ctx.ingest_coords(x_i32, offs, origin=las_origin_host, scale=0.001, out=out)),
            ("E f32 columns", lambda: ctx.ingest_coords(cols_f32, offs, out=out)),
            ("F torch (X - O).float() into a packed buffer, then cc_ingest_points", pass_then_points)]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
# A, B, C, E and F rasterise the same f32 points: the same bytes
ref = ctx.ingest(x_f32, offs, out=torch.zeros_like(out), layout=(12, 0)).clone()
same = {}
for k, f in (("B", lambda o: ctx.ingest_coords(x_f64, offs, origin=O_host, out=o)), ("C", lambda o: ctx.ingest_coords(cols_f64, offs, origin=O_host, out=o)),
             ("E", lambda o: ctx.ingest_coords(cols_f32, offs, out=o))):
    d = f(torch.zeros_like(out))
    torch.cuda.synchronize()
    same[k] = int((d == ref).all(dim=1).sum())
pass_then_points()
torch.cuda.synchronize()
same["F packed copy equals A's input"] = bool((packed == x_f32).all())
del ref
cc.lib().cc_profile_enable(ctx.h, 1)
ms, nl = (C.c_double * 2)(), C.c_int()
cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
rows = {k: [] for k, _ in variants}
pre = []
with open(OUT, "w") as fo:
    def emit(rec):
        line = json.dumps(rec)
        fo.write(line + "\n")
        print(line, flush=True)

    emit({"check": "descriptors equal A's, bytes (scans of %d)" % N, "equal": same})
    for r in range(REPS):
        for k, f in variants:
            pre_ms[0] = 0.0
            f()
            torch.cuda.synchronize()
            cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
            rows[k].append(ms[0] + pre_ms[0])
            if k[0] == "F":
                pre.append(pre_ms[0])
            emit({"rep": r, "variant": k, "k1_ms": round(ms[0], 4), "pass_before_ms": round(pre_ms[0], 4), "k2_ms": round(ms[1], 4), "launches": nl.value,
                  "scans": N, "points": P})
    for k, v in rows.items():
        emit({"variant": k, "total_ms_median": round(float(np.median(v)), 4), "total_ms_mean": round(float(np.mean(v)), 4), "min": round(min(v), 4),
              "max": round(max(v), 4), "reps": len(v), "pass_before_ms_mean": round(float(np.mean(pre)), 4) if k[0] == "F" else 0.0})
    # F's floor: one read of the f64 cloud and one write of the f32 cloud at the HBM's peak (8 TB/s), then row A's sweep
    read_b, write_b = N * P * 24, N * P * 12
    floor_ms = (read_b + write_b) / 8e12 * 1e3
    a = float(np.median(rows[variants[0][0]]))
    emit({"floor_of_F": "one read of the f64 cloud + one write of the f32 cloud at 8 TB/s, + row A's median", "bytes_read": read_b, "bytes_written": write_b,
          "pass_floor_ms": round(floor_ms, 4), "floor_ms": round(floor_ms + a, 4), "B_ms_median": round(float(np.median(rows[variants[1][0]])), 4),
          "B_over_A": round(float(np.median(rows[variants[1][0]])) / a, 3)})
    cc.lib().cc_profile_enable(ctx.h, 0)
