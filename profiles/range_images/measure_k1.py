"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident KITTI-world scans of 64 x 1 875 pixels: the range-image sweep
(cc_ingest_ranges) on u32 millimetre and u16 2-mm words, without knots and with K = 32 knots by column, next to cc_ingest_batch on the
float4 cloud of the same pixels (the kernel every caller ran before) and next to what a caller did before -- a torch pass that expands
the words into a float4 cloud, de-skewing it by column on the way (timed with events), followed by cc_ingest_batch.  Every instance
warmed up, variants alternated, 7 repeats.
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, math, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
from point_layouts import rigid
cc = cc_amd.load()
N, REPS, K, H, W = 1024, 7, 32, 64, 1875
P = H * W
ORIGIN_N, ORIGIN_Z = 0.03, 0.04
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_range_images_kitti_world.jsonl")
world = cc.synth.World(kitti=True)
xyzi, _, _ = cc.synth.make_sequence(N, world=world, device="cuda")
assert xyzi.shape[1] == P
# the scans as range images: |p| in mm (u32) and in 2 mm (u16), 0 for a ray without a return (the caster parks it at 1 000 m)
rg = xyzi[:, :, :3].norm(dim=2)
rg = torch.where(rg > 500.0, torch.zeros_like(rg), rg)
w32 = torch.round(rg * 1000.0).to(torch.int32).reshape(-1).contiguous()
w16 = torch.round(rg * 500.0).to(torch.int32).to(torch.int16).reshape(-1).contiguous()   # below 2^16: reinterpreted as u16 by the library
no_return = float((w32 == 0).float().mean())
# the sensor's angles: the caster's own beam elevations and firing azimuths
dirs = cc.synth._ray_dirs(H, W, torch.device("cuda"), hdl64=getattr(world, "dense", False)).reshape(H, W, 3)
alt = torch.asin(dirs[:, 0, 2].double()).cpu().numpy()
az = np.arange(W) * (2 * math.pi / W)
del xyzi, rg, dirs
rng = np.random.default_rng(5)
knots = np.zeros((N, K, 3, 4), np.float32)    # D, E: a motion of 1 - 2 m and 2 - 4 degrees per sweep
for i in range(N):
    ang, dist, yaw = rng.uniform(-np.pi, np.pi), rng.uniform(1.0, 2.0), np.deg2rad(rng.uniform(2.0, 4.0))
    knots[i] = cc.motion_knots(rigid(yaw, t=(dist * np.cos(ang), dist * np.sin(ang), 0.0)), rigid(0.0), ref=1.0, K=K)
col_knot = (np.arange(W) * K // W).astype(np.int32)
ctx = cc.Context(0, max_batch=N)
mk = dict(beam_alt=alt, col_az=az, origin=(ORIGIN_N, ORIGIN_Z))
s32 = ctx.range_sensor(H, W, word="u32", range_scale=0.001, **mk)
s16 = ctx.range_sensor(H, W, word="u16", range_scale=0.002, **mk)
s32k = ctx.range_sensor(H, W, word="u32", range_scale=0.001, col_knot=col_knot, K=K, **mk)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
offs = np.arange(N + 1, dtype=np.int64) * P
# the torch pass: words -> float4, the header's formula; with knots every pixel is moved by the matrix of its column
row_tab, col_cs = cc.L.range_tables(alt, np.zeros(H), az)
rt, cs = torch.from_numpy(row_tab).cuda(), torch.from_numpy(col_cs).cuda()
ca, sa, co, so = (rt[:, i].reshape(1, H, 1) for i in range(4))
ce, se = (cs[:, i].reshape(1, 1, W) for i in range(2))
dx, dy = ce * co - se * so, se * co + ce * so
kn_cols = torch.from_numpy(np.ascontiguousarray(knots.reshape(N, K, 12)[:, col_knot])).cuda()   # [N, W, 12]: the matrix of every column
CH = 64   # scans per slice of the pass
NAN = float("nan")


def expand(words, scale, dst, with_knots):
    for s0 in range(0, N, CH):
        w = words[s0 * P:(s0 + CH) * P].reshape(CH, H, W)
        d = w.to(torch.float32) * scale - ORIGIN_N
        h = d * ca
        x, y, z = h * dx + ORIGIN_N * ce, h * dy + ORIGIN_N * se, d * sa + ORIGIN_Z
        if with_knots:
            m = kn_cols[s0:s0 + CH].reshape(CH, 1, W, 12)
            x, y, z = (((m[..., 4 * r] * x + m[..., 4 * r + 1] * y) + m[..., 4 * r + 2] * z) + m[..., 4 * r + 3] for r in range(3))
        q = dst[s0 * P:(s0 + CH) * P].reshape(CH, H, W, 4)
        q[..., 0] = torch.where(w == 0, torch.full_like(x, NAN), x)
        q[..., 1] = y
        q[..., 2] = z


q4_plain = torch.zeros((N * P, 4), dtype=torch.float32, device="cuda")   # A: the float4 cloud of the pixels, no knots
expand(w32, 0.001, q4_plain, False)
q4 = torch.zeros((N * P, 4), dtype=torch.float32, device="cuda")         # E: written anew by every repeat
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms = [0.0]


def expand_then_batch():
    ev[0].record()
    expand(w32, 0.001, q4, True)
    ev[1].record()
    ctx.ingest(q4, offs, out=out)
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])


variants = [("A cc_ingest_batch on the float4 cloud", lambda: ctx.ingest(q4_plain, offs, out=out)),
            ("B ranges u32, K = 0", lambda: ctx.ingest_ranges(s32, w32, out=out)),
            ("C ranges u16, K = 0", lambda: ctx.ingest_ranges(s16, w16, out=out)),
            ("D ranges u32, K = 32 by column", lambda: ctx.ingest_ranges(s32k, w32, knots=knots, out=out)),
            ("E torch pass words -> float4 with D's de-skew, then cc_ingest_batch", expand_then_batch)]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
# the same pixels, the same scene: how many descriptors agree byte for byte (the torch pass may contract multiply-adds, so not all must)
d_a = ctx.ingest(q4_plain, offs, out=torch.zeros_like(out)).clone()
d_b = ctx.ingest_ranges(s32, w32, out=torch.zeros_like(out)).clone()
d_d = ctx.ingest_ranges(s32k, w32, knots=knots, out=torch.zeros_like(out)).clone()
d_e = ctx.ingest(q4, offs, out=torch.zeros_like(out)).clone()
torch.cuda.synchronize()
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

    emit({"scans": N, "pixels": P, "no_return_share": round(no_return, 4), "bytes_u32": int(w32.numel() * 4), "bytes_u16": int(w16.numel() * 2),
          "bytes_float4": int(q4.numel() * 4)})
    emit({"check": "descriptors equal byte for byte", "B_vs_A": int((d_a == d_b).all(dim=1).sum()), "D_vs_E": int((d_d == d_e).all(dim=1).sum()), "scans": N})
    for r in range(REPS):
        for k, f in variants:
            pre_ms[0] = 0.0
            f()
            cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
            rows[k].append(ms[0] + pre_ms[0])
            if k[0] == "E":
                pre.append(pre_ms[0])
            emit({"rep": r, "variant": k, "k1_ms": round(ms[0], 4), "pass_before_ms": round(pre_ms[0], 4), "k2_ms": round(ms[1], 4),
                  "launches": nl.value, "scans": N, "pixels": P})
    for k, v in rows.items():
        emit({"variant": k, "total_ms_mean": round(float(np.mean(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v),
              "pass_before_ms_mean": round(float(np.mean(pre)), 4) if k[0] == "E" else 0.0})
    a = float(np.mean(rows[variants[0][0]]))
    floor = (w32.numel() * 4 + q4.numel() * 4) / 8e12 * 1e3 + a
    emit({"E_floor_ms": round(floor, 4), "what": "one read of the u32 words and one write of the float4 cloud at 8 TB/s, plus row A"})
    cc.lib().cc_profile_enable(ctx.h, 0)
