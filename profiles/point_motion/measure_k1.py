"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident 120 000-point KITTI-world scans in 16-byte records whose fourth
word is the point's time: the de-skewing sweep (cc_ingest_points_motion) next to cc_ingest_points with one matrix per scan and next
to what a caller did before -- a torch pass that picks each point's matrix, moves the point and writes a float4 copy (timed with
events), followed by cc_ingest_batch.  Every instance warmed up, variants alternated, 7 repeats.
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
from point_layouts import rigid
cc = cc_amd.load()
N, REPS, K = 1024, 7, 32
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_motion_kitti_world.jsonl")
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
assert P == 120000
SWEEP = 0.1
# the time of a point within its sweep, in the record's fourth word: rising with the azimuth (C), random (D)
az = ((torch.atan2(xyzi[:, :, 1], xyzi[:, :, 0]) + np.pi) / (2 * np.pi)).clamp_(0.0, 0.999999)
x_az = xyzi.clone()
x_az[:, :, 3] = az * SWEEP
x_rnd = xyzi.clone()
x_rnd[:, :, 3] = torch.rand((N, P), device="cuda") * SWEEP
x_az, x_rnd = x_az.reshape(-1, 4).contiguous(), x_rnd.reshape(-1, 4).contiguous()
del az
offs = np.arange(N + 1, dtype=np.int64) * P
rng = np.random.default_rng(5)
knots = np.zeros((N, K, 3, 4), np.float32)                                         # C, D, E: a motion of 1 - 2 m and 2 - 4 degrees per sweep
for i in range(N):
    ang, dist, yaw = rng.uniform(-np.pi, np.pi), rng.uniform(1.0, 2.0), np.deg2rad(rng.uniform(2.0, 4.0))
    knots[i] = cc.motion_knots(rigid(yaw, t=(dist * np.cos(ang), dist * np.sin(ang), 0.0)), rigid(0.0), ref=1.0, K=K)
tfs = np.ascontiguousarray(knots[:, K // 2].reshape(N, 12))                        # A, B: one matrix per scan -- the sweep's middle knot, so that
#                                                                                    every row rasterises the same scene up to the de-skew itself
tb, sc = np.zeros(N, np.float32), np.full(N, np.float32(K) / np.float32(SWEEP), np.float32)
sc1 = np.full(N, np.float32(1.0) / np.float32(SWEEP), np.float32)
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
# E: gather a matrix per point, move the point, write a float4 copy; then cc_ingest_batch
kn_d = torch.from_numpy(knots.reshape(N * K, 12)).cuda()
scan_base = (torch.arange(N, device="cuda", dtype=torch.int64) * K).repeat_interleave(P)
q4 = torch.zeros((N * P, 4), dtype=torch.float32, device="cuda")
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms = [0.0]
CH = 64   # scans per slice of the pass: the gathered matrices of all 1 024 scans at once would be 5.9 GB


def deskew_then_batch():
    ev[0].record()
    for s0 in range(0, N, CH):
        sl = slice(s0 * P, (s0 + CH) * P)
        src = x_az[sl]
        b = (src[:, 3] * float(sc[0])).clamp_(0.0, K - 1).to(torch.int64) + scan_base[sl]
        m = kn_d[b]                                                            # [points, 12]
        for r in range(3):
            q4[sl, r] = ((m[:, 4 * r] * src[:, 0] + m[:, 4 * r + 1] * src[:, 1]) + m[:, 4 * r + 2] * src[:, 2]) + m[:, 4 * r + 3]
    ev[1].record()
    ctx.ingest(q4, offs, out=out)
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])


variants = [("A cc_ingest_points {16,0}+tf", lambda: ctx.ingest(x_az, offs, out=out, layout=(16, 0), tf=tfs)),
            ("B motion, K = 1", lambda: ctx.ingest(x_az, offs, out=out, layout=(16, 0), motion=(12, "f32"), t_begin=tb, scale=sc1, knots=tfs.reshape(N, 1, 12))),
            ("C motion, K = 32, times rising with azimuth", lambda: ctx.ingest(x_az, offs, out=out, layout=(16, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots)),
            ("D motion, K = 32, random times", lambda: ctx.ingest(x_rnd, offs, out=out, layout=(16, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots)),
            ("E torch per-point de-skew into float4, then cc_ingest_batch", deskew_then_batch)]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
# C and E rasterise the same points: the fused sweep and the torch pass agree (the torch pass may contract multiply-adds, so not bitwise)
d_c = ctx.ingest(x_az, offs, out=torch.zeros_like(out), layout=(16, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots)
d_e = ctx.ingest(q4, offs, out=torch.zeros_like(out))
torch.cuda.synchronize()
same = int((d_c == d_e).all(dim=1).sum())
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

    emit({"check": "descriptors of C equal those of E's float4 copy, bytes", "equal_scans": same, "scans": N})
    for r in range(REPS):
        for k, f in variants:
            pre_ms[0] = 0.0
            f()
            cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
            rows[k].append(ms[0] + pre_ms[0])
            if k[0] == "E":
                pre.append(pre_ms[0])
            emit({"rep": r, "variant": k, "k1_ms": round(ms[0], 4), "pass_before_ms": round(pre_ms[0], 4), "k2_ms": round(ms[1], 4),
                  "launches": nl.value, "scans": N, "points": P})
    for k, v in rows.items():
        emit({"variant": k, "total_ms_mean": round(float(np.mean(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v),
              "pass_before_ms_mean": round(float(np.mean(pre)), 4) if k[0] == "E" else 0.0})
    cc.lib().cc_profile_enable(ctx.h, 0)
