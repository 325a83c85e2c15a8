"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident 120 000-point KITTI-world scans in 32-byte records (x, y, z, the
point's time as f32 at 12, a SemanticKITTI-style label as u32 at 16): the rig sweep (cc_ingest_rig) next to the de-skewing sweep it
carries further (cc_ingest_points_motion) and next to what a caller of two sensors did before -- a torch pass that de-skews every
point by the matrix of its time bin, masks the moving classes, and writes the kept points of both sensors as one float4 cloud (timed
with events), followed by cc_ingest_batch.  Every instance warmed up, variants alternated, 7 repeats.
  A  cc_ingest_points_motion, K = 32
  B  cc_ingest_rig, one motion segment per scan, no rule
  C  B with the class rule (7 % of the records dropped, in runs of 20 - 60)
  D  two sensors of 60 000 points in tensors of their own, 16 knots each on one pool of 32, class rule
  E  the torch pass for D's inputs, then cc_ingest_batch; its floor = one read of the records and one write of the kept points at
     8 TB/s plus row A's sweep
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
from point_layouts import rigid
cc = cc_amd.load()
N, REPS, K, STRIDE = 1024, 7, 32, 32
HBM_BYTES_PER_MS = 8.0e9   # 8 TB/s
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_rig_kitti_world.jsonl")
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
assert P == 120000
H = P // 2
SWEEP = 0.1
rng = np.random.default_rng(5)
# labels of one scan, used by all: static classes 0 .. 99, 7 % moving (252 .. 259) in runs of 20 - 60 records, an instance id in the high half
cls = rng.integers(0, 100, P).astype(np.uint32)
moving = np.zeros(P, bool)
while moving.sum() < 0.07 * P:
    a = int(rng.integers(0, P))
    moving[a:a + int(rng.integers(20, 60))] = True
cls[moving] = rng.integers(252, 260, int(moving.sum())).astype(np.uint32)
lab = torch.from_numpy(((rng.integers(1, 2 ** 16, P).astype(np.uint32) << np.uint32(16)) | cls).view(np.int32)).cuda()
rec = torch.zeros((N, P, STRIDE // 4), dtype=torch.float32, device="cuda")
rec[:, :, :3] = xyzi[:, :, :3]
rec[:, :, 3] = ((torch.atan2(xyzi[:, :, 1], xyzi[:, :, 0]) + np.pi) / (2 * np.pi)).clamp_(0.0, 0.999999) * SWEEP   # the time: rising with the azimuth
rec.view(torch.int32)[:, :, 4] = lab
del xyzi
rec_a, rec_b = rec[:, :H].contiguous(), rec[:, H:].contiguous()   # D: the two sensors' buffers
rec = rec.reshape(N * P, STRIDE // 4)
offs = np.arange(N + 1, dtype=np.int64) * P
knots = np.zeros((N, K, 3, 4), np.float32)   # a motion of 1 - 2 m and 2 - 4 degrees per sweep
for i in range(N):
    ang, dist, yaw = rng.uniform(-np.pi, np.pi), rng.uniform(1.0, 2.0), np.deg2rad(rng.uniform(2.0, 4.0))
    knots[i] = cc.motion_knots(rigid(yaw, t=(dist * np.cos(ang), dist * np.sin(ang), 0.0)), rigid(0.0), ref=1.0, K=K)
tb, sc = np.zeros(N, np.float32), np.full(N, np.float32(K) / np.float32(SWEEP), np.float32)
sc16 = float(np.float32(16) / np.float32(SWEEP))
keep = cc.PointFilter.classes(0, "u32", drop=range(252, 260), mask=0xFFFF)
M = cc.SegMotion
one = [[(rec[i * P:(i + 1) * P], (STRIDE, 0), M(12, "f32", 0.0, float(sc[0]), 0, K), None)] for i in range(N)]
one_f = [[(t, lay, m, 16) for (t, lay, m, _k) in s] for s in one]
two = [[(rec_a[i], (STRIDE, 0), M(12, "f32", 0.0, sc16, 0, 16), 16), (rec_b[i], (STRIDE, 0), M(12, "f32", 0.0, sc16, 16, 16), 16)] for i in range(N)]
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
# E: per sensor gather a matrix per point, move the point, test its class; write the kept points of both sensors as one float4 cloud
kn_d = torch.from_numpy(knots.reshape(N * K, 12)).cuda()
q4 = torch.zeros((N, P, 4), dtype=torch.float32, device="cuda")
kept = torch.zeros((N, P), dtype=torch.bool, device="cuda")
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms, kept_pts = [0.0], [0]
CH = 64   # scans per slice of the pass: the gathered matrices of all 1 024 scans at once would be 5.9 GB


def torch_pass_then_batch():
    ev[0].record()
    for s0 in range(0, N, CH):
        base = (torch.arange(s0, s0 + CH, device="cuda", dtype=torch.int64) * K)[:, None]
        for src, k0, cols in ((rec_a[s0:s0 + CH], 0, slice(0, H)), (rec_b[s0:s0 + CH], 16, slice(H, P))):
            b = (src[:, :, 3] * sc16).clamp_(0.0, 15.0).to(torch.int64) + (base + k0)
            m = kn_d[b]                                                            # [scans, points, 12]
            for r in range(3):
                q4[s0:s0 + CH, cols, r] = ((m[:, :, 4 * r] * src[:, :, 0] + m[:, :, 4 * r + 1] * src[:, :, 1]) + m[:, :, 4 * r + 2] * src[:, :, 2]) + m[:, :, 4 * r + 3]
            c = src.view(torch.int32)[:, :, 4] & 0xFFFF
            kept[s0:s0 + CH, cols] = (c < 252) | (c > 259)
    q = q4[kept]                                                                   # the concatenated cloud of the kept points, scan after scan
    o = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    o[1:] = kept.sum(1).cumsum(0)
    ev[1].record()
    oh = o.cpu().numpy()
    ctx.ingest(q, oh, out=out)
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])
    kept_pts[0] = int(oh[-1])
    return q, oh


variants = [("A cc_ingest_points_motion, K = 32", lambda: ctx.ingest(rec, offs, out=out, layout=(STRIDE, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots)),
            ("B rig, one motion segment, no rule", lambda: ctx.ingest_rig(one, knots=knots, out=out)),
            ("C rig, one motion segment, class rule", lambda: ctx.ingest_rig(one_f, knots=knots, keep=keep, out=out)),
            ("D rig, two sensors of 60 000, 16 knots each, class rule", lambda: ctx.ingest_rig(two, knots=knots, keep=keep, out=out)),
            ("E torch de-skew + mask + concatenate, then cc_ingest_batch", torch_pass_then_batch)]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
# D and E rasterise the same points: the fused sweep and the torch pass agree (the torch pass may contract multiply-adds, so not bitwise);
# A and B are the same sweep by two kernels: bytes
d_d = ctx.ingest_rig(two, knots=knots, keep=keep, out=torch.zeros_like(out)).clone()
q, oh = torch_pass_then_batch()
d_e = ctx.ingest(q, oh, out=torch.zeros_like(out)).clone()
d_a = ctx.ingest(rec, offs, out=torch.zeros_like(out), layout=(STRIDE, 0), motion=(12, "f32"), t_begin=tb, scale=sc, knots=knots).clone()
d_b = ctx.ingest_rig(one, knots=knots, out=torch.zeros_like(out)).clone()
torch.cuda.synchronize()
same_de, same_ab = int((d_d == d_e).all(dim=1).sum()), int((d_a == d_b).all(dim=1).sum())
del q
cc.lib().cc_profile_enable(ctx.h, 1)
ms, nl = (C.c_double * 2)(), C.c_int()
cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
rows = {k: [] for k, _ in variants}
pre = []
with open(OUT, "w") as fo:
    def emit(r):
        line = json.dumps(r)
        fo.write(line + "\n")
        print(line, flush=True)

    emit({"check": "descriptors of D equal those of E's float4 cloud, bytes", "equal_scans": same_de, "scans": N})
    emit({"check": "descriptors of B equal those of A, bytes", "equal_scans": same_ab, "scans": N})
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
    mean = {}
    for k, v in rows.items():
        mean[k[0]] = float(np.mean(v))
        emit({"variant": k, "total_ms_mean": round(mean[k[0]], 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v),
              "pass_before_ms_mean": round(float(np.mean(pre)), 4) if k[0] == "E" else 0.0})
    read_b, write_b = N * P * STRIDE, kept_pts[0] * 16
    floor = (read_b + write_b) / HBM_BYTES_PER_MS + mean["A"]
    emit({"floor_of_E_ms": round(floor, 4), "read_bytes": read_b, "write_bytes": write_b, "hbm_bytes_per_ms": HBM_BYTES_PER_MS, "A_ms": round(mean["A"], 4),
          "D_ms": round(mean["D"], 4), "D_under_the_floor": bool(mean["D"] < floor)})
    cc.lib().cc_profile_enable(ctx.h, 0)
