"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident 120 000-point KITTI-world scans: a scan from segments
(cc_ingest_segments) next to cc_ingest_points and next to what a caller did before -- a transform-and-concatenate pass (torch ops,
timed with events) followed by cc_ingest_batch.  Every instance warmed up, variants alternated, 7 repeats.  Then the per-scan loop:
cc_scan_ingest_segments (one scan, three segments) against cc_scan_ingest_points on Q, wall time to cc_scan_ready, 50 scans each.
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
from point_layouts import apply_tf, random_tfs
cc = cc_amd.load()
L = cc.L
N, REPS, S = 1024, 7, 3
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_segments_kitti_world.jsonl")
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
assert P == 120000
PS = P // S
x16 = xyzi.reshape(-1, 4).contiguous()
offs = np.arange(N + 1, dtype=np.int64) * P
tfs = random_tfs(N, seed=3, max_tilt_deg=3.0, max_shift=2.0)              # A, B: one matrix per scan
tf3 = random_tfs(N * S, seed=4, max_tilt_deg=3.0, max_shift=2.0).reshape(N, S, 12)  # C, D, E: one per segment
# D: the three sensors' records in three allocations of their own, 12- / 16- / 32-byte records
parts = x16.view(N, S, PS, 4)
d12 = parts[:, 0, :, :3].contiguous()
d16 = parts[:, 1].contiguous()
d32 = torch.full((N, PS, 8), float("nan"), dtype=torch.float32, device="cuda")
d32[:, :, :3] = parts[:, 2, :, :3]
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
one = [[(x16[i * P:(i + 1) * P], (16, 0), tfs[i])] for i in range(N)]
three = [[(x16[i * P + s * PS:i * P + (s + 1) * PS], (16, 0), tf3[i, s]) for s in range(S)] for i in range(N)]
three_alloc = [[(d12[i], (12, 0), tf3[i, 0]), (d16[i], (16, 0), tf3[i, 1]), (d32[i], (32, 0), tf3[i, 2])] for i in range(N)]
# E: what a caller did for C before: transform every segment, write the concatenated cloud as float4 records, cc_ingest_batch
Rt = torch.from_numpy(np.ascontiguousarray(tf3.reshape(N * S, 3, 4)[:, :, :3].transpose(0, 2, 1))).cuda()
tt = torch.from_numpy(np.ascontiguousarray(tf3.reshape(N * S, 3, 4)[:, :, 3])).cuda()
q4 = torch.zeros((N * S, PS, 4), dtype=torch.float32, device="cuda")
src = x16.view(N * S, PS, 4)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms = [0.0]


def concat_then_batch():
    ev[0].record()
    q4[:, :, :3] = torch.baddbmm(tt[:, None, :], src[:, :, :3], Rt)
    ev[1].record()
    ctx.ingest(q4.view(-1, 4), offs, out=out)
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])


variants = [("A cc_ingest_points {16,0}+tf", lambda: ctx.ingest(x16, offs, out=out, layout=(16, 0), tf=tfs)),
            ("B segments: one per scan", lambda: ctx.ingest_segments(one, out=out)),
            ("C segments: 3 x 40000, one buffer", lambda: ctx.ingest_segments(three, out=out)),
            ("D segments: 3 allocations {12,0} {16,0} {32,0}", lambda: ctx.ingest_segments(three_alloc, out=out)),
            ("E torch transform+concat, then cc_ingest_batch", concat_then_batch)]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
cc.lib().cc_profile_enable(ctx.h, 1)
ms, nl = (C.c_double * 2)(), C.c_int()
rows = {k: [] for k, _ in variants}
pre = []
with open(OUT, "w") as fo:
    def emit(rec):
        line = json.dumps(rec)
        fo.write(line + "\n")
        print(line, flush=True)

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

    # ---- the per-scan loop ----
    lib = cc.lib()
    lib.cc_scan_ingest_points.restype = lib.cc_scan_ready.restype = lib.cc_scan_release.restype = C.c_int
    lib.cc_scan_ready.argtypes = lib.cc_scan_release.argtypes = [C.c_void_p]
    NL = 50
    host = xyzi[:NL].cpu().numpy()
    lay16 = L.PointLayout(16, 0)
    segs, qs = [], []
    for i in range(NL):
        arr = (L.PointSegment * S)()
        bufs = [np.ascontiguousarray(host[i, s * PS:(s + 1) * PS]) for s in range(S)]
        for s in range(S):
            arr[s].points, arr[s].n_points, arr[s].layout, arr[s].has_tf = bufs[s].ctypes.data, PS, lay16, 1
            arr[s].tf[:] = tf3[i, s].tolist()
        segs.append((arr, bufs))
        qs.append(np.ascontiguousarray(np.concatenate([apply_tf(bufs[s], tf3[i, s]) for s in range(S)], 0)))

    def timed(call):
        sc = C.c_void_p()
        t0 = time.perf_counter()
        rc = call(sc)
        assert rc == 0, lib.cc_last_error()
        while lib.cc_scan_ready(sc) == 0:
            pass
        dt = time.perf_counter() - t0
        lib.cc_scan_release(sc)
        return dt * 1e3

    f_seg = lambda i: timed(lambda sc: lib.cc_scan_ingest_segments(ctx.h, C.addressof(segs[i][0]), S, 0, C.byref(sc)))
    f_pts = lambda i: timed(lambda sc: lib.cc_scan_ingest_points(ctx.h, qs[i].ctypes.data, C.addressof(lay16), P, None, 0, C.byref(sc)))
    for i in range(4):
        f_seg(i), f_pts(i)
    t_seg, t_pts = [], []
    for i in range(NL):
        t_seg.append(f_seg(i))
        t_pts.append(f_pts(i))
    emit({"per_scan_loop": "wall ms to cc_scan_ready, %d scans each, alternated" % NL,
          "cc_scan_ingest_segments (3 segments)": {"median": round(float(np.median(t_seg)), 4), "mean": round(float(np.mean(t_seg)), 4)},
          "cc_scan_ingest_points on Q": {"median": round(float(np.median(t_pts)), 4), "mean": round(float(np.mean(t_pts)), 4)}})
