"""K1 alone (cc_profile_enable / cc_profile_read) on 1 024 resident 120 000-point KITTI-world scans in 16-byte records whose fourth
word is a label: the filtered sweep (cc_ingest_points_filtered) next to cc_ingest_points without a filter and next to what a caller
did before -- a torch boolean-mask compaction of the records into a float4 buffer (timed with events, the read-back of the per-scan
counts included: the compacted call needs its offsets), followed by cc_ingest_batch.  Every instance warmed up, variants alternated,
7 repeats.
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
cc = cc_amd.load()
N, REPS, RUN = 1024, 7, 100
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_filter_kitti_world.jsonl")
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
assert P == 120000 and P % RUN == 0
# the label word (SemanticKITTI: class in the low 16 bits, an instance id in the high 16).  Moving objects are runs of neighbouring
# firings: 7 % of the runs of 100 consecutive records are of classes 252 .. 259, everything else of classes 0 .. 99
g = torch.Generator(device="cuda").manual_seed(5)
cls = torch.randint(0, 100, (N, P), device="cuda", generator=g, dtype=torch.int32)
moving_run = torch.rand((N, P // RUN), device="cuda", generator=g) < 0.07
moving = moving_run.repeat_interleave(RUN, dim=1)
cls = torch.where(moving, torch.randint(252, 260, (N, P), device="cuda", generator=g, dtype=torch.int32), cls)
label = cls | (torch.randint(1, 1 << 15, (N, P), device="cuda", generator=g, dtype=torch.int32) << 16)
x_lab = xyzi.clone()
x_lab[:, :, 3] = label.view(torch.float32)
x_lab = x_lab.reshape(-1, 4).contiguous()
x_int = xyzi.clone()                                   # D: an intensity in [0, 1) in the fourth word, the lowest 7 % dropped
x_int[:, :, 3] = torch.rand((N, P), device="cuda", generator=g)
x_int = x_int.reshape(-1, 4).contiguous()
share = float(moving.float().mean())
del cls, moving, moving_run, label
offs = np.arange(N + 1, dtype=np.int64) * P
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
keep_all = cc.PointFilter.classes(12, "u32", drop=[], n_classes=260, mask=0xFFFF)
keep_static = cc.PointFilter.classes(12, "u32", drop=range(252, 260), mask=0xFFFF)
keep_band = cc.PointFilter.range(12, 0.07, 1.0)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms = [0.0]
kept_pts = [0]


CH = 64   # scans per slice of the gather.  (One boolean-mask index over all 1 024 scans, x_lab[m], returned wrong rows from scan 422 on
#           with the torch build this was first run with -- the byte check below caught it; 64 scans are 7.7 M records per gather.)
q4_buf = torch.empty((N * P, 4), dtype=torch.float32, device="cuda")


def compact():
    """what a caller does today: mask, per-scan counts (read back: they become the call's offsets), gather into a float4 copy"""
    lab = x_lab[:, 3].view(torch.int32) & 0xFFFF
    m = (lab < 252) | (lab >= 260)
    cnt = m.view(N, P).sum(1).cpu().numpy()
    o = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    for s0 in range(0, N, CH):
        sl = slice(s0 * P, (s0 + CH) * P)
        torch.index_select(x_lab[sl], 0, m[sl].nonzero().squeeze(1), out=q4_buf[o[s0]:o[s0 + CH]])
    return q4_buf[:o[-1]], o


def compact_then_batch():
    ev[0].record()
    q4, o = compact()
    ev[1].record()
    ctx.ingest(q4, o, out=out)
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])
    kept_pts[0] = int(o[-1])


variants = [("A cc_ingest_points {16,0}, no filter", lambda: ctx.ingest(x_lab, offs, out=out, layout=(16, 0))),
            ("B class filter, everything kept", lambda: ctx.ingest(x_lab, offs, out=out, layout=(16, 0), keep=keep_all)),
            ("C class filter, moving classes dropped", lambda: ctx.ingest(x_lab, offs, out=out, layout=(16, 0), keep=keep_static)),
            ("D range rule on an f32 word", lambda: ctx.ingest(x_int, offs, out=out, layout=(16, 0), keep=keep_band)),
            ("E torch mask compaction into float4, then cc_ingest_batch", compact_then_batch)]
for _, f in variants:   # warm-up launch of every instance
    f()
torch.cuda.synchronize()
# C and E rasterise the same points in the same order: the same bytes
d_c = ctx.ingest(x_lab, offs, out=torch.zeros_like(out), layout=(16, 0), keep=keep_static).clone()
q4, o = compact()
d_e = ctx.ingest(q4, o, out=torch.zeros_like(out))
torch.cuda.synchronize()
same = int((d_c == d_e).all(dim=1).sum())
d_a = ctx.ingest(x_lab, offs, out=torch.zeros_like(out), layout=(16, 0)).clone()
d_b = ctx.ingest(x_lab, offs, out=torch.zeros_like(out), layout=(16, 0), keep=keep_all)
torch.cuda.synchronize()
same_ab = int((d_a == d_b).all(dim=1).sum())
del q4, d_c, d_e, d_a, d_b
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

    emit({"check": "descriptors of C equal those of E's compacted copy, bytes", "equal_scans": same, "scans": N})
    emit({"check": "descriptors of B equal those of A, bytes", "equal_scans": same_ab, "scans": N})
    emit({"dropped_share": round(share, 4), "run_of_records": RUN})
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
    # E's floor: one read of the records and one write of the kept ones at the HBM's peak (8 TB/s), then row A's sweep
    read_b, write_b = N * P * 16, kept_pts[0] * 16
    floor_ms = (read_b + write_b) / 8e12 * 1e3
    emit({"floor_of_E": "one read of the records + one write of the kept ones at 8 TB/s, + row A's mean", "bytes_read": read_b, "bytes_written": write_b,
          "pass_floor_ms": round(floor_ms, 4), "floor_ms": round(floor_ms + float(np.mean(rows[variants[0][0]])), 4),
          "C_ms_mean": round(float(np.mean(rows[variants[2][0]])), 4)})
    cc.lib().cc_profile_enable(ctx.h, 0)
