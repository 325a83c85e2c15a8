"""K1 alone (cc_profile_enable / cc_profile_read, first slot) on 1 024 resident scans of the KITTI-shaped world: the rasteriser on the
clouds (A) next to cc_k_image_list on A's debug images -- without positions (B), with A's positions and minima (C; its descriptors
must be A's bytes for all 1 024 scans, checked here) -- and next to what a caller with an image did before: a torch pass that
expands the image to a one-point-per-cell float4 cloud (timed with events), then cc_ingest_batch (D).  Every instance warmed up,
variants alternated, 7 repeats.  B and C cycle through four copies of the images at distinct addresses (4 x 92 MB, 4 x 276 MB with
positions), so that more than the 256 MiB of the last-level cache pass between two uses of a line; A's 1.9 GB of points pass in between as well.
usage: measure_k1.py [out.jsonl]"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
cc = cc_amd.load()
N, REPS, SETS = 1024, 7, 4
HBM = 6.3e12   # bytes / s: what streaming kernels reach of the MI355X's 8 TB/s peak
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_height_images_kitti_world.jsonl")
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
xyzi = xyzi.reshape(-1, 4).contiguous()
offs = np.arange(N + 1, dtype=np.int64) * P
ctx = cc.Context(0, max_batch=N)
cfg = ctx.cfg
NC = ctx.n_cell
zeros = lambda: torch.zeros((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
out = zeros()
d_a, dbg = ctx.ingest(xyzi, offs, out=zeros(), debug=True)
torch.cuda.synchronize()
mins = cc.desc_to_numpy(d_a)["min_bin_val"].copy()
bev = [dbg["bev"].clone() for _ in range(SETS)]
pix = [dbg["pix_rc"].clone() for _ in range(SETS)]
del dbg
d_c = ctx.ingest_images(bev[0], pix[0], mins, out=zeros())
torch.cuda.synchronize()
same = int((d_a == d_c).all(dim=1).sum())
assert same == N, same

# the byte floors of B and C: the image, the list entries written (u16 cell, u8 level count, f32 height, 2 x f32 position = 15 B), and
# for C the positions gathered for the active cells, counted in whole 64-byte and 128-byte lines of the position array
act = bev[0] > float(cfg.lv_grads[0])
entries = act.sum(dim=1).clamp(max=3072)
lines64 = torch.nn.functional.pad(act, (0, (-NC) % 8)).reshape(N, -1, 8).any(dim=2).sum(dim=1)   # (per scan, as if every scan's array began on a line: close enough for a floor)
lines128 = torch.nn.functional.pad(act, (0, (-NC) % 16)).reshape(N, -1, 16).any(dim=2).sum(dim=1)
floor_b = float(N * NC * 4 + int(entries.sum()) * 15)
floor_c64, floor_c128 = floor_b + float(lines64.sum()) * 64, floor_b + float(lines128.sum()) * 128

# D: the image as a cloud -- one point per occupied cell at its centre (x, y from the cell, z = h - lidar_height), then the point path
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
pre_ms = [0.0]
cell_xy = torch.stack([(torch.arange(NC, device="cuda") // cfg.n_col).float() - cfg.n_row // 2 + 0.5,
                       (torch.arange(NC, device="cuda") % cfg.n_col).float() - cfg.n_col // 2 + 0.5], 1)
turn = [0]


def image_as_cloud():
    b = bev[turn[0] % SETS]
    ev[0].record()
    occ = b > -1000.0
    cnt = occ.sum(dim=1)
    idx = occ.reshape(-1).nonzero().squeeze(1)
    q4 = torch.zeros((idx.numel(), 4), dtype=torch.float32, device="cuda")
    q4[:, :2] = cell_xy[idx % NC]
    q4[:, 2] = b.reshape(-1)[idx] - float(cfg.lidar_height)
    o = np.concatenate([[0], np.cumsum(cnt.cpu().numpy())]).astype(np.int64)   # (the offsets are host memory: the pass ends with a copy back)
    ev[1].record()
    ctx.ingest(q4, o, out=out)
    ev[1].synchronize()
    pre_ms[0] = ev[0].elapsed_time(ev[1])


variants = [("A cc_ingest_batch on the clouds", lambda: ctx.ingest(xyzi, offs, out=out)),
            ("B cc_ingest_images, pos_rc = NULL", lambda: ctx.ingest_images(bev[turn[0] % SETS], None, None, out=out)),
            ("C cc_ingest_images with A's positions and minima", lambda: ctx.ingest_images(bev[turn[0] % SETS], pix[turn[0] % SETS], mins, out=out)),
            ("D torch image -> one-point-per-cell float4 cloud, then cc_ingest_batch", image_as_cloud)]
for s in range(SETS):   # warm-up launch of every instance, every set touched
    turn[0] = s
    for _, f in variants:
        f()
torch.cuda.synchronize()
cc.lib().cc_profile_enable(ctx.h, 1)
ms, nl = (C.c_double * 2)(), C.c_int()
cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
rows = {k: [] for k, _ in variants}
k2 = {k: [] for k, _ in variants}
pre = []
with open(OUT, "w") as fo:
    def emit(rec):
        line = json.dumps(rec)
        fo.write(line + "\n")
        print(line, flush=True)

    emit({"check": "descriptors of C equal A's, bytes", "equal_scans": same, "scans": N, "points_per_scan": P, "entries_mean": round(float(entries.float().mean()), 1),
          "occupied_mean": round(float((bev[0] > -1000.0).sum(dim=1).float().mean()), 1)})
    for r in range(REPS):
        turn[0] = r
        for k, f in variants:
            pre_ms[0] = 0.0
            f()
            cc.lib().cc_profile_read(ctx.h, ms, C.byref(nl))
            rows[k].append(ms[0] + pre_ms[0])
            k2[k].append(ms[1])
            if k[0] == "D":
                pre.append(pre_ms[0])
            emit({"rep": r, "variant": k, "k1_ms": round(ms[0], 4), "pass_before_ms": round(pre_ms[0], 4), "k2_ms": round(ms[1], 4), "launches": nl.value,
                  "image_set": r % SETS})
    for k, v in rows.items():
        emit({"variant": k, "k1_total_ms_mean": round(float(np.mean(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "reps": len(v),
              "k2_ms_mean": round(float(np.mean(k2[k])), 4), "k2_min": round(min(k2[k]), 4), "k2_max": round(max(k2[k]), 4),
              "pass_before_ms_mean": round(float(np.mean(pre)), 4) if k[0] == "D" else 0.0})
    tb, tc = float(np.mean(rows[variants[1][0]])), float(np.mean(rows[variants[2][0]]))
    emit({"floor": "B: image + list writes", "bytes": floor_b, "floor_ms": round(floor_b / HBM * 1e3, 4), "time_over_floor": round(tb / (floor_b / HBM * 1e3), 2)})
    emit({"floor": "C: B + positions in 64-byte lines", "bytes": floor_c64, "floor_ms": round(floor_c64 / HBM * 1e3, 4),
          "time_over_floor": round(tc / (floor_c64 / HBM * 1e3), 2)})
    emit({"floor": "C: B + positions in 128-byte lines", "bytes": floor_c128, "floor_ms": round(floor_c128 / HBM * 1e3, 4),
          "time_over_floor": round(tc / (floor_c128 / HBM * 1e3), 2)})
    cc.lib().cc_profile_enable(ctx.h, 0)
