"""One launch each of cc_ingest_batch on the float4 cloud (A) and of the range sweep on u32 words without knots (B), 64 KITTI-world
scans of 64 x 1 875 pixels, for a counter run of its own:
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVES -d <dir> --output-format csv -- python pmc_a_b.py"""
import math, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
cc = cc_amd.load()
N, H, W = 64, 64, 1875
P = H * W
world = cc.synth.World(kitti=True)
xyzi, _, _ = cc.synth.make_sequence(N, world=world, device="cuda")
rg = xyzi[:, :, :3].norm(dim=2)
rg = torch.where(rg > 500.0, torch.zeros_like(rg), rg)
w32 = torch.round(rg * 1000.0).to(torch.int32).reshape(-1).contiguous()
dirs = cc.synth._ray_dirs(H, W, torch.device("cuda"), hdl64=getattr(world, "dense", False)).reshape(H, W, 3)
alt = torch.asin(dirs[:, 0, 2].double()).cpu().numpy()
ctx = cc.Context(0, max_batch=N)
s32 = ctx.range_sensor(H, W, word="u32", range_scale=0.001, beam_alt=alt, col_az=np.arange(W) * (2 * math.pi / W), origin=(0.03, 0.04))
offs = np.arange(N + 1, dtype=np.int64) * P
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
ctx.ingest(xyzi.reshape(-1, 4), offs, out=out)     # A: cc_k_rasterize
ctx.ingest_ranges(s32, w32, out=out)               # B: cc_k_rasterize_rng
torch.cuda.synchronize()
