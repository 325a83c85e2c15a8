"""One launch each, on 64 KITTI-world scans in 16-byte records whose fourth word is a label, of
  A  cc_ingest_points {16, 0}, 16-byte aligned base: the float4 instance (the parent's kernel)
  R  the same records 4 bytes off a 16-byte boundary: cc_src_rec<16>, a 12-byte load per point, no transform
  B  the class filter that keeps everything: cc_src_flt<CLASS> (run-time stride, the 12-byte load, the label's dword, the table)
  D  the range rule on the same word, nothing dropped: cc_src_flt<RANGE>
for a counter run of its own:
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVES -d <dir> --output-format csv -- python pmc_a_b.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
cc = cc_amd.load()
N = 64
xyzi, _, _ = cc.synth.make_sequence(N, world=cc.synth.World(kitti=True), device="cuda")
P = xyzi.shape[1]
x = xyzi.clone()
x[:, :, 3] = torch.randint(0, 100, (N, P), device="cuda", dtype=torch.int32).view(torch.float32)
x = x.reshape(-1, 4).contiguous()
buf = torch.empty(x.numel() * 4 + 16, dtype=torch.uint8, device="cuda")
x_off = buf[4:4 + x.numel() * 4]
x_off.copy_(x.view(torch.uint8).reshape(-1))
offs = np.arange(N + 1, dtype=np.int64) * P
ctx = cc.Context(0, max_batch=N)
out = torch.empty((N, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
ctx.ingest(x, offs, out=out, layout=(16, 0))                                                                            # A: cc_src_kitti
ctx.ingest(x_off, offs, out=out, layout=(16, 0))                                                                        # R: cc_src_rec<16>
ctx.ingest(x, offs, out=out, layout=(16, 0), keep=cc.PointFilter.classes(12, "u32", drop=[], n_classes=260, mask=0xFFFF))  # B: cc_src_flt<0>
ctx.ingest(x, offs, out=out, layout=(16, 0), keep=cc.PointFilter.range(12, 0.0, 1.0))                                   # D: cc_src_flt<1>
torch.cuda.synchronize()
