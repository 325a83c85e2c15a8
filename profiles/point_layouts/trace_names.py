"""Which K1 instances run: cc_ingest_batch, then cc_ingest_points with the default layout and no transform (10 scans, then 3), then packed xyz."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
import cc_amd
from parity import terrain_scan
cc = cc_amd.load()
ctx = cc.Context(0, max_batch=16)
for n in (10, 3):
    scans = [terrain_scan(i, n=20001) for i in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
    x = torch.from_numpy(np.concatenate(scans)).cuda()
    ctx.ingest(x, offs)                       # cc_ingest_batch
    ctx.ingest(x, offs, layout=(16, 0))       # cc_ingest_points, defaults
    ctx.ingest(x[:, :3].contiguous(), offs, layout="xyz")
    torch.cuda.synchronize()
