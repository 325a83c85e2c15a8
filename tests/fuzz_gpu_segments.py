"""Randomised campaign for scans made of segments ON THE GPU (not collected by pytest; run by hand on the GPU box):
    python tests/fuzz_gpu_segments.py <seed0> <n_iter>
The seven scan generators of tests/fuzz_emu.py; every scan cut at random places into 1 .. 32 segments (some of them empty), every
segment in its own tensor with a layout drawn from {12,0} {16,0} {32,0} {48,8} {64,20} and, half of the time, a matrix of its own
(yaw, tilt, shift); 4 or 24 scans per cc_ingest_segments call (split sweep + merge kernel / one workgroup per scan).  Every
descriptor and every debug output against cc_ingest_batch on the numpy-built cloud Q = T_0(segment 0) ++ T_1(segment 1) ++ ... as
BYTES, and that against the oracle on Q (max-height image, positions, labels bit for bit, the descriptor as tests/fuzz_gpu_ingest.py
compares it)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE]
import cc_amd  # noqa: E402
import oracle_py as oracle  # noqa: E402
from fuzz_emu import gen  # noqa: E402
from parity import compare_desc  # noqa: E402
from point_layouts import apply_tf, random_tfs, repack  # noqa: E402

LAYOUTS = [(12, 0), (16, 0), (32, 0), (48, 8), (64, 20)]


def main():
    import torch
    seed0, n_it = int(sys.argv[1]), int(sys.argv[2])
    cc = cc_amd.load()
    n_bad = n_scan = n_seg = n_empty = 0
    for it in range(n_it):
        rng = np.random.default_rng(seed0 + it)
        n_scans = 4 if it % 2 else 24
        ctx = cc.Context(0, max_batch=n_scans)
        scans, Q, kinds = [], [], []
        while len(scans) < n_scans:
            kind, s = gen(rng)
            s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]   # (undefined behaviour in the reference: tests/test_emu_point_layouts.py)
            if len(s) <= 10:
                continue
            k = int(rng.integers(1, 33))
            cuts = np.sort(rng.integers(0, len(s) + 1, k - 1))
            edges = np.concatenate([[0], cuts, [len(s)]])
            tfs = random_tfs(k, seed=int(rng.integers(1 << 30)), max_tilt_deg=3.0, max_shift=2.0)
            segs, q = [], []
            for j in range(k):
                part = s[edges[j]:edges[j + 1]]
                lay = LAYOUTS[int(rng.integers(len(LAYOUTS)))]
                tf = tfs[j] if rng.random() < 0.5 else None
                shift = 4 * int(rng.integers(4))
                buf = repack(part, lay[0], lay[1])
                t = torch.empty(len(buf) + 16, dtype=torch.uint8, device="cuda")
                v = t[shift:shift + len(buf)]
                v.copy_(torch.from_numpy(np.ascontiguousarray(buf)))
                segs.append((v if len(part) else None, lay, tf))
                moved = apply_tf(part, tf) if tf is not None else part * np.array([1, 1, 1, 0], np.float32)
                q.append(moved.astype(np.float32))
                n_empty += len(part) == 0
            n_seg += k
            scans.append(segs)
            Q.append(np.concatenate(q, 0))
            kinds.append(kind)
        out = torch.zeros((n_scans, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
        ref = torch.zeros_like(out)
        desc, dbg = ctx.ingest_segments(scans, out=out, debug=True)
        offs = np.concatenate([[0], np.cumsum([len(q) for q in Q])]).astype(np.int64)
        ref, rdbg = ctx.ingest(torch.from_numpy(np.concatenate(Q, 0)).cuda(), offs, out=ref, debug=True)
        torch.cuda.synchronize()
        d = cc.desc_to_numpy(desc)
        for i in range(n_scans):
            n_scan += 1
            why = []
            if not torch.equal(desc[i], ref[i]):
                why.append("descriptor bytes differ from cc_ingest_batch on Q")
            why += ["%s differs from cc_ingest_batch on Q" % k for k in dbg if not torch.equal(dbg[k][i], rdbg[k][i])]
            q = Q[i][~(np.isnan(Q[i][:, 0]) | np.isnan(Q[i][:, 1]))]
            o = oracle.Scan(q)
            ob, opix = o.bev()
            if not np.array_equal(ob, dbg["bev"][i].cpu().numpy()) or not np.array_equal(opix, dbg["pix_rc"][i].cpu().numpy()):
                why.append("bev / pix_rc differ from the oracle")
            if not np.array_equal(o.labels(), dbg["labels"][i].cpu().numpy()):
                why.append("labels differ from the oracle")
            if not (d[i]["flags"] & 6):
                why += compare_desc(o.desc()[0], d[i], float_exact=False)[:3]
            if why:
                print("seed %d scan %d (%s, %d points, %d segments): %s" % (seed0 + it, i, kinds[i], len(Q[i]), len(scans[i]), why[:4]))
                n_bad += 1
        ctx.close()
        print("... %d calls, %d scans, %d segments (%d empty), %d bad" % (it + 1, n_scan, n_seg, n_empty, n_bad), flush=True)
    print("done: %d bad of %d scans in %d segments (%d empty)" % (n_bad, n_scan, n_seg, n_empty))
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main())
