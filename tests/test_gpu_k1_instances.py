"""GPU: every leaf of K1's dispatch launched once (k1_instances.walk): 11 point sources x {power-of-two, division} resolution x {split
sweep + merge, one workgroup per scan} = 44 sweep instances and the 11 merge instances, each against the CPU oracle on the points the
library is specified to see.  Scans of 40 001 points and 32 x 1 251 range images: a split part sweeps 5 001 points (one full
4 096-point chunk and a partial one, with the prefetch in between), a whole-scan workgroup nine chunks and a tail."""
import numpy as np
import pytest

import k1_instances as K1

pytestmark = pytest.mark.gpu

N_PTS, H, W = 40001, 32, 1251


def _dev(buf, shift=0):
    """numpy records -> CUDA uint8 tensor whose first byte sits `shift` bytes behind a 16-byte boundary"""
    import torch
    buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    t = torch.empty(len(buf) + 16, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[shift:shift + len(buf)]
    v.copy_(torch.from_numpy(buf))
    return v


class GpuDriver:
    """the entry points through the Python layer, every call into zeroed descriptors (the kernels never write the entries behind
    n_stored / n_pts / n_segs)"""

    def __init__(self, cc):
        self.cc = cc

    def _zeros(self, n):
        import torch
        return torch.zeros((n, self.cc.DESC_BYTES), dtype=torch.uint8, device="cuda")

    def _np(self, desc):
        import torch
        torch.cuda.synchronize()
        return self.cc.desc_to_numpy(desc)

    def context(self, cfg, max_batch):
        return self.cc.Context(0, cfg, max_batch=max_batch)

    def close(self, ctx):
        ctx.close()

    def kitti(self, ctx, cat, offs):
        import torch
        x = torch.from_numpy(np.ascontiguousarray(cat, np.float32)).cuda()
        assert x.data_ptr() % 16 == 0   # (else the dispatch takes the stride-16 record loader)
        return self._np(ctx.ingest(x, offs, out=self._zeros(len(offs) - 1)))

    def points(self, ctx, buf, layout, offs, tf):
        return self._np(ctx.ingest(_dev(buf), offs, out=self._zeros(len(offs) - 1), layout=layout, tf=tf))

    def motion(self, ctx, buf, layout, motion, offs, t_begin, scale, knots):
        t_off, t_type, K = motion
        assert knots.shape[1] == K
        return self._np(ctx.ingest(_dev(buf), offs, out=self._zeros(len(offs) - 1), layout=layout, motion=(t_off, "u32" if t_type else "f32"),
                                   t_begin=t_begin, scale=scale, knots=knots))

    def segments(self, ctx, scans):
        from point_layouts import repack
        dev = [[(_dev(repack(x, *lay), shift), lay, tf) for (x, lay, tf, shift) in sc] for sc in scans]
        return self._np(ctx.ingest_segments(dev, out=self._zeros(len(scans))))

    def ranges(self, ctx, s, images):
        import torch
        cc = self.cc
        m = cc.L.RangeModel(s.H, s.W, cc.RANGE_WORDS[s.word][0], cc.RANGE_ORDERS[s.order], float(s.range_scale), float(s.origin_n), float(s.origin_z), s.K,
                            s.row_tab.ctypes.data, s.col_cs.ctypes.data, None)
        h = cc.RangeSensor(ctx, m, s.word)
        x = torch.from_numpy(np.ascontiguousarray(images).view({"u16": np.int16, "u32": np.int32, "f32": np.float32}[s.word])).cuda()
        d = self._np(ctx.ingest_ranges(h, x, out=self._zeros(len(images))))
        h.close()
        return d


def beam_clouds(cc, n):
    """n scans of the synthetic sensor, beams = H, azim = W: beam-major, already a range image"""
    xyzi, _, _ = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=200.0), device="cuda", start=11, beams=H, azim=W)
    assert xyzi.shape[1] == H * W
    return xyzi.cpu().numpy()


def test_every_k1_leaf(cc, oracle):
    inp = K1.Inputs(N_PTS, H, W, beam_clouds(cc, max(K1.BATCHES)))
    visited = K1.walk(GpuDriver(cc), cc.L, oracle, inp, float_exact=False)
    K1.assert_every_leaf(visited)
