"""Every leaf of K1's dispatch once on the CPU harness (k1_instances.walk): 11 point sources x two resolutions x the split and the
whole-scan path, each against the oracle on the points the library is specified to see.  Scans of 5 000 points and 16 x 313 range
images keep it quick here; test_gpu_k1_instances.py walks the same leaves on the device with shapes that fill the chunk loop."""
import numpy as np

import cc_amd
import k1_instances as K1
from point_motion import MotionApi
from point_segments import Segments, SegmentsApi
from range_images import RangesApi

N_PTS, H, W = 5000, 16, 313


class _Api(MotionApi, SegmentsApi, RangesApi):
    pass


class EmuDriver:
    def __init__(self, L):
        self.api = _Api(L)

    def context(self, cfg, max_batch):
        return self.api.create(cfg, max_batch=max_batch)

    def close(self, ctx):
        self.api.chk(self.api.lib.cc_destroy(ctx), "cc_destroy")

    def kitti(self, ctx, cat, offs):
        cat = np.ascontiguousarray(cat, np.float32)
        assert cat.ctypes.data % 16 == 0   # (else the dispatch takes the stride-16 record loader)
        return self.api.ingest(ctx, cat, offs)

    def points(self, ctx, buf, layout, offs, tf):
        return self.api.ingest_points(ctx, buf, layout, offs, tf)

    def motion(self, ctx, buf, layout, motion, offs, t_begin, scale, knots):
        return self.api.ingest_motion(ctx, buf, layout, motion, offs, t_begin, scale, knots)

    def segments(self, ctx, scans):
        return self.api.ingest_segments(ctx, Segments(scans))

    def ranges(self, ctx, sensor, images):
        h = self.api.sensor(ctx, sensor)
        d = self.api.ingest_ranges(ctx, h, images)
        self.api.sensor_destroy(h)
        return d


def _beam_clouds(n):
    """n scans of the synthetic sensor, beams = H, azim = W: beam-major, already a range image"""
    import torch
    synth = cc_amd.load().synth
    world = synth.World(loop_len=200.0)
    x, y, yaw = synth.trajectory(5 + n, loop_len=world.loop_len, tile=world.tile)
    out = []
    for i in range(n):
        gen = torch.Generator()
        gen.manual_seed(977 + i)
        out.append(synth.cast_scan(world, (x[5 + i], y[5 + i], yaw[5 + i]), beams=H, azim=W, device="cpu", gen=gen).numpy())
    return np.stack(out)


def test_every_k1_leaf(oracle):
    inp = K1.Inputs(N_PTS, H, W, _beam_clouds(max(K1.BATCHES)))
    visited = K1.walk(EmuDriver(oracle.L), oracle.L, oracle, inp, float_exact=True)
    K1.assert_every_leaf(visited)
