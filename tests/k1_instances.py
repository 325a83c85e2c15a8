"""TEST INFRASTRUCTURE: the walk over every leaf of K1's dispatch (csrc/cont2_amd.hip, k1_dispatch / k1_launch) -- 11 point sources x
{power-of-two, division} resolution x {split sweep + merge, one workgroup per scan} = 44 sweep instances and the 11 merge instances,
each chosen by its input.  test_emu_k1_instances.py walks it on the CPU harness, test_gpu_k1_instances.py on the device; `drv` is what
differs between the two (how a context is made and how each entry point is called; every call returns numpy descriptors ingested into
zeroed memory).

The rec, mot and seg leaves are fed the SAME logical points -- one transform per scan: mot brings it as the single knot of a K = 1
call, seg gives it to all three of a scan's segments -- so one set of oracle descriptors per resolution serves all seven, and their
descriptors are equal byte for byte.  kitti is compared on the untransformed cloud, rng on the cloud of its own images."""
import numpy as np

from parity import compare_desc, terrain_scan
from point_layouts import apply_tf, border_scan, random_tfs, repack
from point_motion import TIME_F32, TIME_U32, repack_with_time, u32_bits_as_f32
from range_images import ranges_from_clouds, restate_all, synth_sensor

RESOLUTIONS = {"pow2": None, "div": (1.5, 0.75, 100, 100)}   # default cells (multiply by the reciprocal) / IEEE division: reso_row, reso_col, n_row, n_col
BATCHES = (2, 9)                                              # <= 8 scans: split sweep + merge kernel; more: one workgroup per scan
LEAVES = ("kitti", "rec12", "rec16_tf", "rec_rt", "mot16", "mot32", "mot_rt", "seg", "rng_u16", "rng_u32", "rng_f32")
SAME_POINTS = LEAVES[1:8]                                     # the leaves that see the transformed cloud
RANGE_SCALE = 0.002
# leaf -> (stride, xyz_offset[, time_offset, time_type]); rec_rt / mot_rt: a stride no instance is compiled for, mot_rt with the time
# word in FRONT of x, y, z (a negative offset from x in the kernel)
REC = {"rec12": (12, 0), "rec16_tf": (16, 0), "rec_rt": (48, 8)}
MOT = {"mot16": (16, 0, 12, TIME_F32), "mot32": (32, 0, 20, TIME_U32), "mot_rt": (48, 8, 4, TIME_F32)}
SEG_LAYOUTS = ((12, 0), (32, 0), (48, 8))                     # a scan's three segments


def manager_cfg(L, reso):
    cfg = L.default_manager_cfg()
    if RESOLUTIONS[reso] is not None:
        cfg.reso_row, cfg.reso_col, cfg.n_row, cfg.n_col = RESOLUTIONS[reso]
    return cfg


class Inputs:
    """max(BATCHES) scans of every kind; a batch of nb scans takes the first nb.  n_pts: points of the longest scan (the others are a
    few points shorter each); beam_clouds: [n, H * W, >= 3] beam-major scans of the synthetic sensor for the H x W range images."""

    def __init__(self, n_pts, H, W, beam_clouds):
        n = max(BATCHES)
        self.raw = [border_scan(7, n=n_pts)] + [terrain_scan(40 + i, n=n_pts - 3 * i, scale=1.2) for i in range(1, n)]
        self.tfs = random_tfs(n, seed=29, max_tilt_deg=2.0, max_shift=2.0)
        self.moved = [apply_tf(s, m) for s, m in zip(self.raw, self.tfs)]
        self.sensors, self.images = {}, {}
        u16 = ranges_from_clouds(np.asarray(beam_clouds)[:n], "u16", RANGE_SCALE, seed=5)
        for word, dt in (("u16", np.uint16), ("u32", np.uint32), ("f32", np.float32)):   # the same integers in every word type: one cloud
            self.sensors[word] = synth_sensor(H, W, "row", word, RANGE_SCALE)
            self.images[word] = np.ascontiguousarray(u16.astype(dt))
        self.rng_clouds = restate_all(self.sensors["u16"], self.images["u16"])
        for word in ("u32", "f32"):
            q = restate_all(self.sensors[word], self.images[word][:1])[0]
            assert q.tobytes() == self.rng_clouds[0].tobytes(), word

    def offs(self, nb):
        return np.concatenate([[0], np.cumsum([len(s) for s in self.raw[:nb]])]).astype(np.int64)


def oracle_descs(oracle, clouds, cfg):
    out = []
    for s in clouds:
        s = s[~(np.isnan(s[:, 0]) | np.isnan(s[:, 1]))]   # rejected by the library, undefined behaviour in the reference
        out.append(oracle.Scan(s, cfg).desc()[0])
    return out


def run_leaf(drv, ctx, leaf, inp, nb):
    """the descriptors of leaf `leaf` for the first nb scans"""
    offs, cat = inp.offs(nb), np.concatenate(inp.raw[:nb], 0)
    if leaf == "kitti":
        return drv.kitti(ctx, cat, offs)
    if leaf in REC:
        stride, off = REC[leaf]
        return drv.points(ctx, repack(cat, stride, off), (stride, off), offs, inp.tfs[:nb])
    if leaf in MOT:
        stride, off, t_off, t_type = MOT[leaf]
        w = (np.arange(len(cat), dtype=np.uint32) * np.uint32(2654435761)) if t_type == TIME_U32 else np.linspace(-1.0, 1.0, len(cat)).astype(np.float32).view(np.uint32)
        t_begin = np.full(nb, u32_bits_as_f32(12345) if t_type == TIME_U32 else np.float32(-0.25), np.float32)
        return drv.motion(ctx, repack_with_time(cat, w, stride, off, t_off), (stride, off), (t_off, t_type, 1), offs, t_begin, np.full(nb, 7.5, np.float32),
                          inp.tfs[:nb].reshape(nb, 1, 12))
    if leaf == "seg":
        scans = []
        for i in range(nb):
            s, n = inp.raw[i], len(inp.raw[i])
            cuts = [0, n // 5, n // 5 + n // 2 + 1, n]   # uneven pieces; on the split path parts begin and end inside them
            scans.append([(s[cuts[k]:cuts[k + 1]], SEG_LAYOUTS[k], inp.tfs[i], 4 * k) for k in range(3)])
        return drv.segments(ctx, scans)
    word = leaf[4:]
    return drv.ranges(ctx, inp.sensors[word], inp.images[word][:nb])


def walk(drv, L, oracle, inp, float_exact, resolutions=tuple(RESOLUTIONS), batches=BATCHES, on_leaf=None):
    """Every leaf once.  Returns the list of (resolution, batch size, leaf) visited; on_leaf(reso, nb, leaf, descriptors) sees each."""
    visited = []
    for reso in resolutions:
        cfg = manager_cfg(L, reso)
        ref = {"kitti": oracle_descs(oracle, inp.raw, cfg), "moved": oracle_descs(oracle, inp.moved, cfg), "rng": oracle_descs(oracle, inp.rng_clouds, cfg)}
        assert min(int(d["n_pix"]) for r in ref.values() for d in r) > 200, "every cloud fills the grid"
        for nb in batches:
            ctx = drv.context(cfg, nb)
            first = {}
            for leaf in LEAVES:
                d = run_leaf(drv, ctx, leaf, inp, nb)
                assert len(d) == nb
                group = "kitti" if leaf == "kitti" else ("moved" if leaf in SAME_POINTS else "rng")
                for i in range(nb):
                    bad = compare_desc(ref[group][i], d[i], float_exact=float_exact)
                    assert not bad, (reso, nb, leaf, i, bad[:5])
                if group in first:   # the same logical points: the same bytes
                    assert d.tobytes() == first[group][1].tobytes(), (reso, nb, leaf, "differs from", first[group][0])
                else:
                    first[group] = (leaf, d)
                if on_leaf:
                    on_leaf(reso, nb, leaf, d)
                visited.append((reso, nb, leaf))
            drv.close(ctx)
    return visited


def assert_every_leaf(visited):
    assert len(visited) == len(set(visited)) == len(RESOLUTIONS) * len(BATCHES) * len(LEAVES) == 44, len(visited)
    assert set(visited) == {(r, b, l) for r in RESOLUTIONS for b in BATCHES for l in LEAVES}
