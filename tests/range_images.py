"""TEST INFRASTRUCTURE for the range-image entry points (cc_ingest_ranges and its siblings, include/cont2_amd.h): the numpy restatement
of what the library is specified to do with a range word, the sensor's tables and a scan's knots; a builder of range images from the
synthetic sensor's scans; and a driver of the calls on the CPU harness."""
import ctypes as C
import math

import numpy as np

from point_layouts import PointsApi, apply_tf

ROWS_MAX, COLS_MAX, KNOTS_MAX = 128, 4096, 64
WORDS = {"u16": (0, np.uint16), "u32": (1, np.uint32), "f32": (2, np.float32)}   # CC_RANGE_U16 / _U32 / _F32
ORDERS = {"row": 0, "col": 1}                                                     # CC_RANGE_ROW_MAJOR / _COL_MAJOR
ORIGIN_N, ORIGIN_Z = 0.03, 0.04   # the tests' beam origin
CHUNK = 4096                      # CC_K1_U_DEFAULT * CC_INGEST_BLOCK: the pixels of one chunk of the sweep
SPLIT = 8                         # CC_K1_SPLIT: parts of a scan on the split path


class RangeModel(C.Structure):
    """cc_range_model_t"""
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("word_type", C.c_int32), ("order", C.c_int32), ("range_scale", C.c_float),
                ("origin_n", C.c_float), ("origin_z", C.c_float), ("n_knots", C.c_int32), ("row_tab", C.c_void_p), ("col_cos_sin", C.c_void_p),
                ("col_knot", C.c_void_p)]


def tables(beam_alt, beam_az_off, col_az):
    """angles in radians -> (row_tab [H, 4] f32: cos(alt), sin(alt), cos(az_off), sin(az_off); col_cos_sin [W, 2] f32), made in f64"""
    alt, off, az = (np.asarray(a, np.float64) for a in (beam_alt, beam_az_off, col_az))
    return (np.ascontiguousarray(np.stack([np.cos(alt), np.sin(alt), np.cos(off), np.sin(off)], 1).astype(np.float32)),
            np.ascontiguousarray(np.stack([np.cos(az), np.sin(az)], 1).astype(np.float32)))


class Sensor:
    """A range sensor as the tests describe it: everything cc_range_model_t holds, as numpy values."""

    def __init__(self, H, W, word="u16", order="row", range_scale=0.002, row_tab=None, col_cs=None, origin=(ORIGIN_N, ORIGIN_Z), col_knot=None, K=0):
        self.H, self.W, self.word, self.order, self.range_scale, self.K = int(H), int(W), word, order, np.float32(range_scale), int(K)
        self.row_tab = np.ascontiguousarray(row_tab, np.float32)
        self.col_cs = np.ascontiguousarray(col_cs, np.float32)
        self.origin_n, self.origin_z = np.float32(origin[0]), np.float32(origin[1])
        self.col_knot = None if col_knot is None else np.ascontiguousarray(col_knot, np.int32)
        self.dtype = WORDS[word][1]

    def with_(self, **kw):
        a = dict(H=self.H, W=self.W, word=self.word, order=self.order, range_scale=self.range_scale, row_tab=self.row_tab, col_cs=self.col_cs,
                 origin=(self.origin_n, self.origin_z), col_knot=self.col_knot, K=self.K)
        a.update(kw)
        return Sensor(**a)

    def row_col(self):
        """(row, col) of every pixel in storage order j"""
        j = np.arange(self.H * self.W)
        return (j // self.W, j % self.W) if self.order == "row" else (j % self.H, j // self.H)

    def model(self):
        """(RangeModel, the arrays it points to)"""
        m = RangeModel(self.H, self.W, WORDS[self.word][0], ORDERS[self.order], float(self.range_scale), float(self.origin_n), float(self.origin_z),
                       self.K, self.row_tab.ctypes.data, self.col_cs.ctypes.data, self.col_knot.ctypes.data if self.col_knot is not None else None)
        return m, (self.row_tab, self.col_cs, self.col_knot)


def restate(sensor, words, knots=None):
    """The points the library is specified to see for ONE image `words` ([H * W] of the sensor's word type, storage order), in
    np.float32 operations only, every product and sum rounded once, in the header's association:
        r = (float)w * range_scale;  d = r - origin_n;  h = d * ca
        dx = ce * co - se * so;  dy = se * co + ce * so
        x = h * dx + origin_n * ce;  y = h * dy + origin_n * se;  z = d * sa + origin_z
    then moved by knot col_knot[col] (knots [K, 12]; apply_tf's operations) when K >= 1; a pixel without a return gets x = NaN.
    Returns [H * W, 4] f32 (w = 0) in storage order."""
    words = np.ascontiguousarray(words, sensor.dtype).reshape(-1)
    assert len(words) == sensor.H * sensor.W
    row, col = sensor.row_col()
    ca, sa, co, so = (np.ascontiguousarray(sensor.row_tab[row, i]) for i in range(4))
    ce, se = (np.ascontiguousarray(sensor.col_cs[col, i]) for i in range(2))
    on, oz, scale = sensor.origin_n, sensor.origin_z, sensor.range_scale
    with np.errstate(all="ignore"):
        if sensor.word == "f32":
            none = ~(words > np.float32(0))          # zero, negative or NaN
            r = words * scale
        else:
            none = words == 0
            r = words.astype(np.float32) * scale     # exact, or to nearest even from 2^24 on
        d = r - on
        h = d * ca
        dx = (ce * co) - (se * so)
        dy = (se * co) + (ce * so)
        out = np.zeros((len(words), 4), np.float32)
        out[:, 0] = (h * dx) + (on * ce)
        out[:, 1] = (h * dy) + (on * se)
        out[:, 2] = (d * sa) + oz
        for a in (r, d, h, dx, dy):
            assert a.dtype == np.float32
        if sensor.K > 0:
            knots = np.asarray(knots, np.float32).reshape(sensor.K, 12)
            kc = (sensor.col_knot if sensor.col_knot is not None else np.zeros(sensor.W, np.int32))[col]
            moved = np.zeros_like(out)
            for k in np.unique(kc):
                m = kc == k
                moved[m] = apply_tf(out[m], knots[k])
            out = moved
        else:
            assert knots is None
    out[none, 0] = np.nan
    return out


def restate_all(sensor, images, knots=None):
    """restate() for [n, H * W] images and [n, K, 12] knots -> list of clouds"""
    return [restate(sensor, im, None if knots is None else knots[i]) for i, im in enumerate(images)]


def offsets(n, sensor):
    return np.arange(n + 1, dtype=np.int64) * (sensor.H * sensor.W)


def synth_angles(H, W):
    """the synthetic sensor's elevations (its default linspace(+2 deg, -24.8 deg), as f32 like synth._ray_dirs) and azimuths, plus a
    non-zero azimuth offset per beam (four staggered columns of lasers, +-0.9 deg)"""
    alt = np.linspace(math.radians(2.0), math.radians(-24.8), H).astype(np.float32).astype(np.float64)
    az = (np.arange(W, dtype=np.float32) * np.float32(2 * math.pi / W)).astype(np.float64)
    az_off = np.deg2rad(np.array([-0.9, -0.3, 0.3, 0.9]))[np.arange(H) % 4]
    return alt, az_off, az


_WORLD = {}


def ranges_from_clouds(xyz, word, range_scale, seed=0):
    """Beam-major clouds [n, H * W, >= 3] of the synthetic sensor as range words in ROW-major order [n, H * W]: |p| / range_scale rounded
    (f32 words: |p| / range_scale as it is), 0 for a miss and for a further 5 % of the pixels chosen by seed."""
    xyz = np.asarray(xyz)
    n, hw = xyz.shape[:2]
    out = np.zeros((n, hw), WORDS[word][1])
    rng = np.random.default_rng(1000 + seed)
    for i in range(n):
        p = xyz[i, :, :3].astype(np.float64)
        rg = np.sqrt((p * p).sum(1))
        rg[rg > 500.0] = 0.0                       # a miss: the caster parks it at (1000, 1000, 0)
        rg[rng.choice(hw, (hw + 19) // 20, replace=False)] = 0.0
        v = rg / float(range_scale)
        out[i] = v.astype(np.float32) if word == "f32" else np.rint(v).astype(WORDS[word][1])
    return out


def synth_ranges(cc_synth, H, W, n, word, range_scale, seed=0, start=5):
    """ranges_from_clouds of n scans of the synthetic sensor (synth.cast_scan on the CPU, beams = H, azim = W: beam-major, already a
    range image)"""
    import torch
    if "w" not in _WORLD:
        _WORLD["w"] = cc_synth.World(loop_len=200.0)
    world = _WORLD["w"]
    x, y, yaw = cc_synth.trajectory(start + n, loop_len=world.loop_len, tile=world.tile)
    clouds = []
    for i in range(n):
        gen = torch.Generator()
        gen.manual_seed(77 + seed * 131 + i)
        clouds.append(cc_synth.cast_scan(world, (x[start + i], y[start + i], yaw[start + i]), beams=H, azim=W, device="cpu", gen=gen).numpy())
    return ranges_from_clouds(np.stack(clouds), word, range_scale, seed)


def synth_sensor(H, W, order, word, range_scale, K=0, col_knot=None):
    """the Sensor of the synthetic scanner's angles (synth_angles) with the tests' beam origin; K >= 1: col_knot = col * K // W unless given"""
    alt, az_off, az = synth_angles(H, W)
    row_tab, col_cs = tables(alt, az_off, az)
    if K > 0 and col_knot is None:
        col_knot = (np.arange(W, dtype=np.int64) * K // W).astype(np.int32)
    return Sensor(H, W, word, order, range_scale, row_tab, col_cs, col_knot=col_knot, K=K)


def procedural_ranges(H, W, n, seed, range_scale=0.002):
    """[n, H * W] u16 row-major images of any size, with the beams' altitudes (radians, linspace(+10 deg, -25 deg)): ground under the
    beams that look down (sensor 1.9 m up), a wall whose distance waves with the azimuth in front of the others, 5 % no-return."""
    alt = np.deg2rad(np.linspace(10.0, -25.0, H))
    out = np.zeros((n, H, W), np.uint16)
    for i in range(n):
        rng = np.random.default_rng(seed + i)
        a = np.arange(W) * (2 * np.pi / W)
        wall = 25.0 + 14.0 * np.sin(3 * a + i) + 6.0 * np.sin(11 * a + 0.3 * i)          # 5 - 45 m, horizontal
        top = 1.0 + 2.5 * (1 + np.sin(7 * a + i))                                          # the wall's height above the sensor: 1 - 6 m
        for r in range(H):
            rg = wall / np.cos(alt[r])
            if alt[r] < 0:
                rg = np.minimum(rg, 1.9 / np.sin(-alt[r]))
            else:
                rg = np.where(rg * np.sin(alt[r]) <= top, rg, 0.0)                         # over the wall: no return
            out[i, r] = np.rint(np.minimum(rg, 120.0) / range_scale).astype(np.uint16)
        out[i][rng.random((H, W)) < 0.05] = 0
    return out.reshape(n, H * W), alt


def to_order(images, H, W, order):
    """row-major images [n, H * W] in the storage order `order`"""
    images = np.asarray(images)
    if order == "row":
        return np.ascontiguousarray(images)
    return np.ascontiguousarray(images.reshape(len(images), H, W).transpose(0, 2, 1).reshape(len(images), H * W))


def scene(cc_synth, oracle, H, W, order="row", word="u16", range_scale=0.002, n=3, K=0, col_knot=None, seed=0, check=True):
    """(Sensor, images [n, H * W] in storage order) of a realistic scene; asserts its preconditions on the restated cloud without knots: at
    least 5 % no-return pixels, at least 300 occupied cells, contours on levels 1 - 3 in the oracle's descriptor."""
    sensor = synth_sensor(H, W, order, word, range_scale, K, col_knot)
    images = to_order(synth_ranges(cc_synth, H, W, n, word, range_scale, seed), H, W, order)
    if check:
        assert_scene(oracle, sensor, images)
    return sensor, images


def assert_scene(oracle, sensor, images):
    """the preconditions of a realistic scene, on the restated clouds without knots: at least 5 % no-return pixels, at least 300 occupied
    cells, contours on levels 1 - 3 in the oracle's descriptor"""
    plain = sensor.with_(K=0, col_knot=None)
    for im in images:
        q = restate(plain, im)
        none = np.isnan(q[:, 0])
        assert none.mean() >= 0.05, none.mean()
        d = oracle.Scan(q[~none]).desc()[0]
        assert int(d["n_pix"]) >= 300, int(d["n_pix"])
        assert all(int(d["n_cont"][lv]) > 0 for lv in (1, 2, 3)), d["n_cont"]


def sweep_knots(motion_knots, n, K, seed):
    """[n, K, 12] f32: motion_knots of a per-scan sweep motion of 1 - 2 m and 2 - 4 degrees, referred to the sweep's end"""
    from point_layouts import rigid
    rng = np.random.default_rng(seed)
    out = np.zeros((n, K, 12), np.float32)
    for i in range(n):
        ang, dist, yaw = rng.uniform(-np.pi, np.pi), rng.uniform(1.0, 2.0), np.deg2rad(rng.uniform(2.0, 4.0)) * rng.choice([-1.0, 1.0])
        begin = rigid(yaw, np.deg2rad(rng.uniform(-0.5, 0.5)), np.deg2rad(rng.uniform(-0.5, 0.5)), (dist * np.cos(ang), dist * np.sin(ang), 0.0))
        out[i] = np.asarray(motion_knots(begin, rigid(0.0), 1.0, K), np.float32).reshape(K, 12)
    return out


def part_bounds(hw):
    """scan-relative first pixel of each of the split path's parts (cc_k1_sweep's ranges)"""
    per = (hw + SPLIT - 1) // SPLIT
    return [min(p * per, hw) for p in range(SPLIT)]


def assert_shape_exercises_paths(sensor):
    """more than two 4 096-pixel chunks per sweep and a ragged tail (asserted); returns the number of the split path's part boundaries
    that fall INSIDE a storage row (W pixels row-major, H pixels col-major)"""
    hw = sensor.H * sensor.W
    assert hw > 2 * CHUNK and hw % CHUNK != 0, hw
    run = sensor.W if sensor.order == "row" else sensor.H
    return len([b for b in part_bounds(hw)[1:] if b % run != 0])


def cells(cfg, q):
    """cell index (or -1) of every point of q, as cc_point_cell computes it at a power-of-two resolution; NaN points get -1"""
    with np.errstate(all="ignore"):
        x, y = q[:, 0], q[:, 1]
        hr, hc = cfg.n_row // 2, cfg.n_col // 2
        ok = (np.abs(x) <= hr * cfg.reso_row) & (np.abs(y) <= hc * cfg.reso_col) & ~(x * x + y * y < cfg.blind_sq) & ~np.isnan(x) & ~np.isnan(y)
        row = np.floor(np.where(ok, x, 0) / cfg.reso_row).astype(np.int64) + hr
        col = np.floor(np.where(ok, y, 0) / cfg.reso_col).astype(np.int64) + hc
    return np.where(ok & (row > 0), row * cfg.n_col + col, -1)


def tie_scene(cfg, order, H=16, W=601, K=5, n=3):
    """A sensor whose TOP beam (row 0) has sin(alt) = +0.0 exactly -- every pixel of it has z = origin_z bit for bit -- and whose other
    beams look down, so the top beam is the highest over its cells; knots that are yaw + xy shifts with row 2 = (0, 0, 1, 0), so z
    stays exact across knots; ranges of the top beam that vary slowly with the column, so that neighbouring firings (of different
    knots at the knot boundaries, which the small yaw / shift steps keep in the same cells) share cells.  Returns (Sensor, images
    [n, H * W] u16 in storage order, knots [n, K, 12]); asserts at least 10 cells per scan whose maximum is shared by pixels of
    different columns AND different knots."""
    from point_layouts import rigid
    alt = np.concatenate([[0.0], np.deg2rad(np.linspace(-3.0, -20.0, H - 1))])
    az = np.arange(W) * (2 * np.pi / W)
    row_tab, col_cs = tables(alt, np.deg2rad(np.array([-0.9, -0.3, 0.3, 0.9]))[np.arange(H) % 4], az)
    row_tab[0, 1] = np.float32(0.0)   # sin(alt) = +0.0
    assert row_tab[0, 1] == 0 and not np.signbit(row_tab[0, 1])
    # many firings per knot boundary: the knot index changes every few columns
    col_knot = ((np.arange(W) // 3) % K).astype(np.int32)
    sensor = Sensor(H, W, "u16", order, 0.002, row_tab, col_cs, col_knot=col_knot, K=K)
    images, knots = [], np.zeros((n, K, 12), np.float32)
    for i in range(n):
        rng = np.random.default_rng(300 + i)
        im = np.zeros((H, W), np.uint16)
        im[0] = np.rint((20.0 + 8.0 * np.sin(np.arange(W) * (2 * np.pi / W) * 3 + i)) / 0.002).astype(np.uint16)   # 12 - 28 m: one firing is 0.1 - 0.3 m on
        for r in range(1, H):
            ground = 1.7 / np.sin(-alt[r])
            im[r] = np.rint(np.minimum(ground, 60.0) / 0.002).astype(np.uint16)
        im[rng.random((H, W)) < 0.05] = 0
        images.append(im.reshape(-1))
        for k in range(K):
            m = rigid(np.deg2rad(0.05 * k), t=(0.03 * k, -0.02 * k, 0.0), dtype=np.float32)
            m[2] = (0.0, 0.0, 1.0, 0.0)
            knots[i, k] = m.reshape(12)
    images = to_order(np.stack(images), H, W, order)
    row, col = sensor.row_col()
    for i in range(n):
        q = restate(sensor, images[i], knots[i])
        top = (row == 0) & ~np.isnan(q[:, 0])
        assert np.all(q[top, 2].view(np.uint32) == np.float32(ORIGIN_Z).view(np.uint32)), "the top beam's z is origin_z bit for bit"
        c = cells(cfg, q)
        tied = 0
        for cell in np.unique(c[c >= 0]):
            m = c == cell
            best = m & (q[:, 2] == q[m, 2].max())
            tied += len(np.unique(col[best])) > 1 and len(np.unique(col_knot[col[best]])) > 1
        assert tied >= 10, (i, tied)
    return sensor, images, knots


def first_owner_positions(cfg, q, limit=40):
    """{cell: expected pix_rc of the FIRST point in storage order at the cell's maximum} for up to `limit` cells with more than one such point"""
    c = cells(cfg, q)
    out = {}
    for cell in np.unique(c[c >= 0]):
        m = c == cell
        best = np.flatnonzero(m & (q[:, 2] == q[m, 2].max()))
        if len(best) > 1:
            f = best[0]
            out[int(cell)] = np.array([q[f, 0] / np.float32(cfg.reso_row) + np.float32(cfg.n_row // 2) - np.float32(0.5),
                                       q[f, 1] / np.float32(cfg.reso_col) + np.float32(cfg.n_col // 2) - np.float32(0.5)], np.float32)
            if len(out) >= limit:
                break
    return out


def edge_words(word, n):
    """n range words that include the edge values of the type, repeated: integer 0, 1, the largest u16, u32 words of 2^24 or more whose
    conversion rounds; f32 -1, -0.0, NaN, +inf, a subnormal"""
    if word == "u16":
        special = np.array([0, 1, 65535, 2, 65534, 0, 30000], np.uint16)
    elif word == "u32":
        special = np.array([0, 1, 65535, (1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 0xFFFFFFFF, 20000, 0], np.uint32)
        assert np.any(special.astype(np.float32).astype(np.int64) != special.astype(np.int64)), "words whose conversion rounds"
    else:
        special = np.array([-1.0, -0.0, np.nan, np.inf, 1e-40, 0.0, 1.0, 25.5, -np.inf], np.float32)
        assert special[4] != 0 and special[4] < np.finfo(np.float32).tiny
    return np.resize(special, n).astype(WORDS[word][1])


class RangesApi(PointsApi):
    """point_layouts.PointsApi plus the calls that take a range sensor."""

    def sensor_rc(self, ctx, sensor=None, model=None):
        """cc_range_sensor_create -> (rc, handle)"""
        keep = None
        if model is None:
            model, keep = sensor.model()
        h = C.c_void_p()
        rc = self.lib.cc_range_sensor_create(ctx, C.byref(model), C.byref(h))
        del keep
        return rc, h

    def sensor(self, ctx, sensor):
        rc, h = self.sensor_rc(ctx, sensor)
        self.chk(rc, "cc_range_sensor_create")
        return h

    def sensor_destroy(self, h):
        self.chk(self.lib.cc_range_sensor_destroy(h), "cc_range_sensor_destroy")

    @staticmethod
    def _kn(knots, n):
        return None if knots is None else np.ascontiguousarray(np.asarray(knots, np.float32).reshape(n, -1))

    def ingest_ranges_rc(self, ctx, h, images, n, knots=None, debug=False, ptr=None):
        """cc_ingest_ranges: (rc, descriptors, debug outputs or None); images: a contiguous array of n images (or ptr: an address)"""
        L = self.L
        desc = np.zeros(n, L.scan_desc_dt)
        ncell = self._cfg.n_row * self._cfg.n_col
        dbg, dbg_p = None, None
        if debug:
            dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32),
                   "labels": np.zeros((n, L.NLEV, ncell), np.int16)}
            st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
            dbg_p = C.cast(st, C.c_void_p)
        kn = self._kn(knots, n)
        if ptr is None:
            ptr = None if images is None else images.ctypes.data
        rc = self.lib.cc_ingest_ranges(ctx, h, C.c_void_p(ptr), n, C.c_void_p(kn.ctypes.data) if kn is not None else None,
                                       C.c_void_p(desc.ctypes.data), dbg_p, None)
        return rc, desc, dbg

    def ingest_ranges(self, ctx, h, images, knots=None, debug=False):
        images = np.ascontiguousarray(images)
        rc, desc, dbg = self.ingest_ranges_rc(ctx, h, images, len(images), knots, debug)
        self.chk(rc, "cc_ingest_ranges")
        return (desc, dbg) if debug else desc

    def ingest_ranges_host_rc(self, ctx, h, images, n, knots=None, want_bev=False, ptr=None):
        desc = np.zeros(n, self.L.scan_desc_dt)
        bev = np.zeros((n, self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        kn = self._kn(knots, n)
        if ptr is None:
            ptr = None if images is None else images.ctypes.data
        rc = self.lib.cc_ingest_ranges_host(ctx, h, C.c_void_p(ptr), n, C.c_void_p(kn.ctypes.data) if kn is not None else None,
                                            C.c_void_p(desc.ctypes.data), C.c_void_p(bev.ctypes.data) if want_bev else None)
        return rc, desc, bev

    def scan_ingest_ranges_rc(self, ctx, h, image, knots=None, ptr=None):
        """cc_scan_ingest_ranges -> (rc, the scan's descriptor or None)"""
        sc = C.c_void_p()
        kn = self._kn(knots, 1)
        if ptr is None:
            ptr = None if image is None else image.ctypes.data
        rc = self.lib.cc_scan_ingest_ranges(ctx, h, C.c_void_p(ptr), C.c_void_p(kn.ctypes.data) if kn is not None else None, 0, C.byref(sc))
        return rc, (self._take(sc)[0] if rc == 0 else None)

    def motion_knots(self, pose_begin, pose_end, ref=1.0, K=32):
        pb = np.ascontiguousarray(np.asarray(pose_begin, np.float64).reshape(12))
        pe = np.ascontiguousarray(np.asarray(pose_end, np.float64).reshape(12))
        out = np.zeros((K, 12), np.float32)
        self.lib.cc_motion_knots(C.c_void_p(pb.ctypes.data), C.c_void_p(pe.ctypes.data), C.c_double(ref), C.c_int(K), C.c_void_p(out.ctypes.data))
        return out
