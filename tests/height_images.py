"""TEST INFRASTRUCTURE for the image entry points (cc_ingest_images and its siblings, include/cont2_amd_images.h): the numpy
restatement of the header's rules (sanitise, clamp, defaults), a driver of the calls on any build of the library (ImagesApi on
point_layouts.PointsApi: the CPU harness by default), and the cases, written once over a small back end (test_emu_height_images.py:
the CPU harness, test_gpu_height_images.py: the device).  A back end has
    float_exact                               what parity.compare_desc is asked for against the oracle
    open(cfg, max_batch) -> handle, close(handle)
    points(handle, clouds, debug) -> (descriptors, debug dict or None)        one cc_ingest_batch call, numpy out
    images(handle, height, pos, mins, debug) -> (descriptors, debug dict or None)   one cc_ingest_images call, numpy out
    paths() -> {"list": set, "mid": set, "big": set} of scan indices of the last call, or None where the build cannot say.
    path_counts() -> {"list": n, "mid": n, "big": n, "why": [4]} of the last images() call: the difference of two cc_ingest_path_counts readings
References come from cc_ingest_batch on clouds (the defining property) and from the oracle, never from the new code alone."""
import ctypes as C

import numpy as np

import cc_amd
import key_cases as KC
from parity import compare_desc, terrain_scan
from point_layouts import PointsApi

EMPTY = np.float32(-1000.0)
LIST_CAP, SLOT_CAP, MAXC = 3072, 12800, 320


# ---------------------------------------------------------------- the header's rules, restated ----------------------------------------------------------------
def sanitise(height, cfg):
    """[n, n_cell] f32 as the library reads it: row 0 and every cell that is not > -1000 (NaN too) become -1000"""
    h = np.array(height, np.float32).reshape(-1, cfg.n_row * cfg.n_col)
    with np.errstate(invalid="ignore"):
        occ = h > EMPTY
    occ[:, :cfg.n_col] = False
    return np.where(occ, h, EMPTY)


def centres(cfg):
    """[n_cell, 2] f32: ((float)row, (float)col)"""
    r, c = np.divmod(np.arange(cfg.n_row * cfg.n_col), cfg.n_col)
    return np.stack([r, c], 1).astype(np.float32)


def clamp(pos, cfg):
    """a component that is NaN or outside [centre - 0.5, centre + 0.5] becomes the centre's, per component"""
    p = np.array(pos, np.float32).reshape(-1, cfg.n_row * cfg.n_col, 2)
    cen = centres(cfg)[None]
    with np.errstate(invalid="ignore"):
        ok = (p >= cen - np.float32(0.5)) & (p <= cen + np.float32(0.5))
    return np.where(ok, p, cen)


def expect_debug(height, pos, cfg):
    """(d_bev, d_pix_rc) the library returns: the sanitised image; -1 in the empty cells, the clamped positions in the others"""
    bev = sanitise(height, cfg)
    p = clamp(pos, cfg) if pos is not None else np.broadcast_to(centres(cfg)[None], bev.shape + (2,))
    return bev, np.where((bev > EMPTY)[..., None], p, np.float32(-1.0)).astype(np.float32)


def default_min(height, cfg):
    """min_bin_val without min_height: the minimum over the occupied cells; +1000 for an image without one"""
    bev = sanitise(height, cfg)
    return np.array([b[b > EMPTY].min() if (b > EMPTY).any() else np.float32(1000.0) for b in bev], np.float32)


# ---------------------------------------------------------------- scenes as images and as one-point-per-cell clouds ----------------------------------------------------------------
def grid_h(h):
    """a height on the 1 / 64 grid: lidar_height + (h - lidar_height) is h bit for bit there (asserted in centre_cloud)"""
    return float(np.round(h * 64.0) / 64.0)


def scene_image(scene, cfg):
    img = np.full(cfg.n_row * cfg.n_col, EMPTY, np.float32)
    for (r, c), h in scene.h.items():
        img[r * cfg.n_col + c] = np.float32(grid_h(h))
    return img


def centre_cloud(scene, cfg, seed=0):
    """one point exactly at the centre of every cell of the scene, in a shuffled order; f32(lidar_height) + z == h bit for bit and
    pointToContRowCol of the point is ((float)row, (float)col)"""
    cells = sorted(scene.h)
    assert len(cells) > 10
    rc = np.array(cells, np.float32)
    p = np.zeros((len(cells), 4), np.float32)
    p[:, 0] = (rc[:, 0] - np.float32(cfg.n_row // 2)) + np.float32(0.5)
    p[:, 1] = (rc[:, 1] - np.float32(cfg.n_col // 2)) + np.float32(0.5)
    h = np.array([grid_h(scene.h[c]) for c in cells], np.float32)
    p[:, 2] = h - np.float32(cfg.lidar_height)
    assert np.array_equal((np.float32(cfg.lidar_height) + p[:, 2]).view(np.uint32), h.view(np.uint32)), "lidar_height + z == h bit for bit"
    assert np.array_equal(p[:, 0] / np.float32(cfg.reso_row) + np.float32(cfg.n_row // 2) - np.float32(0.5), rc[:, 0])
    assert np.array_equal(p[:, 1] / np.float32(cfg.reso_col) + np.float32(cfg.n_col // 2) - np.float32(0.5), rc[:, 1])
    return p[np.random.default_rng(seed).permutation(len(cells))]


def blind_cloud(extra=None):
    """11 points inside the blind zone (all rejected), behind `extra` points if given"""
    p = np.zeros((11, 4), np.float32)
    p[:, 0] = np.linspace(-1.0, 1.0, 11)
    p[:, 1] = 0.25
    p[:, 2] = 1.0
    return p if extra is None else np.concatenate([extra, p])


def counts(img, cfg):
    """(list entries, slots) of a sanitised image: cells above lv_grads[0]; the sum of their level counts"""
    lv = np.array(list(cfg.lv_grads), np.float32)
    above = img[:, None] > lv[None, :]
    return int(above[:, 0].sum()), int(above[above[:, 0]].sum())


def plateau_scene(n_active, top=2):
    """one plateau of 55 x 55 cells on levels 0..top plus single cells just above lv_grads[0]: exactly n_active active cells"""
    s = KC.Scene().rect(8, 8, 55, 55, KC.H(top))
    k = n_active - 55 * 55
    assert 0 <= k <= 19 * 40
    spots = [(r, c) for r in range(90, 147, 3) for c in range(10, 130, 3)]
    for r, c in spots[:k]:
        s.cell(r, c, KC.H(0))
    return s


def tall_scene():
    """2 200 cells above all six levels (13 200 slots) under the list's 3 072 entries"""
    return KC.Scene().rect(8, 8, 40, 55, KC.H(5))


def blob_scene():
    """key_cases' "+blobs" construction: more than 320 components on a level"""
    s = KC.Scene()
    for i in range(4):
        s.rect(KC.SPOTS[i][0], KC.SPOTS[i][1], 5, 5, KC.H(5))
    extra = KC._only_blobs(s)
    s.h.update(extra.h)
    return s


def small_scene():
    """case 3's scene: the mesas of key_cases' "group_19" layout and a sprinkle of single cells"""
    s = KC.Scene()
    for i in range(6):
        s.rect(KC.SPOTS[i][0], KC.SPOTS[i][1], KC.BIG[i][0], KC.BIG[i][1], KC.H(2))
    s.rect(KC.SPOTS[8][0], KC.SPOTS[8][1], 4, 5, KC.H(5))
    s.rect(1, 70, 5, 5, KC.H(3))          # touches row 1: the first row an image may fill
    s.rect(144, 72, 6, 5, KC.H(2))        # ... and the last row
    s.sprinkle(21, 0.03, KC.H(1)).sprinkle(22, 0.01, KC.H(4))
    s.h = {rc: h for rc, h in s.h.items() if rc[0] >= 1}   # (the reference's image keeps nothing in row 0)
    return s


# ---------------------------------------------------------------- clouds of the round trip ----------------------------------------------------------------
_CLOUDS = {}


def round_trip_clouds():
    """six parity.terrain_scan clouds of 8 000 points and three scans of synth.make_sequence(beams=16, azim=450)"""
    if "rt" not in _CLOUDS:
        synth = cc_amd.load().synth
        x, _, _ = synth.make_sequence(3, world=synth.World(loop_len=40.0), beams=16, azim=450)
        x = x.numpy().reshape(3, -1, 4)
        _CLOUDS["rt"] = [terrain_scan(40 + i, n=8000) for i in range(6)] + [np.ascontiguousarray(x[i]) for i in range(3)]
    return _CLOUDS["rt"]


_ORACLE = {}


def oracle_of(oracle, key, cloud, cfg=None):
    """(oracle descriptor, bev, pix_rc) of a cloud, computed once per key"""
    if key not in _ORACLE:
        o = oracle.Scan(cloud, cfg)
        bev, pix = o.bev()
        _ORACLE[key] = (o.desc()[0], bev, pix)
    return _ORACLE[key]


def same(a, b, da=None, db=None, keys=("bev", "pix_rc", "labels")):
    assert a.tobytes() == b.tobytes(), "descriptors differ"
    if da is not None:
        for k in keys:
            assert np.asarray(da[k]).tobytes() == np.asarray(db[k]).tobytes(), k


# ---------------------------------------------------------------- the driver ----------------------------------------------------------------
class ImagesApi(PointsApi):
    """point_layouts.PointsApi plus the calls of include/cont2_amd_images.h, through calls.ingest_images / calls.scan_ingest_image"""

    def _dbg(self, n, debug):
        if not debug:
            return None, None, None
        ncell = self._cfg.n_row * self._cfg.n_col
        dbg = {"bev": np.zeros((n, ncell), np.float32), "pix_rc": np.zeros((n, ncell, 2), np.float32), "labels": np.zeros((n, self.L.NLEV, ncell), np.int16)}
        st = (C.c_void_p * 3)(dbg["bev"].ctypes.data, dbg["pix_rc"].ctypes.data, dbg["labels"].ctypes.data)
        return dbg, st, C.addressof(st)

    def ingest_images_rc(self, ctx, height, pos=None, mins=None, n=None, debug=False, hptr=None, pptr=None):
        """cc_ingest_images: (rc, descriptors, debug outputs or None).  "Device" pointers are host pointers on the harness; hptr / pptr
        replace the arrays' addresses (a NULL or misaligned base)"""
        calls = cc_amd.load().calls
        height = None if height is None else np.ascontiguousarray(height, np.float32)
        pos = None if pos is None else np.ascontiguousarray(pos, np.float32)
        n = len(height) if n is None else n
        desc = np.zeros(max(n, 0), self.L.scan_desc_dt)
        dbg, st, dbg_p = self._dbg(max(n, 0), debug)
        hp = (None if height is None else height.ctypes.data) if hptr is None else hptr
        pp = (None if pos is None else pos.ctypes.data) if pptr is None else pptr
        rc = calls.ingest_images(self.lib, ctx, hp or None, pp or None, n, mins, desc.ctypes.data, dbg_p, None)
        return rc, desc, dbg

    def ingest_images(self, ctx, height, pos=None, mins=None, debug=False):
        rc, desc, dbg = self.ingest_images_rc(ctx, height, pos, mins, debug=debug)
        self.chk(rc, "cc_ingest_images")
        return (desc, dbg) if debug else desc

    def ingest_images_host_rc(self, ctx, height, pos=None, mins=None, n=None, want_bev=False, hptr=None, out=True):
        calls = cc_amd.load().calls
        height = None if height is None else np.ascontiguousarray(height, np.float32)
        pos = None if pos is None else np.ascontiguousarray(pos, np.float32)
        n = len(height) if n is None else n
        desc = np.zeros(max(n, 0), self.L.scan_desc_dt)
        bev = np.zeros((max(n, 0), self._cfg.n_row * self._cfg.n_col), np.float32) if want_bev else None
        hp = (None if height is None else height.ctypes.data) if hptr is None else hptr
        rc = calls.ingest_images(self.lib, ctx, hp or None, None if pos is None else pos.ctypes.data, n, mins, desc.ctypes.data if out else None, host=True,
                                 bev=bev.ctypes.data if want_bev else None)
        return rc, desc, bev

    def scan_ingest_image_rc(self, ctx, height, pos=None, min_height=None, want_bev=False, out=True):
        """cc_scan_ingest_image -> (rc, the scan's descriptor or None, cc_scan_bev's image or None)"""
        calls = cc_amd.load().calls
        height = None if height is None else np.ascontiguousarray(height, np.float32)
        pos = None if pos is None else np.ascontiguousarray(pos, np.float32)
        sc = C.c_void_p()
        if not out:
            return self.lib.cc_scan_ingest_image(ctx, height.ctypes.data, None, None, 0, None), None, None
        rc = calls.scan_ingest_image(self.lib, ctx, None if height is None else height.ctypes.data, None if pos is None else pos.ctypes.data, min_height,
                                     want_bev, sc)
        if rc != 0:
            return rc, None, None
        bev = None
        if want_bev:
            p = C.c_void_p()
            self.chk(self.lib.cc_scan_bev(sc, C.byref(p)), "cc_scan_bev")
            ncell = self._cfg.n_row * self._cfg.n_col
            bev = np.frombuffer(C.string_at(p, 4 * ncell), np.float32).copy()
        return rc, self._take(sc)[0], bev


# ---------------------------------------------------------------- the cases ----------------------------------------------------------------
def _cfg(oracle, **kw):
    return KC.make_cfg(oracle.L, **kw)


def _oracle_ok(be, od, d, what):
    bad = compare_desc(od, d, float_exact=be.float_exact)
    assert not bad, (what, bad[:6])


def case_round_trip(be, oracle, n, max_batch):
    """the defining property: ingest(debug) -> (desc, bev, pix_rc); ingest_images(bev, pix_rc, desc.min_bin_val) gives desc and the
    label images byte for byte; the positions handed back are never touched by the clamp; and, with no K1 of the product involved,
    the oracle's image and positions give the oracle's descriptor"""
    cfg = _cfg(oracle)
    clouds = round_trip_clouds()[:n] if n < 9 else round_trip_clouds()
    h = be.open(cfg, max_batch)
    ref, rdbg = be.points(h, clouds, True)
    occ = rdbg["bev"] > EMPTY
    assert np.array_equal(clamp(rdbg["pix_rc"], cfg)[occ], rdbg["pix_rc"][occ]), "K1's own positions lie inside their cells"
    d, dbg = be.images(h, rdbg["bev"], rdbg["pix_rc"], ref["min_bin_val"], True)
    same(ref, d, rdbg, dbg)
    plain, _ = be.images(h, rdbg["bev"], rdbg["pix_rc"], ref["min_bin_val"], False)
    same(ref, plain)
    # min_height = None on the clouds whose lowest accepted point owns its cell (the terrain clouds: mostly one point per cell)
    own = [i for i in range(len(clouds)) if ref["min_bin_val"][i] == rdbg["bev"][i][occ[i]].min()]
    assert len(own) >= (1 if n == 1 else 3), own
    d2, _ = be.images(h, rdbg["bev"][own], rdbg["pix_rc"][own], None, False)
    same(ref[own], d2)
    # the oracle's image and positions -> the oracle's descriptor
    oo = [oracle_of(oracle, ("rt", i), clouds[i]) for i in range(len(clouds))]
    d3, dbg3 = be.images(h, np.stack([o[1] for o in oo]), np.stack([o[2] for o in oo]), np.array([o[0]["min_bin_val"] for o in oo], np.float32), True)
    be.close(h)
    for i, o in enumerate(oo):
        _oracle_ok(be, o[0], d3[i], ("round trip, oracle", i))
        assert np.array_equal(dbg3["bev"][i], o[1]) and np.array_equal(dbg3["pix_rc"][i], o[2]), i


def case_default_positions_and_sanitising(be, oracle):
    cfg = _cfg(oracle)
    s = small_scene()
    img, cloud = scene_image(s, cfg), centre_cloud(s, cfg, 1)
    od, obev, opix = oracle_of(oracle, "small", cloud)
    assert np.array_equal(obev, img) and np.array_equal(opix[img > EMPTY], centres(cfg)[img > EMPTY]), "the helper's cloud is the image"
    h = be.open(cfg, 8)
    ref, rdbg = be.points(h, [cloud], True)
    d0, dbg0 = be.images(h, img[None], None, None, True)
    d1, dbg1 = be.images(h, img[None], centres(cfg)[None], None, True)
    same(d0, d1, dbg0, dbg1)                      # NULL positions are the centres
    same(ref, d0, rdbg, dbg0)                     # ... and the point path on one point per cell centre
    _oracle_ok(be, od, d0[0], "centres")
    ebev, epix = expect_debug(img[None], None, cfg)
    assert np.array_equal(dbg0["bev"], ebev) and np.array_equal(dbg0["pix_rc"], epix)
    # sanitising: the empties written four ways, tall values in row 0
    dirty = []
    for fill in (np.float32(-1000.0), np.float32(-1000.5), np.float32(-np.inf), np.float32(np.nan)):
        x = img.copy()
        x[img <= EMPTY] = fill
        x[:cfg.n_col] = np.float32(3.7)
        dirty.append(x)
    dd, ddbg = be.images(h, np.stack(dirty), None, None, True)
    for i in range(len(dirty)):
        same(d0, dd[i:i + 1])
        assert np.array_equal(ddbg["bev"][i], img) and np.array_equal(ddbg["pix_rc"][i], epix[0]), i
    # wild position components in a few occupied cells, on positions that are not the centres
    rng = np.random.default_rng(5)
    pos = (centres(cfg) + rng.uniform(-0.4, 0.4, (cfg.n_row * cfg.n_col, 2))).astype(np.float32)
    occ = np.flatnonzero(img > np.float32(cfg.lv_grads[0]))
    bad = pos.copy()
    picks = occ[:: max(len(occ) // 12, 1)][:12]
    wild = [np.float32(np.nan), None, np.float32(1e30), np.float32(-5.0)]
    for k, c in enumerate(picks):
        w = wild[k % 4]
        comp = (k // 4) % 2
        bad[c, comp] = w if w is not None else centres(cfg)[c, comp] + np.float32(0.75)
    bad[picks[0], :] = np.float32(np.nan)          # both components of one cell
    fixed = clamp(bad[None], cfg)[0]
    assert int((fixed != pos).sum()) >= len(picks) and np.array_equal(fixed[fixed != pos], centres(cfg)[fixed != pos])
    dw, wdbg = be.images(h, np.stack([img, img]), np.stack([bad, fixed]), None, True)
    be.close(h)
    same(dw[:1], dw[1:])
    assert dw[:1].tobytes() != d0.tobytes(), "the jittered positions change the descriptor: the comparison shows something"
    wb, wp = expect_debug(np.stack([img, img]), np.stack([bad, fixed]), cfg)
    assert np.array_equal(wdbg["bev"], wb) and np.array_equal(wdbg["pix_rc"], wp)
    assert np.array_equal(wdbg["pix_rc"][0], wdbg["pix_rc"][1])


def case_list_edges(be, oracle, which):
    """the capacities of the list, written directly as images; each against the point path on the one-point-per-cell cloud (bytes) and
    the oracle (compare_desc)"""
    kw, want = {}, None
    if which == "entries":
        scenes, want = [plateau_scene(LIST_CAP - 1), plateau_scene(LIST_CAP), plateau_scene(LIST_CAP + 1)], [{"list"}, {"list"}, {"mid"}]
    elif which == "slots":
        scenes, want = [tall_scene()], [{"mid"}]
    elif which == "components":
        scenes, want = [blob_scene()], [{"big"}]
    else:
        scenes, kw, want = [small_scene(), plateau_scene(LIST_CAP - 1)], {"min_cont_cell_cnt": 4}, [{"mid"}, {"mid"}]
    cfg = _cfg(oracle, **kw)
    imgs = np.stack([scene_image(s, cfg) for s in scenes])
    clouds = [centre_cloud(s, cfg, 3 + i) for i, s in enumerate(scenes)]
    oo = [oracle_of(oracle, (which, i), clouds[i], cfg) for i in range(len(scenes))]
    # the preconditions, on the image and the oracle
    cs = [counts(im, cfg) for im in imgs]
    if which == "entries":
        assert [c[0] for c in cs] == [LIST_CAP - 1, LIST_CAP, LIST_CAP + 1] and all(c[1] <= SLOT_CAP for c in cs), cs
    elif which == "slots":
        assert cs[0][0] < LIST_CAP and cs[0][1] > SLOT_CAP, cs
    elif which == "components":
        assert cs[0][0] <= LIST_CAP and cs[0][1] <= SLOT_CAP and int(oo[0][0]["n_cont"].max()) > MAXC, (cs, oo[0][0]["n_cont"])
    else:
        assert all(c[0] <= LIST_CAP and c[1] <= SLOT_CAP for c in cs), cs
    for i in range(len(scenes)):
        assert np.array_equal(oo[i][1], imgs[i]), "the helper's cloud is the image"
    h = be.open(cfg, 8)
    ref, rdbg = be.points(h, clouds, True)
    d, dbg = be.images(h, imgs, None, None, True)
    same(ref, d, rdbg, dbg)
    plain, _ = be.images(h, imgs, None, None, False)   # without the debug outputs: the dense branch only where the list overflows
    paths = be.paths()
    pc = be.path_counts()                              # the call's counts by body, from cc_ingest_path_counts: every back end has them
    assert all(len(w) == 1 for w in want) and {k: pc[k] for k in ("list", "mid", "big")} == {k: sum(w == {k} for w in want) for k in ("list", "mid", "big")}, (which, pc)
    same(ref, plain)
    be.close(h)
    for i in range(len(scenes)):
        _oracle_ok(be, oo[i][0], plain[i], (which, i))
        if paths is not None:
            got = {k for k, v in paths.items() if i in v}
            assert got and got <= want[i], (which, i, paths)


def case_empty_and_tiny(be, oracle):
    cfg = _cfg(oracle)
    ncell = cfg.n_row * cfg.n_col
    one = KC.Scene().cell(20, 30, KC.H(3))
    img1 = scene_image(one, cfg)
    p1 = np.zeros((1, 4), np.float32)
    p1[0, :3] = (20 - 75 + 0.5, 30 - 75 + 0.5, np.float32(grid_h(KC.H(3))) - np.float32(cfg.lidar_height))
    h = be.open(cfg, 4)
    ref, rdbg = be.points(h, [blind_cloud(), blind_cloud(p1)], True)
    d, dbg = be.images(h, np.stack([np.full(ncell, EMPTY, np.float32), img1]), None, None, True)
    be.close(h)
    same(ref, d, rdbg, dbg)
    assert d["n_pix"].tolist() == [0, 1] and d["n_cont"].sum() == 0
    assert d["max_bin_val"][0] == EMPTY and d["min_bin_val"][0] == np.float32(1000.0)   # K1's values for a cloud without an accepted point
    assert d["max_bin_val"][1] == d["min_bin_val"][1] == np.float32(grid_h(KC.H(3)))
