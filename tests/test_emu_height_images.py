"""cc_ingest_images and its siblings (include/cont2_amd_images.h) on the CPU harness: descriptors from caller-made max-height
images.  The cases are tests/height_images.py's; the references are cc_ingest_batch on clouds and the oracle, never the new code
alone.  The harness build prints which K2 body took each scan (CC_EMU_TRACE_K2); the capacity cases assert it."""
import ctypes as C

import numpy as np
import pytest

import cc_amd
import height_images as HI
from parity import compare_desc


class EmuBack:
    float_exact = True

    def __init__(self, oracle, capfd=None):
        self.api = HI.ImagesApi(oracle.L)
        self.capfd = capfd
        self._paths = self._counts = None

    def open(self, cfg, max_batch):
        return self.api.create(cfg=cfg, max_batch=max_batch)

    def close(self, h):
        self.api.lib.cc_destroy(h)

    def points(self, h, clouds, debug):
        offs = np.concatenate([[0], np.cumsum([len(s) for s in clouds])]).astype(np.int64)
        out = self.api.ingest(h, np.concatenate(clouds, 0), offs, debug=debug)
        return out if debug else (out, None)

    def read_counts(self, h):
        out = (C.c_int32 * 6)()
        self.api.chk(self.api.lib.cc_ingest_path_counts(h, out), "cc_ingest_path_counts")
        return np.array(out[:], np.int64)

    def images(self, h, height, pos, mins, debug):
        if self.capfd is not None:
            self.capfd.readouterr()
        before = self.read_counts(h)
        out = self.api.ingest_images(h, height, pos, mins, debug=debug)
        d = self.read_counts(h) - before
        self._counts = {"list": len(height) - int(d[0]), "mid": int(d[0] - d[5]), "big": int(d[5]), "why": [int(v) for v in d[1:5]]}
        if self.capfd is not None:   # (test_emu_keys.py's reading of the trace)
            err = self.capfd.readouterr().err.splitlines()
            handed = {int(l.split("scan")[1].split()[0]) for l in err if "handed to the mid path" in l}
            big = {int(l.split("scan")[1]) for l in err if l.startswith("[k2 big] scan")}
            every = set(range(len(height)))
            assert big <= handed <= every, (handed, big)
            self._paths = {"list": every - handed, "mid": handed - big, "big": big}
            # the getter's own test: the counters of cc_ingest_path_counts agree with the trace lines -- the counts per body, the sum of
            # the reasons, and as many reasons in use as the trace names hand-off lines (topology_cases._call holds each reason's count)
            lines = {int(l.split("line")[1].split(")")[0]) for l in err if "handed to the mid path" in l}
            assert {k: len(v) for k, v in self._paths.items()} == {k: self._counts[k] for k in ("list", "mid", "big")}, (self._paths, self._counts)
            assert sum(self._counts["why"]) == len(handed) and sum(1 for w in self._counts["why"] if w) == len(lines), (self._counts, lines)
        return out if debug else (out, None)

    def paths(self):
        return self._paths

    def path_counts(self):
        return self._counts


@pytest.mark.parametrize("n,max_batch", [(1, 9), (9, 9), (9, 4)])   # one scan; one chunk; three chunks (the minima cross chunks)
def test_round_trip(oracle, n, max_batch):
    HI.case_round_trip(EmuBack(oracle), oracle, n, max_batch)


def test_default_positions_and_sanitising(oracle):
    HI.case_default_positions_and_sanitising(EmuBack(oracle), oracle)


@pytest.mark.parametrize("which", ["entries", "slots", "components", "min_cont_cell_cnt"])
def test_list_edges(oracle, capfd, monkeypatch, which):
    monkeypatch.setenv("CC_EMU_TRACE_K2", "1")
    HI.case_list_edges(EmuBack(oracle, capfd), oracle, which)


def test_empty_and_tiny(oracle):
    HI.case_empty_and_tiny(EmuBack(oracle), oracle)


def test_refusals(oracle):
    """NULL height, a negative n, a device base off by 4 bytes (height, positions) and a NULL out: CC_EINVAL with the entry point's
    name; after each the next good call gives the right bytes; n == 0 is CC_OK; the host call takes an unaligned host pointer"""
    cfg = oracle.L.default_manager_cfg()
    api = HI.ImagesApi(oracle.L)
    ctx = api.create(max_batch=4)
    s = HI.small_scene()
    img = HI.scene_image(s, cfg)
    buf = np.zeros(2 * len(img) + 8, np.float32)
    a0 = (-buf.ctypes.data % 16) // 4
    two = buf[a0:a0 + 2 * len(img)].reshape(2, -1)
    two[:] = img
    assert two.ctypes.data % 16 == 0
    pos = np.ascontiguousarray(np.broadcast_to(HI.centres(cfg), (2,) + HI.centres(cfg).shape))
    assert pos.ctypes.data % 8 == 0
    ref = api.ingest_images(ctx, two, pos)
    bad = {
        "NULL height": dict(height=None, n=2),
        "negative n": dict(n=-1),
        "height off by 4 bytes": dict(hptr=two.ctypes.data + 4, n=1),
        "positions off by 4 bytes": dict(pptr=pos.ctypes.data + 4, n=1),
    }
    for what, over in bad.items():
        a = dict(height=two, pos=pos, n=None, hptr=None, pptr=None)
        a.update(over)
        rc, _, _ = api.ingest_images_rc(ctx, a["height"], a["pos"], None, n=a["n"], hptr=a["hptr"], pptr=a["pptr"])
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_images:"), (what, api.lib.cc_last_error())
        assert api.ingest_images(ctx, two, pos).tobytes() == ref.tobytes(), what
    assert api.lib.cc_ingest_images(ctx, two.ctypes.data, None, 2, None, None, None, None) == -1          # NULL out
    assert api.lib.cc_ingest_images(None, two.ctypes.data, None, 2, None, two.ctypes.data, None, None) == -1   # NULL ctx
    rc, d0, _ = api.ingest_images_rc(ctx, two, pos, None, n=0)
    assert rc == 0
    # the host call: the same refusals, and an unaligned host pointer is fine
    for what, kw in {"NULL height": dict(height=None, n=2), "negative n": dict(height=two, n=-1), "NULL out": dict(height=two, out=False)}.items():
        rc, _, _ = api.ingest_images_host_rc(ctx, kw["height"], None, None, n=kw.get("n"), out=kw.get("out", True))
        assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_images_host:"), what
    assert api.ingest_images_host_rc(ctx, two, None, None, n=0)[0] == 0
    raw = np.zeros(4 * (len(img) + 2) + 1, np.uint8)
    off = (-raw.ctypes.data % 16) + 1
    raw[off:off + 4 * len(img)] = img.view(np.uint8)
    assert (raw.ctypes.data + off) % 4 == 1
    rc, dh, _ = api.ingest_images_host_rc(ctx, None, None, None, n=1, hptr=raw.ctypes.data + off)
    assert rc == 0 and not compare_desc(ref[0], dh[0], float_exact=True)
    # the per-scan call
    rc, _, _ = api.scan_ingest_image_rc(ctx, None)
    assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_image:")
    rc, _, _ = api.scan_ingest_image_rc(ctx, img, out=False)
    assert rc == -1 and api.lib.cc_last_error().decode().startswith("cc_scan_ingest_image:")
    assert api.ingest_images(ctx, two, pos).tobytes() == ref.tobytes()
    api.lib.cc_destroy(ctx)


def test_per_scan_and_host_calls(oracle):
    """cc_scan_ingest_image gives cc_ingest_images_host's descriptor, with and without want_bev; cc_scan_bev and the host call's h_bev
    are the sanitised image; positions, minima and chunks (max_batch = 2, three images) go through the host call"""
    cfg = oracle.L.default_manager_cfg()
    api = HI.ImagesApi(oracle.L)
    ctx = api.create(max_batch=2)
    clouds = HI.round_trip_clouds()[:3]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in clouds])]).astype(np.int64)
    ref, rdbg = api.ingest(ctx, np.concatenate(clouds, 0), offs, debug=True)
    dirty = rdbg["bev"].copy()
    dirty[:, :cfg.n_col] = 3.3          # row 0 is cleared on the way in
    rc, dh, bev = api.ingest_images_host_rc(ctx, dirty, rdbg["pix_rc"], ref["min_bin_val"], want_bev=True)
    assert rc == 0 and np.array_equal(bev, rdbg["bev"])
    for i in range(3):
        assert not compare_desc(ref[i], dh[i], float_exact=True), i
        for want_bev in (False, True):
            rc, d, b = api.scan_ingest_image_rc(ctx, dirty[i], rdbg["pix_rc"][i], ref["min_bin_val"][i], want_bev)
            assert rc == 0 and not compare_desc(dh[i], d, float_exact=True), (i, want_bev)
            assert b is None or np.array_equal(b, rdbg["bev"][i])
    # without positions and minimum: the centres and the minimum over the occupied cells
    rc, dc, _ = api.ingest_images_host_rc(ctx, dirty[:1])
    rc2, d, _ = api.scan_ingest_image_rc(ctx, dirty[0])
    assert rc == 0 and rc2 == 0 and not compare_desc(dc[0], d, float_exact=True)
    assert d["min_bin_val"] == HI.default_min(dirty[:1], cfg)[0] and d["max_bin_val"] == ref["max_bin_val"][0]
    api.lib.cc_destroy(ctx)


def test_host_and_per_scan_calls_return_the_device_calls_bytes(oracle):
    """Three images, with positions and minima and without: cc_ingest_images_host and cc_scan_ingest_image return the BYTES of
    cc_ingest_images into zeroed memory -- also behind a descriptor's counts, where the per-scan call's pool slot holds an earlier
    scan's rows (scan 0 comes by again behind scan 2).  A position read at a wrong place in the staged copy changes the bytes:
    the case without positions differs from the one with them."""
    api = HI.ImagesApi(oracle.L)
    ctx = api.create(max_batch=3)
    clouds = HI.round_trip_clouds()[:3]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in clouds])]).astype(np.int64)
    ref, rdbg = api.ingest(ctx, np.concatenate(clouds, 0), offs, debug=True)
    dev = {}
    for pos, mins in ((rdbg["pix_rc"], ref["min_bin_val"]), (None, None)):
        d3 = dev[pos is None] = api.ingest_images(ctx, rdbg["bev"], pos, mins)
        rc, dh, _ = api.ingest_images_host_rc(ctx, rdbg["bev"], pos, mins)
        assert rc == 0 and dh.tobytes() == d3.tobytes()
        for i in (0, 1, 2, 0):
            rc, d, _ = api.scan_ingest_image_rc(ctx, rdbg["bev"][i], None if pos is None else pos[i], None if mins is None else mins[i])
            assert rc == 0 and d.tobytes() == d3[i].tobytes(), i
    assert dev[False].tobytes() == ref.tobytes() and dev[True].tobytes() != ref.tobytes()
    api.lib.cc_destroy(ctx)


def test_a_drive_through_images_answers_like_the_drive_through_points(cc, oracle):
    """64 scans of a short drive: ingest -> add_scans -> query, and the same with the scans handed over as images: equal result records"""
    L = oracle.L
    n = 64
    x, _, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), beams=16, azim=450)
    xs = x.numpy().reshape(-1, 4)
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    d = L.default_db_cfg()
    d.max_elapse, d.min_elapse = 2.5, 1.5
    api = HI.ImagesApi(L)
    ctx = api.create(max_batch=16)
    ref, rdbg = api.ingest(ctx, xs, offs, debug=True)
    got = api.ingest_images(ctx, rdbg["bev"], rdbg["pix_rc"], ref["min_bin_val"])
    assert got.tobytes() == ref.tobytes()
    seeds, qs = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    res = []
    for desc in (ref, got):
        db = api.db_create(ctx, d, cap=n)
        api.db_add(db, desc, ts, seeds)
        res.append(api.db_query(db, desc, qs))
        api.lib.cc_db_destroy(db)
    assert (res[0]["n_res"] > 0).sum() >= 3, "the drive closes loops"
    assert res[0].tobytes() == res[1].tobytes()
    api.lib.cc_destroy(ctx)


def test_python_binding_shapes(cc):
    """Context.ingest_images' shape checks, as far as they go without a device"""
    class Ctx:
        cfg = cc.L.default_manager_cfg()
        n_cell = 150 * 150
    f = cc.Context._images
    assert f(Ctx, np.zeros((3, 22500), np.float32), None) == 3 and f(Ctx, np.zeros((2, 150, 150), np.float32), np.zeros((2, 22500, 2), np.float32)) == 2
    for h, p in ((np.zeros(22500), None), (np.zeros((2, 100)), None), (np.zeros((2, 150, 149)), None), (np.zeros((2, 22500)), np.zeros((3, 22500, 2))),
                 (np.zeros((2, 22500)), np.zeros((2, 22500, 3)))):
        with pytest.raises(ValueError):
            f(Ctx, h, p)
    with pytest.raises(ValueError):
        cc.calls.ingest_images(None, None, 0, None, 2, min_height=[1.0])
    assert set(cc.EXPORTS_EXT) == {"cc_ingest_images", "cc_ingest_images_host", "cc_scan_ingest_image"}
    assert C.sizeof(cc.IngestDebug) == 24
