"""cc_ingest_images and its siblings (include/cont2_amd_images.h) on the MI355X: cc_k_image_list's 1 024-thread shape (24 cells per
lane in registers, v_mbcnt ranks, DPP scans) exists on hardware only.  The cases are tests/height_images.py's -- the same inputs took
the list, mid and big bodies of K2 on the CPU harness (test_emu_height_images.py asserts that); here the capacity cases assert it on
the counters of cc_ingest_path_counts.  Against
the oracle the ring components of the keys are compared under parity.compare_desc's own bar (the device's exp), everything else to
the bit; against cc_ingest_batch every byte."""

import numpy as np
import pytest

import height_images as HI
from parity import compare_desc

pytestmark = pytest.mark.gpu


def _np(dbg):
    return None if dbg is None else {k: v.cpu().numpy() for k, v in dbg.items()}


class GpuBack:
    float_exact = False

    def __init__(self, cc):
        self.cc = cc
        self._counts = None

    def open(self, cfg, max_batch):
        return self.cc.Context(0, cfg, max_batch=max_batch)

    def close(self, ctx):
        ctx.close()

    def _zeros(self, n):
        import torch
        return torch.zeros((n, self.cc.DESC_BYTES), dtype=torch.uint8, device="cuda")   # rows past n_stored are not written

    def points(self, ctx, clouds, debug):
        import torch
        offs = np.concatenate([[0], np.cumsum([len(s) for s in clouds])]).astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, 0), np.float32)).cuda()
        out = ctx.ingest(x, offs, out=self._zeros(len(clouds)), debug=debug)
        torch.cuda.synchronize()
        return (self.cc.desc_to_numpy(out[0]).copy(), _np(out[1])) if debug else (self.cc.desc_to_numpy(out).copy(), None)

    def images(self, ctx, height, pos, mins, debug):
        import torch
        h = torch.from_numpy(np.ascontiguousarray(height, np.float32)).cuda()
        p = None if pos is None else torch.from_numpy(np.ascontiguousarray(pos, np.float32)).cuda()
        before = ctx.path_counts()
        out = ctx.ingest_images(h, p, mins, out=self._zeros(len(height)), debug=debug)
        after = ctx.path_counts()
        torch.cuda.synchronize()
        mid, big = after["mid"] - before["mid"], after["big"] - before["big"]
        self._counts = {"list": len(height) - mid, "mid": mid - big, "big": big, "why": [a - b for a, b in zip(after["why"], before["why"])]}
        return (self.cc.desc_to_numpy(out[0]).copy(), _np(out[1])) if debug else (self.cc.desc_to_numpy(out).copy(), None)

    def paths(self):
        """per scan only where the counts of the last images() call decide it: all of its scans on one body"""
        c, n = self._counts, sum(self._counts[k] for k in ("list", "mid", "big"))
        return next(({kk: set(range(n)) if kk == k else set() for kk in ("list", "mid", "big")} for k in ("list", "mid", "big") if c[k] == n), None)

    def path_counts(self):
        return self._counts


@pytest.mark.parametrize("n,max_batch", [(1, 9), (9, 9), (9, 4)])   # one scan (K1: split sweep); one chunk; three chunks (the minima cross chunks)
def test_round_trip(cc, oracle, n, max_batch):
    HI.case_round_trip(GpuBack(cc), oracle, n, max_batch)


def test_default_positions_and_sanitising(cc, oracle):
    HI.case_default_positions_and_sanitising(GpuBack(cc), oracle)


@pytest.mark.parametrize("which", ["entries", "slots", "components", "min_cont_cell_cnt"])
def test_list_edges(cc, oracle, which):
    HI.case_list_edges(GpuBack(cc), oracle, which)


def test_empty_and_tiny(cc, oracle):
    HI.case_empty_and_tiny(GpuBack(cc), oracle)


def test_refusals(cc, oracle):
    """NULL height, a negative n, device bases off by 4 bytes: CC_EINVAL, nothing queued -- the next good call gives the right bytes"""
    import torch
    cfg = oracle.L.default_manager_cfg()
    ctx = cc.Context(0, cfg, max_batch=4)
    img = HI.scene_image(HI.small_scene(), cfg)
    h = torch.from_numpy(np.stack([img, img])).cuda()
    p = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(HI.centres(cfg), (2,) + HI.centres(cfg).shape))).cuda()
    assert h.data_ptr() % 16 == 0 and p.data_ptr() % 8 == 0
    out = torch.zeros((2, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    ref = ctx.ingest_images(h, p, out=out.clone()).clone()
    lib = cc.lib()
    for what, args in {"NULL height": (None, p.data_ptr(), 2), "negative n": (h.data_ptr(), p.data_ptr(), -1),
                       "height off by 4 bytes": (h.data_ptr() + 4, p.data_ptr(), 1), "positions off by 4 bytes": (h.data_ptr(), p.data_ptr() + 4, 1)}.items():
        rc = cc.calls.ingest_images(lib, ctx.h, args[0], args[1], args[2], None, out.data_ptr(), None, None)
        assert rc == -1 and lib.cc_last_error().decode().startswith("cc_ingest_images:"), what
        assert torch.equal(ctx.ingest_images(h, p, out=out.clone()), ref), what
    assert cc.calls.ingest_images(lib, ctx.h, h.data_ptr(), None, 0, None, out.data_ptr(), None, None) == 0
    ctx.close()


def test_per_scan_and_host_calls(cc, oracle):
    """cc_scan_ingest_image gives cc_ingest_images_host's descriptor, with and without want_bev; cc_scan_bev is the sanitised image;
    the host call takes an unaligned host pointer"""
    import torch
    cfg = oracle.L.default_manager_cfg()
    be = GpuBack(cc)
    ctx = be.open(cfg, 2)
    clouds = HI.round_trip_clouds()[:3]
    ref, rdbg = be.points(ctx, clouds, True)
    dirty = rdbg["bev"].copy()
    dirty[:, :cfg.n_col] = 3.3
    dh, bev = ctx.ingest_images_host(dirty, rdbg["pix_rc"], ref["min_bin_val"], want_bev=True)
    assert np.array_equal(bev, rdbg["bev"])
    api = HI.ImagesApi(oracle.L, so=cc.LIB_PATH)   # the product library through the C-ABI driver: the calls here take host pointers
    api._cfg = cfg
    for i in range(3):
        assert not compare_desc(ref[i], dh[i], float_exact=True), i
        for want_bev in (False, True):
            rc, d, b = api.scan_ingest_image_rc(ctx.h, dirty[i], rdbg["pix_rc"][i], ref["min_bin_val"][i], want_bev)
            assert rc == 0 and not compare_desc(dh[i], d, float_exact=True), (i, want_bev)
            assert b is None or np.array_equal(b, rdbg["bev"][i])
    raw = np.zeros(4 * (dirty.shape[1] + 2) + 1, np.uint8)
    off = (-raw.ctypes.data % 16) + 1
    raw[off:off + 4 * dirty.shape[1]] = dirty[0].view(np.uint8)
    rc, d1, _ = api.ingest_images_host_rc(ctx.h, None, None, None, n=1, hptr=raw.ctypes.data + off)
    d2 = ctx.ingest_images_host(dirty[:1])
    assert rc == 0 and not compare_desc(d2[0], d1[0], float_exact=True)
    assert d2["min_bin_val"][0] == HI.default_min(dirty[:1], cfg)[0] and d2["max_bin_val"][0] == ref["max_bin_val"][0]
    torch.cuda.synchronize()
    be.close(ctx)


def test_host_and_per_scan_calls_return_the_device_calls_bytes(cc, oracle):
    """Three images, with positions and minima and without: cc_ingest_images_host and cc_scan_ingest_image return the BYTES of
    cc_ingest_images into zeroed memory -- also behind a descriptor's counts, where the per-scan call's pool slot holds an earlier
    scan's rows (scan 0 comes by again behind scan 2)"""
    cfg = oracle.L.default_manager_cfg()
    be = GpuBack(cc)
    ctx = be.open(cfg, 3)
    ref, rdbg = be.points(ctx, HI.round_trip_clouds()[:3], True)
    api = HI.ImagesApi(oracle.L, so=cc.LIB_PATH)   # the product library through the C-ABI driver: the calls here take host pointers
    api._cfg = cfg
    for pos, mins in ((rdbg["pix_rc"], ref["min_bin_val"]), (None, None)):
        d3, _ = be.images(ctx, rdbg["bev"], pos, mins, False)
        assert ctx.ingest_images_host(rdbg["bev"], pos, mins).tobytes() == d3.tobytes()
        for i in (0, 1, 2, 0):
            rc, d, _ = api.scan_ingest_image_rc(ctx.h, rdbg["bev"][i], None if pos is None else pos[i], None if mins is None else mins[i])
            assert rc == 0 and d.tobytes() == d3[i].tobytes(), i
    be.close(ctx)


def test_a_drive_through_images_answers_like_the_drive_through_points(cc, oracle):
    """64 scans of a short drive: ingest -> add_scans -> query, and the same with the scans handed over as images: equal result records"""
    import torch
    L = oracle.L
    n = 64
    x, _, ts = cc.synth.make_sequence(n, world=cc.synth.World(loop_len=40.0), beams=16, azim=450)
    offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
    d = L.default_db_cfg()
    d.max_elapse, d.min_elapse = 2.5, 1.5
    ctx = cc.Context(0, max_batch=16)
    zeros = lambda: torch.zeros((n, cc.DESC_BYTES), dtype=torch.uint8, device="cuda")
    ref, rdbg = ctx.ingest(x.reshape(-1, 4).cuda(), offs, out=zeros(), debug=True)
    mins = cc.desc_to_numpy(ref)["min_bin_val"].copy()
    got = ctx.ingest_images(rdbg["bev"], rdbg["pix_rc"], mins, out=zeros())
    assert torch.equal(ref, got)
    seeds, qs = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    res = []
    for desc in (ref, got):
        db = cc.Database(ctx, d, capacity=n)
        db.add_scans(desc, ts, seeds)
        res.append(db.query(desc, qs))
        db.close()
    assert (res[0]["n_res"] > 0).sum() >= 3, "the drive closes loops"
    assert res[0].tobytes() == res[1].tobytes()
    ctx.close()
