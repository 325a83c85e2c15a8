"""Every K1 instance's answers and launches, to compare two builds of the library: the leaf walk of tests/k1_instances.py on the device
(11 point sources x two resolutions x the split and the whole-scan path, scans of 40 001 points and 32 x 1 251 range images), then one
*_host call and one cc_scan_ingest* call per family (coordinates as one record array and as three arrays, images with positions).  Prints one line per call with a digest of the descriptors it returned.

  drive:    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv json -d DIR -o r -- \\
                python profiles/k1_sources/measure_k1_sources.py                (CC_AMD_LIB=<other build> for the other side)
  extract:  python profiles/k1_sources/measure_k1_sources.py --lists DIR > lists.txt
            per hardware queue (numbered in the order they first appear) the ordered (kernel, grid, workgroup, LDS) of its launches,
            then the ordered (direction, bytes) of the copies.  The K1 kernels' names are written as this tree has them (a build from
            before the point sources has ten kernel templates: cc_k_rasterize_rec<4, true, false, 12> is
            cc_k_rasterize<4, true, false, cc_src_rec<12>> here), so the lists of two builds can be compared line by line.
  table:    python profiles/k1_sources/measure_k1_sources.py --resources kernel_resources_parent.txt kernel_resources_this_tree.txt
            the K1 rows of two tests/kernel_resources.py outputs side by side under this tree's names; rows that differ are marked."""
import csv
import ctypes as C
import glob
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def drive():
    import torch
    import cc_amd
    import oracle_py
    import k1_instances as K1
    from point_layouts import repack
    from point_motion import repack_with_time
    from point_segments import Segments
    from test_gpu_k1_instances import H, N_PTS, W, GpuDriver, beam_clouds
    cc = cc_amd.load()
    L = cc.L
    oracle_py.lib()
    inp = K1.Inputs(N_PTS, H, W, beam_clouds(cc, max(K1.BATCHES)))
    visited = K1.walk(GpuDriver(cc), L, oracle_py, inp, float_exact=False,
                      on_leaf=lambda reso, nb, leaf, d: print("%-5s n=%d %-9s %s" % (reso, nb, leaf, digest(d)), flush=True))
    K1.assert_every_leaf(visited)

    # one *_host call and one per-scan call per family, three scans (one scan), default resolution
    nb = 3
    ctx = cc.Context(0, max_batch=nb)
    offs, cat = inp.offs(nb), np.concatenate(inp.raw[:nb], 0)
    tfs = inp.tfs[:nb]
    w = np.linspace(-1.0, 1.0, len(cat)).astype(np.float32).view(np.uint32)
    segs = [[(inp.raw[i][:9000], (12, 0), tfs[i]), (inp.raw[i][9000:30001], (32, 0), tfs[i]), (inp.raw[i][30001:], (48, 8), tfs[i])] for i in range(nb)]
    seg_host = [[(repack(x, *lay), lay, tf) for (x, lay, tf) in sc] for sc in segs]
    s = inp.sensors["u16"]
    m = L.RangeModel(s.H, s.W, cc.RANGE_WORDS[s.word][0], cc.RANGE_ORDERS[s.order], float(s.range_scale), float(s.origin_n), float(s.origin_z), s.K,
                     s.row_tab.ctypes.data, s.col_cs.ctypes.data, None)
    sensor = cc.RangeSensor(ctx, m, s.word)

    def say(name, d):
        print("%-32s %s" % (name, digest(d)), flush=True)

    say("cc_ingest_host", ctx.ingest_host(cat, offs))
    say("cc_ingest_points_host", ctx.ingest_host(repack(cat, 48, 8), offs, layout=(48, 8), tf=tfs))
    say("cc_ingest_points_motion_host", ctx.ingest_host(repack_with_time(cat, w, 32, 0, 20), offs, layout=(32, 0), motion=(20, "f32"),
                                                        t_begin=np.full(nb, -0.25, np.float32), scale=np.full(nb, 7.5, np.float32), knots=tfs.reshape(nb, 1, 12)))
    say("cc_ingest_segments_host", ctx.ingest_segments_host(seg_host))
    say("cc_ingest_ranges_host", ctx.ingest_ranges_host(sensor, inp.images["u16"][:nb]))
    # the later families: records dropped by a u8 class word at byte 12; f64 coordinates as ONE record array (a [N, 3] view of [N, 4]
    # rows) and as three arrays, an origin per scan; images with positions (K1's own of the same scans, made on the device first)
    words = (np.arange(len(cat)) % 7).astype(np.uint8)
    rec = repack(cat, 16, 0).reshape(-1, 16).copy()
    rec[:, 12] = words
    rec = rec.reshape(-1)
    keep = cc.PointFilter.classes(12, "u8", drop=[3, 5])
    say("cc_ingest_points_filtered_host", ctx.ingest_host(rec, offs, layout=(16, 0), tf=tfs, keep=keep))
    org = np.tile(np.array([[448000.0, 5412000.0, 300.0]]), (nb, 1)) + np.arange(nb)[:, None]
    xyz = np.zeros((len(cat), 4), np.float64)
    xyz[:, :3] = cat[:, :3].astype(np.float64) + np.repeat(org, np.diff(offs), 0)
    cols = tuple(np.ascontiguousarray(xyz[:, k]) for k in range(3))
    say("cc_ingest_coords_host records", ctx.ingest_coords_host(xyz[:, :3], offs, origin=org, tf=tfs))
    say("cc_ingest_coords_host columns", ctx.ingest_coords_host(cols, offs, origin=org, tf=tfs))
    dimg, dbg = ctx.ingest(torch.from_numpy(np.ascontiguousarray(cat, np.float32)).cuda(), offs, debug=True)
    torch.cuda.synchronize()
    height, pos = dbg["bev"].cpu().numpy(), dbg["pix_rc"].cpu().numpy()
    mins = cc.desc_to_numpy(dimg)["min_bin_val"]
    say("cc_ingest_images_host", ctx.ingest_images_host(height, pos, mins))

    lib = cc.lib()
    for f in ("cc_scan_ingest", "cc_scan_ingest_points", "cc_scan_ingest_points_motion", "cc_scan_ingest_segments", "cc_scan_ingest_ranges", "cc_scan_desc",
              "cc_scan_release"):
        getattr(lib, f).restype = C.c_int
    lib.cc_scan_desc.argtypes = [C.c_void_p, C.c_void_p]
    lib.cc_scan_release.argtypes = [C.c_void_p]
    lib.cc_scan_ingest.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]

    def take(name, rc, sc):
        assert rc == 0, (name, lib.cc_last_error())
        p = C.c_void_p()
        assert lib.cc_scan_desc(sc, C.byref(p)) == 0, lib.cc_last_error()
        say(name, np.frombuffer(C.string_at(p, L.scan_desc_dt.itemsize), np.uint8))
        assert lib.cc_scan_release(sc) == 0

    one, n1, tf1 = np.ascontiguousarray(inp.raw[0]), len(inp.raw[0]), np.ascontiguousarray(tfs[:1])
    sc = C.c_void_p()
    take("cc_scan_ingest", lib.cc_scan_ingest(ctx.h, one.ctypes.data, n1, 0, C.byref(sc)), sc)
    lay = L.PointLayout(48, 8)
    buf = repack(one, 48, 8)
    take("cc_scan_ingest_points", lib.cc_scan_ingest_points(ctx.h, buf.ctypes.data, C.addressof(lay), n1, tf1.ctypes.data, 0, C.byref(sc)), sc)
    lay, mo = L.PointLayout(32, 0), L.PointMotion(20, L.TIME_F32, 1, 0)
    buf, tm = repack_with_time(one, w[:n1], 32, 0, 20), np.array([[-0.25, 7.5]], np.float32)
    take("cc_scan_ingest_points_motion", lib.cc_scan_ingest_points_motion(ctx.h, buf.ctypes.data, C.addressof(lay), C.addressof(mo), n1, tm.ctypes.data,
                                                                          tf1.ctypes.data, 0, C.byref(sc)), sc)
    hs = Segments([[(x, lay_, tf, 0) for (x, lay_, tf) in segs[0]]])
    take("cc_scan_ingest_segments", lib.cc_scan_ingest_segments(ctx.h, C.cast(hs.arr, C.c_void_p), 3, 0, C.byref(sc)), sc)
    im = np.ascontiguousarray(inp.images["u16"][0])
    take("cc_scan_ingest_ranges", lib.cc_scan_ingest_ranges(ctx.h, sensor.h, im.ctypes.data, None, 0, C.byref(sc)), sc)
    calls = cc.calls
    lay = L.PointLayout(16, 0)
    take("cc_scan_ingest_points_filtered", calls.scan_ingest_points_filtered(lib, ctx.h, rec.ctypes.data, lay, keep._c, n1, tf1, 0, sc), sc)
    x1 = np.ascontiguousarray(xyz[:n1])
    src = calls.coord_src(x1.ctypes.data, x1.ctypes.data + 8, x1.ctypes.data + 16, "float64", 32)
    take("cc_scan_ingest_coords records", calls.scan_ingest_coords(lib, ctx.h, src, n1, org[0], tf1, 0, sc), sc)
    c1 = [np.ascontiguousarray(c[:n1]) for c in cols]
    src = calls.coord_src(c1[0].ctypes.data, c1[1].ctypes.data, c1[2].ctypes.data, "float64", 8)
    take("cc_scan_ingest_coords columns", calls.scan_ingest_coords(lib, ctx.h, src, n1, org[0], tf1, 0, sc), sc)
    h1, p1 = np.ascontiguousarray(height[0]), np.ascontiguousarray(pos[0])
    take("cc_scan_ingest_image", calls.scan_ingest_image(lib, ctx.h, h1.ctypes.data, p1.ctypes.data, float(mins[0]), 0, sc), sc)
    torch.cuda.synchronize()
    sensor.close()
    ctx.close()


def this_tree_name(name):
    """a K1 kernel's name as this tree has it (spaces dropped), whichever build it comes from"""
    n = re.sub(r"^void", "", name.replace(" ", ""))   # (a template's name comes with its return type, a plain function's without)
    m = re.match(r"^cc_k_rasterize(_merge)?(_rec|_mot|_rng|_seg)?(<(.*)>)?$", n)
    if not m or "cc_src_" in n:
        return n
    merge, fam, args = m.group(1), m.group(2), (m.group(4).split(",") if m.group(4) else [])
    if merge:
        src = {None: "cc_src_kitti", "_seg": "cc_src_seg"}.get(fam) or "cc_src%s<%s>" % (fam, args[0])
        return "cc_k_rasterize_merge<%s>" % src
    if fam is None and len(args) == 2:
        args.append("false")   # (PART's default)
    src = {None: "cc_src_kitti", "_seg": "cc_src_seg"}.get(fam) or "cc_src%s<%s>" % (fam, args[3])
    return "cc_k_rasterize<%s,%s>" % (",".join(args[:3]), src)


def lists(d):
    def rows(pat):
        fs = sorted(glob.glob(os.path.join(d, "**", pat), recursive=True))
        return [r for f in fs for r in csv.DictReader(open(f))]

    def dims(r, k):
        return "x".join(r[k + s] for s in ("_X", "_Y", "_Z")) if k + "_X" in r else r[k]

    per_q, order = {}, []
    for r in sorted(rows("*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"])):
        q = (r.get("Agent_Id"), r.get("Queue_Id"))
        if q not in per_q:
            per_q[q] = []
            order.append(q)
        name = r["Kernel_Name"]
        name = this_tree_name(name.split("(")[0]) if "cc_k_" in name else name
        per_q[q].append("%s grid %s wg %s lds %s" % (name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r.get("LDS_Block_Size", "?")))
    for i, q in enumerate(order):
        print("== queue %d: %d launches" % (i, len(per_q[q])))
        print("\n".join(per_q[q]))
    cp = sorted(rows("*memory_copy_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))

    def find(x, key):  # the lists under `key`, wherever the JSON keeps them
        if isinstance(x, dict):
            return [v for k, v in x.items() if k == key and isinstance(v, list)] + [f for v in x.values() for f in find(v, key)]
        return [f for v in x for f in find(v, key)] if isinstance(x, list) else []

    recs = [c for f in sorted(glob.glob(os.path.join(d, "**", "*results.json"), recursive=True)) for l in find(json.load(open(f)), "memory_copy") for c in l]
    recs.sort(key=lambda c: int(c.get("start_timestamp", 0)))
    print("== copies: %d" % len(cp))
    for i, r in enumerate(cp):
        print("%s %s" % (r.get("Direction", "?"), recs[i].get("bytes", "?") if len(recs) == len(cp) else "?"))


def resources(parent, tree):
    def load(f):
        out = {}
        for line in open(f):
            if line.startswith("cc_k_rasterize"):
                name, rest = re.match(r"^(.*?)\s+(VGPR .*)$", line.rstrip()).groups()
                out[this_tree_name(name)] = (name.strip(), rest)
        return out

    a, b = load(parent), load(tree)
    assert sorted(a) == sorted(b), sorted(set(a) ^ set(b))
    differ = 0
    for k in sorted(a):
        same = a[k][1] == b[k][1]
        differ += 0 if same else 1
        print("%-46s -> %s\n    parent    %s\n    this tree %s%s" % (a[k][0], b[k][0], a[k][1], b[k][1], "" if same else "   <-- differs"))
    print("%d K1 kernels, %d rows differ" % (len(a), differ))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--lists":
        lists(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--resources":
        resources(sys.argv[2], sys.argv[3])
    else:
        drive()
