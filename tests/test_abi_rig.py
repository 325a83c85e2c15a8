"""The add-on header include/cont2_amd_rig.h against its entry of abi.ADDONS, the way tests/test_abi_filter.py holds its header: every
prototype classified by the binding convention is the table's entry, the library and the CPU harness export the symbols, bind() gives
them their types, and cc_rig_segment_t is laid out as the C and the C++ compiler lay it out."""
import ctypes as C
import os
import subprocess

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_rig.h"
CALLS = {"cc_ingest_rig", "cc_ingest_rig_host", "cc_scan_ingest_rig"}


def test_the_headers_entry_matches_the_header(cc):
    assert HDR in cc.abi.ADDONS
    text = open(os.path.join(ROOT, "include", HDR)).read()
    protos, parsed = _prototypes(os.path.join(ROOT, "include", HDR))
    assert len(protos) == len(parsed) == 3 and set(parsed) == CALLS
    table = cc.abi.ADDONS[HDR]
    assert parsed.keys() == table.keys(), parsed.keys() ^ table.keys()
    for name, sig in parsed.items():
        assert table[name] == sig, name
    assert set(table) <= set(cc.EXPORTS_ADDON)
    assert not set(table) & (set(cc.EXPORTS) | set(cc.EXPORTS_EXT))
    assert '#include "cont2_amd.h"' in text and '#include "cont2_amd_filter.h"' in text
    every = [s for t in cc.abi.ADDONS.values() for s in t]
    assert sorted(every) == sorted(cc.EXPORTS_ADDON) and len(set(every)) == len(every)
    # the header says what it leaves out, and the single-step headers point at it
    for word in ("Out of scope", "rule per segment", "more than one filter word", "interpolation", "range images", "64-bit"):
        assert word in text, word
    for other in ("cont2_amd.h", "cont2_amd_filter.h"):
        assert "cont2_amd_rig.h" in open(os.path.join(ROOT, "include", other)).read(), other


def test_symbols_are_exported_and_bound(cc):
    lib = cc.abi.bind(C.CDLL(cc.build()))
    for name, (restype, argtypes) in cc.abi.ADDONS[HDR].items():
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    import emu_api
    emu = cc.abi.bind(C.CDLL(emu_api.build()))
    for name in cc.abi.ADDONS[HDR]:
        assert hasattr(emu, name), name


def test_rig_struct_layout(cc, tmp_path):
    """cc_rig_segment_t as the C compiler and the C++ compiler lay it out (the header's static_asserts are compiled in both languages)
    against layouts.RigSegment, tests/point_rig.py's mirror and the constants"""
    fields = ["points", "n_points", "layout", "mode", "filter_offset", "tf", "time_offset", "time_type", "t_begin", "scale", "knot0", "n_knots"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cont2_amd_rig.h"\nint main(void) { printf("%zu ", sizeof(cc_rig_segment_t));\n' +
                   "".join('printf("%%zu ", offsetof(cc_rig_segment_t, %s));\n' % f for f in fields) +
                   'printf("%d %d %d %d %d %d\\n", CC_RIG_SEG_MAX, CC_RIG_NONE, CC_RIG_TF, CC_RIG_MOTION, CC_SEG_MAX, CC_MOTION_KNOTS_MAX); return 0; }\n')
    S, L = cc.L.RigSegment, cc.L
    exp = [C.sizeof(S)] + [getattr(S, f).offset for f in fields] + [L.RIG_SEG_MAX, L.RIG_NONE, L.RIG_TF, L.RIG_MOTION, L.SEG_MAX, L.MOTION_KNOTS_MAX]
    assert exp[0] == 104 and [f for f, _ in S._fields_] == fields and exp[-6:] == [16, 0, 1, 2, 32, 64]
    assert 8 <= L.RIG_SEG_MAX <= L.SEG_MAX and L.RIG_SEG_MAX & (L.RIG_SEG_MAX - 1) == 0
    for comp, std, name in (("gcc", "-std=c11", "lay_c"), ("g++", "-std=c++17", "lay_cpp")):
        exe = str(tmp_path / name)
        subprocess.check_call([comp, std, "-x", "c" if comp == "gcc" else "c++", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
        assert got == exp, (comp, got, exp)
    import point_rig
    T = point_rig.RigSegment
    assert C.sizeof(T) == 104 and [getattr(T, f).offset for f, _ in T._fields_] == [getattr(S, f).offset for f, _ in S._fields_]


def test_python_segments(cc):
    """SegMotion and the table Context.ingest_rig hands the library: what they put into the struct, and what they refuse"""
    import numpy as np
    import pytest
    L = cc.L
    a = np.zeros(5 * 32, np.uint8)
    b = np.zeros(3 * 16, np.uint8)
    m = cc.SegMotion(12, "u32", np.uint32(4286000000), 1.5e-7, 16, 8)
    arr, scan_segs = cc._rig_table([[(a, (32, 0), m, 16), (b, None, np.arange(12.0), None), (None, "xyzi", None, 12)], [(b, None, None, None)]], device=False)
    assert scan_segs.tolist() == [0, 3, 4]
    g = arr[0]
    assert (g.points, g.n_points, g.layout.stride_bytes, g.mode, g.filter_offset) == (a.ctypes.data, 5, 32, L.RIG_MOTION, 16)
    assert (g.time_offset, g.time_type, g.knot0, g.n_knots) == (12, L.TIME_U32, 16, 8) and g.scale == np.float32(1.5e-7)
    assert C.string_at(C.addressof(g) + L.RigSegment.t_begin.offset, 4) == np.uint32(4286000000).tobytes()
    g = arr[1]
    assert (g.n_points, g.layout.stride_bytes, g.mode, g.filter_offset, list(g.tf)) == (3, 0, L.RIG_TF, -1, list(range(12)))
    assert (arr[2].points, arr[2].n_points, arr[2].mode, arr[2].filter_offset) == (None, 0, L.RIG_NONE, 12)
    assert C.string_at(C.addressof(cc._rig_table([[(b, None, cc.SegMotion(12, "f32", 0.25, 2.0, 0, 1), None)]], False)[0][0]) + 88, 4) == np.float32(0.25).tobytes()
    for bad in ([[(a, (24, 0), None, None)]], [[(b, None, np.zeros(11), None)]]):
        with pytest.raises(ValueError):
            cc._rig_table(bad, device=False)
    with pytest.raises(ValueError):
        cc.SegMotion(12, "f64", 0.0, 1.0, 0, 1)
    # keep together with motion stays ingest()'s ValueError, and says where the combination lives
    with pytest.raises(ValueError, match="ingest_rig"):
        cc._keep_filter(cc.PointFilter.range(12, 0.0, 1.0), (20, "f32"))
