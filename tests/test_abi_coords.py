"""The add-on header include/cont2_amd_coords.h against its entry of abi.ADDONS, the way tests/test_abi_filter.py holds
include/cont2_amd_filter.h: every prototype classified by the binding convention is the table's entry, the library and the CPU
harness export the symbols, bind() gives them their types, cc_coord_src_t is laid out as the compilers lay it out, and the header
says what it leaves out."""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_coords.h"
CALLS = {"cc_ingest_coords", "cc_ingest_coords_host", "cc_scan_ingest_coords"}


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
    assert '#include "cont2_amd.h"' in text
    every = [s for t in cc.abi.ADDONS.values() for s in t]
    assert sorted(every) == sorted(cc.EXPORTS_ADDON) and len(set(every)) == len(every)
    # the header states the three steps and says what it leaves out
    for word in ("X = (double)v", "D = X - origin", "p = (float)D", "round to nearest even", "No fused multiply-add", "Out of scope", "segments", "motion", "filter",
                 "range images", "f16, i16 or u16", "64-bit", "per axis", "unaligned element", "scale\n * per scan"):
        assert word in text, word


def test_symbols_are_exported_and_bound(cc):
    lib = cc.abi.bind(C.CDLL(cc.build()))
    for name, (restype, argtypes) in cc.abi.ADDONS[HDR].items():
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    import emu_api
    emu = cc.abi.bind(C.CDLL(emu_api.build()))
    for name in cc.abi.ADDONS[HDR]:
        assert hasattr(emu, name), name


def test_coord_struct_layout(cc, tmp_path):
    """cc_coord_src_t as the C compiler and the C++ compiler lay it out (the header's static_asserts are compiled in both languages)
    against layouts.CoordSrc and the constants"""
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cont2_amd_coords.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(cc_coord_src_t), offsetof(cc_coord_src_t, x), offsetof(cc_coord_src_t, y), '
                   'offsetof(cc_coord_src_t, z), offsetof(cc_coord_src_t, type), offsetof(cc_coord_src_t, stride_bytes), offsetof(cc_coord_src_t, scale), '
                   'CC_COORD_F32, CC_COORD_F64, CC_COORD_I32); return 0; }\n')
    S, L = cc.L.CoordSrc, cc.L
    exp = [C.sizeof(S), S.x.offset, S.y.offset, S.z.offset, S.type.offset, S.stride_bytes.offset, S.scale.offset, L.COORD_F32, L.COORD_F64, L.COORD_I32]
    assert exp == [56, 0, 8, 16, 24, 28, 32, 0, 1, 2]
    for comp, std, name in (("gcc", "-std=c11", "lay_c"), ("g++", "-std=c++17", "lay_cpp")):
        exe = str(tmp_path / name)
        subprocess.check_call([comp, std, "-x", "c" if comp == "gcc" else "c++", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
        assert got == exp, (comp, got, exp)
    import point_coords
    T = point_coords.CoordSrc
    assert C.sizeof(T) == 56 and [getattr(T, f).offset for f, _ in T._fields_] == [getattr(S, f).offset for f, _ in S._fields_]


def test_the_earlier_headers_are_untouched(cc):
    """the add-on joined without changing what the earlier ABI tests pin"""
    for h in ("cont2_amd.h", "cont2_amd_images.h", "cont2_amd_filter.h"):
        assert not re.search(r"_coords|cc_coord_src_t|CC_COORD_", open(os.path.join(ROOT, "include", h)).read()), h
    assert list(cc.abi.EXTENSIONS) == ["cont2_amd_images.h"] and len(cc.EXPORTS) == 109 and len(cc.EXPORTS_EXT) == 3
    assert list(cc.abi.ADDONS)[:2] == ["cont2_amd_filter.h", HDR] and len(cc.abi.ADDONS["cont2_amd_filter.h"]) == 3


def test_python_coord_sources(cc):
    """calls.coord_src and the stream description of Context.ingest_coords_host: what they put into the struct, and what they refuse"""
    import numpy as np
    L = cc.L
    a = np.zeros((50, 6), np.float64)
    x, y, z, dt, stride, _ = cc._coord_streams(a[:, 2:5], False)
    assert (x, y, z, stride) == (a.ctypes.data + 16, a.ctypes.data + 24, a.ctypes.data + 32, 48) and dt == np.float64
    t = np.zeros((3, 50), np.int32)
    x, y, z, dt, stride, _ = cc._coord_streams(t.T, False)
    assert (x, y, z, stride) == (t.ctypes.data, t.ctypes.data + 200, t.ctypes.data + 400, 4)
    s = cc.calls.coord_src(x, y, z, dt, stride, scale=[0.001, 0.002, 0.01])
    assert (s.type, s.stride_bytes, list(s.scale), s.y) == (L.COORD_I32, 4, [0.001, 0.002, 0.01], t.ctypes.data + 200)
    assert list(cc.calls.coord_src(x, y, z, dt, stride, scale=0.01).scale) == [0.01] * 3 and list(cc.calls.coord_src(x, y, z, dt, stride).scale) == [1.0] * 3
    cols = (a[:, 0], a[:, 3], a[:, 1])
    x, y, z, dt, stride, _ = cc._coord_streams(cols, False)
    assert (x, y, z, stride) == (a.ctypes.data, a.ctypes.data + 24, a.ctypes.data + 8, 48)
    assert cc.calls.coord_src(x, y, z, np.dtype(np.float32), 12).type == L.COORD_F32
    for dtype in (np.float16, np.int64, np.uint32, np.int16):
        with pytest.raises(ValueError):
            cc.calls.coord_src(x, y, z, np.dtype(dtype), 8)
    with pytest.raises(ValueError):
        cc.calls.coord_src(x, y, z, np.dtype(np.float64), 24, scale=[1.0, 1.0, 1.0])   # scale without int32
    for bad in ((a[:, 0], a[:, 1]), (a[:, 0], a[:, 1], a[:, 2].astype(np.float32)), (a[:, 0], a[:, 1], a[::2, 2]), (a[:, 0], a[:, 1], np.zeros(50)), a[:, :2], a[0]):
        with pytest.raises(ValueError):
            cc._coord_streams(bad, False)
