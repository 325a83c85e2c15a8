"""The add-on header include/cont2_amd_filter.h against its entry of abi.ADDONS, the way tests/test_abi_images.py holds
include/cont2_amd_images.h against abi.EXTENSIONS: every prototype classified by the binding convention is the table's entry, the
library and the CPU harness export the symbols, bind() gives them their types, and cc_point_filter_t is laid out as the compiler
lays it out.  The registry is open-ended: this test holds its own header's entry, not the number of entries."""
import ctypes as C
import os
import re
import subprocess

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_filter.h"
CALLS = {"cc_ingest_points_filtered", "cc_ingest_points_filtered_host", "cc_scan_ingest_points_filtered"}


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
    # every symbol of every add-on is in EXPORTS_ADDON, once, and in no other list
    every = [s for t in cc.abi.ADDONS.values() for s in t]
    assert sorted(every) == sorted(cc.EXPORTS_ADDON) and len(set(every)) == len(every)
    assert not set(every) & (set(cc.EXPORTS) | set(cc.EXPORTS_EXT))
    # the header says what it leaves out
    for word in ("Out of scope", "segments", "motion", "range images", "table per scan", "64-bit", "MOVED coordinates"):
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


def test_filter_struct_layout(cc, tmp_path):
    """cc_point_filter_t as the C compiler and the C++ compiler lay it out (the header's static_asserts are compiled in both
    languages) against layouts.PointFilterC and the constants"""
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cont2_amd_filter.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(cc_point_filter_t), offsetof(cc_point_filter_t, offset), '
                   'offsetof(cc_point_filter_t, type), offsetof(cc_point_filter_t, shift), offsetof(cc_point_filter_t, mask), offsetof(cc_point_filter_t, n_classes), '
                   'offsetof(cc_point_filter_t, keep_other), offsetof(cc_point_filter_t, lo), offsetof(cc_point_filter_t, hi), offsetof(cc_point_filter_t, keep_bits), '
                   'CC_FILTER_CLASSES_MAX, CC_FILTER_U8, CC_FILTER_U16, CC_FILTER_U32, CC_FILTER_F32); return 0; }\n')
    F, L = cc.L.PointFilterC, cc.L
    exp = [C.sizeof(F), F.offset.offset, F.type.offset, F.shift.offset, F.mask.offset, F.n_classes.offset, F.keep_other.offset, F.lo.offset, F.hi.offset,
           F.keep_bits.offset, L.FILTER_CLASSES_MAX, L.FILTER_U8, L.FILTER_U16, L.FILTER_U32, L.FILTER_F32]
    assert exp[0] == 40 and exp[-5:] == [4096, 0, 1, 2, 3]
    for comp, std, name in (("gcc", "-std=c11", "lay_c"), ("g++", "-std=c++17", "lay_cpp")):
        exe = str(tmp_path / name)
        subprocess.check_call([comp, std, "-x", "c" if comp == "gcc" else "c++", str(src), "-I", os.path.join(ROOT, "include"), "-o", exe])
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
        assert got == exp, (comp, got, exp)
    import point_filter
    T = point_filter.Filter
    assert C.sizeof(T) == 40 and [getattr(T, f).offset for f, _ in T._fields_] == [getattr(F, f).offset for f, _ in F._fields_]


def test_the_first_two_registries_are_untouched(cc):
    """the add-on joined without changing what tests/test_abi_images.py pins: the first header's 109 symbols, the one extension header"""
    hdr = open(os.path.join(ROOT, "include", "cont2_amd.h")).read()
    assert not re.search(r"_filtered|cont2_amd_filter|cc_point_filter_t", hdr)
    assert list(cc.abi.EXTENSIONS) == ["cont2_amd_images.h"] and len(cc.EXPORTS) == 109 and len(cc.EXPORTS_EXT) == 3


def test_python_filters(cc):
    """PointFilter.classes / PointFilter.range: what they put into the struct, and what they refuse"""
    L = cc.L
    f = cc.PointFilter.classes(12, "u32", drop=range(252, 260), mask=0xFFFF)
    c = f._c
    assert (c.offset, c.type, c.shift, c.mask, c.n_classes, c.keep_other) == (12, L.FILTER_U32, 0, 0xFFFF, 260, 1)
    bits = f._bits
    assert bits.dtype.itemsize == 4 and len(bits) == 9 and c.keep_bits == bits.ctypes.data
    kept = [(int(bits[k >> 5]) >> (k & 31)) & 1 for k in range(260)]
    assert kept == [0 if 252 <= k < 260 else 1 for k in range(260)]
    f = cc.PointFilter.classes(17, "u8", keep=[1, 3, 40], n_classes=64, shift=1, mask=0x3F, other="drop")
    c = f._c
    assert (c.offset, c.type, c.shift, c.mask, c.n_classes, c.keep_other) == (17, L.FILTER_U8, 1, 0x3F, 64, 0)
    assert [k for k in range(64) if (int(f._bits[k >> 5]) >> (k & 31)) & 1] == [1, 3, 40]
    assert cc.PointFilter.classes(2, "u16", keep=[5])._c.n_classes == 6 and cc.PointFilter.classes(2, "u16", keep=[5])._c.mask == 0xFFFFFFFF
    r = cc.PointFilter.range(12, -float("inf"), 0.5)._c
    assert (r.offset, r.type, r.lo, r.hi, r.keep_bits) == (12, L.FILTER_F32, -float("inf"), 0.5, None)
    import pytest
    for bad in (dict(keep=[1], drop=[2]), dict(), dict(keep=[5], n_classes=5), dict(keep=[1], n_classes=4097), dict(keep=[-1]),
                dict(keep=[1], other="maybe")):
        with pytest.raises(ValueError):
            cc.PointFilter.classes(12, "u32", **bad)
    with pytest.raises(ValueError):
        cc.PointFilter.classes(12, "f32", keep=[1])
