"""The extension header include/cont2_amd_images.h against abi.EXTENSIONS, the way tests/test_abi_layout.py holds include/cont2_amd.h
against abi.SIGNATURES: every prototype classified by the binding convention is the table's entry, the library exports the symbols,
and cc.EXPORTS is still exactly what cont2_amd.h declares."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_images.h"


def _prototypes(path):
    hdr = open(path).read()
    hdr = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    protos = re.findall(r"^[ \t]*((?:const\s+)?\w+(?:\s*\*)?)\s*\b(cc_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
    scalar = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float}

    def param(p):
        return C.c_void_p if "*" in p or "[" in p else scalar[[t for t in re.findall(r"\w+", p) if t != "const"][0]]

    def ret(r):
        r = " ".join(r.replace("*", " * ").split())
        return {"int": C.c_int, "void": None, "const char *": C.c_char_p}.get(r, C.c_void_p if "*" in r else r)

    return protos, {name: (ret(r), [param(p) for p in params.split(",") if p.strip() not in ("", "void")]) for r, name, params in protos}


def test_extension_table_matches_its_header(cc):
    assert list(cc.abi.EXTENSIONS) == [HDR]
    protos, parsed = _prototypes(os.path.join(ROOT, "include", HDR))
    assert len(protos) == len(parsed) == 3
    table = cc.abi.EXTENSIONS[HDR]
    assert parsed.keys() == table.keys(), parsed.keys() ^ table.keys()
    for name, sig in parsed.items():
        assert table[name] == sig, name
    assert sorted(cc.EXPORTS_EXT) == sorted(table) and not set(cc.EXPORTS_EXT) & set(cc.EXPORTS)
    assert '#include "cont2_amd.h"' in open(os.path.join(ROOT, "include", HDR)).read()


def test_extension_symbols_are_exported_and_bound(cc):
    lib = cc.abi.bind(C.CDLL(cc.build()))
    for name, (restype, argtypes) in cc.abi.EXTENSIONS[HDR].items():
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
    import emu_api
    emu = C.CDLL(emu_api.build())
    for name in cc.EXPORTS_EXT:
        assert hasattr(emu, name), name


def test_the_first_header_and_its_table_are_untouched(cc):
    """cc.EXPORTS is what include/cont2_amd.h declares -- 109 symbols -- and that header names none of the extension's calls"""
    hdr = open(os.path.join(ROOT, "include", "cont2_amd.h")).read()
    declared = set(re.findall(r"\b(cc_[a-z0-9_]+)\s*\(", hdr)) - {"cc_ctx", "cc_db"}
    assert declared == set(cc.EXPORTS) == set(cc.abi.SIGNATURES) and len(declared) == 109
    assert not declared & set(cc.EXPORTS_EXT)
    _, parsed = _prototypes(os.path.join(ROOT, "include", "cont2_amd.h"))
    assert parsed.keys() == cc.abi.SIGNATURES.keys()
