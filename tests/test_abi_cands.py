"""The add-on header include/cont2_amd_cands.h against its entry of abi.ADDONS, the way tests/test_abi_paths.py holds
include/cont2_amd_paths.h: the prototype classified by the binding convention is the table's entry, the library and the CPU
harness export the symbol, bind() gives it its types, the record has the layout's size; and the earlier headers and registries
are as they were."""
import ctypes as C
import os

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_cands.h"


def test_the_headers_entry_matches_the_header(cc):
    assert HDR in cc.abi.ADDONS
    text = open(os.path.join(ROOT, "include", HDR)).read()
    protos, parsed = _prototypes(os.path.join(ROOT, "include", HDR))
    assert len(protos) == len(parsed) == 1 and set(parsed) == {"cc_db_debug_cands"}
    table = cc.abi.ADDONS[HDR]
    assert parsed == table and table["cc_db_debug_cands"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    assert set(table) <= set(cc.EXPORTS_ADDON) and not set(table) & (set(cc.EXPORTS) | set(cc.EXPORTS_EXT))
    assert '#include "cont2_amd.h"' in text and "/* 40 bytes */" in text and cc.L.cand_dbg_dt.itemsize == 40
    for h in ("cont2_amd.h", "cont2_amd_images.h", "cont2_amd_filter.h", "cont2_amd_coords.h", "cont2_amd_paths.h"):
        assert "debug_cands" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert list(cc.abi.ADDONS)[:4] == ["cont2_amd_filter.h", "cont2_amd_coords.h", "cont2_amd_paths.h", HDR]


def test_symbol_is_exported_and_bound(cc):
    lib = cc.abi.bind(C.CDLL(cc.build()))
    fn = lib.cc_db_debug_cands
    assert fn.restype == C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    import emu_api
    assert hasattr(cc.abi.bind(C.CDLL(emu_api.build())), "cc_db_debug_cands")


def test_refusals_and_a_fresh_database_on_the_harness(oracle):
    """NULL arguments and a negative cap are CC_EINVAL with the call's name; a hint call without hints leaves no candidate"""
    import numpy as np
    import emu_api
    L = oracle.L
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=2)
    db = api.db_create(ctx, cap=4)
    out = np.zeros(4, L.cand_dbg_dt)
    n = C.c_int(7)
    assert api.lib.cc_db_debug_cands(None, out.ctypes.data, 4, C.byref(n)) == -1 and api.lib.cc_last_error().decode().startswith("cc_db_debug_cands:")
    assert api.lib.cc_db_debug_cands(db, None, 4, C.byref(n)) == -1 and api.lib.cc_db_debug_cands(db, out.ctypes.data, -1, C.byref(n)) == -1
    assert api.lib.cc_db_debug_cands(db, out.ctypes.data, 4, None) == -1
    api.check_hints(db, np.zeros(1, L.scan_desc_dt), np.zeros(0, L.hint_dt))
    assert api.lib.cc_db_debug_cands(db, out.ctypes.data, 4, C.byref(n)) == 0 and n.value == 0
