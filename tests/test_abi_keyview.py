"""The add-on header include/cont2_amd_keyview.h against its entry of abi.ADDONS, the way tests/test_abi_cands.py holds
include/cont2_amd_cands.h: the prototype classified by the binding convention is the table's entry, the library and the CPU
harness export the symbol, bind() gives it its types; the call's refusals and an empty layer on the harness."""
import ctypes as C
import os

import numpy as np

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_keyview.h"
SIG = (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])


def test_the_headers_entry_matches_the_header(cc):
    assert HDR in cc.abi.ADDONS
    text = open(os.path.join(ROOT, "include", HDR)).read()
    protos, parsed = _prototypes(os.path.join(ROOT, "include", HDR))
    assert len(protos) == len(parsed) == 1 and set(parsed) == {"cc_db_debug_key_view"}
    table = cc.abi.ADDONS[HDR]
    assert parsed == table and table["cc_db_debug_key_view"] == SIG
    assert set(table) <= set(cc.EXPORTS_ADDON) and not set(table) & (set(cc.EXPORTS) | set(cc.EXPORTS_EXT))
    assert '#include "cont2_amd.h"' in text
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != HDR:
            assert "debug_key_view" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert list(cc.abi.ADDONS)[-1] == HDR


def test_symbol_is_exported_and_bound(cc):
    lib = cc.abi.bind(C.CDLL(cc.build()))
    fn = lib.cc_db_debug_key_view
    assert fn.restype == SIG[0] and list(fn.argtypes) == SIG[1]
    import emu_api
    assert hasattr(cc.abi.bind(C.CDLL(emu_api.build())), "cc_db_debug_key_view")


def test_refusals_and_an_empty_layer_on_the_harness(oracle):
    """NULL arguments, a negative cap and a layer the database does not query are CC_EINVAL with the call's name; a cap below the
    layer's size is CC_ECAPACITY with the size in *n; a fresh database has empty views"""
    import emu_api
    L = oracle.L
    api = emu_api.EmuApi(L)
    ctx = api.create(max_batch=2)
    d = L.default_db_cfg()
    d.n_q_levels = 2
    db = api.db_create(ctx, d, cap=4)
    keys, sid, sact, n = np.zeros((11, 8), np.float32), np.zeros(8, np.int32), np.zeros(8, np.int32), C.c_int32(7)
    a = (keys.ctypes.data, sid.ctypes.data, sact.ctypes.data)
    fn = api.lib.cc_db_debug_key_view
    assert fn(None, 0, 8, *a, C.byref(n)) == -1 and api.lib.cc_last_error().decode().startswith("cc_db_debug_key_view:")
    assert fn(db, 0, 8, None, a[1], a[2], C.byref(n)) == -1 and fn(db, 0, 8, a[0], None, a[2], C.byref(n)) == -1
    assert fn(db, 0, 8, a[0], a[1], None, C.byref(n)) == -1 and fn(db, 0, 8, *a, None) == -1
    assert fn(db, 0, -1, *a, C.byref(n)) == -1 and fn(db, -1, 8, *a, C.byref(n)) == -1 and fn(db, 2, 8, *a, C.byref(n)) == -1
    assert fn(db, 1, 8, *a, C.byref(n)) == 0 and n.value == 0
    desc = np.zeros(2, L.scan_desc_dt)
    desc["keys"][:, 1, :, :] = 1.0
    desc["keys"][:, 1, :, 0] = np.arange(12, 0, -1).reshape(2, 6)
    api.db_add(db, desc, np.zeros(2), np.ones(2, np.int32))
    assert fn(db, 0, 8, *a, C.byref(n)) == -4 and n.value == 12 and not keys.any() and not sid.any()
    keys, sid, sact = np.zeros((11, 12), np.float32), np.zeros(12, np.int32), np.zeros(12, np.int32)
    assert fn(db, 0, 12, keys.ctypes.data, sid.ctypes.data, sact.ctypes.data, C.byref(n)) == 0 and n.value == 12
    assert sid.tolist() == list(range(11, -1, -1)) and keys[0].tolist() == list(range(1, 13)) and (keys[10] == keys[0] ** 2 + 9).all()
    assert fn(db, 1, 12, keys.ctypes.data, sid.ctypes.data, sact.ctypes.data, C.byref(n)) == 0 and n.value == 0
    api.lib.cc_db_destroy(db)
