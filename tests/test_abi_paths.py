"""The add-on header include/cont2_amd_paths.h against its entry of abi.ADDONS, the way tests/test_abi_filter.py holds
include/cont2_amd_filter.h: the prototype classified by the binding convention is the table's entry, the library and the CPU
harness export the symbol, bind() gives it its types; and the earlier headers and registries are as they were."""
import ctypes as C
import os

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_paths.h"


def test_the_headers_entry_matches_the_header(cc):
    assert HDR in cc.abi.ADDONS
    text = open(os.path.join(ROOT, "include", HDR)).read()
    protos, parsed = _prototypes(os.path.join(ROOT, "include", HDR))
    assert len(protos) == len(parsed) == 1 and set(parsed) == {"cc_ingest_path_counts"}
    table = cc.abi.ADDONS[HDR]
    assert parsed == table and table["cc_ingest_path_counts"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert set(table) <= set(cc.EXPORTS_ADDON) and not set(table) & (set(cc.EXPORTS) | set(cc.EXPORTS_EXT))
    assert '#include "cont2_amd.h"' in text
    for h in ("cont2_amd.h", "cont2_amd_images.h", "cont2_amd_filter.h", "cont2_amd_coords.h"):
        assert "path_counts" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert list(cc.abi.ADDONS)[:3] == ["cont2_amd_filter.h", "cont2_amd_coords.h", HDR]


def test_symbol_is_exported_and_bound(cc):
    lib = cc.abi.bind(C.CDLL(cc.build()))
    fn = lib.cc_ingest_path_counts
    assert fn.restype == C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
    import emu_api
    assert hasattr(cc.abi.bind(C.CDLL(emu_api.build())), "cc_ingest_path_counts")


def test_refusals_and_a_fresh_context_on_the_harness(oracle):
    """NULL arguments are CC_EINVAL with the call's name; a context that has ingested nothing reads six zeros"""
    import emu_api
    api = emu_api.EmuApi(oracle.L)
    ctx = api.create(max_batch=2)
    out = (C.c_int32 * 6)(*([7] * 6))
    assert api.lib.cc_ingest_path_counts(None, out) == -1 and api.lib.cc_last_error().decode().startswith("cc_ingest_path_counts:")
    assert api.lib.cc_ingest_path_counts(ctx, None) == -1
    assert api.lib.cc_ingest_path_counts(ctx, out) == 0 and out[:] == [0] * 6
    api.lib.cc_destroy(ctx)
