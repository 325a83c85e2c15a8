"""The add-on header include/cont2_amd_lists.h against its entry of abi.ADDONS, the way tests/test_abi_matches.py holds
include/cont2_amd_matches.h: every prototype classified by the binding convention is the table's entry, the library and the CPU
harness export the symbols, bind() gives them their types; cc_scan_lists_t as gcc and g++ lay it out is the layouts' record; and
the earlier headers and registries are as they were."""
import ctypes as C
import os
import subprocess
import tempfile

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_lists.h"
NAMES = ["cc_db_query_submit_listed", "cc_db_query_batch_host_listed", "cc_db_debug_knn_chunks_listed"]


def test_the_headers_entry_matches_the_header(cc):
    assert HDR in cc.abi.ADDONS
    text = open(os.path.join(ROOT, "include", HDR)).read()
    protos, parsed = _prototypes(os.path.join(ROOT, "include", HDR))
    assert len(protos) == len(parsed) == len(NAMES) and list(parsed) == NAMES
    table = cc.abi.ADDONS[HDR]
    assert list(table) == NAMES
    for name, sig in parsed.items():
        assert table[name] == sig, name
    assert set(table) <= set(cc.EXPORTS_ADDON) and not set(table) & (set(cc.EXPORTS) | set(cc.EXPORTS_EXT))
    assert '#include "cont2_amd.h"' in text and '#include "cont2_amd_matches.h"' in text and "#define CC_LIST_SCANS_MAX 1024" in text
    assert cc.L.LIST_SCANS_MAX == 1024
    # the listed forms: the most general lists of the query flow, `lists` where the mask is
    A = cc.abi.ADDONS["cont2_amd_matches.h"]
    assert table["cc_db_query_submit_listed"][1] == A["cc_db_query_submit_matched"][1]
    assert table["cc_db_query_batch_host_listed"][1] == A["cc_db_query_batch_host_matched"][1]
    assert table["cc_db_debug_knn_chunks_listed"] == cc.abi.SIGNATURES["cc_db_debug_knn_chunks"]
    # nobody else's names in this header, this header's names nowhere else; the entry is the last one
    for word in ("_matched", "debug_cands", "path_counts"):
        assert word not in text, word
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != HDR:
            assert "_listed" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert list(cc.abi.ADDONS)[:6] == ["cont2_amd_filter.h", "cont2_amd_coords.h", "cont2_amd_paths.h", "cont2_amd_cands.h", "cont2_amd_rig.h",
                                      "cont2_amd_matches.h"]
    assert list(cc.abi.ADDONS)[6] == HDR


def test_symbols_are_exported_and_bound(cc):
    import emu_api
    for lib in (cc.abi.bind(C.CDLL(cc.build())), cc.abi.bind(C.CDLL(emu_api.build()))):
        for name, (restype, argtypes) in cc.abi.ADDONS[HDR].items():
            fn = getattr(lib, name)
            assert fn.restype == restype and list(fn.argtypes) == argtypes, name


def test_scan_lists_as_the_c_compiler_lays_it_out(cc):
    """sizeof and offsetof of cc_scan_lists_t from gcc (C99: the header is plain C) and g++, against layouts.ScanListsC"""
    S = cc.L.ScanListsC
    fields = ("h_idx", "h_off", "n_lists", "h_row")
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "cont2_amd_lists.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d\\n", '
            "sizeof(cc_scan_lists_t), " + ", ".join("offsetof(cc_scan_lists_t, %s)" % f for f in fields) + ", CC_LIST_SCANS_MAX); return 0; }\n")
    want = [C.sizeof(S)] + [getattr(S, f).offset for f in fields] + [cc.L.LIST_SCANS_MAX]
    with tempfile.TemporaryDirectory() as td:
        for comp, ext, std in (("gcc", "c", "-std=c99"), ("g++", "cpp", "-std=c++11")):
            src = os.path.join(td, "t." + ext)
            open(src, "w").write(body)
            subprocess.check_call([comp, std, "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(td, "t")])
            got = [int(x) for x in subprocess.check_output([os.path.join(td, "t")]).split()]
            assert got == want, (comp, got, want)
    assert want == [32, 0, 8, 16, 24, 1024]


def test_gate_lists_and_from_lists(cc):
    import numpy as np
    s = cc.ScanLists.from_lists([[1, 2], [], [5]])
    assert s.idx.dtype == np.int32 and s.idx.tolist() == [1, 2, 5] and s.off.tolist() == [0, 2, 2, 3] and s.rows.tolist() == [0, 1, 2]
    assert cc.ScanLists.from_lists([[3, 1]], rows=[0, 0, -1]).idx.tolist() == [3, 1]  # nothing is sorted: the library refuses it
    g = cc.ScanLists.from_gates(np.array([[3, 4], [0, 0], [3.0000002, 4], [np.nan, 0], [1, 1]], np.float32),
                                [[0, 0, 5], [0, 0, 0], [0, 0, -1], [0, 0, np.nan], [np.nan, 0, 100], [1, 1, 0]])
    assert [l.tolist() for l in g.lists()] == [[0, 1, 4], [1], [], [], [], [4]]  # masked_cases.run_gates' special points
