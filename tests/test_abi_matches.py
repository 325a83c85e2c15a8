"""The add-on header include/cont2_amd_matches.h against its entry of abi.ADDONS, the way tests/test_abi_cands.py holds
include/cont2_amd_cands.h: every prototype classified by the binding convention is the table's entry, the library and the CPU
harness export the symbols, bind() gives them their types; the structs as the C compiler lays them out are the layouts' records;
and the earlier headers and registries are as they were."""
import ctypes as C
import os
import subprocess
import tempfile

from test_abi_images import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = "cont2_amd_matches.h"
NAMES = ["cc_match_pairs", "cc_db_query_submit_matched", "cc_db_verify_submit_matched", "cc_db_check_hints_matched",
         "cc_db_query_scan_batch_submit_matched", "cc_db_query_batch_host_matched", "cc_db_verify_batch_host_matched",
         "cc_db_check_hints_host_matched"]


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
    assert '#include "cont2_amd.h"' in text and "/* 96 bytes */" in text
    # each matched form is its flow's most general list followed by one pointer
    S = cc.abi.SIGNATURES
    assert table["cc_db_query_submit_matched"][1] == S["cc_db_query_submit_masked"][1] + [C.c_void_p]
    assert table["cc_db_query_batch_host_matched"][1] == S["cc_db_query_batch_host_masked"][1] + [C.c_void_p]
    assert table["cc_db_query_scan_batch_submit_matched"][1] == S["cc_db_query_scan_batch_submit_ranked_detail"][1] + [C.c_void_p]
    assert table["cc_db_check_hints_matched"][1] == S["cc_db_check_hints_ranked_detail"][1] + [C.c_void_p]
    assert table["cc_db_check_hints_host_matched"][1] == S["cc_db_check_hints_host_ranked_detail"][1] + [C.c_void_p]
    assert table["cc_db_verify_batch_host_matched"][1] == S["cc_db_verify_batch_host_ranked_detail"][1] + [C.c_void_p]
    v = S["cc_db_verify_submit_ranked_detail"][1]
    assert table["cc_db_verify_submit_matched"][1] == v[:3] + [C.c_void_p] + v[3:] + [C.c_void_p]   # (d_qdesc, n_desc) and src
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != HDR:
            assert "_matched" not in open(os.path.join(ROOT, "include", h)).read(), h
    assert list(cc.abi.ADDONS)[:5] == ["cont2_amd_filter.h", "cont2_amd_coords.h", "cont2_amd_paths.h", "cont2_amd_cands.h", "cont2_amd_rig.h"]
    assert list(cc.abi.ADDONS)[5] == HDR


def test_symbols_are_exported_and_bound(cc):
    import emu_api
    for lib in (cc.abi.bind(C.CDLL(cc.build())), cc.abi.bind(C.CDLL(emu_api.build()))):
        for name, (restype, argtypes) in cc.abi.ADDONS[HDR].items():
            fn = getattr(lib, name)
            assert fn.restype == restype and list(fn.argtypes) == argtypes, name


def test_structs_as_the_c_compiler_lays_them_out(cc):
    """sizeof and offsetof of the three structs from gcc, C and C++ (the static_asserts compile in both), against layouts.py"""
    L = cc.L
    fields = ("pairs", "n_pairs", "vote_cnt", "n_props", "area_perc", "res_rms", "res_max", "n_inlier", "flags")
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "cont2_amd_matches.h"\nint main(void) { printf("%zu' + " %zu" * (len(fields) + 7) + '\\n", '
            "sizeof(cc_ranked_match_t), " + ", ".join("offsetof(cc_ranked_match_t, %s)" % f for f in fields) +
            ", sizeof(cc_match_out_t), offsetof(cc_match_out_t, h_match), offsetof(cc_match_out_t, inlier_px), sizeof(cc_match_pair_t), "
            "offsetof(cc_match_pair_t, level), offsetof(cc_match_pair_t, seq_src), offsetof(cc_match_pair_t, seq_tgt)); return 0; }\n")
    dt = L.ranked_match_dt
    want = [96] + [dt.fields[f][1] for f in fields] + [C.sizeof(L.MatchOut), L.MatchOut.h_match.offset, L.MatchOut.inlier_px.offset, 4, 0, 1, 2]
    with tempfile.TemporaryDirectory() as td:
        for comp, ext in (("gcc", "c"), ("g++", "cpp")):
            src = os.path.join(td, "t." + ext)
            open(src, "w").write(body)
            subprocess.check_call([comp, "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(td, "t")])
            got = [int(x) for x in subprocess.check_output([os.path.join(td, "t")]).split()]
            assert got == want, (comp, got, want)
    assert want[1:10] == [0, 56, 60, 64, 68, 72, 80, 88, 92] and want[10:13] == [16, 0, 8]
    assert L.match_buffers(3, 5, 2.0)[0].shape == (3, 5)
