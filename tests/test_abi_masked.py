"""The masked query's C-ABI: cc_scan_mask_t as the compiler lays it out against layouts.py, and the new symbols in EXPORTS and
in the built library."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cc_db_query_submit_masked", "cc_db_query_batch_host_masked", "cc_mask_gates")


def test_scan_mask_layout_matches_the_header(cc):
    L = cc.L
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "cont2_amd.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(cc_scan_mask_t), offsetof(cc_scan_mask_t, bits), '
           'offsetof(cc_scan_mask_t, n_rows), offsetof(cc_scan_mask_t, row_words), offsetof(cc_scan_mask_t, h_row)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "m.c"), os.path.join(d, "m")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])  # the header is plain C
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    M = L.ScanMaskC
    assert got == [C.sizeof(M), M.bits.offset, M.n_rows.offset, M.row_words.offset, M.h_row.offset] == [24, 0, 8, 12, 16]


def test_masked_symbols_are_exported(cc):
    lib = C.CDLL(cc.build())
    for s in SYMBOLS:
        assert s in cc.EXPORTS and hasattr(lib, s), s


def test_pack_mask_rows(cc):
    import numpy as np
    L = cc.L
    a = np.zeros((2, 70), bool)
    a[0, [0, 31, 32, 69]] = True
    t = L.pack_mask_rows(a)
    assert t.dtype == np.uint32 and t.tolist() == [[0x80000001, 1, 1 << 5], [0, 0, 0]]
    assert L.pack_mask_rows([[0, 31, 32, 69], []], n_db=70).tolist() == t.tolist()
    assert L.pack_mask_rows(a, row_words=5).shape == (2, 5)
