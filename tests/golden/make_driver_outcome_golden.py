"""Records tests/golden/outcome-short-loop-drive-harness.txt: the outcome file the unchanged offline driver
(hostcpp/examples/batch_bin_test.cpp) writes on the CPU harness build of a checkout of this repository -- the commit BEFORE the
class mirror knew ranked answers (a37adbb), with its harness built (sh tests/emu/build.sh there).  tests/test_hostcpp_ranked.py
requires the current tree's driver to write the same bytes.
usage: python tests/golden/make_driver_outcome_golden.py <root of the built checkout>"""
import os
import pathlib
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import cc_amd  # noqa: E402
from test_hostcpp_ranked import GOLD, driver_outcome  # noqa: E402

if __name__ == "__main__":
    other = os.path.abspath(sys.argv[1])
    cc = cc_amd.load()
    with tempfile.TemporaryDirectory() as td:
        direct = driver_outcome(cc, pathlib.Path(td), other, False)
        ahead = driver_outcome(cc, pathlib.Path(td), other, True)
    assert direct == ahead, "the checkout's own direct and read-ahead paths differ"
    open(GOLD, "wb").write(direct)
    print("wrote %s: %d bytes, %d rows" % (GOLD, len(direct), len(direct.splitlines())))
