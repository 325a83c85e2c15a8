"""Writes tests/golden/ranked_detail_scans.npz: seven scan descriptors with LONG ellipse-pair lists for the detail tests
(tests/test_emu_ranked_detail.py, tests/test_gpu_ranked_detail.py).  Casting a 64-beam scan of the KITTI-shaped or the dense
world takes seconds on a CPU, so the descriptors -- the CPU oracle's, from this package's synthetic worlds -- are recorded:

  0      scan 1485 of the KITTI-shaped world           1, 2   the same cloud moved by (0.02 rad, 0.4, -0.3) / (-0.05, 1.0, 0.6) m:
                                                              a revisit with a small offset, > 1 280 pairs against scan 0
  3      scan 0 of the dense world                     4, 5   the same two moves of it (257 .. 1 280 pairs)
  6      scan 1 of the dense world

Run from the repository root:  python tests/golden/make_ranked_detail_fixture.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]


def moved(pts, th, tx, ty):
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    m = pts.copy()
    m[:, :2] = pts[:, :2] @ R.T + [tx, ty]
    return m


def main():
    import cc_amd
    import oracle_py as oracle
    cc = cc_amd.load()
    L = oracle.L
    xk, _, _ = cc.synth.make_sequence(0, world=cc.synth.World(kitti=True), indices=np.array([1485]))
    xd, _, _ = cc.synth.make_sequence(2, world=cc.synth.World(dense=True))
    clouds = []
    for x in (xk[0], xd[0]):
        p = x.numpy().reshape(-1, 4)
        clouds += [p, moved(p, 0.02, 0.4, -0.3), moved(p, -0.05, 1.0, 0.6)]
    clouds.append(xd[1].numpy().reshape(-1, 4))
    n = len(clouds)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    _, _, desc = oracle.run_sequence(np.concatenate(clouds), offs, np.arange(n) * 100.0, np.arange(n, dtype=np.int32), dcfg=L.default_db_cfg(),
                                     want_desc=True)
    assert desc.dtype == L.scan_desc_dt and len(desc) == 7
    out = os.path.join(HERE, "ranked_detail_scans.npz")
    np.savez_compressed(out, desc=np.ascontiguousarray(desc).view(np.uint8).reshape(n, -1))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
