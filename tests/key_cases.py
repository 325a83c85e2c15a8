"""TEST INFRASTRUCTURE: the retrieval-key scenes and checks, written once over a small back end (test_emu_keys.py: the CPU harness,
test_gpu_keys.py: the device).  A back end has
    ingest(list of point arrays, manager config, debug=False) -> numpy descriptors (scan_desc_dt), one ingest call
    paths() -> {"list": set, "mid": set, "big": set} of scan indices of the last ingest call, or None where the build cannot say.
    path_counts() -> {"list": n, "mid": n, "big": n} of the last ingest call: the difference of two cc_ingest_path_counts readings.

Reference inputs always come from the oracle (its max-height image, cell positions and contour rows), never from the code under
test; tests/key_reference.py restates the key phase on them.  Every scan's oracle keys must pass check_keys first (a wrong
reference cannot pass silently), then the back end's; everything else in the descriptor is compared bit for bit.

The scenes are hand-built height maps, one point per cell at a jittered position inside the cell: mesas and blobs whose sizes and
heights decide which contours are anchors (the piv_firsts largest of a level, valid from min_cont_key_cnt cells), how long each
anchor's RoI list is (cells above lv_grads[1] within roi_radius - 0.01 of the anchor's mean position) and where its window lies.
Each case asserts on the reference's list lengths and anchor counts that it reaches the edge it is named after; the edges are those
of the key phase in csrc/k_contours.h: four lanes per (anchor, division) (CC_KEYS_KL), 18 anchors per group with the LDS lists
reused (CC_KEYS_GRP), lists clamped at 416 cells (CC_KEYS_CAP), the window's rows read from the raster-ordered entry list through
a 64-cell bitmap, nine 64-entry stretches per round."""
import numpy as np

import key_reference as KR
from parity import compare_desc

KEYS_KL, KEYS_GRP, KEYS_CAP, ROUND_ENTRIES = 4, 18, 416, 9 * 64
INEXACT_KEYS = 4              # CC_DESC_INEXACT_KEYS
AMBIGUOUS_CAP = 1e-3          # ambiguous components / non-zero ring components, over all scenes of the module
N_ROW = N_COL = 150
LV = [1.5, 2.0, 2.5, 3.0, 3.5, 4.0]


def H(k):
    """a height whose cell counts on levels 0..k"""
    return LV[k] + 0.2


class Scene:
    """A height map under construction: cell -> height (the height the reference's image holds: point z + lidar_height)."""

    def __init__(self):
        self.h = {}

    def rect(self, r0, c0, nr, nc, h, skip=()):
        for r in range(r0, r0 + nr):
            for c in range(c0, c0 + nc):
                if (r - r0, c - c0) not in skip:
                    self.cell(r, c, h)
        return self

    def cell(self, r, c, h):
        assert 0 <= r < N_ROW and 0 <= c < N_COL and (r - 75) ** 2 + (c - 75) ** 2 > 32, (r, c)   # blind_sq = 9 around the sensor
        self.h[(r, c)] = h
        return self

    def free(self, r, c, margin):
        return all((rr, cc) not in self.h for rr in range(r - margin, r + margin + 1) for cc in range(c - margin, c + margin + 1))

    def sprinkle(self, seed, p, h, margin=2):
        """single cells at height h, each with probability p, none within `margin` cells of what the scene holds so far"""
        rng = np.random.default_rng(seed)
        taken = dict(self.h)
        probe = Scene()
        probe.h = taken
        for r in range(N_ROW):
            for c in range(N_COL):
                if rng.random() < p and (r - 75) ** 2 + (c - 75) ** 2 > 32 and probe.free(r, c, margin):
                    self.h[(r, c)] = h
        return self

    def blobs(self, n, h):
        """n isolated 3-cell L-shaped blobs (contours of min_cont_cell_cnt cells) on the free spots of a pitch-3 lattice"""
        base = dict(self.h)
        probe = Scene()
        probe.h = base
        b = 0
        for r in range(1, N_ROW - 2, 3):
            for c in range(1, N_COL - 2, 3):
                if b == n:
                    return self
                if (r - 75) ** 2 + (c - 75) ** 2 > 50 and all(probe.free(r + dr, c + dc, 1) for dr, dc in ((0, 0), (0, 1), (1, 0))):
                    for dr, dc in ((0, 0), (0, 1), (1, 0)):
                        self.h[(r + dr, c + dc)] = h + 0.001 * (b % 7)
                    b += 1
        assert b == n, b
        return self

    def points(self, seed):
        rng = np.random.default_rng(seed)
        cells = sorted(self.h)
        assert len(cells) > 10
        p = np.zeros((len(cells), 4), np.float32)
        rc = np.array(cells, np.float64)
        p[:, :2] = rc - 75.0 + 0.5 + rng.uniform(-0.4, 0.4, (len(cells), 2))
        p[:, 2] = np.array([self.h[c] for c in cells]) - 2.0      # the default config adds lidar_height = 2
        return p[rng.permutation(len(cells))]


# 24 mesa corners on a pitch of 30 cells: mesas of up to 8 x 8 cells there stay more than roi_radius + 1 away from each other's cells
SPOTS = [(r, c) for r in (12, 42, 72, 102, 132) for c in (12, 42, 72, 102, 132) if (r, c) != (72, 72)]
BIG = [(7, 7), (7, 6), (7, 5), (6, 6), (6, 5), (5, 5)]       # six low mesas of distinct sizes 49 .. 25
SMALL = [(4, 5), (3, 6), (4, 4), (3, 5), (3, 4), (3, 3)]     # six tall ones of distinct sizes 20 .. 9, all smaller than the low ones


def _pair_8_9(s, r, c):
    """a 9-cell and an 8-cell blob on level 0 side by side (one empty column between them): cell_cnt == min_cont_key_cnt and one
    less; a single higher cell three rows away gives both a list of one cell"""
    s.rect(r, c, 3, 3, H(0))
    s.rect(r, c + 4, 3, 3, H(0), skip=((2, 2),))
    s.cell(r + 5, c + 3, H(1))


def scene_tails_short():
    """six 3 x 3 blobs on level 0 only, k = 0 .. 5 of their cells raised above lv_grads[1]: lists of 0 (empty: NaN rings) .. 5 cells;
    the raised cells of k >= 3 are contours of level 1 below min_cont_key_cnt: anchors without a key"""
    s = Scene()
    for k in range(6):
        r, c = SPOTS[k]
        s.rect(r, c, 3, 3, H(0))
        for j in range(k):
            s.cell(r + j // 3, c + j % 3, H(1))
    return s.points(1)


def scene_tails_mesas():
    """eight 5 x 5 mesas above the highest level, 0 .. 5 single cells above lv_grads[1] two rows off each: 36 valid anchors, lists of
    25 .. 30 cells (n mod 4 = 1, 2, 3, 0, 1, 2)"""
    s = Scene()
    for i in range(8):
        r, c = SPOTS[i]
        s.rect(r, c, 5, 5, H(5))
        for j in range(i % 6):
            s.cell(r - 2, c + 2 * j, H(1))
    return s.points(2)


def _groups(n_big, small, seed, pair=False, big_top=2):
    s = Scene()
    for i in range(n_big):
        s.rect(SPOTS[i][0], SPOTS[i][1], BIG[i][0], BIG[i][1], H(big_top))
    for j, top in enumerate(small):
        s.rect(SPOTS[8 + j][0], SPOTS[8 + j][1], SMALL[j][0], SMALL[j][1], H(top))
    if pair:
        _pair_8_9(s, *SPOTS[20])
    return s.points(seed)


SCENES = {
    "tails_short": scene_tails_short,
    "tails_mesas": scene_tails_mesas,
    # exactly 1, 17, 18, 19, 36 valid anchors.  Low mesas (top level 2) hold levels 0..2 -- the first group of 18 --, the smaller tall
    # ones are anchors only above: the second group's lists are shorter than the first group's in the same LDS slots
    "group_1": lambda: _groups(0, (), 3, pair=True),
    "group_17": lambda: _groups(4, (), 4, pair=True, big_top=3),
    "group_18": lambda: _groups(6, (), 5),
    "group_19": lambda: _groups(6, (3,), 6),
    "group_36": lambda: _groups(6, (5,) * 6, 7),
}


def scene_clip():
    """mesas within roi_pad of every border and corner: four tall 3..4-cell-wide ones in the corners, four low 5..6-cell-wide ones at
    the middle of the sides (the reference's image keeps nothing in row 0); the windows of the bottom ones end in the last row"""
    s = Scene()
    for (r, c), (nr, nc) in zip(((1, 0), (1, 146), (147, 0), (146, 146)), ((3, 3), (3, 4), (3, 4), (4, 4))):
        s.rect(r, c, nr, nc, H(5))
    for (r, c), (nr, nc) in zip(((1, 70), (144, 72), (71, 0), (72, 144)), ((5, 5), (6, 5), (5, 6), (6, 6))):
        s.rect(r, c, nr, nc, H(2))
    return s.sprinkle(11, 0.04, H(1)).sprinkle(12, 0.02, H(3)).points(8)


SEAM_CENTRES = ((43, 15), (20, 50), (52, 85), (84, 120), (107, 15), (116, 50))


def scene_seams():
    """6 x 5 mesas (rows r - 2 .. r + 3: a mean row position of r + 0.5) whose centre rows r put the first window row (43, 107: r_min = 32, 96) or the row after the last (20, 52, 84, 116:
    r_max + 1 = 32, 64, 96, 128) on a cell index that is a multiple of 64: the bitmap word seam of the entry count"""
    s = Scene()
    for r, c in SEAM_CENTRES:
        s.rect(r - 2, c - 2, 6, 5, H(5))
    return s.sprinkle(13, 0.05, H(1)).sprinkle(14, 0.02, H(2)).points(9)


PLATEAU = (10, 10, 50, 50)
TOWERS = ((11, 11), (33, 33), (52, 20), (20, 55))


def scene_plateau(thin=False):
    """a filled plateau of 50 x 50 cells just above lv_grads[2] with four towers on it: the rows of an anchor's window hold more than
    576 list entries (several read rounds); thinned to every third column, fewer (one round)"""
    s = Scene()
    r0, c0, nr, nc = PLATEAU
    for r in range(r0, r0 + nr):
        for c in range(c0, c0 + nc):
            if not thin or c % 3 == 0:
                s.cell(r, c, H(2))
    for r, c in TOWERS:
        s.rect(r, c, 3, 3, H(5))
    return s.sprinkle(15, 0.006, H(1)).points(10 + thin)


SCENES.update({"clip": scene_clip, "seams": scene_seams, "plateau": scene_plateau, "plateau_thin": lambda: scene_plateau(True)})

CAP_RADIUS = 11.5


def scene_cap(holes):
    """the plain plateau with the cells `holes` lowered below lv_grads[1] (still on level 0), and a far mesa with short lists"""
    s = Scene()
    s.rect(*PLATEAU, H(2))
    for rc in holes:
        assert rc in s.h
        s.h[rc] = H(0)
    s.rect(120, 120, 5, 5, H(5))
    return s.points(12)


def make_cfg(L, **kw):
    cfg = L.default_manager_cfg()
    for k, v in kw.items():
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


class Ref:
    """one scan's oracle descriptor and key reference"""

    def __init__(self, oracle, points, cfg):
        self.points = points
        o = oracle.Scan(points, cfg)
        self.od = o.desc()[0]
        self.bev, self.pix = o.bev()
        self.keys, self.amb, self.n_list = KR.key_reference(self.bev, self.pix, self.od["cont"], self.od["n_stored"], cfg)
        self.cfg = cfg
        self.oracle_amb = KR.check_keys(self.keys, self.amb, self.od["keys"])   # the oracle passes first

    @property
    def valid(self):
        return self.n_list >= 0

    def lists(self):
        return self.n_list[self.valid]

    def windows(self):
        """(r_min, r_max) of every valid anchor's window"""
        pad = int(np.ceil(np.float32(self.cfg.roi_radius) + np.float32(1.0)))
        out = []
        for ll, seq in np.argwhere(self.valid):
            r_cen = int(self.od["cont"][ll][seq]["pos_mean"][0])
            out.append((max(0, r_cen - pad), min(N_ROW - 1, r_cen + pad)))
        return out

    def row_entries(self, r_min, r_max):
        """list entries (cells above the lowest level) in rows r_min .. r_max: what the list path's read walks"""
        return int((self.bev.reshape(N_ROW, N_COL)[r_min:r_max + 1] > np.float32(LV[0])).sum())


_REFS = {}
TALLY = {"ambiguous": 0, "ring_nonzero": 0, "scans": 0}


def ref_of(oracle, name, cfg_kw=(), build=None):
    """the cached reference of scene `name` under the config changes cfg_kw (a tuple of (field, value))"""
    key = (name, tuple(cfg_kw))
    if key not in _REFS:
        pts = build() if build is not None else SCENES[name]()
        _REFS[key] = Ref(oracle, pts, make_cfg(oracle.L, **dict(cfg_kw)))
    return _REFS[key]


def check_scan(ref, got, what):
    """one back-end descriptor against its reference; returns the number of ambiguous components (also tallied)"""
    over = ref.n_list > KEYS_CAP
    ignore = np.zeros(ref.keys.shape, bool)
    ignore[over, 3:] = True                                   # a clamped list: components 0..2 stay exact, the rings are flagged
    n_amb = KR.check_keys(ref.keys, ref.amb, got["keys"], ignore=ignore)
    want_flags = int(ref.od["flags"]) | (INEXACT_KEYS if over.any() else 0)
    assert int(got["flags"]) == want_flags, (what, int(got["flags"]), want_flags)
    rest = got.copy()
    rest["keys"] = ref.od["keys"]
    rest["flags"] = ref.od["flags"]
    bad = compare_desc(ref.od, rest, float_exact=True)
    assert not bad, (what, bad[:5])
    TALLY["ambiguous"] += n_amb + ref.oracle_amb
    TALLY["ring_nonzero"] += 2 * int((ref.keys[..., 3:] != 0).sum())
    TALLY["scans"] += 1
    return n_amb


def assert_cap():
    print("key reference: %d ambiguous of %d non-zero ring components over %d scans (oracle and product counted)"
          % (TALLY["ambiguous"], TALLY["ring_nonzero"], TALLY["scans"]))
    assert TALLY["ambiguous"] <= AMBIGUOUS_CAP * TALLY["ring_nonzero"], TALLY


def run(be, oracle, names, cfg_kw=(), debug=False, refs=None, want_path=None):
    """one ingest call of the scenes `names` (or the given refs) under cfg_kw; every scan checked.  -> (refs, descriptors)"""
    refs = refs if refs is not None else [ref_of(oracle, n, cfg_kw) for n in names]
    assert len(refs) <= 24
    cfg = make_cfg(oracle.L, **dict(cfg_kw))
    d = be.ingest([r.points for r in refs], cfg, debug=debug)
    assert len(d) == len(refs)
    for i, r in enumerate(refs):
        check_scan(r, d[i], (names[i] if names else i, cfg_kw))
    paths = be.paths()
    if want_path is not None and paths is not None:
        assert paths[want_path] == set(range(len(refs))), (want_path, paths)
    if want_path is not None:
        pc = be.path_counts()
        assert {k: pc[k] for k in ("list", "mid", "big")} == {k: len(refs) if k == want_path else 0 for k in ("list", "mid", "big")}, (want_path, pc)
    assert_cap()
    return refs, d


def n_valid(ref):
    return int(ref.valid.sum())


# ---------------------------------------------------------------- the cases ----------------------------------------------------------------
def case_quad_tails_and_empty_list(be, oracle):
    (short, mesas), d = run(be, oracle, ["tails_short", "tails_mesas"], want_path="list")
    assert sorted(short.lists().tolist()) == [0, 1, 2, 3, 4, 5], short.n_list          # n = 1 .. 5 and the empty list
    assert n_valid(mesas) == 36 and {int(n) % KEYS_KL for n in mesas.lists()} == {0, 1, 2, 3}, mesas.n_list
    assert mesas.lists().min() >= 25 and mesas.lists().max() <= 30
    ll, seq = np.argwhere(short.n_list == 0)[0]
    for keys in (short.od["keys"], d[0]["keys"]):                                        # 0 * inf: NaN rings, finite components 0..2
        assert np.isfinite(keys[ll, seq, :3]).all() and keys[ll, seq, 0] > 0 and np.isnan(keys[ll, seq, 3:]).all(), keys[ll, seq]
    assert (short.od["n_stored"][1] >= 3) and (d[0]["keys"][1] == 0).all()               # level 1: contours below min_cont_key_cnt only


def case_anchor_groups(be, oracle):
    names = ["group_1", "group_17", "group_18", "group_19", "group_36"]
    refs, d = run(be, oracle, names, want_path="list")
    assert [n_valid(r) for r in refs] == [1, 17, 18, 19, 36], [n_valid(r) for r in refs]
    for r in refs[:2]:                                  # cell_cnt == min_cont_key_cnt - 1 next to == min_cont_key_cnt on level 0
        cnt = r.od["cont"][0]["cell_cnt"][:int(r.od["n_stored"][0])].tolist()
        assert 8 in cnt and 9 in cnt, cnt
        s8, s9 = cnt.index(8), cnt.index(9)
        assert s8 < 6 and r.n_list[0, s8] == -1 and r.n_list[0, s9] >= 0, (cnt, r.n_list[0])
    for r in refs[3:]:                                  # slot by slot, the second group's lists are shorter than the first group's
        v = r.lists()                                   # (ascending anchor order = the kernel's vlist)
        first, second = v[:KEYS_GRP], v[KEYS_GRP:]
        assert len(second) >= 1 and (second < first[:len(second)]).all(), v


def case_clipping_and_seams(be, oracle):
    (clip, seams), _ = run(be, oracle, ["clip", "seams"], want_path="list")
    pad = 11
    cen = [(int(clip.od["cont"][ll][seq]["pos_mean"][0]), int(clip.od["cont"][ll][seq]["pos_mean"][1])) for ll, seq in np.argwhere(clip.valid)]
    near = {(r < pad, r > N_ROW - 1 - pad, c < pad, c > N_COL - 1 - pad) for r, c in cen}
    for edge in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), (0, 1, 0, 1)):
        assert tuple(bool(e) for e in edge) in near, (edge, cen)           # every border and every corner clips a window
    assert any(r_max == N_ROW - 1 for _, r_max in clip.windows())           # a window that ends in the last row: cell >= n_cell
    w = seams.windows()
    assert any(r_min > 0 and (r_min * N_COL) % 64 == 0 for r_min, _ in w), w
    assert any(r_max + 1 < N_ROW and ((r_max + 1) * N_COL) % 64 == 0 for _, r_max in w), w


def _cap_refs(oracle, target):
    """the cap scene whose longest list has exactly `target` cells: cells of the level-0 anchor's list, nearest its centre first (so
    that every anchor on the plateau loses them alike), lowered until the reference counts `target`"""
    cfg_kw = (("roi_radius", CAP_RADIUS),)
    key = ("cap_%d" % target, cfg_kw)
    if key in _REFS:
        return _REFS[key]
    r0, c0, nr, nc = PLATEAU
    order = sorted(((r, c) for r in range(r0, r0 + nr) for c in range(c0, c0 + nc)),
                   key=lambda rc: ((rc[0] - (r0 + nr / 2 - 0.5)) ** 2 + (rc[1] - (c0 + nc / 2 - 0.5)) ** 2, rc))
    k = 0
    for _ in range(12):
        ref = Ref(oracle, scene_cap(order[:k]), make_cfg(oracle.L, **dict(cfg_kw)))
        longest = int(ref.lists().max())
        if longest == target:
            _REFS[key] = ref
            return ref
        assert longest > target or k > 0, (longest, target)
        k += longest - target
        assert 0 <= k < 60, k
    raise AssertionError("no cap scene with a longest list of %d cells" % target)


def case_long_stretches_and_cap(be, oracle):
    (full, thin), _ = run(be, oracle, ["plateau", "plateau_thin"], want_path="list")
    assert int(full.od["layer_cell_cnt"][0]) >= 2500 and n_valid(full) >= 6
    assert max(full.row_entries(*w) for w in full.windows()) > ROUND_ENTRIES            # several rounds of nine 64-entry stretches
    assert 0 < max(thin.row_entries(*w) for w in thin.windows()) < ROUND_ENTRIES        # one round
    assert full.lists().max() <= KEYS_CAP and full.lists().max() > 250
    refs = [_cap_refs(oracle, t) for t in (KEYS_CAP - 1, KEYS_CAP, KEYS_CAP + 1)]
    _, d = run(be, oracle, None, (("roi_radius", CAP_RADIUS),), refs=refs, want_path="list")
    assert [int(r.lists().max()) for r in refs] == [415, 416, 417]
    assert [int(x) & INEXACT_KEYS for x in d["flags"]] == [0, 0, INEXACT_KEYS], d["flags"]
    over = refs[2]
    assert (over.lists() <= KEYS_CAP).any()             # anchors with a list of their own that fits: exact (check_scan) under the flag


def case_radii_and_piv_firsts(be, oracle):
    names = ["tails_short", "tails_mesas", "group_36", "clip", "plateau_thin"]
    refs, _ = run(be, oracle, names, (("roi_radius", 3.5),), want_path="list")            # roi_pad 5
    assert all(r.lists().max() < 45 for r in refs) and n_valid(refs[2]) == 36
    refs, d = run(be, oracle, names, (("piv_firsts", 3),), want_path="list")
    assert n_valid(refs[2]) == 18 and all((r.n_list[:, 3:] == -1).all() for r in refs)
    assert (d["keys"][:, :, 3:] == 0).all() and (d["keys"][2][:, :3, 0] > 0).all()         # the anchors beyond piv_firsts: all-zero


PATH_SCENES = ["tails_short", "tails_mesas", "group_19", "group_36", "clip", "seams", "plateau_thin"]
N_BLOBS = 330


def case_three_paths_both_launch_shapes_and_debug(be, oracle):
    """The same key scenes through the list kernel (LISTED branch), cc_k_contours_mid (min_cont_cell_cnt = 4: the window-probing
    branch) and cc_k_contours_big (about 330 more 3-cell blobs on the two lowest levels); the list run once as a batch of at most 8
    scans without the debug outputs (K1: split sweep + merge kernel) and once as a larger batch with them (one workgroup per scan;
    the dense image changes what K2 reads)."""
    refs, d7 = run(be, oracle, PATH_SCENES, want_path="list")
    assert len(refs) <= 8
    _, d14 = run(be, oracle, PATH_SCENES + PATH_SCENES, debug=True, want_path="list")
    assert d14[:7].tobytes() == d7.tobytes() and d14[7:].tobytes() == d7.tobytes(), "batch shape / debug outputs change a descriptor"
    run(be, oracle, PATH_SCENES, (("min_cont_cell_cnt", 4),), want_path="mid")
    big = []
    for n in PATH_SCENES:
        def build(n=n):
            s = Scene()
            pts = SCENES[n]()
            cells = np.floor(pts[:, :2].astype(np.float64) + 75.0).astype(int)
            for (r, c), z in zip(cells, pts[:, 2]):
                s.h[(int(r), int(c))] = float(z) + 2.0
            return np.concatenate([pts, Scene.points(_only_blobs(s), 40)])
        big.append(ref_of(oracle, n + "+blobs", (), build))
    assert all(int(r.od["n_cont"].max()) > 320 for r in big), [int(r.od["n_cont"].max()) for r in big]
    run(be, oracle, None, refs=big, want_path="big")


def _only_blobs(s):
    """a scene of the N_BLOBS blobs that fit into the free spots of scene s"""
    before = set(s.h)
    s.blobs(N_BLOBS, H(1) + 0.1)
    out = Scene()
    out.h = {k: v for k, v in s.h.items() if k not in before}
    return out
