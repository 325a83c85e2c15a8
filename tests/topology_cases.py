"""TEST INFRASTRUCTURE: images built for K2's front half -- the label forest, the member lists and the statistics walks of
csrc/k_contours_list.h (and of the round-5 body behind it, csrc/k_contours.h) --, written once over the back end of
tests/height_images.py (open, close, images, paths, float_exact; test_emu_topology.py: the CPU harness, test_gpu_topology.py: the
device).  A back end here also has path_counts(): {"list", "mid", "big", "why"} of its last call, from two readings of
cc_ingest_path_counts.

Every image and its in-cell positions come from the oracle (oracle.Scan(points).bev(): one point per cell at a jittered position, a
height that varies from cell to cell inside its level's band), never from the code under test.  Two references judge a descriptor:
  R1  the oracle: parity.compare_desc on the descriptor, the oracle's label images on the debug labels;
  R2  restate(): the partition by scipy.ndimage.label, the leading fields of every kept component's row in numpy with every
      operation rounded as cc_calc_stat_vals (csrc/cc_stats.h) writes it -- sequential f64 sums in raster order, the f32 height
      sum, then f32 expressions.  check_r2 is applied to the ORACLE's descriptor and labels first, then to the back end's.
Which body takes a scan is predicted from the oracle's descriptor alone (expected_path: the capacities of k_contours_list.h restated)
and asserted on the back end's counters; a designed scene also asserts that the prediction is the path it was designed for.

The CPU harness runs a workgroup's threads one after the other: it shows the outcome of ONE order of the unions.  The device
tests are the only evidence about concurrent orders, and they are evidence of outcomes, not of which interleavings occurred."""
import collections
import itertools
import zlib

import numpy as np
from scipy import ndimage

import key_cases as KC
from key_cases import H, Scene
from parity import compare_desc

N = 150
MAXC, LIST_CAP, SLOT_CAP, MEMB, WL_CAP = 320, 3072, 12800, 11264, 5632   # CC_MAXC, CC_K2L_NCAP, _SCAP, _MEMB, _WL_CAP
EMPTY = np.float32(-1000.0)
LEAD = ("level", "cell_cnt", "poi", "pos_mean", "pos_cov", "vol3_mean", "com")


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def vary(s):
    """every cell's height raised by a per-cell multiple of 1 / 64 below 1 / 4: inside the 0.5-wide band of its level (H(k) is
    the band's floor + 0.2), different from cell to cell -- the f32 height sum of a component depends on the order of its members"""
    for (r, c), h in s.h.items():
        s.h[(r, c)] = h + ((7 * r + 13 * c) % 16) / 64.0
    return s


def levels_of(s):
    """[150, 150] level counts of a scene (0: not an entry), from the heights as built"""
    lv = np.zeros((N, N), np.int64)
    for (r, c), h in s.h.items():
        lv[r, c] = int(np.sum(np.float32(h) > np.array(KC.LV, np.float32)))
    return lv


def link_count(levels):
    """Links stage B of the list kernel files for an image of level counts (a precondition helper, never a judge): per entry, with
    sh_x = the levels it shares with its W / NW / N / NE neighbour, W at every level on the first entry of a 64-entry stretch; N
    where not both W and NW share the level; NW where neither N nor W does; NE where N does not."""
    L = np.asarray(levels, np.int64)
    act = L > 0
    idx = np.cumsum(act.ravel()).reshape(L.shape) - 1
    W, NW, Nn, NE = (np.zeros_like(L) for _ in range(4))
    W[:, 1:] = L[:, :-1]
    NW[1:, 1:] = L[:-1, :-1]
    Nn[1:, :] = L[:-1, :]
    NE[1:, :-1] = L[:-1, 1:]
    sw, snw, sn, sne = (np.minimum(L, x) for x in (W, NW, Nn, NE))
    m_w = np.where(idx % 64 == 0, sw, 0)
    m_n = np.maximum(sn - np.minimum(sw, snw), 0)
    m_nw = np.maximum(snw - np.maximum(sn, sw), 0)
    m_ne = np.maximum(sne - sn, 0)
    return int((m_w + m_n + m_nw + m_ne)[act].sum())


def _spiral_cells(n):
    """cells (y, x) of a clockwise inward square spiral of pitch 4 in the box [0, n]^2, from (0, 0)"""
    out = [(0, 0)]
    y = x = 0
    top, left, bottom, right = 0, 0, n, n
    while True:
        if right - x < 1:
            break
        while x < right:
            x += 1
            out.append((y, x))
        top += 4
        if bottom - y < 1:
            break
        while y < bottom:
            y += 1
            out.append((y, x))
        right -= 4
        if x - left < 1:
            break
        while x > left:
            x -= 1
            out.append((y, x))
        bottom -= 4
        if y - top < 1:
            break
        while y > top:
            y -= 1
            out.append((y, x))
        left += 4
    return out


def scene_spirals(flip):
    """two interleaved spirals (arms of one between the arms of the other, one empty cell apart), one component each; as built the
    root of each is the outer end of its arm, turned by 180 degrees it is a corner of the outer turn and the arm winds inward from it"""
    s = Scene()
    n = 56
    cells = [(y, x) for y, x in _spiral_cells(n)] + [(y + 2, x + 2) for y, x in _spiral_cells(n - 4)]
    for y, x in cells:
        if flip:
            y, x = n - y, n - x
        s.cell(2 + y, 8 + x, H(2))
    return vary(s)


def scene_comb(bar_on_top, teeth=50, tall=50):
    s = Scene()
    r0, c0 = 4, 10
    for k in range(teeth):
        s.rect(r0, c0 + 2 * k, tall, 1, H(2))
    s.rect(r0 - 1 if bar_on_top else r0 + tall, c0, 1, 2 * teeth - 1, H(2))
    return vary(s)


def scene_combs_interlocked():
    s = Scene()
    r0, c0 = 4, 10
    s.rect(r0, c0, 1, 100, H(2))
    s.rect(r0 + 43, c0, 1, 100, H(2))
    for k in range(25):
        s.rect(r0 + 1, c0 + 4 * k, 40, 1, H(2))
        s.rect(r0 + 3, c0 + 4 * k + 2, 40, 1, H(2))
    return vary(s)


def scene_serpentine():
    s = Scene()
    r0, c0 = 3, 10
    for k in range(25):
        s.rect(r0 + 2 * k, c0, 1, 100, H(1))
        if k < 24:
            s.cell(r0 + 2 * k + 1, c0 + (99 if k % 2 == 0 else 0), H(1))
    return vary(s)


def scene_checker(rows=40, cols=100, top=4):
    """cells with (r + c) even of a rows x cols block on levels 0..top: every inner cell links NW and NE on every level"""
    s = Scene()
    r0, c0 = 2, 10
    for r in range(r0, r0 + rows):
        for c in range(c0, c0 + cols):
            if (r + c) % 2 == 0:
                s.cell(r, c, H(top))
    return vary(s)


def scene_links(n):
    """exactly n links, every one of them needed (no cycles): 112 diagonals of 11 cells on five levels (50 links each) and one of
    n - 5 599 cells on level 0 -- whichever link the work list has no room for, its union decides a component"""
    s = Scene()
    for k in range(112):
        for i in range(11):
            s.cell(2 + 12 * (k // 40) + i, 10 + 3 * (k % 40) + i, H(4))
    for i in range(n - 5600 + 1):
        s.cell(45 + i, 10 + i, H(0))
    return vary(s)


def scene_ziggurat(pit):
    s = Scene()
    r0, c0, n = 5, 20, 30
    for r in range(n):
        for c in range(n):
            d = min(r, c, n - 1 - r, n - 1 - c, 5)
            s.cell(r0 + r, c0 + c, H(5 - d if pit else d))
    return vary(s)


def scene_staircase():
    """W, NW, N, NE of a cell with four different level counts, in all 24 orders, side by side; under a cell of six levels (its
    links reach the neighbours' counts) and under one of three"""
    s = Scene()
    for row, top in ((10, 5), (20, 2)):
        for k, (w, nw, n_, ne) in enumerate(itertools.permutations((1, 2, 3, 4))):
            c = 8 + 5 * k
            s.cell(row, c + 1, H(top))
            s.cell(row, c, H(w - 1))
            s.cell(row - 1, c, H(nw - 1))
            s.cell(row - 1, c + 1, H(n_ - 1))
            s.cell(row - 1, c + 2, H(ne - 1))
    return vary(s)


def scene_edge_strips():
    s = Scene()
    s.rect(5, 147, 40, 3, H(3))
    s.rect(5, 0, 40, 3, H(3))
    return vary(s)


def scene_edge_alternating():
    """three-cell pieces at the end of a row and at the start of a later one, raster neighbours across the image edge: the next row
    (no neighbours at all), two rows on (cell (r + 2, 0)'s NW field starts at (r, 149), the cell before its true N), the same row
    (cell (r, 149)'s NE field ends at (r, 0)) -- every piece stays a component of its own"""
    s = Scene()
    for k in range(21):
        r = 50 + 4 * k
        s.rect(r, 147, 1, 3, H(3))
        s.rect(r + (1, 2, 0)[k % 3], 0, 1, 3, H(3))
    return vary(s)


def scene_bars_at_stretch_borders():
    """a bar of 140 cells starting at each of the entry positions 60..66 of its 64-entry stretch (single filler cells before it shift
    the entry index): the run crosses the stretch border at every phase"""
    s = Scene()
    n, phases = 0, []
    for j in range(7):
        fr = 2 + 4 * j
        f = (60 + j - n) % 64
        for k in range(f):
            s.cell(fr, 2 + 2 * k, H(1))
        n += f
        phases.append(n % 64)
        s.rect(fr + 2, 5, 1, 140, H(1))
        n += 140
    assert phases == [v % 64 for v in range(60, 67)], phases
    return vary(s)


def scene_diagonals():
    """a diagonal of 70 cells (the NW neighbour's cell index advances by 151 = 23 mod 64 per step: every position of the 3-cell
    neighbour field in its bitmap word) and an anti-diagonal of 58"""
    s = Scene()
    for k in range(70):
        s.cell(2 + k, 60 + k, H(2))
    for k in range(58):
        s.cell(2 + k, 58 - k, H(2))
    nw = {((2 + k - 1) * N + 60 + k - 1) % 64 for k in range(1, 70)}
    assert nw >= {58, 59, 60, 61, 62, 63, 0, 1, 2}
    return vary(s)


def scene_last_rows():
    s = Scene()
    s.rect(148, 100, 2, 50, H(3))
    s.rect(146, 20, 4, 3, H(1))
    return vary(s)


SIZES = [1, 2] + list(range(3, 18)) + [23, 24, 25, 31, 32, 33, 63, 64, 65, 71, 72, 73, 127, 128, 129, 135, 136, 137]


def _shape(kind, a):
    """`a` cells as a one-row bar, a one-cell-wide staircase (diagonal steps, turning every 8 columns) or a two-row slab"""
    if kind == "bar":
        return [(0, x) for x in range(a)]
    if kind == "stair":
        return [(i, abs(((i + 8) % 16) - 8)) for i in range(a)]
    return [(0, x) for x in range((a + 1) // 2)] + [(1, x) for x in range(a // 2)]


def _pack(s, shapes, regions, h):
    """shelf packing of cell lists into rectangles (r0, c0, r1, c1 inclusive), one empty cell at least between any two"""
    it = iter(regions)
    r0, c0, r1, c1 = next(it)
    y, x, shelf = r0, c0, 0
    for cells in sorted(shapes, key=lambda cs: -max(c[0] for c in cs)):
        hh, ww = max(c[0] for c in cells) + 1, max(c[1] for c in cells) + 1
        while True:
            if x + ww - 1 > c1:
                y, x, shelf = y + shelf + 1, c0, 0
            if y + hh - 1 > r1:
                r0, c0, r1, c1 = next(it)
                y, x, shelf = r0, c0, 0
                continue
            break
        for dy, dx in cells:
            s.cell(y + dy, x + dx, h)
        x += ww + 1
        shelf = max(shelf, hh)
    return s


def scene_areas(kind):
    """separate components of SIZES cells each: the lane walk's 8-member steps with every tail, the eight-lane walk from 64 cells
    (list body) and above 128 (round-5 body)"""
    wide = [(1, 0, 66, 149), (84, 0, 149, 149)]
    sides = [(1, 0, 149, 66), (1, 84, 149, 149)]
    return vary(_pack(Scene(), [_shape(kind, a) for a in SIZES], sides if kind == "stair" else wide, H(1)))


def scene_area_3000():
    s = Scene().rect(2, 10, 50, 60, H(0))
    s.cell(60, 10, H(0)).rect(60, 20, 1, 2, H(0)).rect(60, 30, 1, 3, H(1))
    return vary(s)


def scene_tied_bars():
    """310 five-cell bars on levels 0 and 1: every comparison of the size sort is a tie"""
    s = Scene()
    k = 0
    for r in range(2, 150, 2):
        for c in range(1, 144, 7):
            if k < 310 and all((r - 75) ** 2 + (cc - 75) ** 2 > 32 for cc in range(c, c + 5)):
                s.rect(r, c, 1, 5, H(1))
                k += 1
    assert k == 310
    return vary(s)


LATTICE_SHAPES = [
    [(0, 0), (0, 1), (0, 2), (0, 3)],     # bar
    [(0, 1), (1, 1), (2, 1), (2, 0)],     # L opening left
    [(0, 0), (1, 0), (2, 0), (2, 1)],     # L opening right
    [(0, 2), (0, 3), (1, 0), (1, 1)],     # two steps down-left: the second row starts left of the first
    [(0, 0), (0, 1), (1, 2), (1, 3)],     # two steps down-right
]


def scene_parity_lattice(pr, pc):
    """four-cell components of five shapes on level 1 at all four (row, column) parities, inside a level-0 plateau whose first row
    and column have parity (pr, pc)"""
    s = Scene().rect(2 + pr, 10 + pc, 44, 50, H(0))
    t = 0
    for a in range(7):
        for b in range(6):
            oy, ox = 4 + 6 * a + ((t // 5) % 4 >> 1), 12 + 8 * b + ((t // 5) % 4 & 1)
            for dy, dx in LATTICE_SHAPES[t % 5]:
                s.cell(oy + dy, ox + dx, H(1))
            t += 1
    return vary(s)


def scene_tied_cups():
    """A cup of 24 cells (right wall one row taller than the left: its first row holds column x + 10 alone, its second row starts at
    x) around a block of 24: equal areas, and the cup comes first in the insertion order only through the first column of its SECOND
    row (cB < cA, where the first row is the upper row of its pair of rows); at both parities of the first row and of x"""
    s = Scene()
    for r, x in ((10, 10), (11, 30), (30, 11), (31, 31)):
        s.rect(r + 1, x, 6, 1, H(1)).rect(r + 7, x, 1, 11, H(1)).rect(r, x + 10, 7, 1, H(1))
        s.rect(r, x + 2, 4, 6, H(1))
    return vary(s)


def scene_plateau_reason3():
    return vary(Scene().rect(4, 10, 40, 50, H(5)))


def scene_padding_reason3():
    """256 bars of 11 cells on levels 0..3: 11 264 slots -- the member lists' block -- and 256 padding entries per level on top"""
    s = Scene()
    k = 0
    for r in range(2, 50, 2):
        for c in range(1, 140, 13):
            if k < 256:
                s.rect(r, c, 1, 11, H(3))
                k += 1
    assert k == 256
    return vary(s)


def scene_even_11262():
    """two components per level, every area even: 11 262 slots and no padding"""
    s = Scene().rect(2, 10, 20, 50, H(5))
    s.rect(30, 10, 10, 50, H(5)).rect(40, 10, 15, 50, H(2)).rect(55, 10, 1, 4, H(2))
    return vary(s)


def with_filler(base):
    """single level-0 cells, not 8-adjacent to anything, that take the scene past the list's 3 072 entries"""
    probe = Scene()
    probe.h = dict(base.h)
    out = Scene()
    need = LIST_CAP + 1 - len(base.h)
    for r in range(1, N, 2):
        for c in range(0, N, 2):
            if len(out.h) < need and (r - 75) ** 2 + (c - 75) ** 2 > 32 and probe.free(r, c, 1):
                out.h[(r, c)] = H(0)
    assert len(out.h) == need, (len(out.h), need)
    return out


def with_blobs(base):
    probe = Scene()
    probe.h = dict(base.h)
    probe.blobs(330, H(1) + 0.1)
    out = Scene()
    out.h = {k: v for k, v in probe.h.items() if k not in base.h}
    return out


Case = collections.namedtuple("Case", "name scene extra cfg_kw want why n_comp links")


def _case(name, scene, want="list", why=None, cfg_kw=(), extra=None, n_comp=None, links=None):
    return Case(name, scene, extra, tuple(cfg_kw), want, why, n_comp, links)


def designed():
    """name -> Case, the base scenes; n_comp: components scipy must count on level 0 (any size), links: link_count of the image"""
    cs = [
        _case("spirals", scene_spirals(False), n_comp=2),
        _case("spirals_turned", scene_spirals(True), n_comp=2),
        _case("comb_bar_under", scene_comb(False), n_comp=1),
        _case("comb_bar_on_top", scene_comb(True), n_comp=1),
        _case("combs_interlocked", scene_combs_interlocked(), n_comp=2),
        _case("serpentine", scene_serpentine(), n_comp=1),
        _case("checkerboard", scene_checker(), n_comp=1, links=19305),
        _case("links_5631", scene_links(WL_CAP - 1), n_comp=113, links=WL_CAP - 1),
        _case("links_5632", scene_links(WL_CAP), n_comp=113, links=WL_CAP),
        _case("links_5633", scene_links(WL_CAP + 1), n_comp=113, links=WL_CAP + 1),
        _case("ziggurat", scene_ziggurat(False), n_comp=1),
        _case("pit", scene_ziggurat(True), n_comp=1),
        _case("staircase", scene_staircase(), n_comp=48),
        _case("edge_strips", scene_edge_strips(), n_comp=2),
        _case("edge_alternating", scene_edge_alternating(), n_comp=42),
        _case("bars_at_stretch_borders", scene_bars_at_stretch_borders()),
        _case("diagonals", scene_diagonals(), n_comp=2),
        _case("last_rows", scene_last_rows(), n_comp=2),
        _case("tied_bars", scene_tied_bars(), n_comp=310),
        _case("tied_cups", scene_tied_cups(), n_comp=8),
        _case("plateau_reason3", scene_plateau_reason3(), "mid", 3, n_comp=1),
        _case("padding_reason3", scene_padding_reason3(), "mid", 3, n_comp=256),
        _case("even_11262", scene_even_11262(), n_comp=2),
    ]
    for pr in (0, 1):
        for pc in (0, 1):
            cs.append(_case("lattice_%d%d" % (pr, pc), scene_parity_lattice(pr, pc), n_comp=1))
    for mc in (1, 2, 3, 4, 7):
        for kind in ("bar", "stair", "slab"):
            cs.append(_case("areas_%s_min%d" % (kind, mc), scene_areas(kind), "list" if mc <= 3 else "mid", None if mc <= 3 else 0,
                            (("min_cont_cell_cnt", mc),), n_comp=len(SIZES)))
        cs.append(_case("area_3000_min%d" % mc, scene_area_3000(), "list" if mc <= 3 else "mid", None if mc <= 3 else 0,
                        (("min_cont_cell_cnt", mc),), n_comp=4))
    return collections.OrderedDict((c.name, c) for c in cs)


_DESIGNED = {}


def cases(which):
    """the designed cases: "base"; "mid": every base scene with at most 2 300 entries, plus filler past 3 072 entries; "big": the same
    scenes plus 330 blobs.  Both under the default min_cont_cell_cnt of 3 (the areas scenes in their min3 form): with 1 or 2 the
    filler's single cells would be kept components -- more than 320 on level 0, another body than the one meant -- and with 4 or 7 the
    scene is on the mid body already (base)"""
    if "base" not in _DESIGNED:
        base = designed()
        _DESIGNED["base"] = base
        small = [c for c in base.values() if len(c.scene.h) <= 2300 and dict(c.cfg_kw).get("min_cont_cell_cnt", 3) == 3]   # (the areas scenes: their min3 form)
        _DESIGNED["mid"] = collections.OrderedDict(
            (c.name + "+filler", c._replace(name=c.name + "+filler", extra=with_filler(c.scene), want="mid", why=1, n_comp=None, links=None)) for c in small)
        _DESIGNED["big"] = collections.OrderedDict(
            (c.name + "+blobs", c._replace(name=c.name + "+blobs", extra=with_blobs(c.scene), want="big", why=-1, n_comp=None, links=None)) for c in small)
    return _DESIGNED[which]


GROUPS = {
    "forests": ["spirals", "spirals_turned", "comb_bar_under", "comb_bar_on_top", "combs_interlocked", "serpentine"],
    "work_list": ["checkerboard", "links_5631", "links_5632", "links_5633"],
    "ownership": ["ziggurat", "pit", "staircase"],
    "edges": ["edge_strips", "edge_alternating", "bars_at_stretch_borders", "diagonals", "last_rows"],
    "ties": ["tied_bars", "tied_cups", "lattice_00", "lattice_01", "lattice_10", "lattice_11"],
    "hand_off": ["plateau_reason3", "padding_reason3", "even_11262"],
}
for _mc in (1, 2, 3, 4, 7):
    GROUPS["areas_min%d" % _mc] = ["areas_%s_min%d" % (k, _mc) for k in ("bar", "stair", "slab")] + ["area_3000_min%d" % _mc]


# ---------------------------------------------------------------- random images ----------------------------------------------------------------
def rand_image(seed, recipe="list"):
    """A random multi-level image as a Scene.  Four families by seed % 4: independent levels 0..5 per cell; a smooth field plus
    noise (nested level sets); levels capped at 0..2; the cells of one checkerboard colour plus 10 % of the other (diagonal-heavy).
    "list": occupancy uniform in [0.25, 0.65] inside a random rectangle of 20..140 x 20..150 cells, cut at a random budget of
    500..3 060 entries and 12 700 slots; "mid": 3 073 entries or more, occupancy in [0.85, 0.97] inside 62..75 x 62..75 cells (88..100 for the checkerboard family); "big": a 60 x 60 random block plus 330 blobs (added by the caller)."""
    rng = np.random.default_rng([seed, {"list": 0, "mid": 1, "big": 2}[recipe]])
    fam = seed % 4
    if recipe == "big":
        nr = nc = 60
        r0, c0 = 2, 4
    elif recipe == "mid":                 # (small and dense: few components per level)
        nr, nc = (int(rng.integers(88, 101)), int(rng.integers(88, 101))) if fam == 3 else (int(rng.integers(62, 76)), int(rng.integers(62, 76)))
        r0, c0 = int(rng.integers(1, N - nr + 1)), int(rng.integers(0, N - nc + 1))
    else:
        nr, nc = int(rng.integers(20, 141)), int(rng.integers(20, 151))
        r0, c0 = int(rng.integers(1, N - nr + 1)), int(rng.integers(0, N - nc + 1))
    p = rng.uniform(0.85, 0.97) if recipe == "mid" else rng.uniform(0.25, 0.65)
    rr, cc = np.meshgrid(np.arange(r0, r0 + nr), np.arange(c0, c0 + nc), indexing="ij")
    occ = rng.random((nr, nc)) < p
    if fam == 3:
        even = (rr + cc) % 2 == 0
        occ = (even & (rng.random((nr, nc)) < min(1.0, 2 * p))) | (~even & (rng.random((nr, nc)) < 0.1))
    if fam == 1:
        f = np.zeros((nr, nc))
        for _ in range(4):
            f += rng.uniform(0.5, 2.0) * np.sin(rr / rng.uniform(3, 15) + rng.uniform(0, 6)) * np.sin(cc / rng.uniform(3, 15) + rng.uniform(0, 6))
        lev = np.clip(np.floor(2.5 + 1.2 * f + rng.normal(0, 0.5, (nr, nc))), 0, 5).astype(int)
    else:
        lev = rng.integers(0, 3 if fam == 2 else 6, (nr, nc))
    occ &= (rr - 75) ** 2 + (cc - 75) ** 2 > 32
    if recipe == "mid":
        budget_e, budget_s = int(rng.integers(LIST_CAP + 1, 5000)), 10 ** 9
    else:
        budget_e, budget_s = int(rng.integers(500, 3061)), 12700
    s = Scene()
    e = sl = 0
    for k in rng.permutation(nr * nc):
        y, x = divmod(int(k), nc)
        if not occ[y, x]:
            continue
        if e + 1 > budget_e or sl + lev[y, x] + 1 > budget_s:
            break
        s.h[(r0 + y, c0 + x)] = H(int(lev[y, x]))
        e += 1
        sl += int(lev[y, x]) + 1
    return vary(s)


def fuzz_case(seed, recipe):
    s = rand_image(seed, recipe)
    return Case("fuzz_%s_%d" % (recipe, seed), s, with_blobs(s) if recipe == "big" else None, (), None, None, None, None)


# ---------------------------------------------------------------- references ----------------------------------------------------------------
def restate(bev, pix, cfg):
    """R2.  Per level: the kept components (scipy's 8-connected labelling of the cells above the level, those of at least
    min_cont_cell_cnt cells) as a label image (0: none), and each one's leading row fields as a tuple of integers and float bits."""
    f32, f64 = np.float32, np.float64
    lv = np.array(list(cfg.lv_grads), f32)
    bev = np.asarray(bev, f32).reshape(-1)
    px, py = np.asarray(pix, f32)[:, 0].astype(f64), np.asarray(pix, f32)[:, 1].astype(f64)
    out = []
    for l in range(len(lv)):
        lab, _ = ndimage.label((bev > lv[l]).reshape(cfg.n_row, cfg.n_col), structure=np.ones((3, 3)))
        flat = lab.ravel()
        cells = np.flatnonzero(flat)                                   # raster order
        order = np.argsort(flat[cells], kind="stable")
        cells = cells[order]
        cuts = np.flatnonzero(np.diff(flat[cells])) + 1
        rows, kept = [], np.zeros_like(flat)
        for m in np.split(cells, cuts) if len(cells) else []:
            cnt = len(m)
            if cnt < cfg.min_cont_cell_cnt:
                continue
            kept[m] = flat[m[0]]
            x, y, h = px[m], py[m], bev[m]
            ps_x, ps_y = np.cumsum(x)[-1], np.cumsum(y)[-1]
            t_xx, t_xy, t_yy = np.cumsum(x * x)[-1], np.cumsum(x * y)[-1], np.cumsum(y * y)[-1]
            vol3 = np.add.accumulate(h, dtype=f32)[-1]
            tq_x, tq_y = np.cumsum(h.astype(f64) * x)[-1], np.cumsum(h.astype(f64) * y)[-1]
            cntf = f32(cnt)
            pm0, pm1 = f32(ps_x) / cntf, f32(ps_y) / cntf
            vm = vol3 / cntf
            com0, com1 = f32(tq_x) / vol3, f32(tq_y) / vol3
            if cnt < cfg.min_cell_cov:
                sg = f32(cfg.point_sigma)
                ss, zz = f32(1.0) * sg * sg, f32(0.0) * sg * sg
                cov = (ss, zz, zz, ss)
            else:
                den = f32(cnt - 1)
                c00 = (f32(t_xx) - (pm0 * pm0) * cntf) / den
                c01 = (f32(t_xy) - (pm0 * pm1) * cntf) / den
                c10 = (f32(t_xy) - (pm1 * pm0) * cntf) / den
                c11 = (f32(t_yy) - (pm1 * pm1) * cntf) / den
                cov = (c00, c10, c01, c11)
            fl = np.array((pm0, pm1) + cov + (vm, com0, com1), f32)
            assert fl.dtype == f32
            rows.append((l, cnt, int(m[-1]) // cfg.n_col, int(m[-1]) % cfg.n_col) + tuple(int(v) for v in fl.view(np.uint32)))
        out.append({"rows": rows, "kept": kept})
    return out


def _lead(row):
    fl = np.concatenate([np.asarray(row[f], np.float32).reshape(-1) for f in ("pos_mean", "pos_cov", "vol3_mean", "com")])
    return (int(row["level"]), int(row["cell_cnt"]), int(row["poi"][0]), int(row["poi"][1])) + tuple(int(v) for v in fl.view(np.uint32))


def check_r2(r2, d, labels, what):
    """a descriptor (and debug label images, or None) against the restatement, on bits"""
    for l, lev in enumerate(r2):
        rows = lev["rows"]
        cnts = sorted((r[1] for r in rows), reverse=True)
        ns = int(d["n_stored"][l])
        assert int(d["n_cont"][l]) == len(rows), (what, l, "n_cont", int(d["n_cont"][l]), len(rows))
        assert ns == min(len(rows), MAXC), (what, l, "n_stored", ns)
        assert int(d["layer_cell_cnt"][l]) == sum(cnts), (what, l, "layer_cell_cnt", int(d["layer_cell_cnt"][l]), sum(cnts))
        got = d["cont"][l][:ns]
        gc = [int(v) for v in got["cell_cnt"]]
        assert all(a >= b for a, b in zip(gc, gc[1:])), (what, l, "cell_cnt not non-increasing")
        assert gc == cnts[:ns], (what, l, "cell_cnt multiset is not that of the largest")
        have, want = collections.Counter(_lead(r) for r in got), collections.Counter(rows)
        extra = have - want
        assert not extra, (what, l, "stored rows that are no restated row", list(extra)[:2])
        if len(rows) <= MAXC:
            assert have == want, (what, l, "row multisets differ")
        if labels is not None:
            lab, kept = np.asarray(labels[l]).reshape(-1), lev["kept"]
            assert np.array_equal(lab >= 0, kept > 0), (what, l, "labelled cells are not the kept cells")
            on = kept > 0
            pairs = np.unique(np.stack([lab[on].astype(np.int64), kept[on]], 1), axis=0)
            assert len(pairs) == len(rows) and len(set(pairs[:, 0])) == len(rows) and len(set(pairs[:, 1])) == len(rows), (what, l, "labels do not induce the partition")


def expected_path(od, bev, cfg):
    """(path, reason) from the oracle's descriptor and image: the list kernel's capacities (k_contours_list.h) restated"""
    lv = np.array(list(cfg.lv_grads), np.float32)
    above = np.asarray(bev).reshape(-1)[:, None] > lv[None, :]
    entries, slots = int(above[:, 0].sum()), int(above.sum())
    over = int(od["n_cont"].max()) > MAXC
    why = None
    if cfg.min_cont_cell_cnt > 3:
        why = 0
    elif entries > LIST_CAP or slots > SLOT_CAP:
        why = 1
    elif over:
        why = 2
    else:
        padded = sum(int(((od["cont"][l]["cell_cnt"][:int(od["n_stored"][l])].astype(np.int64) + 1) & ~1).sum()) for l in range(len(lv)))
        if padded > MEMB:
            why = 3
    return ("list" if why is None else "big" if over else "mid"), why


class Ref:
    """one case's image, positions, oracle descriptor and labels; its restatement, checked against the oracle, on demand"""

    def __init__(self, oracle, case):
        self.case, self.name = case, case.name
        self.cfg = KC.make_cfg(oracle.L, **dict(case.cfg_kw))
        seed = zlib.crc32(case.name.split("+")[0].encode())        # (a scene keeps its positions when filler or blobs join it)
        pts = case.scene.points(seed)
        if case.extra is not None:
            assert not set(case.extra.h) & set(case.scene.h)
            pts = np.concatenate([pts, case.extra.points(seed + 1)])
        o = oracle.Scan(pts, self.cfg)
        self.od = o.desc()[0]
        self.bev, self.pix = o.bev()
        self.labels = o.labels()
        n_cells = len(case.scene.h) + (len(case.extra.h) if case.extra is not None else 0)
        assert int((self.bev > EMPTY).sum()) == n_cells and not (self.bev[:N] > EMPTY).any(), "one point per cell, row 0 empty"
        self.path, self.why = expected_path(self.od, self.bev, self.cfg)
        self._r2 = None

    def r2(self):
        if self._r2 is None:
            self._r2 = restate(self.bev, self.pix, self.cfg)
            check_r2(self._r2, self.od, self.labels, (self.name, "oracle"))    # the restatement passes on the oracle first
        return self._r2

    def preconditions(self):
        """what the scene was designed to reach, asserted on the oracle / restatement side"""
        c = self.case
        if c.want is not None:
            assert self.path == c.want and c.why in (self.why, -1), (self.name, self.path, self.why)   # (-1: whichever reason)
        if c.n_comp is not None:
            lv0 = np.float32(list(self.cfg.lv_grads)[0])
            _, n = ndimage.label((self.bev > lv0).reshape(N, N), structure=np.ones((3, 3)))
            assert n == c.n_comp, (self.name, "components on level 0", n)
        if c.links is not None:
            lv = np.array(list(self.cfg.lv_grads), np.float32)
            got = link_count((self.bev[:, None] > lv[None, :]).sum(1).reshape(N, N))
            assert got == c.links, (self.name, "links", got)
        if self.cfg.min_cont_cell_cnt < 3:
            assert int(self.od["n_cont"].max()) <= MAXC, self.od["n_cont"]


_REFS = {}


def ref_of(oracle, case):
    """the designed cases' references are kept (the + filler / + blobs forms read their base's); a random image's is made for its one test"""
    if case.name.startswith("fuzz_"):
        return Ref(oracle, case)
    if case.name not in _REFS:
        _REFS[case.name] = Ref(oracle, case)
    return _REFS[case.name]


# ---------------------------------------------------------------- the runs ----------------------------------------------------------------
def _call(be, h, refs, debug):
    d, dbg = be.images(h, np.stack([r.bev for r in refs]), np.stack([r.pix for r in refs]),
                       np.array([r.od["min_bin_val"] for r in refs], np.float32), debug)
    pc = be.path_counts()
    want = collections.Counter(r.path for r in refs)
    whys = [sum(1 for r in refs if r.why == k) for k in range(4)]
    assert (pc["list"], pc["mid"], pc["big"]) == (want["list"], want["mid"], want["big"]) and list(pc["why"]) == whys, \
        ([r.name for r in refs], pc, dict(want), whys)
    paths = be.paths()
    if paths is not None:
        for i, r in enumerate(refs):
            assert i in paths[r.path], (r.name, r.path, paths)
    return d, dbg


def _judge(be, r, d, labels, r2):
    bad = compare_desc(r.od, d, float_exact=be.float_exact)
    assert not bad, (r.name, bad[:6])
    assert int(d["flags"]) == int(r.od["flags"]), (r.name, "flags", int(d["flags"]))
    if labels is not None:
        assert np.array_equal(r.labels, labels), (r.name, "debug labels")
    if r2:
        check_r2(r.r2(), d, labels, (r.name, "back end"))


def run_refs(be, refs, max_batch, singly, r2_every=1, twice=True):
    """The scans of `refs` (one configuration) in one call with the debug outputs and one without, every descriptor judged by R1 and
    every r2_every-th by R2; with `twice` the debug call is repeated with the images in reversed order -- the same scan in another
    workgroup beside other neighbours -- and must return the same bytes; with `singly` every scan also goes alone, the other launch
    shape, which attributes the path to the scan.  Only the debug call is repeated: the plain call and the one-image calls must equal
    the debug call's bytes scan by scan, so each of them already is a second run of every scan beside other (or no) neighbours."""
    h = be.open(refs[0].cfg, max_batch)
    d, dbg = _call(be, h, refs, True)
    plain, _ = _call(be, h, refs, False)
    assert plain.tobytes() == d.tobytes(), "the debug outputs change a descriptor"
    if twice:
        rd, rdbg = _call(be, h, refs[::-1], True)
        assert rd[::-1].tobytes() == d.tobytes(), "the order of the images in the call changes a descriptor"
        assert np.array_equal(rdbg["labels"][::-1], dbg["labels"]), "the order of the images in the call changes a label image"
    failed = []                                      # every scan is judged: the failure names all that fail, with the first one's reason
    for i, r in enumerate(refs):
        try:
            _judge(be, r, d[i], dbg["labels"][i], i % r2_every == 0)
        except AssertionError as e:
            failed.append((r.name, str(e)[:300]))
    if singly:
        for i, r in enumerate(refs):
            one, odbg = _call(be, h, [r], True)
            if not (one.tobytes() == d[i:i + 1].tobytes() and np.array_equal(odbg["labels"][0], dbg["labels"][i])):
                failed.append((r.name, "alone in its call: other bytes"))
    be.close(h)
    assert not failed, ("SCENES THAT FAIL: " + " ".join(sorted({n for n, _ in failed})), failed[0])
    return d


def run_group(be, oracle, names, which="base", twice=True, singly=True):
    refs = [ref_of(oracle, cases(which)[n]) for n in names]
    for r in refs:
        r.preconditions()
    if which != "base":   # the kept components of the original scene reappear unchanged among the restated rows
        for r in refs:
            base = ref_of(oracle, cases("base")[r.name.split("+")[0]])
            for lb, la in zip(base.r2(), r.r2()):
                assert not collections.Counter(lb["rows"]) - collections.Counter(la["rows"]), (r.name, "a base component changed")
    return run_refs(be, refs, max(len(refs), 1), singly, 1, twice)


def variant_names(which, part, parts):
    names = list(cases(which))
    return names[part::parts]


def run_fuzz(be, oracle, recipe, seeds, max_batch, twice):
    refs = [ref_of(oracle, fuzz_case(s, recipe)) for s in seeds]
    over = sum(int((r.od["n_cont"] > MAXC).sum()) for r in refs)
    if recipe == "list":
        assert over <= 0.02 * 6 * len(refs), ("(image, level) pairs with more than 320 components", over)
    elif recipe == "mid":
        assert all(r.why == 1 for r in refs)
    else:
        assert all(r.path == "big" for r in refs)
    return run_refs(be, refs, max_batch, False, 8, twice)
