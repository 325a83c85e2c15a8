"""TEST INFRASTRUCTURE: K3 (csrc/k_knn.h) on built keys -- the cases, the two judges and the comparison shared by
tests/test_emu_knn.py (CPU harness) and tests/test_gpu_knn.py (MI355X).  Cases are data, a back end runs them, the judges live
here; neither judge is the product.

R1, the oracle: oracle_py.DB.query(want_knn=True) for nnk <= 64, knn_oracle.DB.query_knn above, built scan by scan with the
case's timestamps and seeds.

R2, the numpy restatement (restate): f32 distances in nanoflann's accumulation order, dist_ub through the f64 products of
contour_db.h:733-749, the visible buckets {0..mid} | {2 mid + 1..5} from the oracle's bucket ranges, and the activation epochs
of a layer that never splits (one bucket: popBufferMax restated).  R2 states that a case sits on its edge and judges ties.

Comparison (hold): hit_cnt and per hit gidx, level, seq and the bits of dist_sq, of every search of every query.  The one
relaxation is a run of bit-equal dist_sq: both sides are put in key-id order inside a run; a run that the nnk-th place cuts is
held to R1 for its distances and to R2 for which keys are present (the smallest key ids of the run among the visible keys).
Tie runs may occur only in the cases that say `ties`."""
import numpy as np

F32 = np.float32
NPIV, DIM = 6, 10
QLV = (1, 2, 3)
BIG_TS = 1000.0   # a closing scan this late finds every earlier key older than max_elapse


class Case:
    """keys [n, 3, 6, 10]: scan i's keys of layer ll (all-zero: no key); q [nq, 3, 6, 10]; epochs [nq]; edge(F) raises
    AssertionError unless the case sits on the edge its name states (F: Facts, R2's figures)."""

    def __init__(self, name, keys, ts, seeds, q, epochs=None, nnk=50, qlv=QLV, edge=None, ties=False, elapse=(15.0, 25.0),
                 r2=True, prelude=False, modes=(0, 2), late_q=None):
        self.name, self.nnk, self.qlv, self.edge, self.ties, self.elapse, self.r2 = name, nnk, tuple(qlv), edge, ties, elapse, r2
        self.keys = np.ascontiguousarray(keys, F32)
        self.ts, self.seeds = np.asarray(ts, np.float64), np.asarray(seeds, np.int32)
        self.edge_r1 = None    # f(R1's counts [nq, 3, 6]): an edge that only the oracle can state (r2 = False)
        self.late_q = late_q   # f(ranges [3, 7], sorted key[0] per layer) -> q: queries placed on the oracle's bucket ranges
        self.q = None if q is None else np.ascontiguousarray(q, F32)
        self._epochs = epochs
        self.lanes1 = prelude or name.startswith("B")  # one lane: the call's queries are ONE chunk, so a layer's searches are grouped and sorted together
        self.prelude = prelude  # run a full chunk on the same lane first (set_lanes(1)): a count that is not rewritten shows
        self.modes = modes if nnk <= 64 else (0,)   # a large-k database always walks
        self.n = len(self.keys)

    @property
    def epochs(self):
        return np.full(len(self.q), self.n, np.int32) if self._epochs is None else np.asarray(self._epochs, np.int32)

    def dcfg(self, L):
        d = L.default_db_cfg()
        d.nnk, d.n_q_levels = self.nnk, len(self.qlv)
        d.min_elapse, d.max_elapse = self.elapse
        for i, v in enumerate(self.qlv):
            d.q_levels[i] = v
        return d

    def desc(self, L, keys):
        """descriptors whose only content is the retrieval keys (dummy all-zero contour rows keep the checks' lookups in range)"""
        d = np.zeros(len(keys), L.scan_desc_dt)
        for ll, lev in enumerate(self.qlv):
            d["keys"][:, lev] = keys[:, ll]
        d["n_cont"][:] = L.NPIV
        d["n_stored"][:] = L.NPIV
        d["layer_cell_cnt"][:] = 1
        return d


# ---------------------------------------------------------------------------------------------------------------------
# R2
def dist_f32(q, K):
    """L2_Adaptor::evalMetric (nanoflann.hpp:427-461) for dim 10 in exact f32: two groups of four, then two single terms"""
    d = (q[None, :].astype(F32) - K.astype(F32)).astype(F32)
    s = (d * d).astype(F32)
    a = (((s[:, 0] + s[:, 1]).astype(F32) + s[:, 2]).astype(F32) + s[:, 3]).astype(F32)
    b = (((s[:, 4] + s[:, 5]).astype(F32) + s[:, 6]).astype(F32) + s[:, 7]).astype(F32)
    r = (F32(0) + a).astype(F32)
    r = (r + b).astype(F32)
    r = (r + s[:, 8]).astype(F32)
    return (r + s[:, 9]).astype(F32)


def dist_ub(k):
    """contour_db.h:733-749: the bounds are f32 results of f64 products, the rest is f32"""
    k = k.astype(F32)
    b = [F32(np.float64(k[0]) * 0.8), F32(np.float64(k[0]) / 0.8), F32(np.float64(k[1]) * 0.8), F32(np.float64(k[1]) / 0.8),
         F32(np.float64(k[2]) * 0.8 * 0.75), F32(np.float64(k[2]) / (0.8 * 0.75))]
    t = [F32(F32(k[i // 2] - b[i]) * F32(k[i // 2] - b[i])) for i in range(6)]
    return F32(F32(max(t[0], t[1]) + max(t[2], t[3])) + max(t[4], t[5]))


def key_sum(k):
    """RetrievalKey::sum(): a left-to-right f32 sum"""
    s = F32(0)
    for v in k.astype(F32):
        s = F32(s + v)
    return s


class Layer:
    """a layer's stored keys in key-id (insertion) order, with R2's activation epochs"""

    def __init__(self, case, ll):
        k = case.keys[:, ll].reshape(-1, DIM)
        scan = np.repeat(np.arange(case.n), NPIV)
        seq = np.tile(np.arange(NPIV), case.n)
        st = np.array([key_sum(x) != 0 for x in k]) & (k[:, 0] >= -1000.0) & (k[:, 0] < 1000.0)
        self.K, self.scan, self.seq = k[st], scan[st], seq[st]
        # one bucket that never splits: a rebuild of bucket 0 (seed % 8 == 0) at scan i pops, if the oldest buffered key is
        # max_elapse old, every buffered key older than min_elapse; those keys sit in the tree from epoch i + 1
        mn, mx = case.elapse
        self.act = np.full(len(self.K), 1 << 30)
        for i in range(case.n):
            if case.seeds[i] % 8 != 0:
                continue
            buf = np.nonzero((self.act == 1 << 30) & (self.scan <= i))[0]
            if len(buf) and case.ts[self.scan[buf[0]]] <= case.ts[i] - mx:
                self.act[buf[case.ts[self.scan[buf]] < case.ts[i] - mn]] = i + 1


class Facts:
    """R2's figures of one search"""
    pass


def restate(case, layers, rg, q, epoch, ll, assume_active=False):
    """one search -> Facts: the expected list in the device's order (distance, then key id) and what states the edges"""
    Lr, F = layers[ll], Facts()
    F.valid = key_sum(q) != 0 and ll < len(case.qlv)
    F.ids = F.gidx = F.seq = np.zeros(0, np.int64)
    F.dist = np.zeros(0, F32)
    F.cut = F.ntie = 0
    if not F.valid:
        return F
    F.q0 = F32(q[0])
    K = Lr.K
    k0 = K[:, 0] + F32(0)
    mid = 0
    for i in range(6):
        if rg[i] <= q[0] and rg[i + 1] > q[0]:
            mid = i
            break
    bk = np.full(len(K), -1)
    for b in range(6):
        bk[(rg[b] <= k0) & (k0 < rg[b + 1])] = b
    vis = ((bk >= 0) & (bk <= mid)) | (bk >= 2 * mid + 1)
    act = np.ones(len(K), bool) if assume_active else Lr.act <= epoch
    F.mid, F.ub, F.bk, F.vis, F.act, F.K0 = mid, dist_ub(q), bk, vis, act, k0
    F.r = dist_f32(q, K) if len(K) else np.zeros(0, F32)
    ok = vis & act
    F.n_above, F.n_below = int((ok & (k0 >= q[0])).sum()), int((ok & (k0 < q[0])).sum())
    # the first visible range upwards [anchor, end of bucket mid) and downwards [start of bucket 2 mid + 1, anchor)
    F.up_a = int((vis & (bk <= mid) & (k0 >= q[0])).sum())
    F.up_b = int((vis & (bk > mid) & (k0 >= q[0])).sum())
    F.gap = int(((bk > mid) & (bk < 2 * mid + 1)).sum())        # keys of the skipped buckets
    cand = np.nonzero(ok & (F.r < F.ub))[0]
    order = cand[np.lexsort((cand, F.r[cand]))]
    F.in_ub = len(cand)
    F.ids, F.dist = order[:case.nnk], F.r[order[:case.nnk]]
    F.all_ids, F.all_dist = order, F.r[order]
    skipped = (~vis) & act & (bk >= 0)
    F.skipped_best = F.r[skipped].min() if skipped.any() else None
    if len(F.dist):
        last = F.dist[-1]
        F.cut = int((F.all_dist == last).sum() - (F.dist == last).sum())   # keys of the last run that the nnk-th place cuts off
        F.ntie = int(len(F.dist) - len(np.unique(F.dist.view(np.uint32)))) + (1 if F.cut else 0)
    F.gidx, F.seq = Lr.scan[F.ids], Lr.seq[F.ids]
    return F


def hold(what, lst, cnt, ref, ref_cnt, F, level, nnk):
    """one search's list `lst` against the list `ref` of the same format, by the comparison of this module's docstring"""
    assert cnt == ref_cnt, "%s: hit_cnt %d against %d" % (what, cnt, ref_cnt)
    a, b = lst[:cnt], ref[:cnt]
    assert np.array_equal(a["dist_sq"].view(np.uint32), b["dist_sq"].view(np.uint32)), "%s: dist_sq bits" % what
    assert (a["level"] == level).all() and (b["level"] == level).all(), "%s: level" % what
    ida, idb = a["gidx"].astype(np.int64) * NPIV + a["seq"], b["gidx"].astype(np.int64) * NPIV + b["seq"]
    bits = a["dist_sq"].view(np.uint32)
    i = 0
    while i < cnt:
        j = i + 1
        while j < cnt and bits[j] == bits[i]:
            j += 1
        if j == cnt and cnt == nnk and F is not None and F.cut:   # the run the nnk-th place cuts: R2 names the keys
            want = np.sort(F.gidx[i:j].astype(np.int64) * NPIV + F.seq[i:j])
            assert np.array_equal(np.sort(ida[i:j]), want), "%s: keys of the cut run at %d..%d" % (what, i, j)
        else:
            assert np.array_equal(np.sort(ida[i:j]), np.sort(idb[i:j])), "%s: keys at %d..%d" % (what, i, j)
        if j - i > 1 and what.startswith("dev"):  # inside a run the device orders by key id
            assert (np.diff(ida[i:j]) > 0).all(), "%s: key-id order inside the run %d..%d" % (what, i, j)
        i = j


def as_hits(L, F, level):
    h = np.zeros(len(F.ids), L.knn_hit_dt)
    h["gidx"], h["seq"], h["dist_sq"], h["level"] = F.gidx, F.seq, F.dist, level
    return h


# ---------------------------------------------------------------------------------------------------------------------
# R1
class Oracle:
    """the oracle's database of a case, built scan by scan, queried at the epochs the case asks for"""

    def __init__(self, case, oracle):
        import knn_oracle
        L = oracle.L
        self.case, self.L, self.large = case, L, case.nnk > L.KNN_MAX
        self.dcfg = case.dcfg(L)
        self.cfg = L.default_manager_cfg()
        self.odb = knn_oracle.DB(self.dcfg) if self.large else oracle.DB(self.dcfg)
        self.oracle, self.at = oracle, 0
        self.desc = case.desc(L, case.keys)

    def advance(self, epoch):
        c = self.case
        while self.at < epoch:
            i = self.at
            if self.large:
                self.odb.add(self.desc[i], c.ts[i], int(c.seeds[i]))
            else:
                self.odb.add_scan(self.oracle.Scan.from_desc(self.desc[i], self.cfg, int_id=i), c.ts[i])
                self.odb.push_and_balance(int(c.seeds[i]), c.ts[i])
            self.at += 1

    def ranges(self):
        if self.large:
            return None
        return self.odb.bucket_state()[1]

    def query(self, qd, j):
        if self.large:
            knn, cnt = self.odb.query_knn(qd, 100000 + j)
            return knn, cnt
        _, knn, cnt = self.odb.query(self.oracle.Scan.from_desc(qd, self.cfg, int_id=100000 + j), want_knn=True)
        return knn, cnt

    def close(self):
        if self.large:
            self.odb.close()


_R = {}


def references(case, oracle):
    """(R1 lists [nq, 3, 6, stride], R1 counts, Facts [nq][3][6], q) of a case, computed once: R1 and R2 agree on every list and
    the case's edge assertion holds, or this raises"""
    if case.name in _R:
        return _R[case.name]
    L = oracle.L
    O = Oracle(case, oracle)
    layers = [Layer(case, ll) for ll in range(3)]
    if case.late_q is not None:
        O.advance(case.n)
        case.q = np.ascontiguousarray(case.late_q(O.ranges(), [np.sort(l.K[:, 0]) for l in layers], layers), F32)
    ep = case.epochs
    nq = len(case.q)
    stride = L.KNN_MAX_LARGE if case.nnk > L.KNN_MAX else L.KNN_MAX
    knn, cnt = np.zeros((nq, 3, NPIV, stride), L.knn_hit_dt), np.zeros((nq, 3, NPIV), np.int32)
    facts = [None] * nq
    qd = case.desc(L, case.q)
    trivial = np.array([-1000.0] + [1000.0] * 6, F32)
    rg_small = {}
    if case.nnk > L.KNN_MAX:  # knn_oracle exports no bucket state: the same database at nnk 50 has the same buckets
        twin = Case(case.name, case.keys, case.ts, case.seeds, case.q, epochs=case._epochs, elapse=case.elapse)
        T = Oracle(twin, oracle)
    for j in np.argsort(ep, kind="stable"):
        assert ep[j] >= O.at or case.late_q is not None, "epochs only grow while the oracle is built"
        O.advance(int(ep[j]))
        k1, c1 = O.query(qd[j], int(j))
        knn[j, :, :, :k1.shape[-1]], cnt[j] = k1[..., :stride], c1
        if case.nnk > L.KNN_MAX:
            T.advance(int(ep[j]))
            rg = T.ranges()
        else:
            rg = O.ranges()
        facts[j] = [[None] * NPIV for _ in range(3)]
        for ll in range(3):
            if case.r2 and case.late_q is None and ll < len(case.qlv):
                assert np.array_equal(rg[ll], trivial), "%s: R2's activation epochs hold for a layer of one bucket" % case.name
            for s in range(NPIV):
                F = restate(case, layers, rg[ll], case.q[j, ll, s], int(ep[j]), ll, assume_active=case.late_q is not None)
                facts[j][ll][s] = F
                if case.r2:
                    what = "R1 against R2, %s q%d l%d s%d" % (case.name, j, ll, s)
                    lev = case.qlv[ll] if ll < len(case.qlv) else 0
                    hold(what, knn[j, ll, s], int(cnt[j, ll, s]), as_hits(L, F, lev), len(F.ids), F, lev, case.nnk)
                    assert case.ties or F.ntie == 0, "%s: a tie run in a case that names none" % what
    O.close()
    if case.edge is not None:
        case.edge(facts)
    if case.edge_r1 is not None:
        case.edge_r1(cnt)
    _R[case.name] = (knn, cnt, facts)
    return _R[case.name]


def check(back, case, oracle, log):
    """a case on a back end, every mode: every search of every query against R1 (and R2 for a cut run)"""
    knn1, cnt1, facts = references(case, oracle)
    for mode in case.modes:
        knn, cnt, ran = back.run(case, mode)
        want = 1 if mode == 2 else 0
        assert ran[want] > 0 and ran[1 - want] == 0 and ran[2] == 0, "%s: mode %d ran chunks %s" % (case.name, mode, list(ran))
        for j in range(len(case.q)):
            for ll in range(3):
                for s in range(NPIV):
                    lev = case.qlv[ll] if ll < len(case.qlv) else 0
                    hold("dev against R1, %s mode %d q%d l%d s%d" % (case.name, mode, j, ll, s), knn[j, ll, s], int(cnt[j, ll, s]),
                         knn1[j, ll, s], int(cnt1[j, ll, s]), facts[j][ll][s] if case.r2 else None, lev, case.nnk)
        log.append("%-74s mode %d  %5d searches  %6d hits" % (case.name, mode, cnt.size, int(cnt.sum())))


# ---------------------------------------------------------------------------------------------------------------------
# builders
def pack(layers):
    """three arrays [n_l, 10] -> scans [n, 3, 6, 10], six keys per scan and layer in order"""
    n = max(1, max((len(k) + NPIV - 1) // NPIV for k in layers))
    out = np.zeros((n, 3, NPIV, DIM), F32)
    for ll, k in enumerate(layers):
        k = np.asarray(k, F32).reshape(-1, DIM)
        lay = np.zeros((n * NPIV, DIM), F32)
        lay[:len(k)] = k
        out[:, ll] = lay.reshape(n, NPIV, DIM)
    return out


def flat(layers):
    """(keys, ts, seeds) of a database whose layers are ONE bucket each with every key in its tree: the scans arrive at t = 0
    with seeds that never rebuild bucket 0, a closing scan without keys at BIG_TS pops them all into an empty tree (no split:
    both trees are empty when the rebuild looks)"""
    keys = pack(layers)
    keys = np.concatenate([keys, np.zeros((1,) + keys.shape[1:], F32)])
    n = len(keys)
    return keys, np.concatenate([np.zeros(n - 1), [BIG_TS]]), np.concatenate([np.ones(n - 1, np.int32), [0]])


def cloud(rng, n, k0, spread=0.3, centre=8.0):
    """n keys: key[0] as given, the other nine near `centre`"""
    k = (centre + rng.normal(0, spread, (n, DIM))).astype(F32)
    k[:, 0] = k0
    return k


def probe(k0, centre=8.0):
    k = np.full(DIM, centre, F32)
    k[0] = k0
    return k


def geo_bucket(q0):
    """the geometric bucket (ratio 1.04) of cc_k_knn_order's sort key: searches of one bucket are cut into groups of 16 in key[0] order"""
    return int(np.floor(np.log2(max(F32(q0), F32(1e-3))) * F32(17.673)))


def each(facts, f):
    for j, fq in enumerate(facts):
        for ll in range(3):
            for s in range(NPIV):
                if fq[ll][s].valid:
                    f(j, ll, s, fq[ll][s])


# ---------------------------------------------------------------------------------------------------------------------
# the cases
def _nine_ary(nnk):
    """A2: layers whose keys share one key[0]; targets below, above and equal (the lower bound is strict)"""
    out = []
    sizes = [(1, 2, 8), (9, 10, 63), (64, 65, 81), (82, 728, 729), (730, 1, 2)]
    for sz in sizes:
        rng = np.random.default_rng(sum(sz))
        keys, ts, seeds = flat([cloud(rng, n, 10.0) for n in sz])
        q = pack([np.stack([probe(9.5), probe(10.5), probe(10.0)])] * 3)

        def edge(facts, sz=sz):
            for ll in range(3):
                below, above, equal = facts[0][ll][0], facts[0][ll][1], facts[0][ll][2]
                assert (below.n_above, below.n_below) == (sz[ll], 0) and (above.n_above, above.n_below) == (0, sz[ll])
                assert (equal.n_above, equal.n_below) == (sz[ll], 0)   # lb(k[0]) counts the keys strictly below
                assert all(f.in_ub == sz[ll] for f in (below, above, equal))
        out.append(Case("A2 9-ary, layers of %d/%d/%d equal key[0], target below|above|equal, nnk %d" % (sz + (nnk,)), keys, ts, seeds, q,
                        nnk=nnk, edge=edge))
    # the last probe: layers of 9, 81 and 729 DISTINCT key[0] (full 9-ary trees), the anchor on the last key, the one before it and the
    # first, and below and above all keys -- in the tiled search those two are groups of one whose p0 is 0 and n
    sz = (9, 81, 729)
    rng = np.random.default_rng(99)
    keys, ts, seeds = flat([cloud(rng, n, rng.permutation(10.0 + 0.01 * np.arange(n)), spread=0.001) for n in sz])
    q = pack([np.stack([probe(F32(10.0 + 0.01 * (n - 1))), probe(F32(10.0 + 0.01 * (n - 2))), probe(10.0), probe(9.0), probe(18.0)]) for n in sz])

    def edge_last(facts):
        for ll in range(3):
            f = facts[0][ll]
            assert [(f[s].n_above, f[s].n_below) for s in range(5)] == [(1, sz[ll] - 1), (2, sz[ll] - 2), (sz[ll], 0), (sz[ll], 0), (0, sz[ll])]
            assert f[0].K0[f[0].ids[0]] == f[0].K0.max() and f[2].K0[f[2].ids[0]] == F32(10.0), "the anchor's own key is the nearest hit"
            assert len(f[3].ids) > 0 and (len(f[4].ids) > 0 or ll < 2)
            gb = [geo_bucket(f[s].q0) for s in range(5)]
            assert gb[3] not in gb[:3] + gb[4:] and gb[4] not in gb[:4], "below-all and above-all are groups of one in the tiled search: p0 = 0 and p0 = n"
    out.append(Case("A2 9-ary last probe, layers of 9/81/729 distinct key[0], anchor on the last | last but one | first key, below all (p0 = 0), above all (p0 = n), nnk %d" % nnk,
                    keys, ts, seeds, q, nnk=nnk, edge=edge_last))
    return out


def _steps(nnk):
    """A3 on one bucket: (visible keys above the anchor, below it); the anchor at sorted position 0 and n"""
    out = []
    for trio in [((0, 1), (1, 0), (63, 64)), ((64, 65), (65, 63), (128, 0)), ((0, 128), (128, 128), (64, 64)), ((1, 1), (1, 9), (1, 80))]:
        rng = np.random.default_rng(7)
        layers, qs = [], []
        for up, dn in trio:
            n = up + dn
            k0 = np.concatenate([20.0 + 0.01 * np.arange(1, dn + 1)[::-1] * -1, 20.0 + 0.01 * np.arange(up)]).astype(F32)
            layers.append(cloud(rng, n, rng.permutation(k0), spread=1.2))
            qs.append(probe(20.0)[None])
        keys, ts, seeds = flat(layers)

        def edge(facts, trio=trio):
            for ll in range(3):
                F = facts[0][ll][0]
                assert (F.n_above, F.n_below) == trio[ll], (F.n_above, F.n_below)
        out.append(Case("A3 steps, visible above/below the anchor %s, nnk %d" % (" ".join("%d/%d" % t for t in trio), nnk), keys, ts, seeds,
                        pack(qs), nnk=nnk, edge=edge))
    return out


def _shell(n, q, r2):
    """n keys at squared f32 distance exactly r2 (a power of four times small integers) from q: +-sqrt(r2) along one axis"""
    k = np.tile(q, (n, 1)).astype(F32)
    ax = 1 + np.arange(n) % 9
    sg = np.where((np.arange(n) // 9) % 2 == 0, 1.0, -1.0)
    k[np.arange(n), ax] += (sg * np.sqrt(r2)).astype(F32)
    return k


def _radius(nnk):
    """A4: q = (8, 0, 0, 8, 0, ...) has dist_ub = 4.0 exactly; keys AT 4.0 are out, one float below is in; the counts around the
    first tightening; ties at the nnk-th distance on both sides of the holder's id"""
    q = np.zeros(DIM, F32)
    q[0] = 8.0               # k[1] = k[2] = 0: only the first term of dist_ub is not zero, (8 - 10)^2
    below2 = np.nextafter(F32(2.0), F32(0))   # (2 - 2^-23)^2 = 4 - 2^-21 in f32; + (2^-11)^2 = 4 - 2^-22, the float below 4.0

    def at(d, n, axis=3):
        k = np.tile(q, (n, 1))
        k[:, axis] += F32(d)
        return k

    out = []
    for cntc in sorted({c for c in (nnk - 2, nnk - 1, nnk, 2 * nnk - 2, 2 * nnk - 1) if c >= 0}):
        near = at(0.0, cntc)
        near[:, 4] = (0.001 * (1 + np.arange(cntc))).astype(F32)   # distinct distances, all far inside
        just = at(below2, 1)
        just[:, 4] = F32(2.0 ** -11)
        lay = np.concatenate([near, at(2.0, 3), just, at(-2.0, 2, axis=0)])
        keys, ts, seeds = flat([lay, lay[::-1].copy(), lay[:0]])

        def edge(facts, cntc=cntc):
            for ll in (0, 1):
                F = facts[0][ll][0]
                assert F.ub == F32(4.0) and (F.r == F32(4.0)).sum() == 5 and F.in_ub == cntc + 1
                assert (F.r < F32(4.0)).sum() == cntc + 1 and F.r[F.r < 4.0].max() == np.nextafter(F32(4.0), F32(0))
        out.append(Case("A4 radius, dist_ub 4.0 exact: 5 keys at it are out, the float below is in, %d+1 inside, nnk %d" % (cntc, nnk), keys, ts,
                        seeds, pack([q[None], q[None], q[None]]), nnk=nnk, edge=edge))
    # ties at the nnk-th distance: nnk - 1 closer keys, then a crowd at one distance whose ids surround the others'
    for crowd, label in ((2, "two keys"), (5, "five keys"), (70, "70 keys")):
        closer = at(0.0, nnk - 1)
        closer[:, 4] = (0.001 * (1 + np.arange(nnk - 1))).astype(F32)
        tie = _shell(crowd, q, 1.0)
        far = at(1.5, 4)
        la = np.concatenate([tie[:crowd // 2], closer, far, tie[crowd // 2:]])     # tied keys before and after the rest in id
        lb = np.concatenate([far, tie, closer])
        # the same crowd far from any cut: an uncut run
        lc = tie[:min(crowd, nnk)]
        keys, ts, seeds = flat([la, lb, lc])

        def edge(facts, crowd=crowd):
            for ll in (0, 1):
                F = facts[0][ll][0]
                assert F.cut == crowd - 1 and F.dist[-1] == F32(1.0) and len(F.ids) == nnk
            assert facts[0][2][0].cut == 0 and (facts[0][2][0].ntie > 0 or nnk == 1)
        out.append(Case("A4 tie across the nnk-th place, %s at the nnk-th distance, ids below and above the holder, nnk %d" % (label, nnk),
                        keys, ts, seeds, pack([q[None], q[None], q[None]]), nnk=nnk, edge=edge, ties=True))
    # after the tightening: keys AT the nnk-th distance with lower ids than the holders, found in the second step, behind a first step
    # whose outermost key lies at (key[0] - q[0])^2 = the radius
    if 3 <= nnk <= 64:
        # sorted view: 575 keys at key[0] = 8 -- nnk - 3 closer ones, 66 - nnk at distance 1.0 (the holders), 512 far ones --, then at
        # key[0] = 9 a block of 193 far keys G and the three keys T at distance 1.0.  The walk tightens after its first step and meets
        # G's first key as the outermost key of its ninth (575 = 8 * 64 + 63).  The tiled search takes 512 keys upwards per round and
        # has its first pass once 64 pairs are queued: the 65 keys inside dist_ub among the first 512 are filed and cut back to the
        # nnk-th distance 1.0 after the first round (for nnk <= 50: 63 > nnk + 12 keys lie within 1.0, so the bisection ends on 1.0
        # itself); G's first key ends the first step of a wave's second round and T lies in that wave's next step (768).
        t0 = at(1.0, 3, axis=0)
        block = at(1.0, 193, axis=0)
        block[:, 5] = 10.0
        closer = at(0.0, nnk - 3)
        closer[:, 4] = (0.001 * (1 + np.arange(nnk - 3))).astype(F32)
        others = _shell(66 - nnk, q, 1.0)
        inside = at(0.0, 2)
        inside[:, 6] = [1.5, 1.75]                                # two more inside dist_ub: 65 pairs pass the filter in the first round
        far8 = at(0.0, 510)
        far8[:, 5] = 10.0
        lay = np.concatenate([block, t0, closer, others, inside, far8])           # T's ids are lower than the holders'
        lay_hi = np.concatenate([block, closer, others, inside, far8, t0])        # ... and higher
        keys, ts, seeds = flat([lay, lay_hi, lay])

        def edge_post(facts, lay=lay):
            for ll in (0, 1, 2):
                F = facts[0][ll][0]
                assert (lay[:, 0] == 8).sum() == 575 and F.n_above == 771 and F.n_below == 0 and F.dist[-1] == F32(1.0) and F.cut == 66 - nnk
                assert F.in_ub == 68 and (F.r[F.K0 == 8] < F.ub).sum() == 65
            assert set(facts[0][0][0].ids[-3:].tolist()) == {193, 194, 195}       # T pushes two holders out
            assert len(set(facts[0][1][0].ids.tolist()) & {768, 769, 770}) == max(0, 3 - (66 - nnk))   # the same keys with higher ids push nobody out
        out.append(Case("A4 after the tightening: keys at the nnk-th distance found late, behind a step whose outermost key is at the radius, ids lower | higher than the holders, nnk %d" % nnk,
                        keys, ts, seeds, pack([q[None]] * 3), nnk=nnk, edge=edge_post, ties=True))
    # a step's outermost key with (key[0] - q[0])^2 equal to the radius: 64 keys per direction, the 64th at key[0] = q[0] +- 2
    down = 8.0 - 2.0 * (np.arange(1, 65) - 0.5) / 64.0     # no two keys at one distance but the two outermost
    down[-1] = 6.0
    k0 = np.concatenate([8.0 + 2.0 * np.arange(1, 65) / 64.0, down, [10.5, 5.5, 11.0, 5.0]]).astype(F32)
    lay = np.tile(q, (len(k0), 1))
    lay[:, 0] = k0
    keys, ts, seeds = flat([lay, lay[::-1].copy(), lay])

    def edge(facts):
        F = facts[0][0][0]
        assert (F.n_above, F.n_below) == (66, 66) and F.in_ub == 126 and (F.r == F32(4.0)).sum() == 2
    out.append(Case("A4 a step's outermost key at (key[0] - q[0])^2 = dist_ub, nnk %d" % nnk, keys, ts, seeds, pack([q[None]] * 3), nnk=nnk,
                    edge=edge))
    return out


def _epochs_cases():
    """A5: keys that enter the tree later than a query's epoch, mixed epochs in one chunk, keys still in buffers"""
    rng = np.random.default_rng(3)
    n = 14
    keys = np.zeros((n, 3, NPIV, DIM), F32)
    for ll in range(3):
        keys[:, ll] = cloud(rng, n * NPIV, 20.0 + rng.normal(0, 1.0, n * NPIV), spread=1.0).reshape(n, NPIV, DIM)
    ts = np.arange(n) * 10.0              # min 15 / max 25: scan i's rebuild pops the scans up to i - 2 once scan i - 3's waits
    seeds = np.zeros(n, np.int32)
    seeds[5] = 1                          # a scan that rebuilds another bucket pair: its turn is skipped
    q = np.tile(probe(20.0), (n, 3, NPIV, 1)).astype(F32)
    q += rng.normal(0, 0.3, q.shape).astype(F32)
    ep = np.arange(1, n + 1)

    def edge(facts):
        seen = set()
        for j in range(n):
            F = facts[j][0][0]
            seen.add(int(F.act.sum()))
            assert F.act.sum() < len(F.act), "some key is still in a buffer at every epoch"
        assert len(seen) >= 4 and 0 in seen, seen   # the chunk's queries see at least four different trees, one of them empty
    out = [Case("A5 epochs 1..14 in one chunk, keys in buffers (elapse 15/25, scans 10 s apart)", keys, ts, seeds, q, epochs=ep, nnk=50,
                edge=edge)]
    out.append(Case("A5 short elapse 0.5/1.0, scans 0.3 s apart, epochs mixed", keys, np.arange(n) * 0.3, np.zeros(n, np.int32), q,
                    epochs=ep, nnk=50, elapse=(0.5, 1.0), edge=edge))
    return out


def _fixture():
    """A5, the VIS instance: tests/golden/knn_unindexed_bucket_fixture.npz, the keys of a 78-scan drive with short delays in which a
    bucket holds keys its tree does not index; every scan queries at its own epoch.  R2 has no model of the indexed intervals:
    the lists are held to R1 alone, and R1 states the edge (a search with 0 hits beside 50-hit neighbours)."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_unindexed_bucket_fixture.npz"))
    cfg = z["cfg"]
    qlv = tuple(int(v) for v in cfg[5:5 + int(cfg[4])])
    keys = np.stack([z["keys"][:, lev] for lev in qlv], axis=1)
    n = len(keys)
    c = Case("A5 VIS: a bucket whose tree does not index its keys (78-scan fixture, every scan at its own epoch)", keys, z["ts"], z["seeds"], keys,
             epochs=np.arange(n), nnk=int(cfg[2]), qlv=qlv, elapse=(float(cfg[0]), float(cfg[1])), r2=False)
    want = z["knn_cnt"]

    def edge_r1(cnt):
        assert np.array_equal(cnt, want), "the oracle's counts are the fixture's"
        assert cnt[65, 0, 0] == 0 and cnt[64, 0].sum() > 50
    c.edge_r1 = edge_r1
    return [c]


def _gaps():
    """B3: searches at the top of bucket mid = 1 and 2 of a larger bucketed database: the common walk upwards meets >= 64, >= 256 and
    >= 513 keys of skipped buckets at once (the jump, kk >= 1 and kk >= 2); groups whose searches have different mid"""
    keys, ts, seeds = _bucketed(n_bulk=250)

    def late_q(rg, sorted0, layers):
        qs = []
        for ll in range(3):
            k0 = []
            for mid in (1, 2):
                top = np.nextafter(F32(rg[ll][mid + 1]), F32(-np.inf))
                k0 += [top - 0.002 * i for i in range(17)] + [rg[ll][mid + 1] + 0.001, rg[ll][mid + 1]]    # ... and two just above: another mid
            qs.append(np.stack([probe(v, centre=10.0) for v in k0]))
        return pack(qs)

    def edge(facts):
        gaps, mids = set(), set()
        each(facts, lambda j, ll, s, F: (gaps.add(F.gap), mids.add(F.mid)))
        assert min(g for g in gaps if g) >= 64 and any(256 <= g < 513 for g in gaps) and any(g >= 513 for g in gaps), sorted(gaps)
        assert mids == {1, 2, 3}
    return [Case("B3 gaps of >= 64, >= 256 and >= 513 skipped-bucket keys right above a group of searches, groups with two mid", keys, ts, seeds, None,
                 edge=edge, late_q=late_q)]


def _gaps_down():
    """B3, downwards: six buckets inside ONE geometric bucket of the order key (key[0] in 19.75 .. 20.45), so a group of 16 holds
    searches of different mid.  Three searches A sit in bucket 1 (mid 1: bucket 2 is skipped), thirteen searches B are exact copies
    of keys near the top of bucket 3 (mid 3: bucket 2 is visible); the middle search is a B, so the common walk starts in bucket 3.
    nnk is 1: after the first pass every B holds its copy at distance 0 and leaves; the walk downwards then serves A alone, which has
    >= 512 keys of bucket 3 below p0 and then all of bucket 2 (>= 513 keys) to jump over.  A copies the other nine entries of the
    LAST key of bucket 1, the first key behind the jump: it is A's hit."""
    keys, ts, seeds = _bucketed(n_bulk=700, lo=19.75, width=0.7)

    def late_q(rg, sorted0, layers):
        qs = []
        for ll in range(3):
            K = layers[ll].K
            order = np.lexsort((np.arange(len(K)), K[:, 0]))
            s0 = K[order, 0]
            e1, s3, e3 = (int(np.searchsorted(s0, rg[ll][i], side="left")) for i in (2, 3, 4))
            lay = []
            for i in range(3):                       # A: anchors a few keys below the top of bucket 1
                k = K[order[e1 - 1]].copy()
                k[0] = s0[e1 - 3 - 2 * i] + F32(1e-6)
                lay.append(k)
            lay += [K[order[e3 - 2 - 3 * i]].copy() for i in range(13)]     # B: copies of keys at the top of bucket 3
            qs.append(np.stack(lay))
        return pack(qs)

    def edge(facts):
        for ll in range(3):
            f = [facts[j][ll][s] for j in range(3) for s in range(NPIV)][:16]
            assert [x.mid for x in f] == [1] * 3 + [3] * 13
            for a in f[:3]:
                top1 = int(np.argmax(np.where(a.bk == 1, a.K0, -np.inf)))
                assert a.gap >= 513 and len(a.ids) == 1 and a.ids[0] == top1, "A's hit is the last key of bucket 1, behind the jump"
            for b in f[3:]:
                assert b.dist[0] == 0 and ((b.bk == 3) & (b.K0 < b.K0[b.ids[0]])).sum() >= 512, "B finds its copy; >= 512 keys of bucket 3 below it"
            lo_, hi_ = min(x.K0[x.ids[0]] for x in f), max(x.K0[x.ids[0]] for x in f)
            assert int(np.floor(np.log2(lo_) * 17.673)) == int(np.floor(np.log2(hi_) * 17.673)), "one geometric bucket: one group of 16"
    return [Case("B3 downwards: a gap of >= 513 skipped-bucket keys below a group whose mid 3 searches have left and whose mid 1 searches go on (the jump, kk >= 2)",
                 keys, ts, seeds, None, nnk=1, edge=edge, late_q=late_q, modes=(2, 0))]


def _no_search():
    """A6: searches that must write a zero count over what the lane's buffers held before"""
    rng = np.random.default_rng(9)
    lay = cloud(rng, 90, 20.0 + rng.normal(0, 1.0, 90), spread=1.0)
    cancel = np.array([20, -20, 8, -8, 4, -4, 2, -2, 1, -1], F32)       # entries that cancel to an exact zero sum
    lay = np.concatenate([lay, (cancel + rng.normal(0, 0.3, (60, DIM))).astype(F32)])   # ... with 60 keys around it, inside its dist_ub
    keys, ts, seeds = flat([lay, lay[:0], lay])        # layer 1 is empty
    q = np.tile(probe(20.0), (3, 3, NPIV, 1)).astype(F32)
    q[0, :, 1] = 0                                     # an all-zero key
    q[0, :, 2] = cancel
    q[1, :, ::2] = 0                                   # invalid searches interleaved with valid ones

    def edge(facts):
        assert not facts[0][0][1].valid and not facts[0][0][2].valid and facts[0][0][0].valid
        Lr = Layer(facts_case[0], 0)
        assert ((dist_f32(cancel, Lr.K) < dist_ub(cancel)).sum()) == 60, "a search with the cancelling key would find 60 keys"
        assert all(len(facts[j][1][s].ids) == 0 for j in range(3) for s in range(NPIV))
        assert len(facts[2][0][0].ids) == 50
    out, facts_case = [], []
    for qlv in ((1, 2, 3), (1, 2), (1,)):
        out.append(Case("A6 no search: zero key, cancelling key, empty layer, n_q_levels %d, after a full chunk on the lane" % len(qlv), keys, ts,
                        seeds, q, qlv=qlv, edge=edge if len(qlv) == 3 else None, prelude=True))
    facts_case.append(out[0])
    return out


def _bucketed(n_bulk=120, kicks=48, lo=18.0, width=4.0):
    """(keys, ts, seeds) of a database that splits into six buckets per layer: a bulk at t = 0, then scans 100 s apart whose six
    keys per layer spread over the key[0] range and whose seeds visit every bucket pair -- every visited bucket has something to
    pop, so its tree is rebuilt -- and a last cycle of scans without keys that empties the buffers"""
    rng = np.random.default_rng(17)
    n = n_bulk + kicks + 8
    keys = np.zeros((n, 3, NPIV, DIM), F32)
    for ll in range(3):
        k = cloud(rng, (n_bulk + kicks) * NPIV, 0.0, spread=3.0, centre=10.0)
        k[:, 0] = rng.permutation(lo + width * (np.arange(len(k)) + 0.5) / len(k))   # distinct key[0]; buckets narrower than the nnk-th distance
        k = k.reshape(n_bulk + kicks, NPIV, DIM)
        k[n_bulk:, :, 0] = (lo + width * (np.array([0.0, 0.2, 0.4, 0.6, 0.8, 0.875]) + rng.uniform(0, 0.125, (kicks, NPIV)))).astype(F32)
        keys[:n_bulk + kicks, ll] = k
    ts = np.concatenate([np.zeros(n_bulk), 100.0 * (1 + np.arange(kicks + 8))])
    seeds = np.concatenate([np.ones(n_bulk, np.int32), np.arange(kicks + 8, dtype=np.int32)])
    return keys, ts, seeds


def _bucket_rule(nnk):
    """A1: a query key[0] exactly on rg[i], one float below it, below rg[0] and at rg[6]; the other nine entries sit in the
    cloud's centre, so every bucket holds keys closer than the nnk-th hit"""
    keys, ts, seeds = _bucketed()

    def late_q(rg, sorted0, layers):
        qs = []
        for ll in range(3):
            k0 = []
            for i in range(1, 6):
                k0 += [rg[ll][i], np.nextafter(F32(rg[ll][i]), F32(-np.inf))]
            k0 += [-1000.5, 1000.0, 0.5 * (rg[ll][2] + rg[ll][3]), 0.5 * (rg[ll][5] + 22.0)]   # below rg[0], at rg[6]: mid stays 0
            qs.append(np.stack([probe(v, centre=10.0) for v in k0]))
        return pack(qs)

    def edge(facts):
        mids = set()
        for ll in range(3):
            got = [facts[j][ll][s] for j in range(len(facts)) for s in range(NPIV) if facts[j][ll][s].valid]
            assert [f.mid for f in got[:10]] == [1, 0, 2, 1, 3, 2, 4, 3, 5, 4], [f.mid for f in got[:10]]
            assert got[10].mid == 0 and got[11].mid == 0
            for f in got:
                assert np.bincount(f.bk[f.bk >= 0], minlength=6).min() > 0, "six buckets hold keys"
                mids.add(f.mid)
            # mid = 1..4, on rg[mid] and one float below rg[mid + 1]: the buckets above are skipped and hold keys inside the nnk-th distance
            closer = [f.gap > 0 and len(f.ids) == nnk and f.skipped_best < f.dist[-1] for f in got[:10] if 1 <= f.mid <= 4]
            assert len(closer) == 8
            on, below = closer[0::2], closer[1::2]
            assert (sum(below) >= 3 and sum(on) >= 2) if nnk >= 50 else any(closer), "a closer key sits in a skipped bucket: %s" % closer
        assert mids == set(range(6))
    return [Case("A1 bucket rule, key[0] on rg[1..5] and one float below, below rg[0], at rg[6]; closer keys in the skipped buckets, nnk %d" % nnk,
                 keys, ts, seeds, None, nnk=nnk, edge=edge, late_q=late_q)]


def _range_ends(nnk):
    """A3 on six buckets: the first visible range holds exactly 64 (a step boundary) or 40 (mid-step) keys from the anchor up and the
    run goes on in the second range, with (mid 1, 2) and without (mid 0) skipped buckets between them.  The search key copies the other
    nine entries of the FIRST key of the second range (the key at S2), so that key is the nearest hit of the search.  (Downwards the
    walk enters two ranges only for k[0] >= rg[6], where mid = 0 and the ranges touch: there is no second range end to place.)"""
    keys, ts, seeds = _bucketed()

    def late_q(rg, sorted0, layers):
        qs = []
        for ll in range(3):
            K = layers[ll].K
            order = np.lexsort((np.arange(len(K)), K[:, 0]))
            s0, lay = K[order, 0], []
            for mid in (0, 1, 2):
                e1 = int(np.searchsorted(s0, rg[ll][mid + 1], side="left"))        # keys below the end of bucket mid
                s2 = int(np.searchsorted(s0, rg[ll][2 * mid + 1], side="left"))    # the first key of the second range
                for back in (64, 40):
                    k = K[order[s2]].copy()
                    k[0] = s0[e1 - back]          # distinct key[0]: exactly `back` keys of the first range are not below the anchor
                    lay.append(k)
            qs.append(np.stack(lay))
        return pack(qs)

    def edge(facts):
        for ll in range(3):
            got = [facts[0][ll][s] for s in range(NPIV)]
            assert [f.mid for f in got] == [0, 0, 1, 1, 2, 2] and [f.up_a for f in got] == [64, 40, 64, 40, 64, 40], [f.up_a for f in got]
            assert got[0].gap == 0 and got[2].gap >= 64 and got[4].gap >= 256, [f.gap for f in got]
            for f in got:
                k0 = np.where(f.bk == 2 * f.mid + 1, f.K0, np.inf)
                first = int(np.argmin(k0))                      # the key at S2 (distinct key[0])
                assert f.up_b > 0 and len(f.ids) and f.ids[0] == first, "the key at S2 is the search's nearest hit"
    return [Case("A3 the first visible range holds exactly 64 / 40 keys from the anchor up, the nearest hit is the first key of the second range, mid 0..2, nnk %d" % nnk,
                 keys, ts, seeds, None, nnk=nnk, edge=edge, late_q=late_q)]


def _groups():
    """B1/B2: how cc_k_knn_order groups a layer's searches -- 1, 15, 16, 17 and 33 valid searches of one key[0]; searches 4 % apart;
    key[0] <= 1e-3; the sort widths at 170/171 and 682/683 queries.  All on a small layer."""
    rng = np.random.default_rng(23)
    lay = [cloud(rng, 60, 10.0 + rng.normal(0, 0.5, 60), spread=0.5) for _ in range(3)]
    tiny = cloud(rng, 12, 0.0, spread=0.0002, centre=0.002)
    tiny[:, 0] = (rng.uniform(1e-4, 2e-3, 12)).astype(F32)
    keys, ts, seeds = flat([np.concatenate([lay[0], tiny]), lay[1], lay[2]])
    out = []
    for nv in (1, 15, 16, 17, 33):
        nq = (nv + NPIV - 1) // NPIV + 1
        q = np.zeros((nq, 3, NPIV, DIM), F32)
        for ll in range(3):
            flatq = np.zeros((nq * NPIV, DIM), F32)
            pos = np.arange(nv) * 2 if 2 * nv <= len(flatq) else np.arange(nv)   # invalid searches interleaved where there is room
            flatq[pos] = probe(10.0) + rng.normal(0, 0.2, (nv, DIM)).astype(F32)
            flatq[pos, 0] = 10.0
            q[:, ll] = flatq.reshape(nq, NPIV, DIM)
        q2 = np.zeros((2 * nq, 3, NPIV, DIM), F32)
        q2[::2] = q
        out.append(Case("B1 groups, %d valid searches of one key[0] per layer, invalid ones between them" % nv, keys, ts, seeds, q2, modes=(2,),
                        edge=lambda facts, nv=nv: _count_valid(facts, nv)))
    q = np.zeros((4, 3, NPIV, DIM), F32)
    q[:] = probe(10.0)
    q[:, :, :, 0] = (7.0 * 1.04 ** np.arange(24)).reshape(4, 1, NPIV).astype(F32)     # one search per geometric bucket
    q[3, 0, :, :] = 0.002
    q[3, 0, :, 0] = [1e-3, 9e-4, 1e-4, 1e-5, 1.0000001e-3, 2e-3]                    # the clamped log
    out.append(Case("B1 groups, searches 4 % apart (one per geometric bucket) and key[0] <= 1e-3 (the clamped log)", keys, ts, seeds, q,
                    modes=(2,), edge=_apart))
    keys2, ts2, seeds2 = flat([l[:20] for l in lay])   # the width depends on the query count only
    for nq in (170, 171, 682, 683):
        q = np.tile(probe(10.0), (nq, 3, NPIV, 1)).astype(F32)
        q += rng.normal(0, 0.3, q.shape).astype(F32)
        q[rng.uniform(size=(nq, 3, NPIV)) < 0.1] = 0
        _untie(keys2, q)
        out.append(Case("B2 sort widths, %d queries: %d searches per layer" % (nq, nq * NPIV), keys2, ts2, seeds2, q, modes=(2,)))
    return out


def _untie(keys, q):
    """nudge the search keys that have two of a (small) layer's keys at one f32 distance: no chance ties"""
    for ll in range(3):
        K = keys[:, ll].reshape(-1, DIM)
        K = K[np.abs(K).sum(1) != 0]
        Q = q[:, ll].reshape(-1, DIM)
        for _ in range(8):
            d = np.sort(np.stack([dist_f32(k, Q) for k in K], axis=1), axis=1)
            bad = np.nonzero((np.diff(d, axis=1) == 0).any(axis=1) & (np.abs(Q).sum(1) != 0))[0]
            if not len(bad):
                break
            Q[bad, 5] += F32(0.01)
        q[:, ll] = Q.reshape(q[:, ll].shape)


def _apart(facts):
    _some_hits(facts, 3, 0)
    for ll in (1, 2):     # 24 searches 4 % apart: no geometric bucket holds more than two, so no group does
        gb = [geo_bucket(facts[j][ll][s].q0) for j in range(4) for s in range(NPIV)]
        assert len(set(gb)) >= 20 and max(gb.count(b) for b in gb) <= 2, gb
    assert len({geo_bucket(facts[3][0][s].q0) for s in range(NPIV)}) == 2   # key[0] <= 1e-3 all fall in the clamp's bucket, 2e-3 in another


def _count_valid(facts, nv):
    for ll in range(3):
        assert sum(facts[j][ll][s].valid for j in range(len(facts)) for s in range(NPIV)) == nv


def _some_hits(facts, j, ll):
    assert sum(len(facts[j][ll][s].ids) for s in range(NPIV)) > 0


def _queues():
    """B3/B4: layers below 64 keys; a full group over near-identical keys; a crowd of more than 64 bit-equal distances at the
    radius; nnk 64 with 128 candidates; a search that never fills; more than 128 candidates at the end"""
    rng = np.random.default_rng(31)
    out = []
    # layers of 1, 9 and 65 keys, 16 searches each
    lay = [cloud(rng, n, 10.0 + rng.normal(0, 0.5, n), spread=0.5) for n in (1, 9, 65)]
    keys, ts, seeds = flat(lay)
    q = np.tile(probe(10.0), (3, 3, NPIV, 1)).astype(F32) + rng.normal(0, 0.3, (3, 3, NPIV, DIM)).astype(F32)
    q[2, :, 4:] = 0

    def edge_small(facts):
        assert [len(facts[0][ll][0].ids) for ll in range(3)] == [1, 9, 50]
    out.append(Case("B3 layers of 1, 9 and 65 keys under a group of 16 searches (clamped loads count no key twice)", keys, ts, seeds, q,
                    edge=edge_small))
    # a full group over near-identical keys: every pair of a step passes until the first radius is set
    lay = [cloud(rng, 420, 10.0 + rng.normal(0, 0.02, 420), spread=0.02) for _ in range(3)]
    keys, ts, seeds = flat(lay)
    q = np.tile(probe(10.0), (3, 3, NPIV, 1)).astype(F32) + rng.normal(0, 0.01, (3, 3, NPIV, DIM)).astype(F32)
    q[2, :, 4:] = 0

    def edge_full(facts):
        each(facts, lambda j, ll, s, F: _assert(F.in_ub == 420, "all 420 keys of the layer are inside dist_ub: 16 x 64 pairs a step pass"))
        for ll in range(3):
            gb = [geo_bucket(facts[j][ll][s].q0) for j in range(len(facts)) for s in range(NPIV) if facts[j][ll][s].valid]
            assert len(gb) == 16 and len(set(gb)) == 1, "the layer's 16 valid searches lie in one geometric bucket: one full group"
    for nnk in (50, 64):
        out.append(Case("B4 a full group of 16 over 420 near-identical keys, every pair of a step inside dist_ub, nnk %d" % nnk, keys, ts, seeds, q,
                        nnk=nnk, edge=edge_full))
    # a crowd of bit-equal distances at the radius
    qk = np.zeros(DIM, F32)
    qk[0] = 8.0
    closer = np.tile(qk, (49, 1))
    closer[:, 4] = (0.001 * (1 + np.arange(49))).astype(F32)
    crowd = _shell(90, qk, 1.0)
    lay = np.concatenate([crowd[:40], closer, crowd[40:]])
    keys, ts, seeds = flat([lay, lay[::-1].copy(), lay])
    q = np.tile(qk, (3, 3, NPIV, 1)).astype(F32)
    q[2, :, 4:] = 0

    def edge_crowd(facts):
        each(facts, lambda j, ll, s, F: _assert(F.cut == 89 and F.dist[-1] == F32(1.0), "90 keys at the nnk-th distance"))
    out.append(Case("B4 a crowd of 90 bit-equal distances at the nnk-th place (kept > 64)", keys, ts, seeds, q, edge=edge_crowd, ties=True))
    # nnk 64 with 127, 128 and 129 candidates in a buffer: layers that lie inside dist_ub whole and inside the tiled search's first
    # round (<= 512 keys a direction), one search a layer -- the first pass files them all, the first cut-back sees that count
    lay = [cloud(rng, n, 10.0 + rng.normal(0, 0.1, n), spread=0.1) for n in (127, 128, 129)]
    keys, ts, seeds = flat(lay)
    q = np.zeros((1, 3, NPIV, DIM), F32)
    q[0, :, 0] = probe(10.0) + rng.normal(0, 0.05, (3, DIM)).astype(F32)

    def edge_128(facts):
        assert [facts[0][ll][0].in_ub for ll in range(3)] == [127, 128, 129] and [len(facts[0][ll][0].r) for ll in range(3)] == [127, 128, 129]
    out.append(Case("B4 nnk 64 with 127, 128 and 129 candidates in a buffer at the first cut-back (CC_KNN_TTRIG = 128)", keys, ts, seeds, q, nnk=64,
                    edge=edge_128))
    # never fills / more than 128 candidates at the end
    lay = [cloud(rng, 30, 10.0 + rng.normal(0, 0.1, 30), spread=0.1), cloud(rng, 200, 10.0 + rng.normal(0, 0.1, 200), spread=0.1),
           cloud(rng, 49, 10.0 + rng.normal(0, 0.1, 49), spread=0.1)]
    keys, ts, seeds = flat(lay)
    q = np.tile(probe(10.0), (3, 3, NPIV, 1)).astype(F32) + rng.normal(0, 0.05, (3, 3, NPIV, DIM)).astype(F32)
    q[2, :, 4:] = 0

    def edge_fill(facts):
        assert [facts[0][ll][0].in_ub for ll in range(3)] == [30, 200, 49]
    out.append(Case("B4 searches that never fill (30 and 49 of nnk 50) and one with 200 candidates inside dist_ub", keys, ts, seeds, q,
                    edge=edge_fill))
    return out


def _assert(c, msg):
    assert c, msg


def _large():
    """C: cc_k_knn_l -- pending counts that select each sorting network, the exact radius and the ties at nnk 256"""
    rng = np.random.default_rng(41)
    out = []
    for nnk in (65, 128, 129, 256):
        lay = [cloud(rng, n, 10.0 + rng.normal(0, 0.1, n), spread=0.1) for n in (100, 300, 700)]
        keys, ts, seeds = flat(lay)
        q = np.tile(probe(10.0), (2, 3, NPIV, 1)).astype(F32) + rng.normal(0, 0.05, (2, 3, NPIV, DIM)).astype(F32)

        def edge(facts, nnk=nnk):
            got = [facts[0][ll][0].in_ub for ll in range(3)]
            assert got == [100, 300, 700], got
        out.append(Case("C large k, 100/300/700 keys inside dist_ub (the pending counts of every sorting network), nnk %d" % nnk, keys, ts, seeds,
                        q, nnk=nnk, edge=edge))
    out += [c for c in _radius(256)]
    for c in out:
        c.name = c.name.replace("A4", "C A4")
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        c = []
        for nnk in (50, 1, 64):
            c += _bucket_rule(nnk) + _nine_ary(nnk) + _steps(nnk) + _range_ends(nnk) + _radius(nnk)
        c += _epochs_cases() + _fixture() + _no_search() + _groups() + _gaps() + _gaps_down() + _queues() + _large()
        names = [x.name for x in c]
        assert len(set(names)) == len(names)
        _CASES = c
    return _CASES


PARTS = ["A1", "A2", "A3", "A4", "A5", "A6", "B1", "B2", "B3", "B4", "C "]


def part(p):
    return [c for c in cases() if c.name.startswith(p)]


def prelude_queries():
    """a full chunk's worth of searches that all return nnk hits, for the lane a no-search case runs on next"""
    q = np.tile(probe(20.0), (4, 3, NPIV, 1)).astype(F32)
    return q


# ---------------------------------------------------------------------------------------------------------------------
# D: the sorted key view after every append (cc_k_keys_append, cc_k_ksort_new_lds | cc_k_ksort_new, cc_k_ksort_merge, cc_k_ksort_act)
def raw_view(lib, db, layer):
    """cc_db_debug_key_view -> (keys [11, n], sid [n], sact [n])"""
    import ctypes as C
    n = C.c_int32()
    z, zf = np.zeros(1, np.int32), np.zeros(11, F32)
    rc = lib.cc_db_debug_key_view(db, layer, 0, zf.ctypes.data, z.ctypes.data, z.ctypes.data, C.byref(n))
    assert rc == (0 if n.value == 0 else -4), (rc, n.value)     # CC_ECAPACITY names the size
    cap = max(n.value, 1)
    keys, sid, sact = np.zeros((DIM + 1, cap), F32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    assert lib.cc_db_debug_key_view(db, layer, cap, keys.ctypes.data, sid.ctypes.data, sact.ctypes.data, C.byref(n)) == 0
    return keys[:, :n.value], sid[:n.value], sact[:n.value]


def hold_view(what, view, Lr, p):
    """the view of a layer after the append that brought the database to p scans, against the layer's keys in id order"""
    keys, sid, sact = view
    m = Lr.scan < p
    K, act = Lr.K[m], Lr.act[m]
    assert len(sid) == len(K), "%s: %d keys in the view, %d stored" % (what, len(sid), len(K))
    if not len(K):
        return
    want = np.lexsort((np.arange(len(K)), K[:, 0] + F32(0)))     # stable by key[0] with -0 folded onto +0, then by id
    assert np.array_equal(sid, want), "%s: order, first difference at %d" % (what, int(np.argmax(sid != want)))
    assert np.array_equal(keys[:DIM].T.view(np.uint32), np.ascontiguousarray(K[sid]).view(np.uint32)), "%s: key bits" % what
    exact = (K[sid].astype(np.float64) ** 2).sum(1)               # products of two f32 are exact in f64
    err = np.abs(keys[DIM].astype(np.float64) - exact)
    assert (err <= 10 * 2.0 ** -24 * exact).all(), "%s: |k|^2 off by %g relative" % (what, float((err / exact).max()))
    for e in range(1, p + 1):   # the epochs a query can have: the same keys sit in a tree
        assert np.array_equal(sact <= e, act[sid] <= e), "%s: activation at epoch %d" % (what, e)


def check_views(back, case, oracle, log):
    """a database built in the case's pieces: the view after every append, the hit lists of the queries at that epoch against R1,
    and the last view and lists against a database built in a single append"""
    knn1, cnt1, facts = references(case, oracle)
    layers = [Layer(case, ll) for ll in range(3)]
    ep = case.epochs
    single = back.pieces(case, [case.n])[-1]
    got = back.pieces(case, case.pieces)
    for p, (views, sel, knn, cnt) in zip(case.pieces, got):
        for ll, v in enumerate(views):
            hold_view("%s, %d scans, layer %d" % (case.name, p, ll), v, layers[ll], p)
        for i, j in enumerate(sel):
            for ll in range(3):
                for s in range(NPIV):
                    hold("dev against R1, %s epoch %d q%d l%d s%d" % (case.name, p, j, ll, s), knn[i, ll, s], int(cnt[i, ll, s]), knn1[j, ll, s],
                         int(cnt1[j, ll, s]), facts[j][ll][s], case.qlv[ll], case.nnk)
    views, sel, knn, cnt = got[-1]
    for ll in range(3):
        for a, b in zip(views[ll], single[0][ll]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: the view built in pieces is not the view of a single append" % case.name
    assert np.array_equal(cnt, single[3]), "%s: hit counts, pieces against a single append" % case.name
    m = np.arange(knn.shape[-1])[None, None, None, :] < cnt[..., None]      # (what lies behind hit_cnt is not defined)
    for f in ("gidx", "level", "seq", "dist_sq"):
        assert np.array_equal(knn[f][m].view(np.uint32 if f == "dist_sq" else knn[f].dtype), single[2][f][m].view(np.uint32 if f == "dist_sq" else knn[f].dtype)), \
            "%s: %s of the hit lists, pieces against a single append" % (case.name, f)
    log.append("%-74s %3d appends  %5d/%5d/%5d keys  %6d hits at the last epoch" % (case.name, len(case.pieces), *[len(v[1]) for v in views], int(cnt.sum())))


def _view_case(name, keys, ts, seeds, pieces, base_q, edge=None):
    q = np.concatenate([base_q] * len(pieces))
    ep = np.repeat(np.asarray(pieces, np.int32), len(base_q))
    c = Case(name, keys, ts, seeds, q, epochs=ep, edge=edge, modes=(0,))
    c.pieces = list(pieces)
    return c


def view_cases():
    """D"""
    rng = np.random.default_rng(51)
    out = []
    # one scan at a time, more than CC_NVIEW = 4 buffers round, a query after each; scans 10 s apart enter the tree as in A5
    n = 14
    keys = np.zeros((n, 3, NPIV, DIM), F32)
    for ll in range(3):
        keys[:, ll] = cloud(rng, n * NPIV, 20.0 + rng.normal(0, 1.0, n * NPIV), spread=1.0).reshape(n, NPIV, DIM)
    keys[3:6, 0] = 0
    keys[3:6, 2] = 0          # appends that give new keys to one layer only
    keys[8, :, 3:] = 0        # a scan with three keys
    q = (np.tile(probe(20.0), (2, 3, NPIV, 1)) + rng.normal(0, 0.3, (2, 3, NPIV, DIM))).astype(F32)
    out.append(_view_case("D appends of one scan, 14 of them (CC_NVIEW = 4 buffers), three of them into one layer only, a query after each", keys,
                          np.arange(n) * 10.0, np.zeros(n, np.int32), list(range(1, n + 1)), q))
    # where a new key goes among equal key[0]
    old = cloud(rng, 12, [5, 5, 7, 9, 0.0, 7, 12, 12, 3, 9, 9, 7], spread=1.0)
    new = cloud(rng, 12, [7, 6, 6, -2, 30, -0.0, 0.0, -0.0, 9, 5, 12, 6], spread=1.0)
    lay = np.concatenate([old, new])
    k3, ts, seeds = flat([lay, lay[::-1].copy(), np.concatenate([new, old])])
    q = (np.tile(probe(7.0), (1, 3, NPIV, 1)) + rng.normal(0, 0.3, (1, 3, NPIV, DIM))).astype(F32)

    def edge_eq(facts):
        k0 = lay[:, 0]
        assert np.signbit(k0).sum() == 3 and (k0 == 0).sum() == 4 and k0[12:].min() < k0[:12].min() and k0[12:].max() > k0[:12].max()
        assert len(set(k0[12:].tolist()) & set(k0[:12].tolist())) >= 4 and (new[:, 0] == 6).sum() == 3
    out.append(_view_case("D new key[0] equal to an old key's, to another new key's, below and above all old keys, -0.0 beside +0.0", k3, ts, seeds,
                          [2, 4, 5], q, edge=edge_eq))
    # m = 64 / 65 / 66 new keys, then 4 096 / 4 097 / none: cc_k_ksort_new_lds and cc_k_ksort_new in one append
    a = [cloud(rng, m, np.round(rng.uniform(5, 40, m) * 4) / 4, spread=1.0) for m in (64, 65, 66)]
    b = [cloud(rng, m, np.round(rng.uniform(5, 40, m) * 16) / 16, spread=1.0) for m in (4096, 4097)]
    ka, kb = pack(a), pack(b + [np.zeros((0, DIM), F32)])
    assert len(ka) == 11 and len(kb) == 683
    keys = np.concatenate([ka, kb, np.zeros((1, 3, NPIV, DIM), F32)])
    nn = len(keys)
    ts, seeds = np.concatenate([np.zeros(nn - 1), [BIG_TS]]), np.concatenate([np.ones(nn - 1, np.int32), [0]])
    q = (np.tile(probe(20.0), (1, 3, NPIV, 1)) + rng.normal(0, 0.3, (1, 3, NPIV, DIM))).astype(F32)
    out.append(_view_case("D appends of 64/65/66 keys, then 4 096/4 097/0 keys in 683 scans (cc_k_ksort_new_lds | cc_k_ksort_new), then a scan without keys",
                          keys, ts, seeds, [11, 694, 695], q))
    return out
