"""TEST INFRASTRUCTURE: the cases of the listed query (cc_db_query_submit_listed, include/cont2_amd_lists.h; csrc/k_knn_list.h),
shared by the CPU harness (tests/test_emu_listed_query.py) and the GPU (tests/test_gpu_listed_query.py).  A case takes a `dev`:
the adapter of tests/masked_cases.py extended by
  ask(qdesc, epochs, table=None, rows=None, lists=None, ...)   one call: masked (table), listed (lists) or neither
  ask_host(qdesc, epochs, lists, rows)                         cc_db_query_batch_host_listed
  raw_rc_listed(...)                                           cc_db_query_submit_listed with the struct's fields as given
  listed_chunks() / knn_chunks()                               the retrieval counters
  bucket_ranges()                                              cc_db_bucket_state's ranges
A listed call is held against (1) the masked call of the same library whose rows are the lists' bits, byte for byte, and (2) the
filtered oracle (tests/masked_oracle.py) directly."""
import os

import numpy as np

import masked_cases as M
import masked_oracle
import packed_emu as P

LIST_SCANS_MAX = 1024
OUT_KEYS = ("res", "knn", "knn_cnt", "rank", "rank_n", "detail", "match")


def lists_of(table, n):
    """the set bits of every row of a mask table -> index lists"""
    return [np.nonzero(M.bit(row, np.arange(n)))[0].astype(np.int32) for row in table]


def flat(lists):
    """index lists -> (idx int32, off int32 [n_lists + 1])"""
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in lists]) if len(lists) else np.zeros(0, np.int32)
    return np.ascontiguousarray(idx, np.int32), off


def same(a, b, what, keys=None):
    """two calls' outputs, byte for byte (hit lists: counts and the entries up to them -- the rest is never written)"""
    keys = keys or [k for k in OUT_KEYS if k in a or k in b]
    for k in keys:
        assert k in a and k in b, (what, k)
        if k == "knn":
            M.hits_equal(None, a["knn"], a["knn_cnt"], b["knn"], b["knn_cnt"], (what, "knn"))
        else:
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- the adapter of the CPU harness ----
class EmuDev(M.EmuDev):
    def ask(self, qdesc, epochs, table=None, rows=None, lists=None, want_knn=True, ranked=None, detail=False, matches=None, src="desc", rec=None):
        """src: "desc" (qdesc: descriptors), "stored" (rec: database indices) or "packed" (qdesc packed here, rec: its rows)"""
        L, e = self.L, self.e
        nq = len(np.asarray(epochs).reshape(-1))
        ks = e.lib.cc_db_knn_stride(e.db)
        knn = np.zeros((nq, 3, L.NPIV, ks), L.knn_hit_dt) if want_knn else None
        cnt = np.zeros((nq, 3, L.NPIV), np.int32) if want_knn else None
        kw = {}
        if table is not None:
            table = np.ascontiguousarray(table, np.uint32)
            kw["mask"] = (table.ctypes.data, table.shape[0], table.shape[1], rows)
        if lists is not None:
            kw["among"] = flat(lists) + (rows,)
        if src == "desc":
            qd = np.ascontiguousarray(qdesc)
            kw["qdesc"] = qd.ctypes.data
        else:
            qd = e.src(None if src == "stored" else e.pack(qdesc))
            kw.update(src=qd, idx=rec)
        e.keep.append((qd, table, knn, cnt))
        r = P.calls.query(e.lib, e.db, epochs, knn=P._p(knn), knn_cnt=P._p(cnt), ranked=ranked, detail=detail, matches=matches, wait=False,
                          keep=e.keep, **kw)
        e.wait()
        rk = r.rank or (None, None)
        return P.PackedEmu._out(r.res, rk[0], rk[1], r.detail, knn=knn, knn_cnt=cnt, match=r.match)

    def _lists_c(self, idx, off, n_lists, rows):
        a = [None if x is None else np.ascontiguousarray(x, np.int32) for x in (idx, off, rows)]
        self.e.keep.append(a)
        return self.L.ScanListsC(P._p(a[0]), P._p(a[1]), n_lists, P._p(a[2]))

    def ask_host(self, qdesc, epochs, lists, rows, ranked=None, detail=False):
        L, e = self.L, self.e
        lb, ub = L.default_thresholds()
        epochs = np.ascontiguousarray(epochs, np.int32)
        qd = np.ascontiguousarray(qdesc)
        res = np.zeros(len(epochs), L.query_result_dt)
        ro, rc_, rn_, det = e._modes(len(epochs), ranked, detail)
        idx, off = flat(lists)
        c = self._lists_c(idx, off, len(lists), rows)
        rc = e.lib.cc_db_query_batch_host_listed(e.db, P._p(qd), len(epochs), P._p(epochs), P._b(lb), P._b(ub), P._p(res), P._b(ro), P._p(det), P._b(c), None)
        e.api.chk(rc, "cc_db_query_batch_host_listed")
        return P.PackedEmu._out(res, rc_, rn_, det)

    def raw_rc_listed(self, qdesc, epochs, idx, off, n_lists, rows, both=False, neither=False, null=False):
        """cc_db_query_submit_listed with the struct's fields as given (null: lists NULL) -> (return code, message, results)"""
        L, e = self.L, self.e
        lb, ub = L.default_thresholds()
        epochs = np.ascontiguousarray(epochs, np.int32)
        res = np.zeros(len(epochs), L.query_result_dt)
        qd = np.ascontiguousarray(qdesc)
        c = None if null else self._lists_c(idx, off, n_lists, rows)
        own = e.src(None)
        rc = e.lib.cc_db_query_submit_listed(e.db, None if neither else P._p(qd), P._b(own) if both else None, None, len(epochs), P._p(epochs),
                                             P._b(lb), P._b(ub), P._p(res), None, None, None, None, None, P._b(c), None)
        msg = e.lib.cc_last_error().decode()
        e.wait()
        return rc, msg, res

    def ask_null(self, qdesc, epochs):
        rc, msg, res = self.raw_rc_listed(qdesc, epochs, None, None, 0, None, null=True)
        assert rc == 0, msg
        return res

    def listed_chunks(self):
        out = np.zeros(2, np.int64)
        self.e.api.chk(self.e.lib.cc_db_debug_knn_chunks_listed(self.e.db, P._p(out)), "cc_db_debug_knn_chunks_listed")
        return out.tolist()

    def bucket_ranges(self):
        sizes, rg = np.zeros((3, 6), np.int32), np.zeros((3, 7), np.float32)
        self.e.api.chk(self.e.lib.cc_db_bucket_state(self.e.db, P._p(sizes), P._p(rg)), "cc_db_bucket_state")
        return rg


def counters(dev):
    return dev.knn_chunks() + dev.listed_chunks()


def delta(dev, before):
    return [a - b for a, b in zip(counters(dev), before)]


def both_ways(dev, qdesc, epochs, lists, rows, n_db, what, **kw):
    """the listed call and the masked call whose rows are the lists' bits -> the listed call's outputs, held equal to the masked one's"""
    table = M.pack_rows(dev.L, [np.asarray(l, np.int64) for l in lists], n_db)
    a = dev.ask(qdesc, epochs, lists=lists, rows=rows, **kw)
    b = dev.ask(qdesc, epochs, table=table, rows=rows, **kw)
    same(a, b, what)
    return a


# ---- case 1: the loop drive, against the masked call and the filtered oracle ----
def run_loop_drive(dev, cc, oracle, nnk):
    """Every (query, kind) pair of masked_cases.loop_reference in ONE listed call (rows of -1 among them: a mixed chunk), the
    queries at their own epochs -- right after their predecessor was added, so the newest keys are still buffered -- and the
    lists `ones`, `even`, `high` reaching past the epochs of the early queries (entries at and above the epoch never answer)."""
    L = oracle.L
    ref = M.loop_reference(cc, oracle, nnk)
    if nnk == 50:
        M.loop_edges(ref)
    q, rows, odesc, n = ref["q"], ref["rows"], ref["odesc"], ref["n"]
    lists = lists_of(ref["table"], n)
    assert len(lists[0]) == n and len(lists[1]) == 0 and (q[rows == 0] < n - 1).any()  # a full list at an epoch below its entries; an empty one
    dev.open(M.db_cfg(L, nnk), cap=n)
    try:
        dev.add(odesc, ref["ts"], ref["seeds"])
        c0 = counters(dev)
        out = dev.ask(odesc[q], q, lists=lists, rows=rows)
        assert delta(dev, c0) == [1, 0, 0, 0, 1]  # one chunk: the walk, then the list retrieval
        for k in range(len(q)):
            M.check_result(ref["ores"][k], out["res"][k], dev.tol, (int(q[k]), ref["kind"][k]))
        M.hits_equal(L, ref["oknn"], ref["ocnt"], out["knn"], out["knn_cnt"], "listed against the oracle")
        same(out, dev.ask(odesc[q], q, table=ref["table"], rows=rows), "listed against masked")
        # all of a chunk's queries name a list: the list retrieval alone
        named = np.nonzero(rows >= 0)[0]
        c0 = counters(dev)
        only = dev.ask(odesc[q[named]], q[named], lists=lists, rows=rows[named])
        assert delta(dev, c0) == [0, 0, 0, 1, 0]
        same(only, {k: out[k][named] for k in ("res", "knn", "knn_cnt")}, "listed chunk against the mixed chunk's rows")
        # the list of all scans below the epoch: the unrestricted call's bytes
        uq = np.array(M.LOOP_QUERIES, np.int32)
        un = dev.unmasked(odesc[uq], uq)
        below = dev.ask(odesc[uq], uq, lists=[np.arange(e, dtype=np.int32) for e in uq], rows=np.arange(len(uq), dtype=np.int32))
        same(below, un, "every scan below the epoch", ("res", "knn", "knn_cnt"))
        # lists NULL through the listed entry point: the unrestricted call, launch for launch
        c0 = counters(dev)
        assert dev.ask_null(odesc[uq], uq).tobytes() == un["res"].tobytes()
        assert delta(dev, c0) == [1, 0, 0, 0, 0]
        return ref, out
    finally:
        dev.close()


# ---- case 2: the crowded layer ----
_crowd = {}


def crowded_short(oracle):
    """masked_cases.crowded with scans 0..5 keeping 1, 2, 3, 4, 5 and 0 keys per layer (the other anchors' keys zeroed: a zero key is
    not added), so that sets of scans exist with any number of allowed keys"""
    if "d" not in _crowd:
        desc, ts, seeds, q = M.crowded(oracle, 450)
        desc, q = desc.copy(), q.copy()
        for s, keep in enumerate((1, 2, 3, 4, 5, 0)):
            desc["keys"][s, :, keep:, :] = 0
        # the queries' key[0] below every database key's: the anchors lie in the first bucket, from which every bucket is visible,
        # and stay well inside dist_ub (three terms of at least (0.2 * 6.75)^2 against distances of 1.25^2 + noise) -- every allowed
        # key that sits in a tree passes.  1.25: a shift at which no two keys of an oracle list lie at exactly the same f32 distance
        # (run_crowded asserts it) -- the order the reference gives such keys depends on its trees' shape; the library orders them
        # by key id, which run_longest_list holds against the masked call on exact duplicates
        q["keys"][..., 0] -= np.float32(1.25)
        _crowd["d"] = (desc, ts, seeds, q)
    return _crowd["d"]


def key_sets(L, nnk, n=450):
    """scan sets by their number of allowed keys per layer: nnk - 1, nnk, nnk + 1 (the first reduction), 2 nnk, 2 nnk + 1 (the
    second) -- full scans from 6 on, then the scan that keeps the remainder; 0 keys: the scan that keeps none"""
    sets = {}
    for t in (nnk - 1, nnk, nnk + 1, 2 * nnk, 2 * nnk + 1):
        full, part = divmod(t, L.NPIV)
        assert 6 + full <= n
        sets[t] = sorted(([part - 1] if part else [5]) + list(range(6, 6 + full)))
    return sets


def run_crowded(dev, oracle, nnk):
    """Near-identical keys: every allowed key passes the radius.  Allowed-key counts around the two reductions, the list
    lengths around the 64-scan steps, a scan without a key; hit lists against the filtered oracle and the masked call."""
    L = oracle.L
    n = 450
    desc, ts, seeds, q = crowded_short(oracle)
    dcfg = L.default_db_cfg()
    dcfg.nnk = nnk
    odb = masked_oracle.DB(dcfg)
    for i in range(n):
        odb.add(desc[i], ts[i], i)
    dev.open(dcfg, cap=n)
    try:
        dev.add(desc, ts, seeds)
        ksets = key_sets(L, nnk, n)
        lens = (0, 1, 63, 64, 65, 128, 129)
        lists = [np.asarray(s, np.int32) for s in ksets.values()] + [np.arange(100, 100 + m, dtype=np.int32) for m in lens] + [np.array([5], np.int32)]
        nl = len(lists)
        qi = np.repeat(np.arange(2), nl)
        rows = np.tile(np.arange(nl, dtype=np.int32), 2)
        ep = np.full(len(qi), n, np.int32)
        c0 = counters(dev)
        out = both_ways(dev, q[qi], ep, lists, rows, n, "crowded")
        assert delta(dev, c0) == [0, 0, 1, 1, 0]  # (the masked call's chunk and the listed call's)
        table = M.pack_rows(L, [np.asarray(l, np.int64) for l in lists], n)
        for k in range(len(qi)):
            _, oknn, ocnt = odb.query(q[qi[k]], 10000 + int(qi[k]), table[rows[k]])
            for s_ in np.ndindex(ocnt.shape):  # (the fixture: no two entries of an oracle list at the same distance)
                assert (np.diff(oknn["dist_sq"][s_][:ocnt[s_]].view(np.uint32)) != 0).all(), ("a tie in the oracle's list", k, s_)
            M.hits_equal(L, oknn, ocnt, out["knn"][k], out["knn_cnt"][k], ("crowded", k))
        # on the oracle's side: the sets hold the key counts they are named for (scans 6.. were added long before the epoch)
        for j, t in enumerate(ksets):
            assert (out["knn_cnt"][j] == min(t, nnk)).all(), (t, out["knn_cnt"][j])
        assert (out["knn_cnt"][len(ksets)] == 0).all() and (out["knn_cnt"][nl - 1] == 0).all()  # the empty list; the scan without a key
        assert (out["knn_cnt"][len(ksets) + 1] == min(L.NPIV, nnk)).all()
    finally:
        dev.close()
        odb.close()


def run_longest_list(dev, oracle, nnk=50):
    """CC_LIST_SCANS_MAX scans in one list, on the crowded layer repeated (1 350 scans): sixteen full steps, and every key twice or
    three times in the list -- exact ties, ordered by key id: to the bit against the masked call.  Against the oracle the counts
    and the distances to the bit (which of several keys at one distance the reference keeps depends on its trees' shape)."""
    L = oracle.L
    desc, ts, seeds, q = M.crowded(oracle, 450)
    desc = np.concatenate([desc, desc, desc])
    n = len(desc)
    ts = np.arange(n) * 0.1
    seeds = np.arange(n, dtype=np.int32)
    dcfg = L.default_db_cfg()
    dcfg.nnk = nnk
    odb = masked_oracle.DB(dcfg)
    for i in range(n):
        odb.add(desc[i], ts[i], i)
    dev.open(dcfg, cap=n)
    try:
        dev.add(desc, ts, seeds)
        lists = [np.arange(100, 100 + LIST_SCANS_MAX, dtype=np.int32), np.arange(0, 2 * LIST_SCANS_MAX, 2, dtype=np.int32)[:LIST_SCANS_MAX // 2]]
        rows = np.array([0, 1], np.int32)
        out = both_ways(dev, q, np.full(2, n, np.int32), lists, rows, n, "longest list")
        table = M.pack_rows(L, [np.asarray(l, np.int64) for l in lists], n)
        for k in range(2):
            _, oknn, ocnt = odb.query(q[k], 10000 + k, table[k])
            assert np.array_equal(ocnt, out["knn_cnt"][k])
            assert np.array_equal(oknn["dist_sq"][..., :nnk].view(np.uint32), out["knn"]["dist_sq"][k][..., :nnk].view(np.uint32))
            d = out["knn"]["dist_sq"][k][..., :nnk].view(np.uint32)
            assert (np.diff(d, axis=-1) == 0).any()  # ties are there
        assert out["knn_cnt"].min() == nnk
        # one more scan is refused
        rc, msg, _ = dev.raw_rc_listed(q, np.full(2, n, np.int32), np.arange(LIST_SCANS_MAX + 1, dtype=np.int32), np.array([0, LIST_SCANS_MAX + 1], np.int32), 1,
                                    np.zeros(2, np.int32))
        assert rc == M.CC_EINVAL and "CC_LIST_SCANS_MAX" in msg and "mask" in msg, msg
    finally:
        dev.close()
        odb.close()


# ---- case 3: the unindexed-bucket fixture (the VIS instances) and the visible buckets ----
def _unindexed(L):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_unindexed_bucket_fixture.npz"))
    n = len(z["ts"])
    desc = np.zeros(n, L.scan_desc_dt)
    desc["keys"] = z["keys"]
    d = L.default_db_cfg()
    cfg = z["cfg"]
    d.min_elapse, d.max_elapse, d.nnk, d.max_fine_opt, d.n_q_levels = cfg[0], cfg[1], int(cfg[2]), int(cfg[3]), int(cfg[4])
    for i in range(3):
        d.q_levels[i] = int(cfg[5 + i])
    return z, n, desc, d


def run_unindexed(dev, oracle, nnk=None):
    """Queries at epochs at which a bucket's tree does not index its whole range: the VIS instances, listed against masked.
    nnk: None = the fixture's own (the KM 64 instance, its recorded counts asserted), or a value above 64 (the KM 256 instance)."""
    L = oracle.L
    z, n, desc, d = _unindexed(L)
    if nnk is not None:
        assert d.nnk <= 64 < nnk
        d.nnk = nnk
    dev.open(d, cap=n)
    try:
        dev.add(desc, z["ts"], z["seeds"])
        q = np.arange(52, n, dtype=np.int32)
        un = dev.unmasked(desc[q], q)
        if nnk is None:
            assert np.array_equal(un["knn_cnt"], z["knn_cnt"][q])
        else:
            assert un["knn"].shape[-1] == 256 and un["knn_cnt"].max() > 64  # the large instance, and lists it alone can hold
        lists = [np.arange(0, n, 2, dtype=np.int32), np.nonzero(np.arange(n) % 3 != 0)[0].astype(np.int32)]
        rows = (np.arange(len(q)) % 2).astype(np.int32)
        out = both_ways(dev, desc[q], q, lists, rows, n, "unindexed")
        assert (out["knn_cnt"] != un["knn_cnt"]).any()
        below = dev.ask(desc[q], q, lists=[np.arange(e, dtype=np.int32) for e in q], rows=np.arange(len(q), dtype=np.int32))
        same(below, un, "unindexed: every scan below the epoch", ("knn", "knn_cnt"))
    finally:
        dev.close()


_wide = {}


def wide_layer(oracle, n=250):
    """250 scans whose keys are the crowded layer's but for key[0], spread over 6 .. 14: with the loop drive's short delays the
    balancing has split every layer into six populated buckets by the last epoch (asserted by run_buckets).  The seeds are 3 i:
    with seeds 0, 1, 2, .. the bucket pairs are balanced in the cycle 0 1 2 3 4 3 2 1, pair (3, 4) always empties the fifth
    bucket's buffer one scan before pair (4, 5) looks at it, and the sixth bucket never gets a key at any size."""
    if "d" not in _wide:
        from test_hostdb_bookkeeping import _fake_desc
        L = oracle.L
        rng = np.random.default_rng(33)
        desc = _fake_desc(L, rng, n)
        base = rng.uniform(8.0, 12.0, L.KEY_DIM).astype(np.float32)
        keys = (base[None, None, None, :] + rng.normal(0, 0.05, (n, L.NLEV, L.NPIV, L.KEY_DIM))).astype(np.float32)
        keys[..., 0] = rng.uniform(6.0, 14.0, (n, L.NLEV, L.NPIV)).astype(np.float32)
        desc["keys"] = keys
        _wide["d"] = (desc, np.arange(n) * 0.1, (3 * np.arange(n)).astype(np.int32))
    return _wide["d"]


def run_buckets(dev, cc, oracle):
    """The anchor's bucket `mid` decides which buckets are visible: {0 .. mid} and {2 mid + 1 .. 5}.  The database's own scans as
    queries at the last epoch, with anchors in all six buckets: mid = 0 (2 mid + 1 == mid + 1: everything), 1 and 2 (a gap),
    3 and 4 (2 mid + 1 beyond the ranges) and 5 (rg[mid + 1] is rg[6]: the first range runs to the end), and database keys in the
    sixth bucket under `key[0] < rg[6]`.  The ranges are key[0] values of database keys (the balancing splits AT a key), so keys
    lie exactly on a range.  Hit lists against the masked call and against the filtered oracle."""
    L = oracle.L
    desc, ts, seeds = wide_layer(oracle)
    n = len(desc)
    dcfg = M.db_cfg(L, 50)
    odb = masked_oracle.DB(dcfg)
    for i in range(n):
        odb.add(desc[i], ts[i], int(seeds[i]))
    dev.open(dcfg, cap=n)
    try:
        dev.add(desc, ts, seeds)
        rg = dev.bucket_ranges()
        lv = [dcfg.q_levels[i] for i in range(dcfg.n_q_levels)]  # (the descriptor keeps the levels from 0; the hot record from 1)
        k0 = desc["keys"][..., 0][:, lv]  # [n, layers, NPIV]
        per_bucket = np.zeros(6, np.int64)
        on_range = 0
        for l in range(len(lv)):
            r = rg[l]
            assert (np.diff(r) > 0).all() and r[5] < 1000.0 == r[6], r  # six populated buckets
            for b in range(6):
                per_bucket[b] += int(((r[b] <= k0[:, l]) & (k0[:, l] < r[b + 1])).sum())
            on_range += int((k0[:, l, :, None] == r[None, None, 1:6]).sum())
        assert (per_bucket > 0).all() and on_range >= 5 * len(lv), (per_bucket, on_range)
        q = np.arange(0, n, 5, dtype=np.int32)  # 50 scans: 900 anchors, every bucket among them in every layer
        qa = k0[q]
        for l in range(len(lv)):
            for b in range(6):
                assert ((rg[l][b] <= qa[:, l]) & (qa[:, l] < rg[l][b + 1])).any(), (l, b)
        ep = np.full(len(q), n, np.int32)
        # (the last list: 8 scans, fewer keys than nnk -- every visible key inside dist_ub answers, also those beyond the gap)
        lists = [np.arange(0, n, 2, dtype=np.int32), np.arange(1, n, 2, dtype=np.int32), np.arange(n, dtype=np.int32), np.arange(3, n, 25, dtype=np.int32)]
        rows = (np.arange(len(q)) % 4).astype(np.int32)
        out = both_ways(dev, desc[q], ep, lists, rows, n, "buckets")
        un = dev.unmasked(desc[q], ep)
        full = np.nonzero(rows == 2)[0]
        same({k: out[k][full] for k in ("knn", "knn_cnt")}, {k: un[k][full] for k in ("knn", "knn_cnt")}, "the list of every scan")
        table = M.pack_rows(L, [np.asarray(l, np.int64) for l in lists], n)
        far, sixth = 0, [0, 0]
        for i in range(len(q)):
            _, oknn, ocnt = odb.query(desc[q[i]], 10000 + i, table[rows[i]])
            for s_ in np.ndindex(ocnt.shape):
                assert (np.diff(oknn["dist_sq"][s_][:ocnt[s_]].view(np.uint32)) != 0).all(), ("a tie in the oracle's list", i, s_)
            M.hits_equal(L, oknn, ocnt, out["knn"][i], out["knn_cnt"][i], ("buckets", i))
            # every hit lies in a visible bucket of its anchor; for mid = 1 and 2 some come from beyond the gap
            for l in range(len(lv)):
                for a in range(L.NPIV):
                    mid = int(np.searchsorted(rg[l][1:6], qa[i, l, a], side="right"))
                    h = out["knn"][i][l, a][:out["knn_cnt"][i][l, a]]
                    hb = np.searchsorted(rg[l][1:6], desc["keys"][h["gidx"], lv[l], h["seq"], 0], side="right")
                    assert ((hb <= mid) | (hb >= 2 * mid + 1)).all(), (i, l, a, mid)
                    far += int((hb > mid).sum()) if mid in (1, 2) else 0
                    sixth[0] += int((hb == 5).sum()) if mid == 5 else 0  # an anchor in the sixth bucket finds keys of it
                    sixth[1] += int((hb == 5).sum()) if mid < 3 else 0   # ... and so do anchors that see it across the gap
        assert far > 0 and sixth[0] > 0 and sixth[1] > 0, (far, sixth)
        return per_bucket, on_range
    finally:
        dev.close()
        odb.close()


# ---- case 4: mixing ----
def run_mixing(dev, cc, oracle):
    """Lists and -1 in one call, a list shared by many queries, the stored / packed / host forms, ranked lists with detail and
    match rows -- each against the masked call, with the retrieval counters."""
    L = oracle.L
    ref = M._loop_db(dev, cc, oracle)
    try:
        odesc, n = ref["odesc"], ref["n"]
        lists = lists_of(ref["table"], n)
        high = int(ref["rows"][M._pick(ref, 57, "high")])
        nb37 = int(ref["rows"][M._pick(ref, 37, "not_best")])
        q = np.array([37, 37, 57, 60, 33, 50, 63], np.int32)
        rows = np.array([-1, nb37, high, high, -1, high, high], np.int32)  # `high` shared by four queries
        kinds = ["unmasked", "not_best", "high", "high", "unmasked", "high", "high"]
        c0 = counters(dev)
        out = both_ways(dev, odesc[q], q, lists, rows, n, "mixing")
        assert delta(dev, c0) == [1, 0, 1, 0, 1]
        un = dev.unmasked(odesc[q], q)
        for i in (0, 4):
            assert out["res"][i].tobytes() == un["res"][i].tobytes()
            M.hits_equal(L, out["knn"][i], out["knn_cnt"][i], un["knn"][i], un["knn_cnt"][i], "rows of -1")
        for i in range(len(q)):
            k = M._pick(ref, int(q[i]), kinds[i])
            M.check_result(ref["ores"][k], out["res"][i], dev.tol, (int(q[i]), kinds[i]))
            M.hits_equal(L, ref["oknn"][k], ref["ocnt"][k], out["knn"][i], out["knn_cnt"][i], (int(q[i]), kinds[i]))
        assert out["res"]["cand_gidx"][1] == 17 and out["res"]["cand_gidx"][2] == 32
        # rows of -1 only: what the call launches without lists
        c0 = counters(dev)
        same(dev.ask(odesc[q], q, lists=lists, rows=np.full(len(q), -1, np.int32)), un, "no query names a list", ("res", "knn", "knn_cnt"))
        assert delta(dev, c0) == [1, 0, 0, 0, 0]
        # the stored and packed forms
        same(dev.ask(None, q, lists=lists, rows=rows, src="stored", rec=q), out, "stored")
        same(dev.ask(odesc[q], q, lists=lists, rows=rows, src="packed"), out, "packed")
        # the host form (results only)
        h = dev.ask_host(odesc[q], q, lists, rows)
        assert h["res"].tobytes() == out["res"].tobytes()
        # ranked lists, detail and match rows
        rk = both_ways(dev, odesc[q], q, lists, rows, n, "ranked", ranked=4, detail=True, matches=2.0)
        assert rk["res"].tobytes() == out["res"].tobytes() and rk["detail"].shape == (len(q), 4) and rk["match"].shape == (len(q), 4)
        assert rk["rank_n"].max() >= 1 and rk["match"]["n_pairs"][rk["rank_n"] > 0, 0].min() > 0
        for i in np.nonzero(rows >= 0)[0]:
            assert np.isin(rk["rank"]["cand_gidx"][i, :int(rk["rank_n"][i])], lists[rows[i]]).all(), i
        same(dev.ask(None, q, lists=lists, rows=rows, src="stored", rec=q, ranked=4, detail=True, matches=2.0), rk, "stored, ranked")
    finally:
        dev.close()


def run_chunks(dev, cc, oracle, nq=130):
    """130 queries over four lanes: chunks of 64, 64 and 2 -- a mixed one, one that names no list, one in which every query does."""
    L = oracle.L
    z, n, desc, d = _unindexed(L)
    dev.open(d, cap=n, lanes=4)
    try:
        dev.add(desc, z["ts"], z["seeds"])
        q = (np.arange(nq) * 7 % n).astype(np.int32)
        lists = [np.arange(0, n, 2, dtype=np.int32), np.nonzero(np.arange(n) % 3 != 0)[0].astype(np.int32), np.arange(40, dtype=np.int32)]
        rows = (np.arange(nq) % 4 - 1).astype(np.int32)
        rows[64:128] = -1
        rows[128:] = 2
        c0 = counters(dev)
        out = dev.ask(desc[q], q, lists=lists, rows=rows)
        assert delta(dev, c0) == [2, 0, 0, 1, 1], delta(dev, c0)
        table = M.pack_rows(L, [np.asarray(l, np.int64) for l in lists], n)
        same(out, dev.ask(desc[q], q, table=table, rows=rows), "chunks against masked")
        for c0_ in range(0, nq, 26):
            s = slice(c0_, min(c0_ + 26, nq))
            same(dev.ask(desc[q[s]], q[s], lists=lists, rows=rows[s]), {k: out[k][s] for k in ("res", "knn", "knn_cnt")}, ("part", c0_))
        un = dev.unmasked(desc[q[64:128]], q[64:128])
        M.hits_equal(L, un["knn"], un["knn_cnt"], out["knn"][64:128], out["knn_cnt"][64:128], "the chunk without a list")
        # 300 queries: chunks of 128, 128 and 44 -- above the size up to which rows and entries are read where the host staged them
        q3 = (np.arange(300) * 7 % n).astype(np.int32)
        rows3 = (np.arange(300) % 4 - 1).astype(np.int32)
        c0 = counters(dev)
        big = dev.ask(desc[q3], q3, lists=lists, rows=rows3)
        assert delta(dev, c0) == [3, 0, 0, 0, 3], delta(dev, c0)
        same(big, dev.ask(desc[q3], q3, table=table, rows=rows3), "large chunks against masked")
        same({k: big[k][:nq] for k in ("res", "knn", "knn_cnt")}, dev.ask(desc[q3[:nq]], q3[:nq], lists=lists, rows=rows3[:nq]), "large chunks against small ones")
    finally:
        dev.close()


def run_tiled_mode(dev, cc, oracle):
    """CC_KNN_MODE=2 (set by the caller before the database exists): a mixed chunk's first launch is the tiled search."""
    L = oracle.L
    ref = M._loop_db(dev, cc, oracle)
    try:
        odesc, n = ref["odesc"], ref["n"]
        lists = lists_of(ref["table"], n)
        q = np.array([37, 57, 60], np.int32)
        kinds = ["not_best", "high", "unmasked"]
        rows = np.array([ref["rows"][M._pick(ref, 37, "not_best")], ref["rows"][M._pick(ref, 57, "high")], -1], np.int32)
        c0 = counters(dev)
        out = dev.ask(odesc[q], q, lists=lists, rows=rows)
        assert delta(dev, c0) == [0, 1, 0, 0, 1]
        for i in range(3):
            k = M._pick(ref, int(q[i]), kinds[i])
            M.check_result(ref["ores"][k], out["res"][i], dev.tol, (int(q[i]), kinds[i]))
            M.hits_equal(L, ref["oknn"][k], ref["ocnt"][k], out["knn"][i], out["knn_cnt"][i], (int(q[i]), kinds[i]))
        c0 = counters(dev)
        only = dev.ask(odesc[q[:2]], q[:2], lists=lists, rows=rows[:2])
        assert delta(dev, c0) == [0, 0, 0, 1, 0]
        same(only, {k: out[k][:2] for k in ("res", "knn", "knn_cnt")}, "tiled mode: the listed chunk")
        c0 = counters(dev)
        dev.unmasked(odesc[q], q)
        assert delta(dev, c0) == [0, 1, 0, 0, 0]
    finally:
        dev.close()


# ---- case 5: refusals ----
def run_refusals(dev, cc, oracle):
    L = oracle.L
    ref = M._loop_db(dev, cc, oracle)
    try:
        odesc, n = ref["odesc"], ref["n"]
        q = np.array([37, 57], np.int32)
        nb37 = lists_of(ref["table"], n)[int(ref["rows"][M._pick(ref, 37, "not_best")])]
        idx = np.array([1, 5, 9, 2, 3], np.int32)
        off = np.array([0, 3, 5], np.int32)
        ok_rows = np.array([0, -1], np.int32)
        i32 = lambda *v: np.array(v, np.int32)  # noqa: E731

        def usable():
            out = dev.ask(odesc[q], q, lists=[nb37], rows=np.array([0, -1], np.int32))
            assert out["res"]["cand_gidx"][0] == 17

        c0 = counters(dev)
        for what, args, word in (
                ("n_lists < 1", (idx, off, 0, ok_rows), "n_lists"),
                ("h_off does not start at 0", (idx, i32(1, 3, 5), 2, ok_rows), "h_off"),
                ("h_off decreases", (idx, i32(0, 4, 3), 2, ok_rows), "h_off"),
                ("row too large", (idx, off, 2, i32(2, -1)), "h_row"),
                ("row below -1", (idx, off, 2, i32(0, -2)), "h_row"),
                ("a list that is not strictly increasing", (i32(1, 5, 5, 2, 3), off, 2, ok_rows), "increasing"),
                ("a list that decreases", (i32(1, 9, 5, 2, 3), off, 2, ok_rows), "increasing"),
                ("an entry below 0", (i32(-1, 5, 9, 2, 3), off, 2, ok_rows), "cc_db_size"),
                ("an entry at cc_db_size", (i32(1, 5, n, 2, 3), off, 2, ok_rows), "cc_db_size"),
                ("a list longer than the capacity", (np.arange(LIST_SCANS_MAX + 1, dtype=np.int32) % n, i32(0, LIST_SCANS_MAX + 1), 1, ok_rows), "CC_LIST_SCANS_MAX"),
        ):
            rc, msg, _ = dev.raw_rc_listed(odesc[q], q, *args)
            assert rc == M.CC_EINVAL and word in msg, (what, rc, msg)
            assert delta(dev, c0) == [0, 0, 0, 0, 0], what  # nothing queued
            usable()
            c0 = counters(dev)
        # an entry at or above the query's epoch is legal: list 0 at epochs 3 and 9
        rc, msg, _ = dev.raw_rc_listed(odesc[[3, 9]], i32(3, 9), idx, off, 2, i32(0, 0))
        assert rc == 0, msg
        # both or neither of d_qdesc and src
        rc, msg, _ = dev.raw_rc_listed(odesc[q], q, idx, off, 2, ok_rows, both=True)
        assert rc == M.CC_EINVAL and "exactly one" in msg
        rc, msg, _ = dev.raw_rc_listed(odesc[q], q, idx, off, 2, ok_rows, neither=True)
        assert rc == M.CC_EINVAL and "exactly one" in msg
        # what the unrestricted call refuses: an epoch beyond the database
        rc, msg, _ = dev.raw_rc_listed(odesc[q], i32(37, n + 1), idx, off, 2, ok_rows)
        assert rc == M.CC_EINVAL and "epoch" in msg
        usable()
        # dynamic thresholds
        dev.set_dyn(1)
        rc, msg, _ = dev.raw_rc_listed(odesc[q], q, idx, off, 2, ok_rows)
        assert rc == M.CC_EINVAL and "dynamic" in msg, msg
        dev.set_dyn(0)
        usable()
    finally:
        dev.close()
