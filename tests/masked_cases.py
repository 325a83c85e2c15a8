"""TEST INFRASTRUCTURE: the cases of the masked query (cc_db_query_submit_masked, cc_mask_gates), shared by the CPU harness
(tests/test_emu_masked_query.py) and the GPU (tests/test_gpu_masked_query.py).  A case takes a `dev`: an adapter with
open / add / query / raw_rc / gates / close over one of the two (EmuDev below, GpuDev in the GPU test file).  The oracle is
tests/masked_oracle.py: the reference's query on trees filtered to the allowed scans."""
import numpy as np

import masked_oracle
import packed_emu as P

INT_FIELDS = ["n_res", "cand_gidx", "cand_aft_check1", "cand_aft_check2", "cand_aft_check3", "n_cand_pose", "n_cand_tidy",
              "n_knn_hits"]
HIT_FIELDS = ("gidx", "level", "seq", "dist_sq")
LOOP_QUERIES = (20, 33, 37, 50, 57, 60, 63)
CC_EINVAL = -1


def pack_rows(L, allowed, n_db, row_words=None):
    return L.pack_mask_rows(allowed, n_db=n_db, row_words=row_words)


def bit(row, g):
    g = np.asarray(g)
    return (row[g >> 5] >> (g & 31).astype(np.uint32)) & 1 != 0


# ---- the adapter of the CPU harness ----
class EmuDev:
    """One database on tests/emu/libcc_emu.so ("device" pointers are host pointers there)."""
    tol = 1e-6

    def __init__(self, L):
        self.L = L
        self.e = None

    def open(self, dcfg, cap, lanes=None, dyn=False):
        self.e = P.PackedEmu(self.L, dcfg, cap=cap, lanes=lanes, dyn=dyn)
        return self

    def close(self):
        if self.e is not None:
            self.e.close()
            self.e = None

    def add(self, desc, ts, seeds):
        self.desc = np.ascontiguousarray(desc)
        self.e.add(desc, ts, seeds)

    def set_dyn(self, on):
        self.e.api.chk(self.e.lib.cc_db_set_dynamic_thres(self.e.db, on), "cc_db_set_dynamic_thres")

    def query(self, qdesc, epochs, table=None, rows=None, want_knn=True, ranked=None, detail=False, src="desc", rec=None, host=False):
        """src: "desc" (qdesc: descriptors), "stored" (rec: database indices) or "packed" (qdesc packed here, rec: its rows);
        host: cc_db_query_batch_host_masked (descriptors only, no hit lists)."""
        L, e = self.L, self.e
        nq = len(np.asarray(epochs).reshape(-1))
        ks = e.lib.cc_db_knn_stride(e.db)
        knn = np.zeros((nq, 3, L.NPIV, ks), L.knn_hit_dt) if want_knn and not host else None
        cnt = np.zeros((nq, 3, L.NPIV), np.int32) if want_knn and not host else None
        if table is not None:
            table = np.ascontiguousarray(table, np.uint32)
        if host:
            lb, ub = L.default_thresholds()
            epochs, rows = np.ascontiguousarray(epochs, np.int32), np.ascontiguousarray(rows, np.int32)
            qd = np.ascontiguousarray(qdesc)
            res = np.zeros(nq, L.query_result_dt)
            ro, rc_, rn_, det = e._modes(nq, ranked, detail)
            m = None if table is None else L.ScanMaskC(table.ctypes.data, table.shape[0], table.shape[1], rows.ctypes.data)
            rc = e.lib.cc_db_query_batch_host_masked(e.db, P._p(qd), nq, P._p(epochs), P._b(lb), P._b(ub), P._p(res), P._b(ro), P._p(det), P._b(m))
            e.api.chk(rc, "cc_db_query_batch_host_masked")
            return P.PackedEmu._out(res, rc_, rn_, det)
        if table is None:  # the masked entry point with mask NULL: a form of the C-ABI alone
            assert src == "desc" and ranked is None
            lb, ub = L.default_thresholds()
            epochs, qd, res = np.ascontiguousarray(epochs, np.int32), np.ascontiguousarray(qdesc), np.zeros(nq, L.query_result_dt)
            e.keep.append((qd, epochs, res, knn, cnt, lb, ub))
            e.api.chk(e.lib.cc_db_query_submit_masked(e.db, P._p(qd), None, None, nq, P._p(epochs), P._b(lb), P._b(ub), P._p(res), P._p(knn),
                                                      P._p(cnt), None, None, None, None), "cc_db_query_submit_masked")
            e.wait()
            return P.PackedEmu._out(res, None, None, None, knn=knn, knn_cnt=cnt)
        kw = {"mask": (table.ctypes.data, table.shape[0], table.shape[1], rows)}
        if src == "desc":
            qd = np.ascontiguousarray(qdesc)
            kw["qdesc"] = qd.ctypes.data
        else:
            qd = e.src(None if src == "stored" else e.pack(qdesc))
            kw.update(src=qd, idx=rec)
        e.keep.append((qd, table, knn, cnt))
        r = P.calls.query(e.lib, e.db, epochs, knn=P._p(knn), knn_cnt=P._p(cnt), ranked=ranked, detail=detail, wait=False, keep=e.keep, **kw)
        e.wait()
        rk = r.rank or (None, None)
        return P.PackedEmu._out(r.res, rk[0], rk[1], r.detail, knn=knn, knn_cnt=cnt)

    def unmasked(self, qdesc, epochs, want_knn=True, ranked=None, detail=False):
        """the descriptor form's existing entry points (cc_db_query_submit[_ranked[_detail]])"""
        return self.e.query(qdesc, None, epochs, ranked=ranked, detail=detail, want_knn=want_knn)

    def raw_rc(self, qdesc, epochs, bits_ptr, n_rows, row_words, rows, both=False, neither=False):
        """cc_db_query_submit_masked with the mask's fields as given -> (return code, message)"""
        L, e = self.L, self.e
        lb, ub = L.default_thresholds()
        epochs = np.ascontiguousarray(epochs, np.int32)
        rows = np.ascontiguousarray(rows, np.int32)
        res = np.zeros(len(epochs), L.query_result_dt)
        qd = np.ascontiguousarray(qdesc)
        m = L.ScanMaskC(bits_ptr, n_rows, row_words, rows.ctypes.data)
        own = e.src(None)
        rc = e.lib.cc_db_query_submit_masked(e.db, None if neither else P._p(qd), P._b(own) if both else None, None, len(epochs), P._p(epochs),
                                             P._b(lb), P._b(ub), P._p(res), None, None, None, None, None, P._b(m))
        msg = e.lib.cc_last_error().decode()
        e.wait()
        return rc, msg

    def knn_chunks(self):
        out = np.zeros(3, np.int64)
        self.e.api.chk(self.e.lib.cc_db_debug_knn_chunks(self.e.db, P._p(out)), "cc_db_debug_knn_chunks")
        return out.tolist()

    def table_ptr(self, table):
        """the address cc_scan_mask_t.bits takes for this table (kept alive)"""
        t = np.ascontiguousarray(table, np.uint32)
        self.e.keep.append(t)
        return t.ctypes.data

    def query_gate_bits(self, qdesc, epochs, xy, gate, rows):
        """a masked query whose table comes straight from cc_mask_gates"""
        return self.query(qdesc, epochs, self.gates(xy, gate, (len(xy) + 31) // 32), rows)

    def gates(self, xy, gates, row_words, n_scans=None, raw=False):
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        gates = np.ascontiguousarray(gates, np.float32).reshape(-1, 3)
        n = len(xy) if n_scans is None else n_scans
        out = np.full((len(gates), max(row_words, 1)), 0xDEADBEEF, np.uint32)
        pad = np.zeros(2, np.float32)
        rc = self.e.lib.cc_mask_gates(self.e.ctx, P._p(xy if len(xy) else pad), n, P._p(gates), len(gates), P._p(out), row_words, None)
        if raw:
            return rc, self.e.lib.cc_last_error().decode()
        self.e.api.chk(rc, "cc_mask_gates")
        return out


# ---- shared checks ----
def hits_equal(L, knn_a, cnt_a, knn_b, cnt_b, what):
    """two sets of hit lists [.., NQLEV, NPIV, stride] (strides may differ): counts and every entry up to the count, to the bit"""
    assert np.array_equal(cnt_a, cnt_b), (what, np.argwhere(cnt_a != cnt_b)[:5])
    w = int(cnt_a.max()) if cnt_a.size else 0
    m = np.arange(w) < cnt_a[..., None]
    for f in HIT_FIELDS:
        a, b = knn_a[f][..., :w], knn_b[f][..., :w]
        if f == "dist_sq":
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a[m], b[m]), (what, f)


def check_result(ores, res, tol, what):
    for f in INT_FIELDS:
        assert ores[f] == res[f], (what, f, ores[f], res[f])
    if ores["n_res"]:
        assert abs(ores["correlation"] - res["correlation"]) < tol, what
        assert np.abs(ores["tf"] - res["tf"]).max() < tol, what


def check_properties(knn_u, cnt_u, knn_m, cnt_m, row, nnk, what):
    """Case 3, per search: (a) where the unmasked search returned fewer than nnk hits the masked list is the unmasked list
    filtered by the row, in order; (b) where it was full, its allowed entries are a prefix of the masked list."""
    n_full = n_short = 0
    for idx in np.ndindex(cnt_u.shape):
        cu, cm = int(cnt_u[idx]), int(cnt_m[idx])
        u, m = knn_u[idx][:cu], knn_m[idx][:cm]
        keep = u[bit(row, u["gidx"])] if cu else u
        if cu < nnk:
            n_short += 1
            assert cm == len(keep) and m.tobytes() == keep.tobytes(), (what, "a", idx)
        else:
            n_full += 1
            assert cm >= len(keep) and m[:len(keep)].tobytes() == keep.tobytes(), (what, "b", idx)
    return n_short, n_full


# ---- case 1: the loop drive ----
def db_cfg(L, nnk):
    d = L.default_db_cfg()
    d.max_elapse, d.min_elapse = 2.5, 1.5
    d.nnk = nnk
    return d


_drive = {}


def loop_drive(cc, oracle):
    """the 64-scan loop drive of tests/test_emu_large_nnk.py::_sequence: descriptors, times, seeds, poses (made once)"""
    if "d" not in _drive:
        w = cc.synth.World(loop_len=40.0)
        n = 64
        x, poses, ts = cc.synth.make_sequence(n, world=w, beams=16, azim=450)
        xs = x.numpy().reshape(-1, 4)
        offs = np.arange(n + 1, dtype=np.int64) * x.shape[1]
        seeds = np.arange(n, dtype=np.int32)
        out = {}
        for nnk in (50, 128):
            ores, _, odesc = oracle.run_sequence(xs, offs, ts, seeds, dcfg=db_cfg(oracle.L, nnk), want_desc=True)
            out[nnk] = ores
        _drive["d"] = (n, ts, seeds, odesc, np.asarray(poses), out)
    return _drive["d"]


_loop_ref = {}


def loop_reference(cc, oracle, nnk):
    """Case 1's queries, rows and filtered-oracle answers at this nnk (made once, shared by the tests that need them):
    q [nq] scan index of every (query, kind) pair, rows [nq] its row (-1: the unmasked call), table [n_rows, 2],
    kind [nq] the name of the pair's mask, ores / oknn / ocnt the oracle's."""
    if nnk in _loop_ref:
        return _loop_ref[nnk]
    L = oracle.L
    n, ts, seeds, odesc, poses, ores_all = loop_drive(cc, oracle)
    ores_u = ores_all[nnk]
    allow = {"ones": np.ones(n, bool), "none": np.zeros(n, bool), "even": np.arange(n) % 2 == 0, "low": np.arange(n) < 32,
             "high": np.arange(n) >= 32}
    names = list(allow)
    rows_bool = [allow[k] for k in names]
    q, rows, kind = [], [], []
    for qi in LOOP_QUERIES:
        q.append(qi), rows.append(-1), kind.append("unmasked")
        for k in names:
            q.append(qi), rows.append(names.index(k)), kind.append(k)
        best = int(ores_u["cand_gidx"][qi])
        if best >= 0:
            a = np.ones(n, bool)
            a[best] = False
            rows_bool.append(a), q.append(qi), rows.append(len(rows_bool) - 1), kind.append("not_best")
            a = np.zeros(n, bool)
            a[best] = True
            rows_bool.append(a), q.append(qi), rows.append(len(rows_bool) - 1), kind.append("only_best")
    table = pack_rows(L, np.array(rows_bool), n)
    q, rows = np.array(q, np.int32), np.array(rows, np.int32)
    odb = masked_oracle.DB(db_cfg(L, nnk))
    ores = np.zeros(len(q), L.query_result_dt)
    oknn = np.zeros((len(q), L.NQLEV, L.NPIV, 256), L.knn_hit_dt)
    ocnt = np.zeros((len(q), L.NQLEV, L.NPIV), np.int32)
    for i in range(n):
        for k in np.nonzero(q == i)[0]:
            ores[k], oknn[k], ocnt[k] = odb.query(odesc[i], int(seeds[i]), None if rows[k] < 0 else table[rows[k]])
        odb.add(odesc[i], ts[i], int(seeds[i]))
    odb.close()
    # the unmasked filtered-oracle call is the oracle's own replay; all ones is too
    for k in np.nonzero((rows < 0) | (np.array(kind) == "ones"))[0]:
        for f in INT_FIELDS:
            assert ores[f][k] == ores_u[f][q[k]], (k, f)
    _loop_ref[nnk] = dict(q=q, rows=rows, kind=np.array(kind), table=table, ores=ores, oknn=oknn, ocnt=ocnt, odesc=odesc, ts=ts, seeds=seeds, n=n,
                          poses=poses)
    return _loop_ref[nnk]


def _pick(ref, qi, kind):
    k = np.nonzero((ref["q"] == qi) & (ref["kind"] == kind))[0]
    assert len(k) == 1, (qi, kind)
    return int(k[0])


def loop_edges(ref):
    """The drive reaches its edges (the oracle's side, nnk = 50)."""
    o = ref["ores"]
    g = lambda qi, kind: (int(o["n_res"][_pick(ref, qi, kind)]), int(o["cand_gidx"][_pick(ref, qi, kind)]))  # noqa: E731
    assert g(33, "unmasked") == (1, 17) and g(33, "not_best")[0] == 0
    assert g(37, "unmasked") == (1, 0) and g(37, "not_best") == (1, 17)
    assert g(57, "high") == (1, 32)
    assert g(60, "unmasked") == (1, 20) and g(60, "even") == (1, 0)
    differ = False
    for qi in (50, 57, 60):
        ku, kb = _pick(ref, qi, "unmasked"), _pick(ref, qi, "not_best")
        cu, cb = ref["ocnt"][ku], ref["ocnt"][kb]
        for idx in np.argwhere((cu == 50) & (cb == 50)):
            a, b = ref["oknn"][ku][tuple(idx)][:50], ref["oknn"][kb][tuple(idx)][:50]
            best = int(o["cand_gidx"][ku])
            shared = a[a["gidx"] != best]
            # the masked list goes past the unmasked one's last entry for the keys that replace the excluded ones
            if len(shared) < 50 and b[:len(shared)].tobytes() == shared.tobytes() and b["dist_sq"][-1] >= a["dist_sq"][-1]:
                differ = True
    assert differ, "a full search whose list changes when the best scan is excluded"
    for k in np.nonzero(ref["q"] == 20)[0]:
        assert o["n_res"][k] == 0


def run_loop_drive(dev, cc, oracle, nnk):
    """Case 1 (and case 3 on it): every (query, kind) pair in ONE masked call; first the unmasked call against the oracle."""
    L = oracle.L
    ref = loop_reference(cc, oracle, nnk)
    if nnk == 50:
        loop_edges(ref)
    q, rows, odesc = ref["q"], ref["rows"], ref["odesc"]
    dev.open(db_cfg(L, nnk), cap=ref["n"])
    try:
        dev.add(odesc, ref["ts"], ref["seeds"])
        uq = np.array(LOOP_QUERIES, np.int32)
        un = dev.unmasked(odesc[uq], uq)
        for i, qi in enumerate(uq):
            k = _pick(ref, qi, "unmasked")
            check_result(ref["ores"][k], un["res"][i], dev.tol, ("unmasked", qi))
        ku = np.array([_pick(ref, qi, "unmasked") for qi in uq])
        hits_equal(L, ref["oknn"][ku], ref["ocnt"][ku], un["knn"], un["knn_cnt"], "unmasked")
        out = dev.query(odesc[q], q, ref["table"], rows)
        for k in range(len(q)):
            check_result(ref["ores"][k], out["res"][k], dev.tol, (int(q[k]), ref["kind"][k]))
        hits_equal(L, ref["oknn"], ref["ocnt"], out["knn"], out["knn_cnt"], "masked")
        # the -1 rows of the mixed call are the unmasked call, byte for byte
        assert out["res"][ku].tobytes() == un["res"].tobytes()
        hits_equal(L, out["knn"][ku], out["knn_cnt"][ku], un["knn"], un["knn_cnt"], "rows of -1")
        n_full = 0
        for k in np.nonzero(rows >= 0)[0]:
            i = list(uq).index(q[k])
            n_full += check_properties(un["knn"][i], un["knn_cnt"][i], out["knn"][k], out["knn_cnt"][k], ref["table"][rows[k]], nnk,
                                       (int(q[k]), ref["kind"][k]))[1]
        if nnk == 50:
            assert n_full > 0
        return ref, un, out
    finally:
        dev.close()


# ---- case 2: the crowded layer ----
def crowded(oracle, n=450):
    from test_hostdb_bookkeeping import _fake_desc
    L = oracle.L
    rng = np.random.default_rng(21)
    desc = _fake_desc(L, rng, n)
    base = rng.uniform(8.0, 12.0, L.KEY_DIM).astype(np.float32)
    desc["keys"] = (base[None, None, None, :] + rng.normal(0, 0.05, (n, L.NLEV, L.NPIV, L.KEY_DIM))).astype(np.float32)
    q = desc[[3, 420]].copy()
    q["keys"] += np.float32(0.01)
    return desc, np.arange(n) * 0.1, np.arange(n, dtype=np.int32), q


def run_crowded(dev, oracle, nnk):
    """450 scans of near-identical keys, both queries at epoch 450: whole 64-key steps pass the radius and the pending buffer
    reaches its capacity.  Hit lists and counts against the filtered oracle's whole lists."""
    L = oracle.L
    n = 450
    desc, ts, seeds, q = crowded(oracle, n)
    dcfg = L.default_db_cfg()
    dcfg.nnk = nnk
    odb = masked_oracle.DB(dcfg)
    for i in range(n):
        odb.add(desc[i], ts[i], i)
    dev.open(dcfg, cap=n)
    try:
        dev.add(desc, ts, seeds)
        ep = np.full(2, n, np.int32)
        un = dev.unmasked(q, ep)
        # the nearest scans of query 0's first search, for the sets of nnk - 1, nnk and nnk + 1 scans
        ok0, oc0 = odb.query(q[0], 10000)[1:]
        assert oc0[0, 0] == nnk
        near = list(dict.fromkeys(ok0["gidx"][0, 0, :nnk].tolist()))
        rest = [g for g in range(n) if g not in set(near)]
        order = near + rest
        sets = [np.arange(n)[np.arange(n) % 2 == 0], [7], [31, 32, 33, 448, 449], order[:nnk - 1], order[:nnk], order[:nnk + 1], np.arange(n), []]
        a = np.zeros((len(sets), n), bool)
        for i, s in enumerate(sets):
            a[i, np.asarray(s, np.int64)] = True
        table = pack_rows(L, a, n)
        assert table.shape[1] == 15 and table[0, 0] == 0x55555555 and table[2, 14] == 0x3 and table[6, 14] == 0x3
        qi = np.repeat(np.arange(2), len(sets))
        rows = np.tile(np.arange(len(sets), dtype=np.int32), 2)
        out = dev.query(q[qi], np.full(len(qi), n, np.int32), table, rows)
        for k in range(len(qi)):
            _, oknn, ocnt = odb.query(q[qi[k]], 10000 + int(qi[k]), table[rows[k]])
            hits_equal(L, oknn, ocnt, out["knn"][k], out["knn_cnt"][k], ("crowded", k))
            check_properties(un["knn"][qi[k]], un["knn_cnt"][qi[k]], out["knn"][k], out["knn_cnt"][k], table[rows[k]], nnk, ("crowded", k))
        ones = np.nonzero(rows == 6)[0]
        hits_equal(L, out["knn"][ones], out["knn_cnt"][ones], un["knn"], un["knn_cnt"], "all ones")
        assert (out["knn_cnt"][np.nonzero(rows == 7)[0]] == 0).all()
        assert out["knn_cnt"][ones].min() == nnk
    finally:
        dev.close()
        odb.close()


# ---- case 3 on the unindexed-bucket fixture: the VIS instances, masked ----
def run_unindexed(dev, oracle):
    import os
    L = oracle.L
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_unindexed_bucket_fixture.npz"))
    n = len(z["ts"])
    desc = np.zeros(n, L.scan_desc_dt)
    desc["keys"] = z["keys"]
    d = L.default_db_cfg()
    cfg = z["cfg"]
    d.min_elapse, d.max_elapse, d.nnk, d.max_fine_opt, d.n_q_levels = cfg[0], cfg[1], int(cfg[2]), int(cfg[3]), int(cfg[4])
    for i in range(3):
        d.q_levels[i] = int(cfg[5 + i])
    dev.open(d, cap=n)
    try:
        dev.add(desc, z["ts"], z["seeds"])
        q = np.arange(52, n, dtype=np.int32)
        un = dev.unmasked(desc[q], q)
        assert np.array_equal(un["knn_cnt"], z["knn_cnt"][q]) and z["knn_cnt"][65, 0, 0] == 0
        a = np.array([np.arange(n) % 2 == 0, np.arange(n) % 3 != 0])
        table = pack_rows(L, a, n)
        rows = (np.arange(len(q)) % 2).astype(np.int32)
        out = dev.query(desc[q], q, table, rows)
        changed = 0
        for i in range(len(q)):
            check_properties(un["knn"][i], un["knn_cnt"][i], out["knn"][i], out["knn_cnt"][i], table[rows[i]], d.nnk, ("unindexed", int(q[i])))
            changed += int((out["knn_cnt"][i] != un["knn_cnt"][i]).any())
        assert changed > 0
    finally:
        dev.close()


# ---- case 6: cc_mask_gates ----
def gates_numpy(xy, gates, row_words):
    """the f32 restatement: dx = x_g - x_r; dy = y_g - y_r; dx * dx + dy * dy <= rad * rad, rad >= 0"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    gates = np.asarray(gates, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = xy[None, :, 0] - gates[:, None, 0]
        dy = xy[None, :, 1] - gates[:, None, 1]
        lhs = (dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)
        rad = gates[:, None, 2]
        inside = (lhs <= (rad * rad).astype(np.float32)) & (rad >= 0)
    return _pack(inside, row_words)


def _pack(inside, row_words):
    pad = np.zeros((inside.shape[0], 32 * row_words), bool)
    pad[:, :inside.shape[1]] = inside
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little").view("<u4").reshape(inside.shape[0], row_words))


def run_gates(dev):
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 64, 65, 450):
        for nr in (1, 3):
            for extra in (0, 2):
                rw = (n + 31) // 32 + extra
                xy = rng.uniform(-50, 50, (n, 2)).astype(np.float32)
                g = np.concatenate([rng.uniform(-50, 50, (nr, 2)), rng.uniform(5, 60, (nr, 1))], 1).astype(np.float32)
                got = dev.gates(xy, g, rw)
                want = gates_numpy(xy, g, rw)
                assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (n, nr, rw)
    # the special points
    xy = np.array([[3, 4], [0, 0], [3.0000002, 4], [np.nan, 0], [1, 1]], np.float32)
    got = dev.gates(xy, [[0, 0, 5], [0, 0, 0], [0, 0, -1], [0, 0, np.nan], [np.nan, 0, 100], [1, 1, 0]], 1)
    assert got.reshape(-1).tolist() == [0b10011, 0b00010, 0, 0, 0, 0b10000]
    assert got.tobytes() == gates_numpy(xy, [[0, 0, 5], [0, 0, 0], [0, 0, -1], [0, 0, np.nan], [np.nan, 0, 100], [1, 1, 0]], 1).tobytes()
    # refusals
    rc, msg = dev.gates(np.zeros((33, 2), np.float32), [[0, 0, 1]], 1, raw=True)
    assert rc == CC_EINVAL and "row_words" in msg
    rc, msg = dev.gates(np.zeros((3, 2), np.float32), [[0, 0, 1]], 0, raw=True)
    assert rc == CC_EINVAL
    assert dev.gates(np.zeros((3, 2), np.float32), [[0, 0, 1]], 1).tolist() == [[7]]


# ---- case 4: mixing ----
def _loop_db(dev, cc, oracle, nnk=50, lanes=None):
    ref = loop_reference(cc, oracle, nnk)
    dev.open(db_cfg(oracle.L, nnk), cap=ref["n"], lanes=lanes)
    dev.add(ref["odesc"], ref["ts"], ref["seeds"])
    return ref


def _same(a, b, keys=None):
    """two calls' outputs, byte for byte (the hit lists: up to their counts -- the entries behind them are never written)"""
    for k in (keys or a.keys()):
        assert a[k].shape == b[k].shape, k
        if k == "knn":
            hits_equal(None, a["knn"], a["knn_cnt"], b["knn"], b["knn_cnt"], "knn")
        else:
            assert a[k].tobytes() == b[k].tobytes(), k


def run_mixing(dev, cc, oracle):
    """Rows and -1 in one call, a shared row, the stored / packed / host forms, ranked lists with detail."""
    L = oracle.L
    ref = _loop_db(dev, cc, oracle)
    try:
        odesc, n = ref["odesc"], ref["n"]
        high = int(ref["rows"][_pick(ref, 57, "high")])
        nb37 = int(ref["rows"][_pick(ref, 37, "not_best")])
        q = np.array([37, 37, 57, 60, 33], np.int32)
        rows = np.array([-1, nb37, high, high, -1], np.int32)
        kinds = ["unmasked", "not_best", "high", "high", "unmasked"]
        un = dev.unmasked(odesc[q], q)
        out = dev.query(odesc[q], q, ref["table"], rows)
        for i in (0, 4):  # the -1 queries: the bytes of the unmasked call
            assert out["res"][i].tobytes() == un["res"][i].tobytes()
            hits_equal(L, out["knn"][i], out["knn_cnt"][i], un["knn"][i], un["knn_cnt"][i], "rows of -1")
        for i in range(len(q)):
            k = _pick(ref, int(q[i]), kinds[i])
            check_result(ref["ores"][k], out["res"][i], dev.tol, (int(q[i]), kinds[i]))
            hits_equal(L, ref["oknn"][k], ref["ocnt"][k], out["knn"][i], out["knn_cnt"][i], (int(q[i]), kinds[i]))
        assert out["res"]["cand_gidx"][1] == 17 and out["res"]["cand_gidx"][2] == 32
        # mask NULL: the unmasked call's bytes
        _same(dev.query(odesc[q], q, None, None), un)
        # the stored and packed forms: the bytes of the descriptor form
        _same(dev.query(None, q, ref["table"], rows, src="stored", rec=q), out)
        _same(dev.query(odesc[q], q, ref["table"], rows, src="packed"), out)
        # the host form (results only)
        h = dev.query(odesc[q], q, ref["table"], rows, host=True)
        assert h["res"].tobytes() == out["res"].tobytes()
        # ranked lists with detail: entry 0 is the masked answer, nobody names a masked-out scan
        rk = dev.query(odesc[q], q, ref["table"], rows, ranked=4, detail=True)
        assert rk["res"].tobytes() == out["res"].tobytes() and rk["detail"].shape == (len(q), 4)
        for i in range(len(q)):
            m = int(rk["rank_n"][i])
            assert (m > 0) == (out["res"]["n_res"][i] > 0)
            if m:
                assert rk["rank"]["cand_gidx"][i, 0] == out["res"]["cand_gidx"][i]
                assert rk["rank"]["correlation"][i, 0] == out["res"]["correlation"][i]
            if rows[i] >= 0:
                assert bit(ref["table"][rows[i]], rk["rank"]["cand_gidx"][i, :m]).all(), i
        assert rk["rank_n"].max() >= 1
    finally:
        dev.close()


def run_chunks(dev, cc, oracle, nq=130):
    """A call of 130 queries cut into several chunks (four lanes: three chunks of 64, 64 and 2; some of them with and some
    without a row) gives what calls of one chunk give.  The unindexed-bucket fixture's keys: the retrieval alone."""
    import os
    L = oracle.L
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_unindexed_bucket_fixture.npz"))
    n = len(z["ts"])
    desc = np.zeros(n, L.scan_desc_dt)
    desc["keys"] = z["keys"]
    d = L.default_db_cfg()
    cfg = z["cfg"]
    d.min_elapse, d.max_elapse, d.nnk, d.max_fine_opt, d.n_q_levels = cfg[0], cfg[1], int(cfg[2]), int(cfg[3]), int(cfg[4])
    for i in range(3):
        d.q_levels[i] = int(cfg[5 + i])
    dev.open(d, cap=n, lanes=4)
    try:
        dev.add(desc, z["ts"], z["seeds"])
        q = (np.arange(nq) * 7 % n).astype(np.int32)
        table = pack_rows(L, np.array([np.arange(n) % 2 == 0, np.arange(n) % 3 != 0, np.arange(n) < 40]), n)
        rows = (np.arange(nq) % 4 - 1).astype(np.int32)
        rows[64:128] = -1  # the second chunk names no row: the unmasked launches
        before = dev.knn_chunks()
        out = dev.query(desc[q], q, table, rows)
        after = dev.knn_chunks()
        assert after[2] - before[2] == 2 and sum(after) - sum(before) == 3, (before, after)
        for c0 in range(0, nq, 26):
            s = slice(c0, min(c0 + 26, nq))
            part = dev.query(desc[q[s]], q[s], table, rows[s])
            _same(part, {k: out[k][s] for k in ("res", "knn", "knn_cnt")})
        un = dev.unmasked(desc[q[64:128]], q[64:128])
        hits_equal(L, un["knn"], un["knn_cnt"], out["knn"][64:128], out["knn_cnt"][64:128], "the chunk without a row")
    finally:
        dev.close()


def run_tiled_mode(dev, cc, oracle):
    """CC_KNN_MODE=2 (set by the caller before the database exists): a masked call still walks and gives the masked answers,
    an unmasked call on the same handle still runs the tiled search."""
    L = oracle.L
    ref = _loop_db(dev, cc, oracle)
    try:
        odesc = ref["odesc"]
        q = np.array([37, 57], np.int32)
        kinds = ["not_best", "high"]
        rows = np.array([ref["rows"][_pick(ref, int(q[i]), kinds[i])] for i in range(2)], np.int32)
        c0 = dev.knn_chunks()
        out = dev.query(odesc[q], q, ref["table"], rows)
        c1 = dev.knn_chunks()
        assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (0, 0, 1)
        for i in range(2):
            k = _pick(ref, int(q[i]), kinds[i])
            check_result(ref["ores"][k], out["res"][i], dev.tol, (int(q[i]), kinds[i]))
            hits_equal(L, ref["oknn"][k], ref["ocnt"][k], out["knn"][i], out["knn_cnt"][i], (int(q[i]), kinds[i]))
        un = dev.unmasked(odesc[q], q)
        c2 = dev.knn_chunks()
        assert (c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]) == (0, 1, 0)
        for i in range(2):
            k = _pick(ref, int(q[i]), "unmasked")
            check_result(ref["ores"][k], un["res"][i], dev.tol, (int(q[i]), "unmasked"))
        # rows of -1 only: no query names a row, the chunk runs the unmasked (tiled) launches
        o2 = dev.query(odesc[q], q, ref["table"], np.full(2, -1, np.int32))
        c3 = dev.knn_chunks()
        assert c3[1] - c2[1] == 1 and c3[2] == c2[2]
        _same(o2, un)
    finally:
        dev.close()


# ---- case 5: refusals ----
def run_refusals(dev, cc, oracle):
    L = oracle.L
    ref = _loop_db(dev, cc, oracle)
    try:
        odesc = ref["odesc"]
        q = np.array([37, 57], np.int32)
        table = np.ascontiguousarray(ref["table"][:3])  # [3, 2]: 64 scans
        ptr = dev.table_ptr(table)
        ok_rows = np.array([0, -1], np.int32)

        def usable():
            out = dev.query(odesc[q], q, ref["table"], np.array([ref["rows"][_pick(ref, 37, "not_best")], -1], np.int32))
            assert out["res"]["cand_gidx"][0] == 17

        for what, args, word in (
                ("n_rows < 1", (ptr, 0, 2, ok_rows), "n_rows"),
                ("row_words < 1", (ptr, 3, 0, ok_rows), "row_words"),
                ("row too large", (ptr, 3, 2, np.array([3, -1], np.int32)), "h_row"),
                ("row below -1", (ptr, 3, 2, np.array([0, -2], np.int32)), "h_row"),
                ("row_words too small for the epoch", (ptr, 3, 1, ok_rows), "epoch"),
        ):
            rc, msg = dev.raw_rc(odesc[q], q, *args)
            assert rc == CC_EINVAL and word in msg, (what, rc, msg)
            usable()
        # 32 * row_words = 32 >= epoch 20 is enough for a query at epoch 20; the query without a row does not count
        rc, msg = dev.raw_rc(odesc[[20, 57]], np.array([20, 57], np.int32), ptr, 3, 1, ok_rows)
        assert rc == 0, msg
        # both or neither of d_qdesc and src
        rc, msg = dev.raw_rc(odesc[q], q, ptr, 3, 2, ok_rows, both=True)
        assert rc == CC_EINVAL and "exactly one" in msg
        rc, msg = dev.raw_rc(odesc[q], q, ptr, 3, 2, ok_rows, neither=True)
        assert rc == CC_EINVAL and "exactly one" in msg
        usable()
        # dynamic thresholds
        dev.set_dyn(1)
        rc, msg = dev.raw_rc(odesc[q], q, ptr, 3, 2, ok_rows)
        assert rc == CC_EINVAL and "dynamic" in msg, msg
        dev.set_dyn(0)
        usable()
    finally:
        dev.close()


# ---- case 6, end to end: a gate row through query(mask=) ----
def run_gate_end_to_end(dev, cc, oracle):
    """A gate mask built from the drive's poses for query 57 with a 6 m radius gives the answer of the same set passed as
    a host-packed table."""
    L = oracle.L
    ref = _loop_db(dev, cc, oracle)
    try:
        poses = np.asarray(ref["poses"], np.float64)
        xy = np.ascontiguousarray(poses[:, :2], np.float32)  # (x, y, theta) per scan
        assert xy.shape == (ref["n"], 2)
        gate = np.array([[xy[57, 0], xy[57, 1], 6.0]], np.float32)
        bits = dev.gates(xy, gate, 2)
        allowed = np.nonzero(bit(bits[0], np.arange(ref["n"])))[0]
        assert 57 in allowed and 0 < len(allowed) < ref["n"]
        table = pack_rows(L, [allowed], ref["n"])
        assert table.tobytes() == bits.tobytes()
        q = np.array([57], np.int32)
        a = dev.query_gate_bits(ref["odesc"][q], q, xy, gate, np.zeros(1, np.int32))
        b = dev.query(ref["odesc"][q], q, table, np.zeros(1, np.int32))
        _same(a, b, ("res", "knn", "knn_cnt"))
        un = dev.unmasked(ref["odesc"][q], q)
        check_properties(un["knn"][0], un["knn_cnt"][0], a["knn"][0], a["knn_cnt"][0], bits[0], 50, "gate")
    finally:
        dev.close()
