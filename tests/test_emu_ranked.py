"""The ranked list of a query's refined candidates (the *_ranked entry points, cc_k_final_r) on the CPU harness: against the
oracle peeled candidate by candidate (ranked_common.py), against the plain calls' results byte for byte, over the hint and
verify flows, across chunks and lanes, under dynamic thresholds, and every refusal."""
import ctypes as C

import numpy as np

import ranked_common as RC
from test_dyn_thres_oracle import INT_FIELDS
from emu_api import calls
from test_emu_verify import Verify

EINVAL = -1
_state = {}


class Ranked(Verify):
    """ctypes helper for the five *_ranked entry points on the harness ("device" pointers are host pointers there)."""

    @staticmethod
    def p(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    @staticmethod
    def b(s):
        return None if s is None else C.cast(C.byref(s), C.c_void_p)

    def query(self, qdesc, epochs, k, submit=False, lb=None, ub=None):
        """-> (results, cands [n, k], counts [n]); with submit valid after api.db_query_wait"""
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        if submit:
            self.keep.append(qdesc)
            r = calls.query(self.lib, self.db, epochs, qdesc=qdesc.ctypes.data, lb=lb, ub=ub, ranked=k, wait=False, keep=self.keep)
            return (r.res,) + r.rank
        if lb is None:
            lb, ub = L.default_thresholds()
        epochs = np.ascontiguousarray(epochs, np.int32)
        res = np.zeros(len(qdesc), L.query_result_dt)
        cands, cnt, ro = L.rank_buffers(len(qdesc), k)
        rc = self.lib.cc_db_query_batch_host_ranked(self.db, self.p(qdesc), len(qdesc), self.p(epochs), self.b(lb), self.b(ub), self.p(res), self.b(ro))
        self.api.chk(rc, "ranked query")
        return res, cands, cnt

    def hints(self, qdesc, hints, k, mfo=10):
        """cc_db_check_hints_ranked with h_scores NULL, a form calls.check_hints does not have"""
        L = self.L
        lb, ub = L.default_thresholds()
        qdesc = np.ascontiguousarray(qdesc)
        hints = np.ascontiguousarray(hints, L.hint_dt)
        res = np.zeros(1, L.query_result_dt)
        cands, cnt, ro = L.rank_buffers(1, k)
        rc = self.lib.cc_db_check_hints_ranked(self.db, self.p(qdesc), self.p(hints), len(hints), self.b(lb), self.b(ub), int(mfo), self.p(res), None,
                                               None, self.b(ro))
        self.api.chk(rc, "cc_db_check_hints_ranked")
        return res[0], cands, cnt

    def verify(self, qdesc, cand_lists, k, qidx=None, mfo=10, submit=False, bound=1000.0):
        """-> (results, cands [n, k], counts [n], hint lists); the synchronous form is submit + wait"""
        L = self.L
        qdesc = np.ascontiguousarray(qdesc)
        n = len(cand_lists)
        hints = np.zeros((max(n, 1), L.HINT_MAX), L.hint_dt)
        hcnt = np.zeros(max(n, 1), np.int32)
        self.keep.append((qdesc, hints, hcnt))
        r = calls.verify(self.lib, self.db, cand_lists, qdesc=qdesc.ctypes.data, n_desc=len(qdesc), qidx=qidx, levels=None, max_fine_opt=mfo,
                         max_key_dist_sq=bound, hints=hints.ctypes.data, n_hints=hcnt.ctypes.data, ranked=k, wait=not submit, keep=self.keep)
        return (r.res,) + r.rank + ((hints, hcnt),)


def ranked_setup(cc, oracle):
    """one harness database of the drive and its plain + ranked answers at every scan's own epoch, computed once per session"""
    if not _state:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        v = Ranked(oracle.L, desc, ts, seeds, dcfg)
        plain, knn, cnt = v.api.db_query(v.db, desc, seeds, want_knn=True)
        r16 = v.query(desc, seeds, 16)
        _state.update(v=v, plain=plain, knn=knn, cnt=cnt, r16=r16)
    return _state["v"], _state["plain"], _state["knn"], _state["cnt"], _state["r16"]


def eligible(cc, oracle, plain, knn, cnt):
    """the drive's queries with 2 .. max_fine_opt survivors for which peeling is valid -> {q: peeled list}"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    out = {}
    for q in np.nonzero((ores["n_cand_tidy"] >= 2) & (ores["n_cand_tidy"] <= dcfg.max_fine_opt))[0]:
        lst, _ = RC.peel_query(cc, oracle, int(q), knn[q], cnt[q], key="drive")
        if lst is not None:
            out[int(q)] = lst
    return out


def test_abi_layout(cc):
    """sizeof(cc_ranked_cand_t) == 40, the numpy record has the C struct's offsets, cc_rank_out_t is two pointers and two ints"""
    import os
    import subprocess
    import tempfile
    L = cc.L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "cont2_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", '
           'sizeof(cc_ranked_cand_t), offsetof(cc_ranked_cand_t, cand_gidx), offsetof(cc_ranked_cand_t, flags), offsetof(cc_ranked_cand_t, correlation), '
           'offsetof(cc_ranked_cand_t, tf), sizeof(cc_rank_out_t), offsetof(cc_rank_out_t, h_cands), offsetof(cc_rank_out_t, h_n), '
           'offsetof(cc_rank_out_t, max_ret), CC_RANK_MAX); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(td, "t")]).split()]
    dt = L.ranked_cand_dt
    assert got == [40, dt.fields["cand_gidx"][1], dt.fields["flags"][1], dt.fields["correlation"][1], dt.fields["tf"][1],
                   C.sizeof(L.RankOut), L.RankOut.h_cands.offset, L.RankOut.h_n.offset, L.RankOut.max_ret.offset, L.RANK_MAX], got
    assert dt.itemsize == 40 and got[1:5] == [0, 4, 8, 16] and L.RANK_MAX == RC.K == 16


def test_query_lists_structure_and_peeled_oracle(cc, oracle):
    """Part A"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, plain, knn, cnt, (res, cands, n) = ranked_setup(cc, oracle)
    assert res.tobytes() == plain.tobytes(), "h_res of the ranked call differs from the plain call's"
    for f in INT_FIELDS:
        assert np.array_equal(res[f], ores[f]), f
    RC.check_structure(L, res, cands, n, 16, dcfg.max_fine_opt)
    assert int((n >= 2).sum()) >= 20, "the drive should give many queries several survivors"
    # a shorter list is the prefix of the longer one
    sub = np.nonzero(ores["n_cand_tidy"] >= 2)[0][:12]
    r3, c3, n3 = v.query(desc[sub], seeds[sub], 3)
    assert r3.tobytes() == plain[sub].tobytes()
    RC.check_structure(L, r3, c3, n3, 3, dcfg.max_fine_opt)
    assert np.array_equal(n3, np.minimum(n[sub], 3)) and c3.tobytes() == np.ascontiguousarray(cands[sub][:, :3]).tobytes()
    # against the oracle, peeled
    el = eligible(cc, oracle, plain, knn, cnt)
    for q, lst in el.items():
        RC.check_against_peeled(cands[q], int(n[q]), lst, ("query", q))
    assert len(el) >= 5 and sum(len(x) >= 4 for x in el.values()) >= 3, {q: len(x) for q, x in el.items()}


def test_hint_and_verify_flows(cc, oracle):
    """Part B"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, plain, knn, cnt, _ = ranked_setup(cc, oracle)
    el = eligible(cc, oracle, plain, knn, cnt)
    # the hint flow on the queries' own kNN hits: the lists of the query path, and the peeled oracle's
    n_cmp = 0
    for q, lst in list(el.items())[:5]:
        hints = RC.to_hint_dt(L, RC.hints_of_knn(L, knn[q], cnt[q]))
        one, _ = v.api.check_hints(v.db, desc[q:q + 1], hints, max_fine_opt=dcfg.max_fine_opt)
        r, c, n = v.hints(desc[q:q + 1], hints, 16, mfo=dcfg.max_fine_opt)
        assert r.tobytes() == one.tobytes()
        RC.check_structure(L, np.array([r]), c, n, 16, dcfg.max_fine_opt)
        RC.check_against_peeled(c[0], int(n[0]), lst, ("hints", q))
        n_cmp += 1
    assert n_cmp >= 3
    # verification of [0, 1, 2, 3] for queries 38-40: one item lists every candidate; the hint flow on the generated list
    # gives the same bytes; both match the oracle peeled on that list
    qs = [38, 39, 40]
    res, c, n, (hl, hc) = v.verify(desc[qs], [[0, 1, 2, 3]] * 3 + [[]], 16, qidx=[0, 1, 2, 1], mfo=5)
    ref, _ = v.run(desc[qs], [[0, 1, 2, 3]] * 3 + [[]], qidx=[0, 1, 2, 1], mfo=5)
    assert res.tobytes() == ref.tobytes()
    RC.check_structure(L, res, c, n, 16, 5)
    assert n[3] == 0 and res[3]["n_res"] == 0, "an item with an empty list has no entries"
    n_multi = 0
    for i, q in enumerate(qs):
        h = hl[i, :hc[i]]
        r1, c1, n1 = v.hints(desc[q:q + 1], h, 16, mfo=5)
        assert r1.tobytes() == res[i].tobytes() and c1.tobytes() == c[i:i + 1].tobytes() and n1[0] == n[i]
        hints = np.stack([h["cand_gidx"], h["level"], h["seq_src"], h["seq_tgt"]], 1).astype(np.int32)
        lst, first = RC.peel(oracle, desc, dcfg, q, hints, 5)
        assert int(first["n_cand_tidy"]) <= 5 and all(lst[k][1] - lst[k + 1][1] > RC.TIE_GAP for k in range(len(lst) - 1)), (q, lst)
        RC.check_against_peeled(c[i], int(n[i]), lst, ("verify", q))
        n_multi += int(n[i] >= 2)
    assert n_multi >= 2, "the verify items should list several candidates each"


def test_chunks_lanes_and_streaming(cc, oracle):
    """Part C: lists of a chunk that starts at b0 > 0, and of chunks submitted around a plain batch, equal one synchronous call's"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, plain, knn, cnt, (res, cands, n) = ranked_setup(cc, oracle)
    # 64 queries that see an empty database, then eight with lists: two lanes cut the batch at 64, so the lists are chunk 2's
    tail = np.array([36, 37, 38, 39, 40, 41, 48, 54], np.int32)
    qd = np.concatenate([desc[:1].repeat(64), desc[tail]])
    ep = np.concatenate([np.zeros(64, np.int32), tail])
    rb, cb, nb = v.query(qd, ep, 16)
    assert not rb["n_res"][:64].any() and not nb[:64].any() and not cb[:64].tobytes().strip(b"\0")
    assert rb[64:].tobytes() == plain[tail].tobytes() and cb[64:].tobytes() == np.ascontiguousarray(cands[tail]).tobytes()
    assert np.array_equal(nb[64:], n[tail]) and nb[64:].min() >= 2
    # the same eight in two halves, a plain batch between them, everything collected by one wait (max_ret differs per half)
    a1 = v.query(desc[tail[:4]], tail[:4], 16, submit=True)
    aq, keep = v.api.db_query_submit(v.db, desc[58:], seeds[58:])
    a2 = v.query(desc[tail[4:]], tail[4:], 5, submit=True)
    v.api.db_query_wait(v.db)
    assert a1[0].tobytes() == plain[tail[:4]].tobytes() and a2[0].tobytes() == plain[tail[4:]].tobytes() and aq.tobytes() == plain[58:].tobytes()
    assert a1[1].tobytes() == np.ascontiguousarray(cands[tail[:4]]).tobytes() and np.array_equal(a1[2], n[tail[:4]])
    assert a2[1].tobytes() == np.ascontiguousarray(cands[tail[4:]][:, :5]).tobytes() and np.array_equal(a2[2], np.minimum(n[tail[4:]], 5))
    # 192 queries over two lanes: a chunk above the zero-copy limit (its lists are copied out beside the results) and one below
    big = np.arange(64, dtype=np.int32).repeat(3)
    rg, cg, ng = v.query(desc[big], big, 16)
    assert rg.tobytes() == plain[big].tobytes() and cg.tobytes() == np.ascontiguousarray(cands[big]).tobytes() and np.array_equal(ng, n[big])
    # a plain chunk on a lane that carried a ranked one delivers no list: the buffers of the earlier call stay as they are
    before = (a1[1].tobytes(), a2[1].tobytes())
    again = v.api.db_query(v.db, desc[tail], tail)
    assert again.tobytes() == plain[tail].tobytes() and (a1[1].tobytes(), a2[1].tobytes()) == before


def test_dynamic_thresholds(cc, oracle):
    """Part D: structure and h_res identity (the bars depend on the candidates before: peeling is not valid)"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v = Ranked(L, desc, ts, seeds, dcfg)
    assert v.lib.cc_db_set_dynamic_thres(v.db, 1) == 0
    qs = np.arange(34, 58, dtype=np.int32)
    plain = v.api.db_query(v.db, desc[qs], qs)
    res, c, n = v.query(desc[qs], qs, 16)
    assert res.tobytes() == plain.tobytes()
    RC.check_structure(L, res, c, n, 16, dcfg.max_fine_opt)
    assert int((n >= 2).sum()) >= 5


def test_refusals(cc, oracle):
    """Part E: a refused call queues nothing, leaves the handle usable and a chunk in flight untouched"""
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    L = oracle.L
    v, plain, knn, cnt, (res16, cands16, n16) = ranked_setup(cc, oracle)
    lb, ub = L.default_thresholds()
    q = np.array([38, 40], np.int32)
    qd = np.ascontiguousarray(desc[q])
    res = np.zeros(2, L.query_result_dt)
    good = L.rank_buffers(2, 16)
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, knn[38], cnt[38]))
    tab = v.table([[0, 1], [2]])
    cfg = L.VerifyCfg(0, 5, 1000.0, 0)
    p, b = v.p, v.b

    def bad_ranks():
        cands, cnt_, _ = good
        yield "rank NULL", None
        yield "h_cands NULL", L.RankOut(None, cnt_.ctypes.data, 16, 0)
        yield "h_n NULL", L.RankOut(cands.ctypes.data, None, 16, 0)
        yield "max_ret 0", L.RankOut(cands.ctypes.data, cnt_.ctypes.data, 0, 0)
        yield "max_ret -1", L.RankOut(cands.ctypes.data, cnt_.ctypes.data, -1, 0)
        yield "max_ret 17", L.RankOut(cands.ctypes.data, cnt_.ctypes.data, 17, 0)

    def calls(ro):
        r = b(ro)
        yield "submit", v.lib.cc_db_query_submit_ranked(v.db, p(qd), 2, p(q), b(lb), b(ub), p(res), None, None, None, r)
        yield "batch_host", v.lib.cc_db_query_batch_host_ranked(v.db, p(qd), 2, p(q), b(lb), b(ub), p(res), r)
        yield "scan_batch", v.lib.cc_db_query_scan_batch_submit_ranked(v.db, None, 1, p(q), b(lb), b(ub), p(res), r)
        yield "verify", v.lib.cc_db_verify_submit_ranked(v.db, p(qd), 2, None, p(tab), 2, b(cfg), b(lb), b(ub), p(res), None, None, None, r)
        yield "hints", v.lib.cc_db_check_hints_ranked(v.db, p(qd), p(hints), len(hints), b(lb), b(ub), 5, p(res), None, None, r)

    # a ranked chunk in flight while every refusal is made: collected afterwards with the right answer
    pend = v.query(qd, q, 16, submit=True)
    for what, ro in bad_ranks():
        for fn, rc in calls(ro):
            assert rc == EINVAL, (what, fn, rc)
    # what the plain calls refuse, the ranked ones refuse too (and before anything is queued)
    _, _, ro = good
    bad_ub = L.Score.from_buffer_copy(bytes(ub))
    bad_ub.i_ovlp_sum = lb.i_ovlp_sum
    assert v.lib.cc_db_query_submit_ranked(v.db, p(qd), 2, p(q), b(lb), b(bad_ub), p(res), None, None, None, b(ro)) == EINVAL
    assert v.lib.cc_db_query_batch_host_ranked(v.db, p(qd), 2, p(q), b(lb), b(bad_ub), p(res), b(ro)) == EINVAL
    assert v.lib.cc_db_query_batch_host_ranked(v.db, p(qd), 2, p(np.array([38, 65], np.int32)), b(lb), b(ub), p(res), b(ro)) == EINVAL
    assert v.lib.cc_db_query_batch_host_ranked(v.db, None, 2, p(q), b(lb), b(ub), p(res), b(ro)) == EINVAL
    assert v.lib.cc_db_verify_submit_ranked(v.db, p(qd), 2, None, p(v.table([[0, 0], [2]])), 2, b(cfg), b(lb), b(ub), p(res), None, None, None,
                                            b(ro)) == EINVAL
    # the scan-batch call on a VALID handle (the plain call refuses a NULL handle array whatever `rank` holds): every bad rank, and
    # thresholds that fail lb.strictSmaller(ub), which the ranked call tests before the handles are gathered
    x, _, _ = cc.synth.make_sequence(64, world=cc.synth.World(loop_len=40.0), beams=16, azim=450)
    pts = np.ascontiguousarray(x[38].numpy().reshape(-1, 4), np.float32)
    h = C.c_void_p()
    v.api.chk(v.lib.cc_scan_ingest(v.ctx, p(pts), len(pts), 0, C.byref(h)), "cc_scan_ingest")
    hs = (C.c_void_p * 1)(h)
    scan_fn = v.lib.cc_db_query_scan_batch_submit_ranked
    for what, bad in bad_ranks():
        assert scan_fn(v.db, hs, 1, p(q), b(lb), b(ub), p(res), b(bad)) == EINVAL, what
    assert scan_fn(v.db, hs, 1, p(q), b(lb), b(bad_ub), p(res), b(ro)) == EINVAL
    assert b"cc_db_query_scan_batch_submit_ranked: thresholds" in v.lib.cc_last_error()
    assert not res.tobytes().strip(b"\0") and not good[0].tobytes().strip(b"\0") and not good[1].any(), "a refused call wrote an answer"
    v.api.db_query_wait(v.db)
    assert pend[0].tobytes() == plain[q].tobytes() and pend[1].tobytes() == np.ascontiguousarray(cands16[q]).tobytes()
    assert np.array_equal(pend[2], n16[q])
    after = v.api.db_query(v.db, desc[q], q)
    assert after.tobytes() == plain[q].tobytes()
    # ... and the same handle, well-formed: the list of the batch call on the descriptors (the harness ingests the oracle's descriptor)
    one = np.zeros(1, L.query_result_dt)
    c1, n1, ro1 = L.rank_buffers(1, 16)
    v.api.chk(scan_fn(v.db, hs, 1, p(q), b(lb), b(ub), p(one), b(ro1)), "cc_db_query_scan_batch_submit_ranked")
    v.api.db_query_wait(v.db)
    assert one.tobytes() == plain[38:39].tobytes() and c1.tobytes() == np.ascontiguousarray(cands16[38:39]).tobytes() and n1[0] == n16[38]
    v.lib.cc_scan_release(h)
