"""Randomised campaign of cc_db_verify_batch on the GPU (run by hand, not collected by pytest):
    python tests/fuzz_gpu_verify.py <seed0> <n_iter>
Per seed a random world and drive (64 scans), a database of its scans (nnk 50 or 128), and one batch of 16-48 items with random
candidate sets (the place a query revisits, its neighbours, unrelated scans; 0 to 8 per item, descriptors shared through qidx), a
random level mask, key-distance bound and max_fine_opt.  Three ways: the batch, the loop of cc_db_check_hints over the returned
hint lists (memcmp), and the oracle's hint flow on the same lists (integers equal, correlation and pose within 1e-4); the hint
lists themselves against the demo's loop in numpy wherever no key distance is within 1e-4 of the bound."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle"), HERE]
import cc_amd  # noqa: E402
import oracle_py as oracle  # noqa: E402
from test_emu_hints import INT_FIELDS  # noqa: E402


def _numpy_hints(L, hdesc, q, cands, mask, bound):
    """the demo's loop, candidate outermost -> (rows (cand, level, seq_src, seq_tgt), marginal: some distance sits at the bound)"""
    out, marginal = [], False
    for c in cands:
        for lv in (1, 2, 3, 4):
            if not (mask >> (lv - 1)) & 1:
                continue
            k1, k2 = hdesc["keys"][c][lv], hdesc["keys"][q][lv]
            for a in range(L.NPIV):
                for b in range(L.NPIV):
                    if k1[a].sum() == 0 or k2[b].sum() == 0:
                        continue
                    d = float(((k1[a].astype(np.float64) - k2[b].astype(np.float64)) ** 2).sum())
                    if np.isfinite(bound) and abs(d - bound) <= 1e-4 * bound:
                        marginal = True
                    if d > bound:
                        continue
                    out.append((c, lv, a, b))
    return out, marginal


def one(cc, seed):
    import torch
    L = cc.L
    rng = np.random.default_rng(seed)
    dcfg = L.default_db_cfg()
    dcfg.nnk = int(rng.choice([50, 128]))
    if rng.random() < 0.4:
        dcfg.cont_sim.ta_cell_cnt, dcfg.cont_sim.tp_cell_cnt = float(rng.uniform(3, 12)), float(rng.uniform(0.1, 0.4))
        dcfg.cont_sim.tp_eigval, dcfg.cont_sim.ta_h_bar = float(rng.uniform(0.1, 0.4)), float(rng.uniform(0.2, 0.8))
    kind = int(rng.integers(2))
    loop = float(rng.uniform(28, 44))
    w = cc.synth.World(loop_len=loop, dense=(kind == 1), seed=int(rng.integers(1 << 20)))
    n = 64
    full = rng.random() < 0.3
    x, poses, ts = cc.synth.make_sequence(n, world=w, device="cuda", **({} if full else dict(beams=16, azim=450)))
    ctx = cc.Context(0, max_batch=n)
    desc = ctx.ingest(x.reshape(-1, 4), np.arange(n + 1, dtype=np.int64) * x.shape[1])
    db = cc.Database(ctx, dcfg, capacity=n)
    db.add_scans(desc, ts, np.arange(n, dtype=np.int32))
    hdesc = cc.desc_to_numpy(desc).copy()
    mask = int(rng.integers(1, 16)) if rng.random() < 0.5 else 15
    bound = float(rng.choice([1000.0, float("inf"), float(rng.uniform(100, 3000))]))
    mfo = int(rng.choice([1, 2, 5, 10]))
    n_items = int(rng.integers(16, 49))
    qs = np.sort(rng.choice(np.arange(int(loop) + 2, n), min(8, n - int(loop) - 2), replace=False))
    qidx = rng.integers(0, len(qs), n_items).astype(np.int32)
    cands = []
    for i in range(n_items):
        qi = int(qs[qidx[i]])
        m = int(rng.integers(0, 9))
        pool = [qi - int(round(loop)) + d for d in (0, -1, 1)] + [int(v) for v in rng.integers(0, n, 8)]
        c = [g for g in dict.fromkeys(pool) if 0 <= g < n]
        if rng.random() < 0.3:
            c = [c[k] for k in rng.permutation(len(c))]
        cands.append(c[:m])
    qdesc = desc[torch.as_tensor(qs, device=desc.device)].contiguous()
    res, hl = db.verify(qdesc, cands, qidx=qidx, levels=[lv for lv in (1, 2, 3, 4) if (mask >> (lv - 1)) & 1], max_key_dist_sq=bound,
                        max_fine_opt=mfo, want_hints=True)
    bad = n_hints = n_closed = 0
    for i in range(n_items):
        qi = int(qs[qidx[i]])
        exp, marginal = _numpy_hints(L, hdesc, qi, cands[i], mask, bound)
        got = [(int(h["cand_gidx"]), int(h["level"]), int(h["seq_src"]), int(h["seq_tgt"])) for h in hl[i]]
        if not marginal and got != exp:
            print("  MISMATCH seed %d item %d: %d hints generated, the demo's loop gives %d" % (seed, i, len(got), len(exp)))
            bad += 1
        one_res, _ = db.check_hints(qdesc[int(qidx[i])], hl[i], max_fine_opt=mfo)
        if one_res.tobytes() != res[i].tobytes():
            print("  MISMATCH seed %d item %d: batch %s against cc_db_check_hints %s" % (seed, i, res[i], one_res))
            bad += 1
        n_hints += len(got)
        n_closed += int(res[i]["n_res"])
        if not got:
            continue
        where = {g: k for k, g in enumerate(cands[i])}
        oh = np.array([(where[g], lv, a, b) for (g, lv, a, b) in got], np.int32)
        eres, _ = oracle.check_hints(oracle.Scan.from_desc(hdesc[qi], int_id=qi), [oracle.Scan.from_desc(hdesc[g], int_id=int(g)) for g in cands[i]],
                                     oh, sim=dcfg.cont_sim, max_fine_opt=mfo)
        for f in INT_FIELDS:
            e = eres[f] if f != "cand_gidx" or eres["n_res"] == 0 else cands[i][int(eres[f])]
            if e != res[i][f]:
                print("  MISMATCH seed %d item %d field %s: oracle %s kernels %s" % (seed, i, f, e, res[i][f]))
                bad += 1
        if eres["n_res"] and res[i]["n_res"]:
            e = max(abs(eres["correlation"] - res[i]["correlation"]), float(np.abs(eres["tf"] - res[i]["tf"]).max()))
            if e > 1e-4:
                print("  MISMATCH seed %d item %d float error %.3g" % (seed, i, e))
                bad += 1
    print("seed %d kind %d%s nnk %d mask %d bound %g mfo %d items %d hints %d closed %d: %s" % (
        seed, kind, " full-size" if full else "", dcfg.nnk, mask, bound, mfo, n_items, n_hints, n_closed, "ok" if not bad else "%d MISMATCHES" % bad), flush=True)
    db.close()
    ctx.close()
    return bad


if __name__ == "__main__":
    s0, it = int(sys.argv[1]), int(sys.argv[2])
    cc = cc_amd.load()
    tot = 0
    for s in range(s0, s0 + it):
        tot += one(cc, s)
    print("done: %d mismatches" % tot)
