"""The matched contour pairs behind each ranked entry (include/cont2_amd_matches.h: cc_k_merge_m / cc_k_merge_lm, cc_k_match_emit /
cc_k_match_emit_l) on the MI355X: the cases of match_cases.py on device databases made through the Python API, and
Database.query / query_submit / check_hints / verify with matches=inlier_px held to the same rows."""
import numpy as np
import pytest

import constell_cases as K
import match_cases as M
import ranked_common as RC
from test_emu_large_nnk import _db_cfg

pytestmark = pytest.mark.gpu

_state = {}


def _tensor(a):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


class GpuBack:
    """a cc.Database and what match_cases.py needs of it"""
    stream = None

    def __init__(self, cc, desc, ts, seeds, dcfg, lanes=None, dyn=False):
        self.cc, self.L, self.lib = cc, cc.L, cc.lib()
        if "ctx" not in _state:
            _state["ctx"] = cc.Context(0, max_batch=16)
        self.ctx = _state["ctx"]
        self.d = _tensor(desc).reshape(len(desc), cc.DESC_BYTES)
        self.dbo = cc.Database(self.ctx, dcfg, capacity=len(desc))
        if lanes is not None:
            self.dbo.set_lanes(lanes)
        self.dbo.add_scans(self.d, ts, seeds)
        if dyn:
            self.dbo.set_dynamic_thres(True)
        self.db = self.dbo.h
        self.keep, self.outs = [], {}

    def dev(self, a):
        t = _tensor(a)
        self.keep.append(t)
        return t.data_ptr()

    def dev_out(self, a):
        import torch
        t = torch.zeros(a.nbytes, dtype=torch.uint8, device="cuda")
        self.outs[id(a)] = t
        self.keep.append((a, t))
        return t.data_ptr()

    def fetch(self, a):
        self.sync()
        a.view(np.uint8).reshape(-1)[...] = self.outs.pop(id(a)).cpu().numpy()
        return a

    def sync(self):
        import torch
        torch.cuda.synchronize()


def scenes_back(cc):
    if "E" not in _state:
        d = K.database(cc.L)
        _state["E"] = GpuBack(cc, d, np.arange(len(d)) * 100.0, np.arange(len(d), dtype=np.int32), cc.L.default_db_cfg())
    return _state["E"]


def drive_back(cc, oracle, key="nnk 50", **kw):
    if key not in _state:
        desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
        _state[key] = GpuBack(cc, desc, ts, seeds, _db_cfg(cc.L, 128) if key == "nnk 128" else dcfg, **kw)
    return _state[key]


def test_merge_scenes(cc, oracle):
    """case 1"""
    log = []
    st = M.check_merge_scenes(scenes_back(cc), cc.L, oracle, log)
    print("\n".join(log))
    assert st["merged"] >= 1 and st["multi"] >= 5


def test_bit_edges(cc, oracle):
    """case 2"""
    M.check_bit_edges(scenes_back(cc), cc.L, oracle)


@pytest.mark.parametrize("key", ["nnk 50", "nnk 128"])
def test_drive(cc, oracle, key):
    """case 3 (nnk 128: the large-k instances) with case 4's tolerance on every entry"""
    B = drive_back(cc, oracle, key)
    assert B.dbo.knn_stride == (256 if key == "nnk 128" else 64)
    M.check_drive(B, cc, oracle, key)


def test_inlier_bars(cc, oracle):
    """case 4"""
    M.check_bars(scenes_back(cc), cc.L, oracle)


def test_nothing_else_moves(cc, oracle):
    """case 5"""
    M.check_nothing_else_moves(drive_back(cc, oracle), cc, oracle, "nnk 50")


def test_forms(cc, oracle):
    """case 6: stored, packed, masked and host forms"""
    B = drive_back(cc, oracle)
    hot, feat = B.ctx.pack(B.d)
    B.keep.append((hot, feat))
    B.sync()
    M.check_forms(B, cc, oracle, "nnk 50", (hot.data_ptr(), feat.data_ptr(), int(hot.shape[0])))


def test_verify(cc, oracle):
    """case 6: one item of eight candidates"""
    M.check_verify(scenes_back(cc), cc.L, oracle)


def test_four_lanes(cc, oracle):
    """case 6: 130 queries over four lanes, max_ret 1, 4 and 16"""
    _, ref = M.drive_reference(drive_back(cc, oracle), cc, oracle, "nnk 50")
    M.check_lanes(drive_back(cc, oracle, "four lanes", lanes=4), cc, oracle, ref)


def test_refusals(cc, oracle):
    """case 7"""
    M.check_refusals(drive_back(cc, oracle), cc, oracle, drive_back(cc, oracle, "dynamic", dyn=True))


def test_python_api(cc, oracle):
    """Database.query / query_submit / check_hints / verify / verify_submit with matches=: one more array, the rows of the calls above;
    with db.stored(...), Packed(...), mask= and detail=True; cc.match_pairs"""
    import torch
    L = cc.L
    desc, ts, seeds, dcfg, ores = RC.drive(cc, oracle)
    B = drive_back(cc, oracle)
    db, d = B.dbo, B.d
    _, ref = M.drive_reference(B, cc, oracle, "nnk 50")
    res, (cands, n), rows = db.query(d, seeds, ranked=16, matches=0.0)
    M.same(res, ref.res, "query: res")
    M.same(cands, ref.rank[0], "query: lists")
    M.same(rows, ref.match, "query: match rows")
    assert rows.dtype == L.ranked_match_dt and rows.shape == (64, 16)
    qs = np.array([36, 38, 40, 41], np.int32)
    want = np.ascontiguousarray(ref.match[qs])
    out = db.query(d[qs.tolist()].contiguous(), qs, want_knn=True, ranked=16, detail=True, matches=0.0)
    assert len(out) == 6
    M.same(out[5], want, "query with every option")
    M.same(out[4], np.ascontiguousarray(ref.detail[qs]), "detail beside matches")
    M.same(db.query(db.stored(qs), qs, ranked=16, matches=0.0)[2], want, "stored")
    hot, feat = B.ctx.pack(d)
    M.same(db.query(cc.Packed(hot, feat, qs), qs, ranked=16, matches=0.0)[2], want, "packed")
    mask = cc.ScanMask(torch.full((1, 2), -1, dtype=torch.int32, device="cuda"), np.zeros(len(qs), np.int32))
    M.same(db.query(d[qs.tolist()].contiguous(), qs, ranked=16, matches=0.0, mask=mask)[2], want, "masked (every scan allowed)")
    sub = db.query_submit(d[qs.tolist()].contiguous(), qs, ranked=16, matches=0.0)
    db.query_wait()
    M.same(sub[2], want, "query_submit")
    q = int(qs[1])
    hints = RC.to_hint_dt(L, RC.hints_of_knn(L, ref.knn[q], ref.kcnt[q]))
    r1, sc, (c1, n1), m1 = db.check_hints(d[q], hints, max_fine_opt=dcfg.max_fine_opt, ranked=16, matches=0.0)
    assert n1[0] == ref.rank[1][q] > 0
    M.same(m1[0], ref.match[q], "check_hints")
    pairs = cc.match_pairs(m1[0, 0])
    assert pairs.dtype == np.int8 and pairs.shape == (int(m1[0, 0]["n_pairs"]), 3) and (np.diff(pairs[:, 0] * 100 + pairs[:, 1] * 10 + pairs[:, 2]) > 0).all()
    items = [[int(g) for g in c1[0]["cand_gidx"][:int(n1[0])]][:8]]
    v = db.verify(d[q:q + 1].contiguous(), items, ranked=16, matches=0.0)
    vs = db.verify_submit(d[q:q + 1].contiguous(), items, ranked=16, matches=0.0)
    db.query_wait()
    M.same(vs[2], v[2], "verify_submit")
    assert v[1][1][0] == int((v[2][0]["n_pairs"] > 0).sum()) and v[2].shape == (1, 16)
    with pytest.raises(ValueError):
        db.query(d[qs.tolist()].contiguous(), qs, matches=1.0)
