"""K4 (csrc/k_check.h) on built scans, on the MI355X through the Python package (constell_cases.py): every scene is one
cc_db_check_hints call whose per-hint scores, pass records (cc_db_debug_passes) and result record are held against the oracle
(R1) and, up to the individual similarity, against the numpy restatement (R2).

The hint flow runs the 64-stride kernels (cc_k_check_a, cc_k_check_b1<64 | 256>, cc_k_check_b2, cc_k_merge); the large-k
instances are not reached from here.  Which B1 instance and which rank variant a case takes follows from its pair count alone
(profiles/k4_constell/scenes.txt); nothing the kernels return names them."""
import numpy as np
import pytest

import constell_cases as K

pytestmark = pytest.mark.gpu

_state = {}
PARTS = ["A gate", "A rings", "A classes", "A shapes", "B deep", "B sort/", "B sort, capped", "C window", "C cap", "D b2", "D acos", "D nrm"]


class GpuBack:
    name = "MI355X"

    def __init__(self, cc):
        import torch
        self.cc, self.L, self.torch = cc, cc.L, torch
        self.ctx = cc.Context(0, max_batch=2)
        descs = K.database(self.L)
        self.db = cc.Database(self.ctx, self.L.default_db_cfg(), capacity=len(descs))
        self.db.add_scans(self._tensor(descs), np.arange(len(descs)) * 100.0, np.arange(len(descs), dtype=np.int32))
        self.q = {}

    def _tensor(self, desc):
        desc = np.ascontiguousarray(desc).reshape(-1)
        return self.torch.from_numpy(np.frombuffer(desc.tobytes(), np.uint8).reshape(len(desc), self.cc.DESC_BYTES).copy()).cuda()

    def hints(self, sc, h, lb, ub):
        lib, db, q, stream = self.raw(sc)
        out = K.raw_hints(lib, db, q, h, lb, ub, self.L, stream)
        self.torch.cuda.synchronize()
        return out

    def cands(self):
        return K.raw_cands(self.cc.lib(), self.db.h, self.L)

    def raw(self, sc):
        key = id(sc.share or sc)
        if key not in self.q:
            self.q[key] = self._tensor(sc.tgt)
        q = self.q[key]
        return self.cc.lib(), self.db.h, q.data_ptr(), self.torch.cuda.current_stream(q.device).cuda_stream

    def sync(self):
        self.torch.cuda.synchronize()

    def dynamic(self, on):
        self.db.set_dynamic_thres(on)

    def verify(self, qdesc, qidx, cands):
        res, hints = self.db.verify(self._tensor(qdesc), cands, qidx=qidx, max_key_dist_sq=float("inf"), want_hints=True, allow_flagged=True)
        self.torch.cuda.synchronize()
        return res, hints


def back(cc):
    if "B" not in _state:
        _state["B"] = GpuBack(cc)
    return _state["B"]


@pytest.mark.parametrize("part", PARTS)
def test_scenes(cc, oracle, part):
    log = []
    sel = [sc for sc in K.scenes(cc.L) if sc.name.startswith(part)]
    assert sel
    for sc in sel:
        K.check_scene(back(cc), cc.L, oracle, sc, log)
    print("\n".join(log))


def test_merge(cc, oracle):
    """E: every candidate's merged proposal through cc_db_debug_cands against the oracle's export"""
    log = []
    for sc in K.merge_scenes(cc.L):
        K.check_merge(back(cc), cc.L, oracle, sc, log)
    print("\n".join(log))


def test_getter_against_ranked_detail(cc, oracle):
    sel = [sc for sc in K.merge_scenes(cc.L) if sc.name in ("E proposals", "E 65 candidates")]
    assert [K.check_ranked_entries(back(cc), cc.L, oracle, sc) for sc in sel] == [10, 16]


def test_batch(cc, oracle):
    """F, on 100 items"""
    log = []
    K.check_batch(back(cc), cc.L, oracle, 100, log)
    print("\n".join(log))


def test_table_under_dynamic_thresholds(cc, oracle):
    log = []
    assert K.check_dynamic(back(cc), cc.L, oracle, log) >= 25
    print("\n".join(log))
