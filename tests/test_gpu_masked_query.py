"""Masked queries on the MI355X (Database.query(mask=), ScanMask, Context.gate_mask; cc_k_knn_m / cc_k_knn_lm /
cc_k_mask_gates): the shared cases of tests/masked_cases.py against the filtered oracle (tests/masked_oracle.py), correlation
and pose within 1e-4."""
import ctypes as C

import numpy as np
import pytest

import masked_cases as M

pytestmark = pytest.mark.gpu


class GpuDev:
    """The adapter of tests/masked_cases.py over the Python API (and, for the refusals and the host form, the C-ABI)."""
    tol = 1e-4

    def __init__(self, cc):
        self.cc, self.L = cc, cc.L
        self.ctx = self.db = None
        self.keep = []

    def open(self, dcfg, cap, lanes=None, dyn=False):
        self.ctx = self.cc.Context(0, max_batch=8)
        self.db = self.cc.Database(self.ctx, dcfg, capacity=cap)
        if lanes is not None:
            self.db.set_lanes(lanes)
        if dyn:
            self.db.set_dynamic_thres(True)
        return self

    def close(self):
        import torch
        if self.db is not None:
            torch.cuda.synchronize()
            self.db.close()
            self.ctx.close()
            self.db = self.ctx = None
        self.keep = []

    def _t(self, desc):
        import torch
        d = np.ascontiguousarray(desc)
        return torch.from_numpy(d.view(np.uint8).reshape(len(d), -1)).cuda()

    def add(self, desc, ts, seeds):
        self.db.add_scans(self._t(desc), ts, seeds)

    def set_dyn(self, on):
        self.db.set_dynamic_thres(bool(on))

    def knn_chunks(self):
        out = np.zeros(3, np.int64)
        assert self.cc.lib().cc_db_debug_knn_chunks(self.db.h, out.ctypes.data) == 0
        return out.tolist()

    def _mask(self, table, rows):
        import torch
        if table is None:
            return None
        table = np.ascontiguousarray(table, np.uint32)
        allowed = np.unpackbits(table.view(np.uint8), axis=1, bitorder="little").astype(bool)  # [n_rows, 32 * row_words]
        m = self.cc.ScanMask.from_allowed(allowed, rows)
        assert m.bits.cpu().numpy().view(np.uint32).tobytes() == table.tobytes()
        return m

    @staticmethod
    def _pack_out(o, want_knn, ranked, detail):
        o = o if isinstance(o, tuple) else (o,)
        out = {"res": o[0]}
        i = 1
        if want_knn:
            out["knn"], out["knn_cnt"] = o[1], o[2]
            i = 3
        if ranked is not None:
            out["rank"], out["rank_n"] = o[i]
            i += 1
        if detail:
            out["detail"] = o[i]
        return out

    def query(self, qdesc, epochs, table=None, rows=None, want_knn=True, ranked=None, detail=False, src="desc", rec=None, host=False):
        cc, L = self.cc, self.L
        if host:
            return self._host(qdesc, epochs, table, rows, ranked, detail)
        if src == "desc":
            q = self._t(qdesc)
        elif src == "stored":
            q = self.db.stored(rec)
        else:
            hot, feat = self.ctx.pack(self._t(qdesc))
            q = cc.Packed(hot, feat, rec)
        o = self.db.query(q, epochs, want_knn=want_knn, ranked=ranked, detail=detail, mask=self._mask(table, rows))
        return self._pack_out(o, want_knn, ranked, detail)

    def unmasked(self, qdesc, epochs, want_knn=True, ranked=None, detail=False):
        o = self.db.query(self._t(qdesc), epochs, want_knn=want_knn, ranked=ranked, detail=detail)
        return self._pack_out(o, want_knn, ranked, detail)

    def _host(self, qdesc, epochs, table, rows, ranked, detail):
        L, lib = self.L, self.cc.lib()
        lb, ub = L.default_thresholds()
        qd = np.ascontiguousarray(qdesc)
        epochs = np.ascontiguousarray(epochs, np.int32)
        res = np.zeros(len(epochs), L.query_result_dt)
        table = np.ascontiguousarray(table, np.uint32)
        rows = np.ascontiguousarray(rows, np.int32)
        m = L.ScanMaskC(table.ctypes.data, table.shape[0], table.shape[1], rows.ctypes.data)
        rc = lib.cc_db_query_batch_host_masked(self.db.h, qd.ctypes.data, len(epochs), epochs.ctypes.data, C.addressof(lb), C.addressof(ub),
                                               res.ctypes.data, None, None, C.addressof(m))
        assert rc == 0, lib.cc_last_error()
        return {"res": res}

    def table_ptr(self, table):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(table, np.uint32).view(np.int32)).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def raw_rc(self, qdesc, epochs, bits_ptr, n_rows, row_words, rows, both=False, neither=False):
        L, lib = self.L, self.cc.lib()
        lb, ub = L.default_thresholds()
        qd = self._t(qdesc)
        epochs = np.ascontiguousarray(epochs, np.int32)
        rows = np.ascontiguousarray(rows, np.int32)
        res = np.zeros(len(epochs), L.query_result_dt)
        m = L.ScanMaskC(bits_ptr, n_rows, row_words, rows.ctypes.data)
        own = L.PackedSrc(None, None, 0, 0)
        rc = lib.cc_db_query_submit_masked(self.db.h, None if neither else qd.data_ptr(), C.addressof(own) if both else None, None, len(epochs),
                                           epochs.ctypes.data, C.addressof(lb), C.addressof(ub), res.ctypes.data, None, None, None, None, None,
                                           C.addressof(m))
        msg = lib.cc_last_error().decode()
        self.db.query_wait()
        return rc, msg

    def gates(self, xy, gates, row_words, n_scans=None, raw=False):
        import torch
        xy = torch.from_numpy(np.ascontiguousarray(xy, np.float32).reshape(-1, 2)).cuda()
        g = torch.from_numpy(np.ascontiguousarray(gates, np.float32).reshape(-1, 3)).cuda()
        if raw:
            try:
                self.ctx.gate_mask(xy, g, row_words)
            except self.cc.CCError as e:
                return e.rc, str(e)
            return 0, ""
        bits = self.ctx.gate_mask(xy, g, row_words)
        torch.cuda.synchronize()
        return bits.cpu().numpy().view(np.uint32)

    def query_gate_bits(self, qdesc, epochs, xy, gate, rows):
        import torch
        bits = self.ctx.gate_mask(torch.from_numpy(np.ascontiguousarray(xy, np.float32)).cuda(),
                                  torch.from_numpy(np.ascontiguousarray(gate, np.float32)).cuda())
        o = self.db.query(self._t(qdesc), epochs, want_knn=True, mask=self.cc.ScanMask(bits, rows))
        return self._pack_out(o, True, None, False)


@pytest.fixture()
def dev(cc):
    d = GpuDev(cc)
    yield d
    d.close()


@pytest.mark.parametrize("nnk", [50, 128])
def test_loop_drive_matches_the_filtered_oracle(cc, oracle, dev, nnk):
    """Case 1 and the properties of case 3 on it: cc_k_knn_m / cc_k_knn_lm."""
    M.run_loop_drive(dev, cc, oracle, nnk)


@pytest.mark.parametrize("nnk", [50, 200])
def test_crowded_layer_matches_the_filtered_oracle(oracle, dev, nnk):
    """Case 2: whole 64-key steps pass the radius, the pending buffer reaches its capacity."""
    M.run_crowded(dev, oracle, nnk)


def test_unindexed_buckets_masked(oracle, dev):
    """Case 3 on the unindexed-bucket fixture: the VIS instances run masked."""
    M.run_unindexed(dev, oracle)


def test_mixing(cc, oracle, dev):
    M.run_mixing(dev, cc, oracle)


def test_chunks_over_lanes(cc, oracle, dev):
    M.run_chunks(dev, cc, oracle, nq=130)


def test_tiled_mode_masked_chunks_walk(cc, oracle, dev, monkeypatch):
    monkeypatch.setenv("CC_KNN_MODE", "2")
    M.run_tiled_mode(dev, cc, oracle)


def test_refusals(cc, oracle, dev):
    M.run_refusals(dev, cc, oracle)


def test_mask_gates(cc, dev):
    dev.open(cc.L.default_db_cfg(), cap=4)
    M.run_gates(dev)


def test_gate_mask_end_to_end(cc, oracle, dev):
    M.run_gate_end_to_end(dev, cc, oracle)


def test_query_submit_keeps_the_mask_alive(cc, oracle, dev):
    """query_submit(mask=) + query_wait(): the pending list holds the mask until the wait; the answers are query(mask=)'s."""
    ref = M._loop_db(dev, cc, oracle)
    q = np.array([37, 57], np.int32)
    rows = np.array([ref["rows"][M._pick(ref, 37, "not_best")], ref["rows"][M._pick(ref, 57, "high")]], np.int32)
    d = dev._t(ref["odesc"][q])
    want = dev.db.query(d, q, mask=dev._mask(ref["table"], rows))
    res = dev.db.query_submit(d, q, mask=dev._mask(ref["table"], rows))
    assert any(isinstance(p, tuple) and any(isinstance(x, cc.ScanMask) for x in p[0]) for p in dev.db._pending)
    dev.db.query_wait()
    assert res.tobytes() == want.tobytes() and res["cand_gidx"].tolist() == [17, 32]


def test_from_allowed_packs_like_the_table(cc):
    import torch
    a = np.zeros((2, 70), bool)
    a[0, [0, 31, 32, 69]] = True
    m = cc.ScanMask.from_allowed(a)
    m2 = cc.ScanMask.from_allowed([[0, 31, 32, 69], []], n_db=70)
    assert m.bits.shape == (2, 3) and torch.equal(m.bits, m2.bits) and m.rows.tolist() == [0, 1]
    assert m.bits.cpu().numpy().view(np.uint32).tolist() == [[0x80000001, 1, 1 << 5], [0, 0, 0]]
