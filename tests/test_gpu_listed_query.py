"""Listed queries on the MI355X (Database.query(among=), ScanLists; cc_k_knn_list / cc_k_knn_list_l): the shared cases of
tests/listed_cases.py through the Python API against the masked call (mask=ScanMask.from_allowed of the same lists), byte for
byte, and against the filtered oracle (tests/masked_oracle.py), correlation and pose within 1e-4."""
import ctypes as C

import numpy as np
import pytest

import listed_cases as LC
from test_gpu_masked_query import GpuDev as MaskedGpuDev

pytestmark = pytest.mark.gpu


class GpuDev(MaskedGpuDev):
    """The adapter of tests/listed_cases.py over the Python API (and, for the refusals and the host form, the C-ABI)."""

    def ask(self, qdesc, epochs, table=None, rows=None, lists=None, want_knn=True, ranked=None, detail=False, matches=None, src="desc", rec=None):
        cc = self.cc
        if src == "desc":
            q = self._t(qdesc)
        elif src == "stored":
            q = self.db.stored(rec)
        else:
            hot, feat = self.ctx.pack(self._t(qdesc))
            q = cc.Packed(hot, feat, rec)
        among = None if lists is None else cc.ScanLists.from_lists(lists, rows)
        o = self.db.query(q, epochs, want_knn=want_knn, ranked=ranked, detail=detail, matches=matches, mask=self._mask(table, rows), among=among)
        out = self._pack_out(o, want_knn, ranked, detail)
        if matches is not None:
            out["match"] = o[-1]
        return out

    def _lists_c(self, idx, off, n_lists, rows):
        a = [None if x is None else np.ascontiguousarray(x, np.int32) for x in (idx, off, rows)]
        self.keep.append(a)
        return self.L.ScanListsC(*[None if x is None else x.ctypes.data for x in a[:2]], n_lists, None if a[2] is None else a[2].ctypes.data)

    def ask_host(self, qdesc, epochs, lists, rows):
        L, lib = self.L, self.cc.lib()
        lb, ub = L.default_thresholds()
        qd = np.ascontiguousarray(qdesc)
        epochs = np.ascontiguousarray(epochs, np.int32)
        res = np.zeros(len(epochs), L.query_result_dt)
        idx, off = LC.flat(lists)
        c = self._lists_c(idx, off, len(lists), rows)
        rc = lib.cc_db_query_batch_host_listed(self.db.h, qd.ctypes.data, len(epochs), epochs.ctypes.data, C.addressof(lb), C.addressof(ub),
                                               res.ctypes.data, None, None, C.addressof(c), None)
        assert rc == 0, lib.cc_last_error()
        return {"res": res}

    def raw_rc_listed(self, qdesc, epochs, idx, off, n_lists, rows, both=False, neither=False, null=False):
        L, lib = self.L, self.cc.lib()
        lb, ub = L.default_thresholds()
        qd = self._t(qdesc)
        epochs = np.ascontiguousarray(epochs, np.int32)
        res = np.zeros(len(epochs), L.query_result_dt)
        c = None if null else self._lists_c(idx, off, n_lists, rows)
        own = L.PackedSrc(None, None, 0, 0)
        rc = lib.cc_db_query_submit_listed(self.db.h, None if neither else qd.data_ptr(), C.addressof(own) if both else None, None, len(epochs),
                                           epochs.ctypes.data, C.addressof(lb), C.addressof(ub), res.ctypes.data, None, None, None, None, None,
                                           None if c is None else C.addressof(c), None)
        msg = lib.cc_last_error().decode()
        self.db.query_wait()
        return rc, msg, res

    def ask_null(self, qdesc, epochs):
        rc, msg, res = self.raw_rc_listed(qdesc, epochs, None, None, 0, None, null=True)
        assert rc == 0, msg
        return res

    def listed_chunks(self):
        out = np.zeros(2, np.int64)
        assert self.cc.lib().cc_db_debug_knn_chunks_listed(self.db.h, out.ctypes.data) == 0
        return out.tolist()

    def bucket_ranges(self):
        sizes, rg = np.zeros((3, 6), np.int32), np.zeros((3, 7), np.float32)
        assert self.cc.lib().cc_db_bucket_state(self.db.h, sizes.ctypes.data, rg.ctypes.data) == 0
        return rg


@pytest.fixture()
def dev(cc):
    d = GpuDev(cc)
    yield d
    d.close()


@pytest.mark.parametrize("nnk", [50, 128])
def test_loop_drive_listed(cc, oracle, dev, nnk):
    """The loop drive at its own epochs, both KM instances: the oracle, the masked call, the list of every scan below the epoch."""
    LC.run_loop_drive(dev, cc, oracle, nnk)


@pytest.mark.parametrize("nnk", [50, 200])
def test_crowded_layer_listed(oracle, dev, nnk):
    """Allowed-key counts around the two reductions, list lengths around the 64-scan steps, a scan without a key."""
    LC.run_crowded(dev, oracle, nnk)


def test_longest_list(oracle, dev):
    LC.run_longest_list(dev, oracle)


@pytest.mark.parametrize("nnk", [None, 128])
def test_unindexed_buckets_listed(oracle, dev, nnk):
    """The VIS instances: at the fixture's own nnk (KM 64) and at 128 (cc_k_knn_list_l<true>)."""
    LC.run_unindexed(dev, oracle, nnk)


def test_visible_buckets(cc, oracle, dev):
    LC.run_buckets(dev, cc, oracle)


def test_mixing(cc, oracle, dev):
    LC.run_mixing(dev, cc, oracle)


def test_chunks_over_lanes(cc, oracle, dev):
    LC.run_chunks(dev, cc, oracle, nq=130)


def test_tiled_mode_mixed_chunk(cc, oracle, dev, monkeypatch):
    monkeypatch.setenv("CC_KNN_MODE", "2")
    LC.run_tiled_mode(dev, cc, oracle)


def test_refusals(cc, oracle, dev):
    LC.run_refusals(dev, cc, oracle)


def test_among_and_mask_together_are_refused(cc, oracle, dev):
    ref = LC.M._loop_db(dev, cc, oracle)
    q = np.array([37], np.int32)
    d = dev._t(ref["odesc"][q])
    with pytest.raises(ValueError, match="not both"):
        dev.db.query(d, q, mask=dev._mask(ref["table"], np.zeros(1, np.int32)), among=cc.ScanLists.from_lists([[1, 2]]))
    with pytest.raises(TypeError):
        dev.db.query(d, q, among=[[1, 2]])
    res = dev.db.query(d, q, among=cc.ScanLists.from_lists([np.arange(37)]))  # the handle answers afterwards
    assert res["cand_gidx"][0] == 0


def test_query_submit_among(cc, oracle, dev):
    """query_submit(among=) + query_wait(): the lists are read before the submit returns (the arrays may go), the answers are query(among=)'s."""
    ref = LC.M._loop_db(dev, cc, oracle)
    n = ref["n"]
    lists = LC.lists_of(ref["table"], n)
    q = np.array([37, 57], np.int32)
    rows = np.array([ref["rows"][LC.M._pick(ref, 37, "not_best")], ref["rows"][LC.M._pick(ref, 57, "high")]], np.int32)
    d = dev._t(ref["odesc"][q])
    want = dev.db.query(d, q, among=cc.ScanLists.from_lists(lists, rows))
    a = cc.ScanLists.from_lists(lists, rows)
    res = dev.db.query_submit(d, q, among=a)
    a.idx[:] = -7  # (overwritten after the submit: the library has staged what it needs)
    dev.db.query_wait()
    assert res.tobytes() == want.tobytes() and res["cand_gidx"].tolist() == [17, 32]


def test_from_gates_lists_are_the_gate_masks_bits(cc, dev):
    """ScanLists.from_gates against Context.gate_mask on the device, to the bit; then a gate list through query(among=)."""
    import torch
    dev.open(cc.L.default_db_cfg(), cap=4)
    rng = np.random.default_rng(5)
    for n, nr in ((1, 1), (33, 3), (450, 3)):
        xy = rng.uniform(-50, 50, (n, 2)).astype(np.float32)
        g = np.concatenate([rng.uniform(-50, 50, (nr, 2)), rng.uniform(5, 60, (nr, 1))], 1).astype(np.float32)
        bits = dev.gates(xy, g, (n + 31) // 32)
        sl = cc.ScanLists.from_gates(torch.from_numpy(xy).cuda(), g)
        for r, l in enumerate(sl.lists()):
            assert l.tolist() == np.nonzero(LC.M.bit(bits[r], np.arange(n)))[0].tolist(), (n, r)


def test_gate_lists_end_to_end(cc, oracle, dev):
    ref = LC.M._loop_db(dev, cc, oracle)
    xy = np.ascontiguousarray(np.asarray(ref["poses"], np.float64)[:, :2], np.float32)
    gate = np.array([[xy[57, 0], xy[57, 1], 6.0]], np.float32)
    q = np.array([57], np.int32)
    a = dev.ask(ref["odesc"][q], q, lists=cc.ScanLists.from_gates(xy, gate).lists(), rows=np.zeros(1, np.int32))
    b = dev.query_gate_bits(ref["odesc"][q], q, xy, gate, np.zeros(1, np.int32))
    LC.same(a, b, "gate lists against the gate mask", ("res", "knn", "knn_cnt"))
