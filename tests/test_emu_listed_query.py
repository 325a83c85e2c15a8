"""Listed queries on the CPU harness (cc_db_query_submit_listed, cc_db_query_batch_host_listed; cc_k_knn_list / cc_k_knn_list_l run by
tests/emu unchanged): the shared cases of tests/listed_cases.py against the masked call, byte for byte, and against the filtered
oracle (tests/masked_oracle.py), correlation and pose within 1e-6."""
import numpy as np
import pytest

import listed_cases as LC


@pytest.fixture()
def dev(oracle):
    d = LC.EmuDev(oracle.L)
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


def test_gate_lists_are_the_gate_masks_bits(cc, oracle, dev):
    """layouts.gate_lists (what ScanLists.from_gates runs) against cc_mask_gates on the harness, to the bit -- the special points of
    masked_cases.run_gates among them."""
    L = oracle.L
    dev.open(L.default_db_cfg(), cap=4)
    rng = np.random.default_rng(5)
    cases = [(rng.uniform(-50, 50, (n, 2)).astype(np.float32),
              np.concatenate([rng.uniform(-50, 50, (nr, 2)), rng.uniform(5, 60, (nr, 1))], 1).astype(np.float32)) for n in (1, 33, 450) for nr in (1, 3)]
    cases.append((np.array([[3, 4], [0, 0], [3.0000002, 4], [np.nan, 0], [1, 1]], np.float32),
                  np.array([[0, 0, 5], [0, 0, 0], [0, 0, -1], [0, 0, np.nan], [np.nan, 0, 100], [1, 1, 0]], np.float32)))
    for xy, g in cases:
        bits = dev.gates(xy, g, (len(xy) + 31) // 32)
        idx, off = L.gate_lists(xy, g)
        assert idx.dtype == np.int32 and off.dtype == np.int32 and len(off) == len(g) + 1
        for r in range(len(g)):
            assert idx[off[r]:off[r + 1]].tolist() == np.nonzero(LC.M.bit(bits[r], np.arange(len(xy))))[0].tolist(), r
