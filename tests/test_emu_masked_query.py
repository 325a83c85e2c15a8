"""Masked queries on the CPU harness (cc_db_query_submit_masked, cc_db_query_batch_host_masked, cc_mask_gates): the shared cases
of tests/masked_cases.py against the filtered oracle (tests/masked_oracle.py), correlation and pose within 1e-6."""
import numpy as np
import pytest

import masked_cases as M


@pytest.fixture()
def dev(oracle):
    d = M.EmuDev(oracle.L)
    yield d
    d.close()


def test_masked_oracle_all_ones_is_the_oracle(cc, oracle):
    """The filtered oracle with an all-ones row reproduces oracle.run_sequence's integer fields for all 64 scans of the drive."""
    import masked_oracle
    L = oracle.L
    n, ts, seeds, odesc, poses, ores_all = M.loop_drive(cc, oracle)
    ores = ores_all[50]
    odb = masked_oracle.DB(M.db_cfg(L, 50))
    ones = np.full(2, 0xFFFFFFFF, np.uint32)
    for i in range(n):
        r, _, cnt = odb.query(odesc[i], int(seeds[i]), ones)
        for f in M.INT_FIELDS:
            assert r[f] == ores[f][i], (i, f)
        assert cnt.sum() == ores["n_knn_hits"][i]
        odb.add(odesc[i], ts[i], int(seeds[i]))
    odb.close()


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
    """Case 4 on the harness."""
    M.run_mixing(dev, cc, oracle)


def test_chunks_over_lanes(cc, oracle, dev):
    M.run_chunks(dev, cc, oracle, nq=130)


def test_tiled_mode_masked_chunks_walk(cc, oracle, dev, monkeypatch):
    monkeypatch.setenv("CC_KNN_MODE", "2")
    M.run_tiled_mode(dev, cc, oracle)


def test_refusals(cc, oracle, dev):
    """Case 5: every CC_EINVAL of the masked submit; the handle stays usable."""
    M.run_refusals(dev, cc, oracle)


def test_mask_gates(oracle, dev):
    """Case 6: cc_k_mask_gates against the numpy f32 restatement, to the bit."""
    dev.open(oracle.L.default_db_cfg(), cap=4)
    M.run_gates(dev)


def test_gate_mask_end_to_end(cc, oracle, dev):
    M.run_gate_end_to_end(dev, cc, oracle)
