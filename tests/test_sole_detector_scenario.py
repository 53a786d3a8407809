"""Preconditions of the sole-detector REMOVE scenario (scenarios.py
sole_detector_state), on the CPU oracle alone: the GPU parity test
test_gpu_rows.py::test_sole_detector_remove_rows is only worth its name if,
in the reference, round D detects every crashed member once, round D + 1
delivers REMOVEs to rows that do not know the member, and rows on another
row shard than the sole detector merge the member back from it. This is a
condition on the inputs (it keeps the GPU test from passing vacuously), not
a tolerance."""
import numpy as np
import pytest

import scenarios as sc


def sole_merges(n, world, det, before, after, alive):
    """(cells, columns): cells (i, c) absent before the round and present
    after it, row i alive, not c's detector j, and owned by another row shard
    than j (shard = i // ceil(n / world))."""
    nrs = -(-n // world)
    shard = np.arange(n) // nrs
    cells = cols = 0
    for c, j in det.items():
        new = (before[:, c] == -1) & (after[:, c] >= 0) & (alive != 0) & (shard != j // nrs)
        new[j] = False
        cells += int(new.sum())
        cols += bool(new.any())
    return cells, cols


@pytest.mark.parametrize("world,seed,lead,p", sc.SOLE_CASES)
def test_sole_detector_preconditions(oracle_mod, world, seed, lead, p):
    n, r0, n_cols = sc.SOLE_N, sc.SOLE_R0, 32
    hb, ts, alive, det = sc.sole_detector_state(n, world, seed, n_cols=n_cols, p=p, r0=r0, lead=lead)
    assert len(det) == n_cols and 0 not in det and all(alive[j] and not alive[c] for c, j in det.items())
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **sc.sole_detector_cfg(seed)), threads=8)
    try:
        orc.import_state(hb, ts, alive, r0)
        d_round = r0 + 1 + lead
        for r in range(r0 + 1, d_round):
            assert orc.step(1)["detections"] == 0, r
        st = orc.step(1)  # round D: each crashed member detected by its one detector
        assert st["last_round"] == d_round and st["detections"] == n_cols, st
        failed = np.flatnonzero(np.unpackbits(orc.read_failed().view(np.uint8), bitorder="little"))
        assert failed.tolist() == sorted(det), st
        assert sorted(orc.read_detectors().tolist()) == sorted(set(det.values())), st
        before = orc.export_state()[0].copy()
        st = orc.step(1)  # round D + 1: REMOVE to everyone but the detector
        after, _, al = orc.export_state()
        assert st["remove_unknown"] > 0 and st["tombstoned"] > 0, st
        cells, cols = sole_merges(n, world, det, before, after, al)
        print(f"world {world} seed {seed} lead {lead} p {p}: {cells} cells in {cols} columns merge from a sole "
              f"detector on another row shard; {st}")
        assert cells >= 5 and cols >= 3, (cells, cols)
    finally:
        orc.close()
