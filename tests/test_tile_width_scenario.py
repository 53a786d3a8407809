"""Preconditions of the tile-width runs of tests/test_gpu_tile_widths.py
(scenarios.py TILE_WIDTHS, tile_bounds, width_victims, width_churn), on the CPU
oracle alone, in the style of test_ragged_scenario.py. Part A of that module
demands the nibble path at 64- and 128-member tiles in the healthy and the
REMOVE rounds and looks for tier tombstones in the victims' columns: for every
victim set it crashes, the reference must detect every victim, make tombstones
the round after, and keep the views running rows hold of running members
inside the 4-bit tier's window (csrc/gh_internal.h c4_enc: lag <= 11, age <=
15) through round 29, the round before the rejoin. Part B's churn at N = 300
must put stopped rows, tombstones, absent cells and a column too wide for a
16-bit segment into the table. These are conditions on the inputs (they keep
the GPU tests from passing vacuously), not tolerances."""
import numpy as np
import pytest

import scenarios as sc
from test_ragged_scenario import ROUNDS, assert_wave, run_wave

THROUGH = sc.RAGGED_REJOIN - 1


def test_tile_bounds_and_victims():
    """The table of the victim sets: both sides of the first and of the last
    tile boundary of each width beside the tail members."""
    assert sc.tile_bounds(263, 64) == [64, 256] and sc.tile_bounds(263, 128) == [128, 256]
    assert sc.tile_bounds(1000, 64) == [64, 960] and sc.tile_bounds(1000, 128) == [128, 896]
    assert sc.tile_bounds(263, 256) == [256] and sc.tile_bounds(64, 64) == [] and sc.tile_bounds(300, 8) == [8, 296]
    assert sc.width_victims(263, 64) == [63, 64, 255, 256, 262]
    assert sc.width_victims(263, 128) == [127, 128, 255, 256, 262]
    assert sc.width_victims(1000, 64) == [63, 64, 767, 768, 959, 960, 992, 999]
    assert sc.width_victims(1000, 128) == [127, 128, 767, 768, 895, 896, 992, 999]
    assert sc.width_victims(263, 64, 3, 0) == [63, 64, 95, 96, 191, 192, 255, 256, 262]
    assert sc.width_victims(263, 128, 2, 1) == [127, 128, 131, 132, 255, 256, 262]
    for n in sc.WIDTH_NS:
        for tw in sc.TIER_WIDTHS:
            v = sc.width_victims(n, tw)
            assert all(b - 1 in v and b in v for b in sc.tile_bounds(n, tw)) and set(sc.tail_members(n)) <= set(v)
            assert n % tw and n % 16  # a partial last tile and a partial last lane
    assert sc.WIDTH_N % 8 and all(sc.WIDTH_N % tw for tw in sc.TILE_WIDTHS)


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("tw", sc.TIER_WIDTHS)
@pytest.mark.parametrize("n", sc.WIDTH_NS)
def test_width_wave_preconditions(oracle_mod, n, tw, k):
    """width_victims(n, tw) crashed at round 8, k = 3 and 4."""
    victims = sc.width_victims(n, tw)
    trace = run_wave(oracle_mod, n, sc.ragged_cfg(k), sc.ragged_wave(n, victims, rejoin=False))
    assert_wave(trace, victims, f"N={n} TW={tw} k={k}", through=THROUGH)


@pytest.mark.parametrize("label,world,layout", sc.WIDTH_SHARDS, ids=[x[0] for x in sc.WIDTH_SHARDS])
@pytest.mark.parametrize("tw", sc.TIER_WIDTHS)
def test_width_shard_preconditions(oracle_mod, tw, label, world, layout):
    """N = 263 on 3 column shards and 2 row shards: the victims also stand on
    both sides of every shard boundary."""
    n = 263
    bounds = sc.shard_bounds(n, world, layout) + sc.tile_bounds(n, tw)
    victims = sc.width_victims(n, tw, world, layout)
    assert all(b - 1 in victims and b in victims for b in bounds), (bounds, victims)
    trace = run_wave(oracle_mod, n, sc.ragged_cfg(4), sc.ragged_wave(n, victims, rejoin=False))
    assert_wave(trace, victims, f"{label}: N={n} TW={tw}", through=THROUGH)


@pytest.mark.parametrize("tw", sc.TIER_WIDTHS)
def test_width_counter_preconditions(oracle_mod, tw):
    """The same victims from the counter offset `f24` (heartbeats and rounds
    through 2^24), the wave shifted by R0."""
    n = 263
    h, r0 = sc.COUNTER_OFFSETS["f24"]
    victims = sc.width_victims(n, tw)
    trace = run_wave(oracle_mod, n, sc.ragged_cfg(4), sc.shifted_wave(n, r0, victims), ROUNDS, hb0=h, r0=r0)
    assert len(trace) == ROUNDS
    det, tomb = assert_wave(trace, victims, f"f24: N={n} TW={tw}", through=THROUGH)
    assert set(r for r in det if r < sc.RAGGED_REJOIN) <= {23, 24} and set(r for r in tomb if r < sc.RAGGED_REJOIN) <= {24, 25}


def test_width_quirk_victims():
    """The quirk runs reuse RAGGED_QUIRK[263] (test_ragged_scenario.py holds
    its preconditions): its run of candidates 254, 255, 256 crosses the last
    tile boundary of both widths."""
    v = sc.RAGGED_QUIRK[263]
    for tw in sc.TIER_WIDTHS:
        last = sc.tile_bounds(263, tw)[-1]
        assert last - 1 in v and last in v, (tw, v)


def test_width_churn_preconditions(oracle_mod):
    """Part B's churn at N = 300 from width_state: some round's table holds
    stopped rows, tombstones, absent cells in running rows, and the column
    whose views stand millions above its owner's own counter (no 16-bit
    segment holds both); detections, REMOVEs and releases all happen, and a
    stopped row and the last row exist for the gh_lsm probes."""
    n, rounds = sc.WIDTH_N, 30
    cfg, sched = sc.width_churn(n, rounds)
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    seen = dict(stopped=0, tombs=0, absent=0, wide=0, det=0, tombstoned=0, released=0)
    try:
        orc.import_state(*sc.width_state(n), 0)
        for r in range(1, rounds + 1):
            if sched.get(r):
                orc.apply_events(sched[r])
            st = orc.step(1)
            hb, ts, alive = orc.export_state()
            run = alive != 0
            seen["stopped"] += int((~run).sum() > 0)
            seen["tombs"] += int((hb[run] == -2).any())
            seen["absent"] += int((hb[run] == -1).any())
            col = hb[:, n - 3].astype(np.int64)
            seen["wide"] += int(col[col >= 0].max() - col[col >= 0].min() > 2**16) if (col >= 0).any() else 0
            seen["det"] += st["detections"]
            seen["tombstoned"] += st["tombstoned"]
            seen["released"] += st["released"]
    finally:
        orc.close()
    print(f"N={n} churn: rounds with (stopped rows, tombstones, absent cells, the wide column), totals: {seen}")
    assert all(v > 0 for v in seen.values()), seen
    assert seen["stopped"] >= rounds // 2 and seen["tombs"] >= rounds // 2 and seen["wide"] >= 1, seen
