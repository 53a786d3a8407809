"""Preconditions of the ragged-N runs of tests/test_gpu_ragged.py (sizes that
are no multiple of the nibble path's 256-member tile; scenarios.py
tail_members, ragged_wave), on the CPU oracle alone. The GPU tests demand the
nibble path in the healthy and the REMOVE rounds and look for tier tombstones
in the victims' columns; that is only fair, and only worth its name, if in
the reference every victim is detected, REMOVE'd and released inside the run
and the views of the running members stay inside the 4-bit tier's window
(csrc/gh_internal.h c4_enc: lag <= 11, age <= 15) in every round. The quirk
schedule must make quirk detection differ from canonical detection. These
are conditions on the inputs (they keep the GPU tests from passing
vacuously), not tolerances."""
import numpy as np
import pytest

import scenarios as sc

ROUNDS = 44        # past the releases (and the second detection at N = 2,049)
LAG_MAX, AGE_MAX = 11, 15


def failed_of(orc):
    return set(np.flatnonzero(np.unpackbits(orc.read_failed().view(np.uint8), bitorder="little")).tolist())


def run_wave(om, n, cfg, sched, rounds=ROUNDS, hb0=2, r0=0):
    """The schedule on the oracle from full membership (heartbeat hb0, imported
    at round r0; `sched` is keyed by the rounds r0 + 1 ..): per round (stats,
    the failed set, max lag, max age), lag and age over the views running rows
    hold of running members. A round the oracle refuses (GH_ERANGE: an own
    counter at INT32_MAX) ends the trace."""
    orc = om.Oracle(om.default_config(n, **cfg), threads=8)
    out = []
    try:
        orc.import_state(*sc.full_state(n, hb0=hb0, ts0=r0), r0)
        for r in range(r0 + 1, r0 + rounds + 1):
            if sched.get(r):
                orc.apply_events(sched[r])
            rc, st = orc.step_rc(1)
            if rc != 0:
                assert rc == om.GH_ERANGE and st["rounds"] == 0, (r, rc, st)
                break
            hb, ts, alive = orc.export_state()
            run = alive != 0
            own = hb.diagonal().astype(np.int64)
            views = run[:, None] & run[None, :] & (hb >= 0)
            lag = int(np.where(views, own[None, :] - hb, 0).max())
            age = int(np.where(views, r - ts.astype(np.int64), 0).max())
            out.append((st, failed_of(orc), lag, age))
    finally:
        orc.close()
    return out


def assert_wave(trace, victims, what, released=True, through=None):
    """Every victim detected, tombstones the round after a detection, releases
    later; the running members' views inside the tier's window every round
    (through round `through`, where given). Rounds count from the import."""
    det_rounds = [r for r, (_, failed, _, _) in enumerate(trace, 1) if failed]
    seen = set().union(*(failed for _, failed, _, _ in trace))
    assert set(victims) <= seen, (what, sorted(set(victims) - seen))
    d = det_rounds[0]
    assert sc.RAGGED_CRASH < d < sc.RAGGED_REJOIN, (what, det_rounds)
    tomb = [r for r, (st, _, _, _) in enumerate(trace, 1) if st["tombstoned"] > 0]
    assert d + 1 in tomb, (what, det_rounds, tomb)
    if released:
        assert any(st["released"] > 0 for st, _, _, _ in trace[d + 1:]), what
    window = trace[:through]
    lag, age = max(x[2] for x in window), max(x[3] for x in window)
    print(f"{what}: detection {det_rounds}, REMOVE {tomb}, max lag {lag}, max age {age}")
    assert lag <= LAG_MAX and age <= AGE_MAX, (what, lag, age)
    return det_rounds, tomb


def test_tail_members():
    """The table of the sizes' tail members, and the shard boundaries."""
    assert {n: sc.tail_members(n) for n in sc.RAGGED_NS} == {
        250: [240, 248, 249], 263: [255, 256, 262], 520: [511, 512, 519], 1000: [767, 768, 992, 999],
        2049: [2047, 2048]}
    assert sc.tail_members(256) == [240, 248, 255] and sc.tail_members(9) == [8] and sc.tail_members(1) == []
    assert sc.shard_bounds(263, 2) == [160] and sc.shard_bounds(263, 3) == [96, 192]
    assert sc.shard_bounds(250, 8) == list(range(32, 250, 32)) and 250 - 7 * 32 == 26
    assert sc.shard_bounds(263, 2, 1) == [132] and sc.shard_bounds(263, 3, 1) == [88, 176]
    assert sc.shard_bounds(1000, 3, 1) == [334, 668]
    assert sc.tail_members(263, [160]) == [159, 160, 255, 256, 262]
    assert all(0 < x < n for n in sc.RAGGED_NS for x in sc.tail_members(n, [0, n]))


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("n", sc.RAGGED_NS)
def test_ragged_wave_preconditions(oracle_mod, n, k):
    """tail_members(n) crashed at round 8, k = 3 and 4."""
    victims = sc.tail_members(n)
    trace = run_wave(oracle_mod, n, sc.ragged_cfg(k), sc.ragged_wave(n, rejoin=False))
    det, tomb = assert_wave(trace, victims, f"N={n} k={k}")
    if n == 2049:
        # a victim is detected once more, by one row, long after the wave: a
        # sole detector, whose REMOVE reaches everyone but that row
        late = [r for r in det if r > 35]
        print(f"N={n} k={k}: late detections {[(r, sorted(trace[r - 1][1]), trace[r - 1][0]['detections']) for r in late]}")
        assert late and all(trace[r - 1][1] <= set(victims) for r in late), det
        assert [trace[r - 1][0]["detections"] for r in late] == [1] * len(late)


@pytest.mark.parametrize("label,n,world,layout", sc.RAGGED_SHARDS, ids=[x[0] for x in sc.RAGGED_SHARDS])
def test_ragged_shard_preconditions(oracle_mod, label, n, world, layout):
    """The sharded runs' victims: the tail members and both sides of every
    shard boundary of that layout."""
    bounds = sc.shard_bounds(n, world, layout)
    victims = sc.tail_members(n, bounds)
    assert all(b - 1 in victims and b in victims for b in bounds), (bounds, victims)
    trace = run_wave(oracle_mod, n, sc.ragged_cfg(4), sc.ragged_wave(n, victims, rejoin=False))
    assert_wave(trace, victims, f"{label}: N={n} G={world} layout {layout}")


@pytest.mark.parametrize("n", sorted(sc.RAGGED_QUIRK))
def test_ragged_quirk_preconditions(oracle_mod, n):
    """The quirk runs' victims form candidate runs at the row's end (the last
    list entry among them; at N = 2,049 across the 2,048-cell window edge).
    Quirk detection (slave/slave.go:464-477: a removal shifts the slice under
    the range loop, so the candidate after a detected one is skipped) must
    detect differently from canonical detection in some round. Crashed at
    round 8 the victims are detected one per row (scenarios.py RAGGED_QUIRK)
    and the two modes agree, whichever tail members crash; that schedule is
    kept as the wave in quirk mode, with the wave's preconditions. Crashed at
    round 1 every row detects the whole run at once, and the modes differ."""
    victims = sc.RAGGED_QUIRK[n]
    assert n - 1 in victims and n - 2 in victims  # a run that ends on the row's last list entry
    if n == 2049:
        assert 2047 in victims and 2048 in victims  # ... and crosses the window edge
    differ = {}
    for crash in sc.RAGGED_QUIRK_CRASH:
        sched = sc.ragged_wave(n, victims, rejoin=False, crash=crash)
        rounds = crash + 20  # past the detections (T_fail = 16) and the REMOVE round
        quirk = run_wave(oracle_mod, n, sc.ragged_cfg(4, 1), sched, rounds)
        canon = run_wave(oracle_mod, n, sc.ragged_cfg(4, 0), sched, rounds)
        differ[crash] = [(r, q[0]["detections"], c[0]["detections"]) for r, (q, c) in enumerate(zip(quirk, canon), 1)
                         if q[0]["detections"] != c[0]["detections"]]
        if crash == sc.RAGGED_CRASH:
            assert_wave(quirk, victims, f"N={n} quirk", released=False)
    print(f"N={n}: (round, quirk, canonical detections) where they differ, by crash round: {differ}")
    assert differ[1], differ
    # every running row detects the run's even offsets and the last entry
    # first, the skipped candidates a round later
    (r1, q1, c1), (r2, q2, c2) = differ[1]
    assert r2 == r1 + 1 and q1 < c1 and q1 + q2 == c1 and c2 == 0, differ
