"""Preconditions of the counter-offset runs of tests/test_gpu_counters.py
(scenarios.py COUNTER_OFFSETS, shifted_wave, staggered_state), on the CPU
oracle alone. The GPU tests start the ragged crash wave from heartbeats and
rounds far from 0 -- the tier's per-column base through its sign change, both
counters through 2^15, 2^16 and 2^24, sums of two of them past 2^31, own
counters at INT32_MAX and the refused round after it -- and demand the nibble
path there. That is only fair if, in the reference, every victim is detected,
REMOVE'd and released and the running members' views stay inside the 4-bit
tier's window (lag <= 11, age <= 15) from every one of those starts. These
are conditions on the inputs, not tolerances: the figures asserted are the
oracle's own (detections in the shifted rounds 23 / 24, REMOVE in 24 / 25, a
lag of at most 9 and an age of at most 8 through round 29; `cap` runs 33
rounds and its 34th is refused).

Also here, because the oracle is the reference for all of it: tablesim from
heartbeat H equals tablesim from heartbeat 2 with H - 2 added (nothing in the
rules but `hb > 1` looks at a heartbeat's value), and listsim = tablesim on
churn with joins from 2^24."""
import numpy as np
import pytest

import scenarios as sc
from test_oracle_crosscheck import run_pair
from test_ragged_scenario import AGE_MAX, LAG_MAX, ROUNDS, assert_wave, failed_of, run_wave

THROUGH = sc.RAGGED_REJOIN - 1  # the window is asserted through round 29, before the rejoin
# the N = 2,048 cases: (label, H, R0)
BIG = [("u16_f24", *sc.COUNTER_MIXED), ("cap", *sc.COUNTER_OFFSETS["cap"])]


def test_counter_offsets_table():
    """What the 40 rounds of each offset cross (base = own heartbeat - 1000)."""
    I, off = sc.I32MAX, sc.COUNTER_OFFSETS
    assert len(off) == 10 and all(0 <= r0 <= 2**30 and 2 <= h for h, r0 in off.values())
    h, r0 = off["base0"]
    assert h - 1000 < 0 < h + 40 - 1000 and r0 == 0
    h, r0 = off["round985"]
    assert r0 < 1000 < r0 + 40 and h == 2
    for name, p in (("i16", 15), ("u16", 16), ("f24", 24)):
        h, r0 = off[name]
        assert h < 2**p < h + 40 and r0 < 2**p < r0 + 40 and h == r0 + 2
    assert sum(off["p30"]) == 2**31 and off["hb30"] == (2**30, 0) and off["round30"] == (2, 2**30)
    assert off["top"][0] + 40 == I - 3
    assert off["cap"][0] + sc.CAP_ROUNDS == I and sc.CAP_ROUNDS < 40


def check_offset(om, n, k, h, r0, what):
    """The wave (with its rejoin) from (h, r0): assert_wave's conditions and
    the oracle's figures; returns the number of rounds that ran."""
    trace = run_wave(om, n, sc.ragged_cfg(k), sc.shifted_wave(n, r0), ROUNDS, hb0=h, r0=r0)
    ran = len(trace)
    capped = h + ROUNDS > sc.I32MAX
    if capped:  # own counter h + r after round r: the round that would pass INT32_MAX is refused
        assert ran == sc.I32MAX - h < ROUNDS, (what, ran)
    else:
        assert ran == ROUNDS, (what, ran)
    # T_cleanup = 16: the releases come 16 rounds after the REMOVE round, at 41 / 42
    det, tomb = assert_wave(trace, sc.tail_members(n), what, released=ran >= 42, through=THROUGH)
    wave_det = [r for r in det if r < sc.RAGGED_REJOIN]
    wave_tomb = [r for r in tomb if r < sc.RAGGED_REJOIN]
    assert wave_det and set(wave_det) <= {23, 24}, (what, det)
    assert wave_tomb and set(wave_tomb) <= {24, 25}, (what, tomb)
    lag, age = max(x[2] for x in trace[:THROUGH]), max(x[3] for x in trace[:THROUGH])
    assert lag <= 9 and age <= 8, (what, lag, age)
    return ran


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("name", list(sc.COUNTER_OFFSETS))
def test_counter_wave_preconditions(oracle_mod, name, k):
    """N = 263, every offset, k = 3 and 4."""
    h, r0 = sc.COUNTER_OFFSETS[name]
    ran = check_offset(oracle_mod, 263, k, h, r0, f"{name}: N=263 k={k}")
    if name == "cap":
        assert ran == sc.CAP_ROUNDS
    if name == "top":
        assert ran == ROUNDS - 1  # (44 rounds asked of the oracle here; the GPU run's 40 all run)


@pytest.mark.parametrize("label,h,r0", BIG, ids=[x[0] for x in BIG])
def test_counter_wave_preconditions_n2048(oracle_mod, label, h, r0):
    ran = check_offset(oracle_mod, 2048, 4, h, r0, f"{label}: N=2048 k=4")
    assert ran == (sc.CAP_ROUNDS if label == "cap" else ROUNDS)


def run_plain(om, n, cfg, sched, rounds, hb0, r0):
    """per round (stats, hb, ts, alive, failed, detectors) of tablesim from full_state(n, hb0, r0)"""
    orc = om.Oracle(om.default_config(n, **cfg), threads=8)
    out = []
    try:
        orc.import_state(*sc.full_state(n, hb0=hb0, ts0=r0), r0)
        for r in range(r0 + 1, r0 + rounds + 1):
            if sched.get(r):
                orc.apply_events(sched[r])
            st = orc.step(1)
            out.append((st,) + orc.export_state() + (failed_of(orc), orc.read_detectors().tolist()))
    finally:
        orc.close()
    return out


@pytest.mark.parametrize("detect_mode", [0, 1], ids=["canonical", "quirk"])
@pytest.mark.parametrize("h,r0", [(2**24 - 12, 2**24 - 14), (2**30, 2**30), (sc.I32MAX - 43, 7)],
                         ids=["f24", "p30", "top"])
def test_heartbeat_shift_identity(oracle_mod, h, r0, detect_mode):
    """Without JOINs nothing but `hb > 1` looks at a heartbeat's value: the
    wave (no rejoin) from (H, R0) is the wave from (2, R0) with H - 2 added to
    every present heartbeat; stats, ts, alive, failed sets and detectors are
    the same. This pins the oracle itself at large H."""
    n = 263
    cfg, sched = sc.ragged_cfg(4, detect_mode), sc.shifted_wave(n, r0, rejoin=False)
    big = run_plain(oracle_mod, n, cfg, sched, 40, h, r0)
    small = run_plain(oracle_mod, n, cfg, sched, 40, 2, r0)
    assert any(x[0]["detections"] for x in small) and any(x[0]["tombstoned"] for x in small)
    for r, (a, b) in enumerate(zip(big, small), 1):
        assert a[0] == b[0], (r, a[0], b[0])
        want = np.where(b[1] >= 0, b[1].astype(np.int64) + (h - 2), b[1])
        np.testing.assert_array_equal(a[1], want, err_msg=f"hb, round {r}")
        np.testing.assert_array_equal(a[2], b[2], err_msg=f"ts, round {r}")
        np.testing.assert_array_equal(a[3], b[3], err_msg=f"alive, round {r}")
        assert a[4] == b[4] and a[5] == b[5], r


@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
@pytest.mark.parametrize("quirk", [False, True], ids=["canonical", "quirk"])
def test_listsim_matches_tablesim_from_2p24(oracle_mod, peer_mode, quirk):
    """The two CPU restatements of the reference on seeded churn with joins at
    N = 40 from heartbeat 2^24 - 6 at round 2^24 - 8: a joiner's counter
    restarts 2^24 below its neighbours'."""
    n, r0 = 40, 2**24 - 8
    churn = sc.random_churn(n, 30, 0xC0 + int(quirk), p_crash=0.05, p_leave=0.02, p_join=0.3)
    sched = {r0 + r: ev for r, ev in churn.items()}
    assert sum(kind == sc.JOIN for ev in sched.values() for kind, _ in ev) > 0
    state = sc.full_state(n, hb0=2**24 - 6, ts0=r0) + (r0,)
    orc, ls = run_pair(oracle_mod, n, 30, sched, peer_mode, quirk=quirk, seed=0x5EED0C20, t_fail=12, t_cleanup=14,
                       state=state)
    hb = orc.export_state()[0]
    assert hb.max() > 2**24 and ((hb >= 0) & (hb < 100)).any()  # old members past 2^24 beside restarted ones
    orc.close()


STAG_R0 = 2**16 - 20


def staggered_trace(om, n, rounds=40):
    """The wave on staggered_state(n, STAG_R0, seed n): per round (stats, max lag, max age)"""
    orc = om.Oracle(om.default_config(n, **sc.ragged_cfg(4)), threads=8)
    sched = sc.shifted_wave(n, STAG_R0)
    out = []
    try:
        orc.import_state(*sc.staggered_state(n, STAG_R0, n), STAG_R0)
        for r in range(STAG_R0 + 1, STAG_R0 + rounds + 1):
            if sched.get(r):
                orc.apply_events(sched[r])
            st = orc.step(1)
            hb, ts, alive = orc.export_state()
            run = alive != 0
            own = hb.diagonal().astype(np.int64)
            views = run[:, None] & run[None, :] & (hb >= 0)
            out.append((st, int(np.where(views, own[None, :] - hb, 0).max()),
                        int(np.where(views, r - ts.astype(np.int64), 0).max())))
    finally:
        orc.close()
    return out


@pytest.mark.parametrize("n", [263, 1000])
def test_staggered_state_stays_inside_the_window(oracle_mod, n):
    """staggered_state: every own counter value is drawn, the views lag by at
    most 3 and are at most 3 rounds old at the import, and on the wave every
    view running rows hold of running members stays inside the tier's window
    through round 29; the victims are detected and REMOVE'd."""
    hb, ts, alive = sc.staggered_state(n, STAG_R0, n)
    own = hb.diagonal().astype(np.int64)
    assert set(own.tolist()) == set(sc.STAGGERED_OWN) and alive.all()
    lag0 = own[None, :] - hb
    assert lag0.min() == 0 and lag0.max() == 3 and (hb >= 0).all()
    age0 = STAG_R0 - ts.astype(np.int64)
    assert age0.min() == 0 and age0.max() == 3 and (age0.diagonal() == 0).all()
    # neighbours in one 8-cell chunk with bases more than 2^30 apart
    assert (np.abs(np.diff(own))[np.arange(n - 1) % 8 != 7] > 2**30).any()
    trace = staggered_trace(oracle_mod, n)
    lag, age = max(x[1] for x in trace[:THROUGH]), max(x[2] for x in trace[:THROUGH])
    det = [r for r, x in enumerate(trace, 1) if x[0]["detections"]]
    tomb = [r for r, x in enumerate(trace, 1) if x[0]["tombstoned"]]
    print(f"staggered N={n}: detection {det}, REMOVE {tomb}, max lag {lag}, max age {age}")
    assert lag <= LAG_MAX and age <= AGE_MAX, (lag, age)
    assert det and tomb and det[0] + 1 in tomb and sc.RAGGED_CRASH < det[0] < sc.RAGGED_REJOIN, (det, tomb)
