"""tablesim's or_step(k) against k calls of or_step(1): the summed counters,
last_round, the tables, the failed set and the detectors of the last round.
tests/test_gpu_bench_dump.py compares the engine with orc.step(steps), and
tests/test_gpu_call_partition.py goes the other way (the engine in one call,
the oracle round by round); both rest on the two being the same. Also the CPU
side of that module's arena-growth state (staggered_age_state): ages that
climb past the narrow field row group by row group with nothing detected."""
import numpy as np
import pytest

import scenarios as sc

SUMMED = ("rounds", "detections", "failed_members", "remove_unknown", "ring_empty", "active_rows", "merged_cells",
          "released", "tombstoned")


def call_bounds(sched, rounds, cuts=(), first=1):
    """(first round, rounds) of the step() calls that run rounds first..rounds:
    a call ends after every round in `cuts` and before every round that has
    events (queued events belong to the next round run)."""
    edges = sorted({first, rounds + 1} | {c + 1 for c in cuts if first <= c <= rounds} |
                   {r for r in sched if first <= r <= rounds})
    return [(a, b - a) for a, b in zip(edges, edges[1:])]


def sum_stats(per_round):
    """One call's gh_round_stats from its rounds': counters summed, last_round the last."""
    out = {f: sum(s[f] for s in per_round) for f in SUMMED}
    out["last_round"] = per_round[-1]["last_round"]
    return {f: out[f] for f in per_round[-1]}


def step_summed(orc, k):
    """k rounds of the oracle one at a time; (the call's stats, each round's)"""
    per = [orc.step(1) for _ in range(k)]
    return sum_stats(per), per


def wave(n, seed=0x5EED0D10, detect_mode=0, **kw):
    """The crash wave of tests/test_gpu_knobs.py at any N: k=4 pull, T_fail =
    T_cleanup = 16, 1% crash at round 8, one of them rejoins at round 30."""
    cfg = dict(fanout=4, seed=seed, t_fail=16, t_cleanup=16, detect_mode=detect_mode)
    cfg.update(kw)
    crashed = sc.crash_ids(n, 0.01, seed + 1)
    return cfg, {8: [(sc.CRASH, int(c)) for c in crashed], 30: [(sc.JOIN, int(crashed[0]))]}


def staggered_age_state(n, stopped, pre, per_round, r0=0):
    """(hb, ts, alive), to import at round r0: the members `stopped` have
    crashed and every row holds them at the heartbeat 2 (equal everywhere, so
    no merge ever refreshes them), last heard of at a time staggered by
    observer row: the first `pre` running rows 40 rounds before r0, the others
    in groups of `per_round` rows 30, 29, 28, ... rounds before r0. In the
    state round r0 + j + 1 leaves (whose ages count to the round after it)
    group j's entries are 32 rounds old: one more group per round passes age
    31. Every other cell is fresh (hb 2, ts r0)."""
    hb, ts, alive = sc.full_state(n, ts0=r0)
    stopped = np.asarray(stopped)
    alive[stopped] = 0
    running = np.flatnonzero(alive)
    t = np.empty(len(running), np.int32)
    t[:pre] = r0 - 40
    t[pre:] = r0 - 30 + np.arange(len(running) - pre) // per_round
    for c in stopped:
        ts[running, c] = t
    return hb, ts, alive


def both(om, n, cfg, state, r0=0):
    a, b = (om.Oracle(om.default_config(n, **cfg), threads=4) for _ in range(2))
    for o in (a, b):
        o.import_state(*state, r0)
    return a, b


def assert_same_state(a, b, what):
    for x, y, name in zip(a.export_state(), b.export_state(), ("hb", "ts", "alive")):
        np.testing.assert_array_equal(x, y, err_msg=f"{name} {what}")
    np.testing.assert_array_equal(a.read_failed(), b.read_failed(), err_msg=f"failed {what}")
    np.testing.assert_array_equal(a.read_detectors(), b.read_detectors(), err_msg=f"detectors {what}")


def batched_equals_stepwise(om, n, cfg, sched, rounds, cuts):
    a, b = both(om, n, cfg, sc.full_state(n))
    try:
        seen = dict.fromkeys(SUMMED, 0)
        for r0, k in call_bounds(sched, rounds, cuts):
            if sched.get(r0):
                a.apply_events(sched[r0])
                b.apply_events(sched[r0])
            want, _ = step_summed(a, k)
            got = b.step(k)
            assert got == want, f"rounds {r0}..{r0 + k - 1}: step({k}) {got} != summed {want}"
            assert got["last_round"] == r0 + k - 1 and got["rounds"] == k
            assert_same_state(a, b, f"after round {r0 + k - 1}")
            for f in SUMMED:
                seen[f] += got[f]
        return seen
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("detect_mode", [0, 1], ids=["canonical", "quirk"])
@pytest.mark.parametrize("cuts", [(), (24, 25), (3, 11, 12, 20, 27)], ids=["fewest", "around_detection", "ragged"])
def test_step_k_is_k_steps_wave(oracle_mod, detect_mode, cuts):
    """The crash wave at N=256 through detection and REMOVE (both occur)."""
    n = 256
    cfg, sched = wave(n, detect_mode=detect_mode)
    seen = batched_equals_stepwise(oracle_mod, n, cfg, sched, 36, cuts)
    assert seen["detections"] > 0 and seen["tombstoned"] > 0 and seen["merged_cells"] > 0


@pytest.mark.parametrize("peer_mode", [0, 1], ids=["pull", "ring"])
def test_step_k_is_k_steps_churn(oracle_mod, peer_mode):
    """Seeded crash / leave / join churn at N=300 with short timeouts:
    detections, REMOVEs of unknown members and releases inside the calls."""
    n = 300
    sched = {r: ev for r, ev in sc.random_churn(n, 40, 0x51, p_crash=0.03, p_leave=0.01, p_join=0.05).items()
             if r % 5 == 0}  # (events every 5th round only: calls of 5 rounds)
    cfg = dict(peer_mode=peer_mode, fanout=3, seed=0x5EED0F01, t_fail=4, t_cleanup=6)
    seen = batched_equals_stepwise(oracle_mod, n, cfg, sched, 40, ())
    assert seen["detections"] > 0 and seen["released"] > 0


@pytest.mark.parametrize("case", ["pull", "ring_quirk"])
def test_recorded_append_run_is_listsims(case):
    """tests/golden/call_partition_append.json (tests/call_partition_golden.py)
    is what listsim gives: its first rounds replayed, the first event batch
    among them; the whole run has double entries at the introducer, lists out
    of ID order and a stretch of at least 3 rounds without events."""
    import call_partition_golden as cg
    gold = cg.load()[case]
    assert len(gold) == cg.ROUNDS and sorted(cg.CASES) == sorted(cg.load())
    assert cg.replay(case, 2) == gold[:2]
    assert max(x["dual"] for x in gold) > 0 and max(x["reordered"] for x in gold) > 0
    assert sorted(cg.schedule(case)) == list(range(1, cg.ROUNDS + 1, cg.GAP)) and cg.GAP >= 3


def test_staggered_ages_detect_nothing(oracle_mod):
    """staggered_age_state as the GPU arena-growth cases use it: 14 rounds
    with no detection, no tombstone and no release, and the stopped members'
    entries keep their time stamps in every running row, so their ages do
    climb by one a round."""
    n, stopped = 200, [1, 2, 3]
    state = staggered_age_state(n, stopped, 8, 8)
    a, b = both(oracle_mod, n, dict(fanout=3, seed=0x5EED0F02, t_fail=100, t_cleanup=100), state)
    try:
        st = a.step(14)
        assert st == sum_stats([b.step(1) for _ in range(14)])
        assert (st["detections"], st["tombstoned"], st["released"], st["remove_unknown"]) == (0, 0, 0, 0)
        assert st["active_rows"] == 14 * (n - len(stopped))
        hb, ts, _ = a.export_state()
        run = np.flatnonzero(state[2])
        np.testing.assert_array_equal(ts[np.ix_(run, stopped)], state[1][np.ix_(run, stopped)])
        assert (hb[np.ix_(run, stopped)] == 2).all()
    finally:
        a.close()
        b.close()
