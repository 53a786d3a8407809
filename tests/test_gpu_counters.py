"""GPU parity far from round 0: large heartbeat and round counters.

A run never stays near round 0, but every other test that puts the table on
the 4-bit tier starts from full_state(n) (hb 2, ts 0) at round 0 and runs a
few dozen rounds: the tier's per-column base (own heartbeat - GH_BASE_LAG =
-998 .. -950 there) is never positive, never changes sign, and neither counter
comes near 2^15, 2^16, 2^24, a sum past 2^31 or INT32_MAX. Here the ragged
crash wave (tests/test_gpu_ragged.py) and the read-only passes start from
scenarios.COUNTER_OFFSETS -- (H, R0): full_state(n, hb0=H, ts0=R0) imported
at round R0, the schedule shifted by R0 -- and from scenarios.staggered_state,
whose neighbouring columns have bases billions apart. `cap` takes every own
counter to INT32_MAX in its 33rd round; its 34th is refused (GH_ERANGE) by
the engine and by the oracle alike.

Every comparison is equality with the oracle (oracle/tablesim.c, which keeps
exact int32 hb and ts and takes a start round) or with the model a feature
was built against, every round: stats, hb, ts, alive, failed set, detectors,
the maintained counts. tests/test_counter_scenario.py holds the preconditions
on the oracle alone. Rounds in docstrings count from the import ("shifted").
Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import groups_ref as gr
import journal_ref as jr
import scenarios as sc
from census_ref import assert_census_equal, census_ref
from test_counter_scenario import STAG_R0, THROUGH
from test_gpu_call_partition import Scenario, assert_final, remove_inside_hook
from test_gpu_config_space import both, make_engine
from test_gpu_parity import compare
from test_gpu_ragged import check_padding, is_tier_tombstone, last_running_row, tier_cells
from test_gpu_tier8 import remove_run
from test_oracle_step_batch import call_bounds, sum_stats

pytestmark = pytest.mark.gpu

I32MAX = sc.I32MAX
ROUNDS = sc.RAGGED_ROUNDS
CAP = sc.CAP_ROUNDS
N = 263
OFFSETS = sc.COUNTER_OFFSETS


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def tier_on(monkeypatch):
    monkeypatch.setenv("GH_PLANE", "1")
    for k in ("GH_C8", "GH_TMODE", "GH_GX_DIRECT", "GH_QUIRK_ROWS"):
        monkeypatch.delenv(k, raising=False)


def nibble_from(h):
    """The first round demanded of the nibble path after an import at
    heartbeat h. gh_import_state keeps the per-column bases the engine holds
    (a new engine's lie below 0), and a 16-bit cell reaches 2,047 above its
    base: a state imported further up than that is stored in wide segments,
    round 1 re-bases every column by the per-cell rule (encoding_info counts
    every segment), which sends round 2 to the storm variant and round 3 to
    the lean one on its 16-bit table; the nibble path runs from round 4.
    From heartbeats under 1,000 it runs from round 2, as from hb 2."""
    return 2 if h < 1000 else 4


def rounds_of(h):
    """the rounds a full start at heartbeat h runs out of the wave's 40"""
    return min(ROUNDS, I32MAX - h)


def lockstep(eng, orc, sched, first, last, per_round=None):
    """Rounds first..last one at a time, compared after each; returns the oracle's stats."""
    out = []
    for r in range(first, last + 1):
        if sched.get(r):
            eng.apply_events(sched[r])
            orc.apply_events(sched[r])
        s1, s2 = eng.step(1), orc.step(1)
        assert s1 == s2, f"round {r}: gpu {s1} != cpu {s2}"
        compare(eng, orc, r)
        out.append(s2)
        if per_round:
            per_round(r, s2)
    return out


# ---- a. the crash wave at every offset ---------------------------------------------------------

_WAVES = {}


def counter_wave(gs, om, n, k, h, r0):
    """The wave at (n, k) from (h, r0) on one engine, one round per call,
    checked against the oracle every round (remove_run); kept per case:
    (trace, final export, per-round diagnostics keyed by the shifted round)."""
    key = (n, k, h, r0)
    if key not in _WAVES:
        victims = sc.tail_members(n)
        probe_rows = [0, last_running_row(n, victims), n - 1]
        diag = {}

        def per_round(eng, r):
            if n % 16:
                check_padding(eng, n, r)
            tombs = {row: 0 for row in probe_rows}
            for row in probe_rows:
                for c in victims:
                    tombs[row] += bool(is_tier_tombstone(int(tier_cells(eng, row, c & ~7, 8)[c & 7])))
            diag[r - r0] = dict(launched=eng.debug_variant(), tombs=tombs, enc=eng.encoding_info(full=True),
                                tier=eng.tier_info(full=True), jobs=eng.job_info())

        trace, final = remove_run(gs, om, n, sc.ragged_cfg(k), sc.shifted_wave(n, r0), rounds_of(h),
                                  per_round=per_round, init=sc.full_state(n, hb0=h, ts0=r0), round0=r0)
        _WAVES[key] = (trace, final, diag)
    return _WAVES[key]


def assert_counter_wave(what, n, trace, diag, rounds, h):
    """test_ragged_crash_wave's assertions, rounds shifted; the healthy rounds
    demanded of the nibble path are nibble_from(h)..7."""
    victims = sc.tail_members(n)
    rows = [(r, s["detections"], s["tombstoned"], s["released"], var, diag[r]["launched"], jobs, diag[r]["enc"],
             diag[r]["tier"], diag[r]["tombs"]) for r, (s, var, jobs) in enumerate(trace, 1)]
    print(f"{what}: (shifted round, detections, tombstoned, released, variant, launched, lane jobs, encoding_info, "
          f"tier_info, tier tombstones by row)")
    for x in rows:
        print("  ", x)
    assert len(trace) == rounds, (what, len(trace))
    tomb_rounds = [r for r, (s, _, _) in enumerate(trace, 1) if s["tombstoned"] > 0]
    assert tomb_rounds and any(s["detections"] for s, _, _ in trace), rows
    assert all(trace[r - 1][1] == 3 for r in range(nibble_from(h), sc.RAGGED_CRASH)), rows
    assert all(trace[r - 1][1] == 3 for r in tomb_rounds), rows
    assert 4 in {diag[r]["launched"] for r in tomb_rounds}, rows
    assert any(trace[r - 1][2] > 0 for r in range(sc.RAGGED_CRASH, rounds + 1)), rows
    seen = {row: sum(diag[r]["tombs"][row] for r in diag) for row in diag[1]["tombs"]}
    assert seen[0] > 0 and seen[last_running_row(n, victims)] > 0, seen
    assert seen[n - 1] == 0, seen
    return rows


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("name", list(OFFSETS))
def test_counter_crash_wave(gs, oracle_mod, name, k):
    """test_ragged_crash_wave at N = 263 from every offset: tail_members crash
    at round 8, are detected (23 / 24) and REMOVE'd (24 / 25), the last member
    rejoins at round 30 -- its column's base drops by the whole of H. Parity,
    the maintained counts and the padding cells every round; the nibble path
    ran the rounds 2..7 (4..7 where the import lies beyond the bases' narrow
    range, nibble_from) and every round that made tombstones, its REMOVE form
    (debug_variant 4) one of them, lane jobs ran, tier tombstones stand in the
    victims' columns of row 0 and of the last running row. `cap` runs 33
    rounds: in its rounds 31..33 every own counter is INT32_MAX - 2 or more.
    At every offset the rejoin's JOIN broadcast at round 30 makes lane jobs
    of half the lanes and sends the next two or three rounds to the storm and
    the lean variant, which on `cap` are the last three; the
    nibble path with every own counter at the cap is
    test_cap_refused_on_the_tier's, which has no rejoin. `top` ends on the
    nibble path with the table in the tier, own counters at INT32_MAX - 3."""
    h, r0 = OFFSETS[name]
    rounds = rounds_of(h)
    assert rounds == (CAP if name == "cap" else ROUNDS)
    trace, final, diag = counter_wave(gs, oracle_mod, N, k, h, r0)
    assert_counter_wave(f"{name}: N={N} k={k}", N, trace, diag, rounds, h)
    if name in ("cap", "top"):
        own = final[0].diagonal()
        assert own.max() == (I32MAX if name == "cap" else I32MAX - 3), own.max()
    if name == "top":
        assert trace[rounds - 1][1] == 3 and diag[rounds]["tier"][1] == 1, diag[rounds]["tier"]


BIG = [("u16_f24", *sc.COUNTER_MIXED), ("cap", *OFFSETS["cap"])]


@pytest.mark.parametrize("label,h,r0", BIG, ids=[x[0] for x in BIG])
def test_counter_crash_wave_n2048(gs, oracle_mod, label, h, r0):
    """The same at N = 2,048, k = 4 (whole tiles, eight of them): heartbeats
    through 2^16 while the round passes 2^24, and `cap`."""
    n = 2048
    trace, _, diag = counter_wave(gs, oracle_mod, n, 4, h, r0)
    assert_counter_wave(f"{label}: N={n} k=4", n, trace, diag, rounds_of(h), h)


# ---- b. the refusal on the tier ----------------------------------------------------------------------

def test_cap_refused_on_the_tier(gs, oracle_mod):
    """`cap` at N = 263 with the tail members crashed before the first round:
    one step(40) and the same 40 rounds as single calls both return GH_ERANGE
    with rounds == 33, as the oracle does; the detections lie inside.
    The tier is current and the rounds 31..33 (own counters INT32_MAX - 2 ..
    INT32_MAX) ran on the nibble path, gh_census after every round equals the
    census of the oracle's export (hb_sum, hb_min, hb_max of tier columns
    whose owner is at the cap); the export equals the oracle's; a second call
    runs nothing."""
    h, r0 = OFFSETS["cap"]
    cfg, state = sc.ragged_cfg(4), sc.full_state(N, hb0=h, ts0=r0)
    crash = [(sc.CRASH, c) for c in sc.tail_members(N)]
    orc = oracle_mod.Oracle(oracle_mod.default_config(N, **cfg), threads=8)
    one, single = make_engine(gs, N, cfg, "single"), make_engine(gs, N, cfg, "single")
    try:
        for x in (orc, one, single):
            x.import_state(*state, r0)
            x.apply_events(crash)
        per, tier = [], []
        for q in range(ROUNDS):
            rc, st = orc.step_rc(1)
            got_rc, got = single.step_rc(1)
            assert (got_rc, got) == (rc, st), (q, got_rc, got, rc, st)
            if rc == 0:
                per.append(st)
                compare(single, orc, r0 + q + 1)
                tier.append((single.tier_info()[1], single.tier_info(full=True)[3], single.job_info()[0]))
                hb, ts, alive = orc.export_state()
                assert_census_equal(single.census(), census_ref(hb, ts, alive, r0 + q + 1), f"cap round {q + 1}")
            else:
                assert rc == gs._abi.GH_ERANGE and st["rounds"] == 0 and q >= CAP, (q, rc, st)
        print(f"cap: (tier current, variant, lane jobs) per round {tier}")
        # (crashed before their first heartbeat, the victims are detected by every row at once, in
        # round 17: the REMOVE round finds them tombstoned everywhere and makes no tombstone itself)
        assert len(per) == CAP and sum(s["detections"] for s in per) >= (N - 3) * 3
        assert all(t[:2] == (1, 3) for t in tier[CAP - 3:]), tier  # own counters INT32_MAX - 2 .. INT32_MAX
        assert hb.diagonal().max() == I32MAX
        compare(single, orc, r0 + CAP)
        rc, st = one.step_rc(ROUNDS)
        assert rc == gs._abi.GH_ERANGE and st == sum_stats(per) and st["rounds"] == CAP, (rc, st, sum_stats(per))
        assert one.tier_info()[1] == 1 and one.tier_info(full=True)[3] == 3, one.tier_info(full=True)
        compare(one, orc, r0 + CAP)
        assert one.export_state()[0].diagonal().max() == I32MAX
        rc2, st2 = one.step_rc(5)
        rc3, st3 = orc.step_rc(5)
        assert rc2 == rc3 == gs._abi.GH_ERANGE and st2 == st3 and st2["rounds"] == 0
        compare(one, orc, r0 + CAP)
    finally:
        for x in (orc, one, single):
            x.close()


def test_staggered_columns_reach_the_cap(gs, oracle_mod):
    """staggered_state at N = 263: only the INT32_MAX - 60 columns reach the
    cap, beside columns at 62, 1,050, 2^16, 2^24 and 2^30. One step(70) runs 60
    rounds and is refused on the tier; crashing those members in the refused
    round lets both sides go on (test_int32_overflow_refused_like_the_oracle),
    and parity continues for 20 more rounds: the stopped columns, whose base
    is now INT32_MAX - 1000, are detected 16 rounds on, and the lanes that
    hold them run as lane jobs (job_chunk) beside the nibble path."""
    cfg, state = sc.ragged_cfg(4), sc.staggered_state(N, STAG_R0, N)
    top = np.flatnonzero(state[0].diagonal() == I32MAX - 60)
    assert 0 < len(top) < N // 3
    orc = oracle_mod.Oracle(oracle_mod.default_config(N, **cfg), threads=8)
    eng = make_engine(gs, N, cfg, "single")
    try:
        eng.import_state(*state, STAG_R0)
        orc.import_state(*state, STAG_R0)
        rc1, s1 = eng.step_rc(70)
        rc2, s2 = orc.step_rc(70)
        assert rc1 == rc2 == gs._abi.GH_ERANGE and s1 == s2 and s1["rounds"] == 60, (rc1, s1, rc2, s2)
        compare(eng, orc, STAG_R0 + 60)
        print(f"after the 60 rounds: tier_info {eng.tier_info(full=True)}, lane jobs {eng.job_info()}")
        assert eng.tier_info()[:2] == (1, 1), eng.tier_info(full=True)
        own = eng.export_state()[0].diagonal()
        assert (own[top] == I32MAX).all() and own.max() == I32MAX and (np.delete(own, top) <= 2**30 + 60).all()
        rc1, s1 = eng.step_rc(1)
        rc2, s2 = orc.step_rc(1)
        assert rc1 == rc2 == gs._abi.GH_ERANGE and s1 == s2 and s1["rounds"] == 0
        ev = [(sc.CRASH, int(c)) for c in top]
        eng.apply_events(ev)
        orc.apply_events(ev)
        seen = []
        stats = lockstep(eng, orc, {}, STAG_R0 + 61, STAG_R0 + 80,
                         per_round=lambda r, st: seen.append((eng.tier_info()[1], eng.tier_info(full=True)[3],
                                                              eng.job_info()[0])))
        print(f"after the crash: (tier current, variant, lane jobs) per round {seen}")
        assert not eng.export_state()[2][top].any()
        assert sum(s["detections"] for s in stats) > 0
        assert any(cur == 1 and var == 3 and jobs > 0 for cur, var, jobs in seen), seen
    finally:
        eng.close()
        orc.close()


# ---- c. the staggered state ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [263, 1000])
def test_staggered_wave(gs, oracle_mod, n):
    """The wave (crash at 8, rejoin at 30) on staggered_state, k = 4: own
    counters 2, 990, 2^16 - 6, 2^24 - 6, 2^30 and INT32_MAX - 60 side by side
    in one chunk. Parity every round. The oracle's views stay inside the
    tier's window through round 29 (test_counter_scenario.py), so the table is
    held in the tier and the nibble path runs in the rounds 4..29 (the first
    three re-base the imported columns, nibble_from)."""
    diag = {}

    def per_round(eng, r):
        check_padding(eng, n, r)
        diag[r - STAG_R0] = (eng.encoding_info(full=True), eng.tier_info(full=True), eng.job_info())

    trace, _ = remove_run(gs, oracle_mod, n, sc.ragged_cfg(4), sc.shifted_wave(n, STAG_R0), ROUNDS, per_round=per_round,
                          init=sc.staggered_state(n, STAG_R0, n), round0=STAG_R0)
    print(f"staggered N={n}: (shifted round, detections, tombstoned, variant, lane jobs, encoding_info, tier_info)")
    for r, (s, var, jobs) in enumerate(trace, 1):
        print("  ", (r, s["detections"], s["tombstoned"], var, jobs, diag[r][0], diag[r][1]))
    assert any(s["detections"] for s, _, _ in trace) and any(s["tombstoned"] for s, _, _ in trace)
    for r in range(nibble_from(I32MAX - 60), THROUGH + 1):
        assert diag[r][1][1] == 1 and trace[r - 1][1] == 3, (r, diag[r])


# ---- d. batched calls ------------------------------------------------------------------------------------

def run_calls(eng, orc, sched, first, last, cuts, at_call_end=None):
    """run_partitioned (test_gpu_call_partition.py) for a run that may be
    refused: the engine in one step_rc(k) per call, the oracle round by round;
    a call whose round q is refused returns GH_ERANGE with the q rounds
    before it, from both. Stops after the refused call. Returns (the
    engine's export, the call that was refused or None)."""
    for a, k in call_bounds(sched, last, cuts, first):
        if sched.get(a):
            eng.apply_events(sched[a])
            orc.apply_events(sched[a])
        rc, got = eng.step_rc(k)
        per, want_rc, st = [], 0, None
        for _ in range(k):
            want_rc, st = orc.step_rc(1)
            if want_rc != 0:
                break
            per.append(st)
        want = sum_stats(per) if per else st
        assert (rc, got) == (want_rc, want), f"call {a}..{a + k - 1}: gpu {rc} {got} != cpu, summed {want_rc} {want}"
        compare(eng, orc, a + len(per) - 1)
        assert eng.round == orc.round == a + len(per) - 1
        if at_call_end and per:
            at_call_end(eng, a, len(per), per)
        if rc != 0:
            return eng.export_state(), (a, k, len(per))
    return eng.export_state(), None


@pytest.mark.parametrize("part", ["fewest", "remove_inside"])
@pytest.mark.parametrize("name", ["base0", "u16", "cap"])
def test_counter_batched_calls(gs, oracle_mod, name, part):
    """test_ragged_batched_calls at N = 263 from `base0`, `u16` and `cap`:
    `fewest` is the calls 1..7, 8..29, 30..40, `remove_inside` ends a call on
    the REMOVE round d + 1, which then runs inside a call as the looped
    1/8-grid form. After every call the summed stats and the tables against
    the oracle stepped singly, the final tables against the stepwise engine's
    (section a). For `cap` the call that starts at round 30 is refused at
    q = 4: it returns GH_ERANGE with its 4 rounds run."""
    h, r0 = OFFSETS[name]
    rounds = rounds_of(h)
    state = sc.full_state(N, hb0=h, ts0=r0)
    sched = sc.shifted_wave(N, r0)
    scen = Scenario(("counters", name), N, sc.ragged_cfg(4), sched, r0 + rounds, state=state, r0=r0)
    d = scen.d(oracle_mod)
    assert sc.RAGGED_CRASH < d - r0 and d + 1 - r0 < sc.RAGGED_REJOIN, d
    seen = []
    eng = make_engine(gs, N, scen.cfg, "single")
    orc = scen.oracle(oracle_mod)
    try:
        eng.import_state(*state, r0)
        final, refused = run_calls(eng, orc, sched, r0 + 1, r0 + ROUNDS, scen.cuts(oracle_mod, part),
                                   at_call_end=remove_inside_hook(scen, oracle_mod, part, seen))
        if name == "cap":
            assert refused == (r0 + sc.RAGGED_REJOIN, ROUNDS - sc.RAGGED_REJOIN + 1, CAP - sc.RAGGED_REJOIN + 1), refused
            assert eng.tier_info()[1] == 1, eng.tier_info(full=True)
            assert eng.step_rc(3) == orc.step_rc(3)  # refused again, nothing runs
            compare(eng, orc, r0 + CAP)
        else:
            assert refused is None
    finally:
        eng.close()
        orc.close()
    if part == "remove_inside":
        assert seen == [d + 1], seen
    assert_final(final, counter_wave(gs, oracle_mod, N, 4, h, r0)[1], f"{name}/{part}")


# ---- e. census, journal, groups ---------------------------------------------------------------------------

LOG_ROUNDS = 16  # shorter than the run


def census_case(name):
    if name == "staggered":
        return sc.staggered_state(N, STAG_R0, N), STAG_R0, ROUNDS
    h, r0 = OFFSETS[name]
    return sc.full_state(N, hb0=h, ts0=r0), r0, rounds_of(h)


@pytest.mark.parametrize("name", ["f24", "p30", "cap", "staggered"])
def test_counter_census_journal_groups(gs, oracle_mod, name):
    """test_ragged_census_journal far from round 0: gh_census after every
    round against the numpy census of the ORACLE's export, every field
    (hb_sum, hb_min and hb_max are the point: on `cap` the columns' owners
    stand at INT32_MAX - 2 .. INT32_MAX in the rounds 31..33 while the table is
    in the tier); the journal in GH_JOURNAL_VIEWS mode with a 16-round log
    against journal_ref.drive on the oracle from round R0 + 1; gh_groups
    against groups_ref at the detection and REMOVE rounds."""
    state, r0, rounds = census_case(name)
    cfg, sched = sc.ragged_cfg(4), sc.shifted_wave(N, r0)
    eng = make_engine(gs, N, cfg, "single")
    orc = oracle_mod.Oracle(oracle_mod.default_config(N, **cfg), threads=8)
    try:
        eng.import_state(*state, r0)
        orc.import_state(*state, r0)
        eng.journal_enable(jr.VIEWS, LOG_ROUNDS)
        ref = jr.JournalRef(N, orc.export_state()[2], jr.VIEWS, LOG_ROUNDS)
        tiered, grouped, steps, want = [], [], [], {}

        def listed_of(o):
            hb, ts, alive = o.export_state()
            want["census"], want["state"] = census_ref(hb, ts, alive, o.round), (hb, alive)
            return want["census"].listed

        def per_round(r):  # (the oracle has run round r and fed the reference)
            if sched.get(r):
                eng.apply_events(sched[r])
            got = eng.step(1)
            assert_census_equal(eng.census(), want["census"], f"{name} round {r - r0}")
            if eng.tier_info()[1] == 1:
                tiered.append(r - r0)
            steps.append(got)
            if got["detections"] or got["tombstoned"]:
                gr.assert_groups_equal(eng.groups(), gr.groups_ref(*want["state"]), f"{name} round {r - r0}")
                grouped.append(r - r0)

        stats = jr.drive(orc, sched, rounds, ref, lambda o: o.export_state()[2], listed_of, r0=r0 + 1, per_round=per_round)
        assert steps == stats
        det = [q for q, s in enumerate(stats, 1) if s["detections"]]
        tomb = [q for q, s in enumerate(stats, 1) if s["tombstoned"]]
        print(f"{name}: detections {det}, REMOVE {tomb}, tier current in {tiered}")
        assert det and tomb and set(det + tomb) <= set(grouped)
        assert 7 in tiered and set(tomb) <= set(tiered) and rounds in tiered, tiered
        if name == "cap":
            assert want["census"].hb_max.max() == I32MAX
        assert eng.journal_total() == rounds > LOG_ROUNDS
        jr.assert_journal_equal(eng.journal(), eng.journal_rounds(), ref, name)
        compare(eng, orc, r0 + rounds)
    finally:
        eng.close()
        orc.close()


# ---- f. shards ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f24", "cap"])
@pytest.mark.parametrize("label,world,layout", [("cols3", 3, 0), ("rows2", 2, 1)])
def test_counter_shards(gs, oracle_mod, label, world, layout, name):
    """test_ragged_shards from `f24` and `cap`: 3 column shards and 2 row
    shards at N = 263, the victims the tail members and both sides of every
    shard boundary; the whole group's table against the oracle every round.
    Row shards: every shard keeps the tier in the rounds 3..7 and runs the
    nibble path in the rounds 4..7 (nibble_from)."""
    h, r0 = OFFSETS[name]
    victims = sc.tail_members(N, sc.shard_bounds(N, world, layout))
    seen = {}

    def per_round(grp, r):
        if layout == 1:
            seen[r - r0] = grp.run("tier_info", full=True)

    trace, _ = remove_run(gs, oracle_mod, N, sc.ragged_cfg(4), sc.shifted_wave(N, r0, victims), rounds_of(h),
                          world=world, layout=layout, per_round=per_round, init=sc.full_state(N, hb0=h, ts0=r0),
                          round0=r0)
    assert any(s["detections"] for s, _, _ in trace) and any(s["tombstoned"] for s, _, _ in trace)
    if layout == 1:
        print(f"{label}/{name}: per round, every shard's variant: { {r: [x[3] for x in v] for r, v in seen.items()} }")
        for r in range(3, sc.RAGGED_CRASH):
            for g, (kept, _, _, variant) in enumerate(seen[r]):
                assert kept == 1 and (variant == 3 or r < nibble_from(h)), (r, g, seen[r])


# ---- g. quirk detection ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,name,quirk_rows", [(263, "u16", None), (263, "p30", None), (2049, "f24", 1)],
                         ids=["n263-u16", "n263-p30", "n2049-f24-rows1"])
def test_counter_quirk(gs, oracle_mod, monkeypatch, n, name, quirk_rows):
    """test_ragged_quirk's crash1 schedule (the victims never heartbeat, every
    row detects the whole run in round 17, the quirk skips every second
    candidate) from `u16` and `p30`, and once at N = 2,049 from `f24` with the
    one-pass row walk k_quirk_rows across the 2,048-cell window edge."""
    if quirk_rows is not None:
        monkeypatch.setenv("GH_QUIRK_ROWS", str(quirk_rows))
    h, r0 = OFFSETS[name]
    sched = sc.shifted_wave(n, r0, sc.RAGGED_QUIRK[n], crash=1)

    def created(eng):
        if quirk_rows is not None:
            assert eng.knobs()["GH_QUIRK_ROWS"] == quirk_rows, eng.knobs()

    trace, _ = remove_run(gs, oracle_mod, n, sc.ragged_cfg(4, 1), sched, 21, on_create=created,
                          per_round=lambda eng, r: check_padding(eng, n, r), init=sc.full_state(n, hb0=h, ts0=r0),
                          round0=r0)
    det = [r for r, (s, _, _) in enumerate(trace, 1) if s["detections"]]
    assert det[:2] == [17, 18], det
    assert all(trace[r - 1][1] == 3 for r in range(nibble_from(h), 8)), [t[1] for t in trace]


# ---- h. off the tier -----------------------------------------------------------------------------------------------

RING_WARM, _RING_WARM = 110, {}
RING_CASES = [("f24", 0, 0), ("f24", 1, 0), ("p30", 0, 0), ("p30", 1, 0), ("f24", 0, 1)]


@pytest.mark.parametrize("name,detect_mode,remove_mode", RING_CASES,
                         ids=[f"{a}-{'quirk' if b else 'canonical'}{'-remove_list' if c else ''}" for a, b, c in RING_CASES])
def test_counter_ring_no_plane(gs, oracle_mod, monkeypatch, name, detect_mode, remove_mode):
    """N = 300 without a plane (the 16-bit form), ring mode, rejoin_churn for
    30 rounds from `f24` and `p30`: canonical and quirk detection, and the
    reference's REMOVE recipients once. A ring of 300 needs ~100 rounds to
    carry a heartbeat round, so the start is what the oracle itself holds at
    (H, R0) after 110 rounds with timeouts out of reach (as
    test_gpu_call_partition.ring_scenario). A joiner's counter restarts 2^24
    or 2^30 below its neighbours'; the broken ring collapses near the end."""
    monkeypatch.delenv("GH_PLANE")
    n = 300
    h, r0 = OFFSETS[name]
    base = dict(peer_mode=1, fanout=3, seed=0x5EED0C30 + detect_mode, detect_mode=detect_mode, remove_mode=remove_mode)
    cfg = dict(t_fail=6, t_cleanup=8, **base)
    if (name, detect_mode, remove_mode) not in _RING_WARM:
        w = oracle_mod.Oracle(oracle_mod.default_config(n, t_fail=1000, t_cleanup=1000, **base), threads=8)
        try:
            w.import_state(*sc.full_state(n, hb0=h - RING_WARM, ts0=r0 - RING_WARM), r0 - RING_WARM)
            st = w.step(RING_WARM)
            assert st["detections"] == 0 and st["active_rows"] == n * RING_WARM
            _RING_WARM[name, detect_mode, remove_mode] = w.export_state()
        finally:
            w.close()
    state = _RING_WARM[name, detect_mode, remove_mode]
    assert (state[0].diagonal() == h).all()
    sched = {r0 + r: ev for r, ev in sc.rejoin_churn(n, 30, 0xC1 + detect_mode, p_out=0.01).items()}
    assert sum(kind == sc.JOIN for ev in sched.values() for kind, _ in ev) > 0
    eng = make_engine(gs, n, cfg, "single")
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    mixed = []

    def per_round(r, st):
        hb = orc.export_state()[0]
        mixed.append(bool(hb.max() > h and ((hb >= 0) & (hb < 100)).any()))

    try:
        assert eng.plane_info()[0] == 0 and eng.tier_info()[0] == 0
        eng.import_state(*state, r0)
        orc.import_state(*state, r0)
        stats = lockstep(eng, orc, sched, r0 + 1, r0 + 30, per_round=per_round)
        assert stats[0]["active_rows"] > 0.9 * n and stats[0]["detections"] == 0  # a healthy start
        assert sum(s["detections"] for s in stats) > 0 and sum(s["tombstoned"] for s in stats) > 0
        assert sum(mixed) >= 10, mixed  # old counters beside restarted ones
    finally:
        eng.close()
        orc.close()


def append_order_ring_quirk(gs, on_create=None, **cfg_kw):
    """The run of test_counter_append_order_ring_quirk (GH_PLANE unset by the
    caller); `cfg_kw` adds to the engine's configuration, on_create(eng) runs
    before the import."""
    from oracle.listsim import ListSim
    import test_gpu_list_order as lo
    n, rounds = 64, 40
    h, r0 = OFFSETS["f24"]
    seed = 0x5EED0C40
    sched = {r0 + r: ev for r, ev in sc.random_churn(n, rounds, 0xC2, p_crash=0.03, p_leave=0.02, p_join=0.08).items()}
    state = sc.full_state(n, hb0=h, ts0=r0)
    eng = gs.Engine(gs.default_config(n, peer_mode=gs.GH_PEER_RING, fanout=3, detect_mode=1, seed=seed,
                                      list_order=lo.APPEND, **cfg_kw))
    try:
        if on_create:
            on_create(eng)
        eng.import_state(*state, r0)
        ls = ListSim.from_dense(*state, r0, seed=seed, peer_mode="ring", fanout=3, quirk=True, order="append")
        reordered, detections = 0, 0
        for r in range(r0 + 1, r0 + rounds + 1):
            if sched.get(r):
                eng.apply_events(sched[r])
                ls.apply_events(sched[r])
            s1, s2 = eng.step(1), ls.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != listsim {s2}"
            bm = eng.read_failed()
            assert [c for c in range(n) if bm[c >> 5] >> (c & 31) & 1] == ls.last_failed, r
            assert sorted(eng.read_detectors()) == sorted(ls.last_detectors), r
            lo.compare(eng, ls, n, r)
            reordered = max(reordered, sum(1 for x in lo.lists_ref(ls) if x != sorted(x)))
            detections += s2["detections"]
        assert reordered > 0 and detections > 0
    finally:
        eng.close()


def test_counter_append_order_ring_quirk(gs, monkeypatch):
    """GH_ORDER_APPEND at N = 64 against live listsim from `f24`, ring mode
    with the quirk sweep: counters, tables, failed set, detectors and every
    row's gh_lsm order each round."""
    monkeypatch.delenv("GH_PLANE")
    append_order_ring_quirk(gs)


def test_counter_file_ops(gs, oracle_mod, monkeypatch):
    """gh_put, gh_put_conflicts(window = 60), one crash, gh_repair and
    gh_get_files at N = 64 from `p30` against the oracle: the conflict window
    is a difference of rounds near 2^30, the versions' stamps are rounds."""
    monkeypatch.delenv("GH_PLANE")
    n, F = 64, 200
    h, r0 = OFFSETS["p30"]
    cfg = dict(max_files=F, seed=0x5EED0C50, fanout=4, t_fail=16, t_cleanup=16)
    eng = make_engine(gs, n, cfg, "single")
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    allf = np.arange(F, dtype=np.int32)
    try:
        state = sc.full_state(n, hb0=h, ts0=r0)
        eng.import_state(*state, r0)
        orc.import_state(*state, r0)
        lockstep(eng, orc, {}, r0 + 1, r0 + 2)
        rep, ver, st = both(eng, orc, "put", allf[:120])
        assert (np.asarray(ver) == 1).all()
        lockstep(eng, orc, {}, r0 + 3, r0 + 10)
        c1 = both(eng, orc, "put_conflicts", allf, 60)
        assert np.asarray(c1)[:120].all() and not np.asarray(c1)[120:].any()  # 8 rounds ago: inside the window
        victim = int(np.asarray(rep)[0][0])
        assert victim != 0
        stats = lockstep(eng, orc, {r0 + 11: [(sc.CRASH, victim)]}, r0 + 11, r0 + 72)
        assert sum(s["detections"] for s in stats) > 0
        c2 = both(eng, orc, "put_conflicts", allf, 60)
        assert not np.asarray(c2).any()  # 70 rounds ago: outside
        for obs in (0, 5):
            plan = both(eng, orc, "repair", obs)
            assert obs != 0 or len(plan) > 0
        both(eng, orc, "get_files", allf)
        both(eng, orc, "put", allf[100:150])
        both(eng, orc, "get_files", allf)
        both(eng, orc, "put_conflicts", allf, 60)
    finally:
        eng.close()
        orc.close()


# ---- i. loss features and ensembles -----------------------------------------------------------------------------------

def shifted(sched, r0):
    return {r0 + r: ev for r, ev in sched.items()}


def model_lockstep(eng, model, cmp, sched, first, last, before=None, per_round=None):
    for r in range(first, last + 1):
        if before:
            before(r)
        if sched.get(r):
            eng.apply_events(sched[r])
            model.apply_events(sched[r])
        want, got = model.step(1), eng.step(1)
        assert got == want, f"round {r}: gpu {got} != model {want}"
        cmp(eng, model, r)
        if per_round:
            per_round(r, want)


def test_counter_lossy_links(gs):
    """test_gpu_loss.py's nib263 (GH_PLANE=1, k=4, T=16, uniform 0.10, a mute
    and a deaf member, the 1% crash at round 8), imported at R0 = 2^24 - 14
    with heartbeat R0 + 2, against LossModel imported at the same round."""
    import loss_ref as lr
    import test_gpu_loss as tl
    case = tl.CASES["nib263"]
    h, r0 = OFFSETS["f24"]
    n, c = case["n"], case["cfg"]
    state = sc.full_state(n, hb0=h, ts0=r0)
    eng = gs.Engine(gs.default_config(n, **c))
    model = lr.LossModel(n, c["fanout"], c["t_fail"], c["t_cleanup"], c["seed"])
    seen = []
    try:
        eng.import_state(*state, r0)
        model.import_state(*state, r0)
        eng.set_loss(case["out"], case["inn"])
        model.set_loss(case["out"], case["inn"])
        assert eng.tier_info()[0] == 1
        model_lockstep(eng, model, tl.compare, shifted(case["sched"], r0), r0 + 1, r0 + case["rounds"],
                       per_round=lambda r, st: seen.append((eng.tier_info()[1], eng.tier_info(full=True)[3],
                                                            st["detections"])))
        print(f"nib263 from f24: (tier current, variant, detections) per round {seen}")
        assert any(t == 1 for t, _, _ in seen) and any(v == 3 for _, v, _ in seen) and any(d for _, _, d in seen)
        assert model.loss_stats()[1] > 0 and model.hb.max() > 2**24
    finally:
        eng.close()


def test_counter_partition(gs, monkeypatch):
    """test_gpu_partition.py's two16 (N=263, k=3, T=5 on the 16-bit path, sides
    of 43 and 220 from round 3), imported at `f24`, against PartitionModel
    imported at the same round."""
    import partition_ref as pr
    import test_gpu_partition as tp
    monkeypatch.delenv("GH_PLANE")
    case = tp.CASES["two16"]
    h, r0 = OFFSETS["f24"]
    n, c = case["n"], case["cfg"]
    state = sc.full_state(n, hb0=h, ts0=r0)
    eng = gs.Engine(gs.default_config(n, **c))
    model = pr.PartitionModel(n, c["fanout"], c["t_fail"], c["t_cleanup"], c["seed"])
    try:
        eng.import_state(*state, r0)
        model.import_state(*state, r0)
        assert eng.tier_info()[0] == 0 and case.get("loss") is None

        def before(r):
            if r == r0 + case["split"]:
                eng.set_partition(case["side"])
                model.set_partition(case["side"])

        model_lockstep(eng, model, tp.compare, shifted(case["sched"], r0), r0 + 1, r0 + case["rounds"], before=before)
        assert model.cut > 0 and eng.partition()[0]
    finally:
        eng.close()


def test_counter_control_loss(gs):
    """test_gpu_control_loss.py's nib263 (GH_PLANE=1, k=4, T=16, 0.2 on both
    ends of every link, REMOVE lossy, the 1% crash at round 8), imported at
    `f24`, against ControlLossModel imported at the same round."""
    import control_loss_ref as cl
    import test_gpu_control_loss as tc
    case = tc.CASES["nib263"]
    h, r0 = OFFSETS["f24"]
    n, c = case["n"], case["cfg"]
    state = sc.full_state(n, hb0=h, ts0=r0)
    eng = gs.Engine(gs.default_config(n, **c))
    model = cl.ControlLossModel(n, c["fanout"], c["t_fail"], c["t_cleanup"], c["seed"])
    seen = []
    try:
        eng.import_state(*state, r0)
        model.import_state(*state, r0)
        for x in (eng, model):
            x.set_loss(case["out"], case["inn"])
            x.set_control_loss(case["kinds"])
        assert eng.tier_info()[0] == 1 and case["side"] is None
        model_lockstep(eng, model, tc.compare, shifted(case["sched"], r0), r0 + 1, r0 + case["rounds"],
                       per_round=lambda r, st: seen.append((eng.tier_info(full=True)[3],
                                                            st["tombstoned"] + st["remove_unknown"])))
        assert any(v == 3 and rm > 0 for v, rm in seen), seen
        assert model.ctl["remove_missed"] > 0
    finally:
        eng.close()


ENS_STARTS = [("p30", 2**30, 2**30 - 1, 2**30), ("f24", 2**24 - 6, 2**24 - 9, 2**24 - 8)]


@pytest.mark.parametrize("start,hb0,ts0,r0", ENS_STARTS, ids=[x[0] for x in ENS_STARTS])
@pytest.mark.parametrize("name", ["n64k3", "n33k3"])
def test_counter_ensembles(gs, name, start, hb0, ts0, r0):
    """The ensemble groups n64k3 and n33k3 from init_full(hb0, ts0 = R0 - 1,
    R0) at 2^30 and at 2^24 - 8, per round against ensemble_ref.run on
    LossModel imported at the same round."""
    import ensemble_ref as er
    import test_gpu_ensemble as te
    cases = [dict(c, crash={r0 + r: ms for r, ms in c["crash"].items()}) for c in er.GROUPS[name]]
    n, rounds = cases[0]["n"], cases[0]["rounds"]
    state = sc.full_state(n, hb0, ts0)
    traces = [er.run(er.model(c, state, r0), rounds, c["crash"]) for c in cases]
    assert sum(er.total(t, "detections") for t in traces) > 0
    ens, cs = te.make(gs, cases)
    with ens:
        ens.init_full(hb0, ts0, r0)
        for q in range(rounds):
            te.crash_round(ens, cs, r0 + q + 1)
            te.check_round(ens, ens.step(1), traces, q, f"{name} from {start}")
