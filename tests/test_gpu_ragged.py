"""The nibble path (csrc/round.hip: k_round IN 2 / 4 / 6 / 7, k_round_jobs,
k_round_jobs_flat, k_round_redo, the quirk pre-pass k_quirk_rows /
k_quirk_sum32, k_census) at cluster sizes that are no multiple of its
geometry: a 256-member tile, a 256-row block, a 16-cell lane, an 8-cell chunk
in one 32-bit word, 2,048-cell quirk windows and columns padded to a multiple
of 2,048. The rest of the suite asserts that this path ran only at N = 2,048
and at full-size powers of two, where every tile, row block, lane and chunk is
whole; its ragged sizes compare tables without asking which variant ran, with
crashes drawn by seed.

Here the sizes are 250 (one partial tile), 263 (a full tile plus 7 cells: a
last chunk of 7 real cells and one padding cell, seven of eight tiles padding
only), 520 (a last lane of exactly one chunk), 1,000 (N % 16 = 8, a row-block
tail of 232) and 2,049 (one row and one column past eight full tiles and past
the first quirk window). The crashed members are scenarios.tail_members: the
last cell, the first cell of the last lane and of the last chunk, both sides
of the last tile boundary and of every shard boundary, so REMOVE bits,
tombstones, escapes and lane jobs land beside the padding. Every run is
bit-exact against the oracle (oracle/tablesim.c) every round -- stats, hb,
ts, alive, failed set, detectors, the maintained row counts -- and the runs
on one engine assert which k_round variant ran and that no padding cell is
ever visible. tests/test_ragged_scenario.py holds the preconditions on the
oracle. GH_PLANE=1 keeps the plane and the tier at these sizes.
Run on a MI355X: pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

import journal_ref as jr
import scenarios as sc
from census_ref import assert_census_equal, census_ref
from test_gpu_call_partition import Scenario, assert_final, remove_inside_hook, run_case
from test_gpu_parity import compare
from test_gpu_sharded import run_group
from test_gpu_tier8 import ranged_state, remove_run

pytestmark = pytest.mark.gpu

ROUNDS = sc.RAGGED_ROUNDS
HEALTHY = range(2, sc.RAGGED_CRASH)  # rounds 2..7: the table is in the tier, nothing has crashed


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def tier_on(monkeypatch):
    monkeypatch.setenv("GH_PLANE", "1")
    monkeypatch.delenv("GH_C8", raising=False)


# ---- what the engine's diagnostics show of a row's tier cells ----------------------------

def tier_cells(eng, row, c0, cnt):
    """gh_debug_tier: (lag code << 4) | age nibble of the cells [c0, c0 + cnt)
    of row `row` in the current buffer, 0xFF for an absent cell, a cell of an
    escaped chunk, or any cell of a 16-bit buffer."""
    eng.lib.gh_debug_tier.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
    out = np.zeros(cnt, np.uint8)
    assert eng.lib.gh_debug_tier(eng.h, row, c0, cnt, out.ctypes.data_as(C.c_void_p)) == 0, (row, c0, cnt)
    return out


def pad_rows(n):
    """rows 0, 255, 256 (both sides of the first row-block edge) where they exist, and the last"""
    return sorted({i for i in (0, 255, 256, n - 1) if i < n})


def check_padding(eng, n, r):
    """The padding cells of the last real lane, columns n .. 16 * ceil(n / 16),
    read 0xFF: absent or in an escaped chunk, never visible."""
    end = -(-n // 16) * 16
    assert end > n  # (every size here has a partial last lane)
    for row in pad_rows(n):
        cells = tier_cells(eng, row, n, end - n)
        assert (cells == 0xFF).all(), f"r={r}: row {row}, padding columns {n}..{end - 1} read {cells.tolist()}"


def is_tier_tombstone(v):
    """lag code 15 with an age nibble 1..14 (gh_internal.h: a4)"""
    return v != 0xFF and (v >> 4) == 15 and 1 <= (v & 15) <= 14


def last_running_row(n, victims):
    return max(i for i in range(n) if i not in victims)


# ---- 1. the crash wave on one engine --------------------------------------------------------

_WAVES = {}


def stepwise_wave(gs, om, n, k):
    """The wave at (n, k) on one engine, one round per call, checked against
    the oracle every round (remove_run: stats, tables, failed set, detectors,
    the maintained counts); kept per (n, k): (trace, final export, per round
    diagnostics) for the tests that compare another run with it."""
    if (n, k) not in _WAVES:
        victims = sc.tail_members(n)
        probe_rows = [0, last_running_row(n, victims), n - 1]
        diag = {}

        def per_round(eng, r):
            check_padding(eng, n, r)
            tombs = {row: 0 for row in probe_rows}
            for row in probe_rows:
                for c in victims:
                    tombs[row] += bool(is_tier_tombstone(int(tier_cells(eng, row, c & ~7, 8)[c & 7])))
            diag[r] = dict(launched=eng.debug_variant(), tombs=tombs, enc=eng.encoding_info(full=True),
                           tier=eng.tier_info(full=True), jobs=eng.job_info())

        trace, final = remove_run(gs, om, n, sc.ragged_cfg(k), sc.ragged_wave(n), ROUNDS, per_round=per_round)
        _WAVES[n, k] = (trace, final, diag)
    return _WAVES[n, k]


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("n", sc.RAGGED_NS)
def test_ragged_crash_wave(gs, oracle_mod, n, k):
    """tail_members(n) crash at round 8, are detected (rounds 23 / 24) and
    REMOVE'd (24 / 25); the last member rejoins at round 30, whose base jump
    makes lane jobs of the last, partial lane. Every round: parity, the
    maintained counts, the padding cells of rows 0, 255, 256 and N - 1. The
    nibble path ran the healthy rounds 2..7 and every round that made
    tombstones, its REMOVE-taking form (debug_variant 4) at least one of them,
    lane jobs ran, and tier tombstones (lag code 15, age nibble 1..14) appear
    in the victims' columns of row 0 and of the last running row. Row N - 1 is
    itself a victim: stopped through the REMOVE round, its chunks stay escaped
    (gh_internal.h: a4), and the row it restarts with at round 30 never held
    the other victims, so it shows no tombstone, which is asserted too."""
    victims = sc.tail_members(n)
    trace, _, diag = stepwise_wave(gs, oracle_mod, n, k)
    rows = [(r, s["detections"], s["tombstoned"], s["released"], var, diag[r]["launched"], jobs, diag[r]["enc"],
             diag[r]["tombs"]) for r, (s, var, jobs) in enumerate(trace, 1)]
    print(f"N={n} k={k}: (round, detections, tombstoned, released, variant, launched, lane jobs, encoding_info, "
          f"tier tombstones by row)")
    for x in rows:
        print("  ", x)
    tomb_rounds = [r for r, (s, _, _) in enumerate(trace, 1) if s["tombstoned"] > 0]
    assert tomb_rounds and any(s["detections"] for s, _, _ in trace), rows
    assert all(trace[r - 1][1] == 3 for r in HEALTHY), rows
    assert all(trace[r - 1][1] == 3 for r in tomb_rounds), rows
    assert 4 in {diag[r]["launched"] for r in tomb_rounds}, rows
    assert any(trace[r - 1][2] > 0 for r in range(sc.RAGGED_CRASH, ROUNDS + 1)), rows
    seen = {row: sum(diag[r]["tombs"][row] for r in diag) for row in diag[1]["tombs"]}
    assert seen[0] > 0 and seen[last_running_row(n, victims)] > 0, seen
    assert seen[n - 1] == 0, seen


# ---- 2. escaped chunks that share their word with padding --------------------------------------

@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("n", [263, 1000])
def test_ragged_escapes(gs, oracle_mod, n, k):
    """test_gpu_tier8.test_tier_escapes_exact at ragged N: lags, ages and
    tombstones outside the nibbles, so chunks are escaped, the last real chunk
    (7 real cells and one padding cell at N = 263) among them. (At N = 1,000
    the two rounds in which the imported ages pass the narrow age field in
    every row at once take the engine 3 and 6 s, as one does at N = 1,024 in
    test_tier_escapes_exact: these two cases take 8 to 11 s, DESIGN.md.)"""
    cfg = dict(fanout=k, seed=0x5EED0110 + k, t_fail=60, t_cleanup=60)
    eng = gs.Engine(gs.default_config(n, **cfg))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    esc = []
    try:
        hb, ts, alive = ranged_state(n, k)
        eng.import_state(hb, ts, alive, 40)
        orc.import_state(hb, ts, alive, 40)
        for r in range(1, 16):
            s1, s2 = eng.step(1), orc.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != cpu {s2}"
            compare(eng, orc, r)
            check_padding(eng, n, r)
            esc.append(eng.tier_info()[2])
    finally:
        eng.close()
        orc.close()
    assert sum(esc) > 0, esc


# ---- 3. shards whose last one is short ----------------------------------------------------------

@pytest.mark.parametrize("label,n,world,layout", sc.RAGGED_SHARDS, ids=[x[0] for x in sc.RAGGED_SHARDS])
def test_ragged_shards(gs, oracle_mod, label, n, world, layout):
    """The wave over column shards (ncs = 160, 96 and 32 columns: the last
    shard holds 103, 71 and 26) and row shards (nrs = 132, 88 and 334 rows:
    the last holds 131, 87 and 332), the victims the tail members and both
    sides of every shard boundary; the group's table against the oracle's
    every round. Row shards: every shard kept the tier and ran the nibble
    path in the healthy rounds."""
    victims = sc.tail_members(n, sc.shard_bounds(n, world, layout))
    seen = {}

    def per_round(grp, r):
        if layout == 1:
            seen[r] = grp.run("tier_info", full=True)

    run_group(gs, oracle_mod, world, dict(shard_layout=layout, **sc.ragged_cfg(4)), n, ROUNDS,
              sc.ragged_wave(n, victims), init=sc.full_state(n), per_round=per_round)
    if layout == 1:
        print(f"{label}: per round, every shard's variant: { {r: [x[3] for x in v] for r, v in seen.items()} }")
        for r in range(3, sc.RAGGED_CRASH):  # (round 2 still fills the ghost table's tier)
            for g, (kept, _, _, variant) in enumerate(seen[r]):
                assert kept == 1 and variant == 3, (r, g, seen[r])


# ---- 4. the quirk pre-pass at the row's end ---------------------------------------------------------

@pytest.mark.parametrize("crash", sc.RAGGED_QUIRK_CRASH, ids=["crash8", "crash1"])
@pytest.mark.parametrize("quirk_rows", [1, 0], ids=["rows1", "rows0"])
@pytest.mark.parametrize("n", sorted(sc.RAGGED_QUIRK))
def test_ragged_quirk(gs, oracle_mod, monkeypatch, n, quirk_rows, crash):
    """Quirk detection (detect_mode 1) with the one-pass row walk k_quirk_rows
    (GH_QUIRK_ROWS=1) and the two-sweep pre-pass: candidate runs that end on
    the row's last list entry and, at N = 2,049, cross the edge of the first
    2,048-cell window, whose second window holds one real cell. crash8 is the
    wave's schedule; crash1 (the victims never heartbeat, every row detects
    the whole run in round 17) is the one on which the oracle's quirk and
    canonical detections differ (test_ragged_scenario.py)."""
    monkeypatch.setenv("GH_QUIRK_ROWS", str(quirk_rows))
    sched = sc.ragged_wave(n, sc.RAGGED_QUIRK[n], crash=crash)
    rounds = ROUNDS if crash == sc.RAGGED_CRASH else crash + 20

    def created(eng):
        assert eng.knobs()["GH_QUIRK_ROWS"] == quirk_rows, eng.knobs()

    trace, _ = remove_run(gs, oracle_mod, n, sc.ragged_cfg(4, 1), sched, rounds, on_create=created,
                          per_round=lambda eng, r: check_padding(eng, n, r))
    assert any(s["detections"] for s, _, _ in trace)
    if crash == sc.RAGGED_CRASH:
        assert any(s["tombstoned"] for s, _, _ in trace)
    else:  # the run's skipped candidates are detected a round after the others
        det = [r for r, (s, _, _) in enumerate(trace, 1) if s["detections"]]
        assert det[:2] == [crash + 16, crash + 17], det


# ---- 5. the switches that change tail code -------------------------------------------------------------

KNOBS = [("GH_DNW", 0), ("GH_NREC", 0), ("GH_JOBS_FLAT", 0), ("GH_JOBS_FLAT", 1), ("GH_ROUND_XMAP", 0),
         ("GH_ROUND_XMAP", 2), ("GH_NIB_RMV", 0), ("GH_NIB_RMV", 2), ("GH_RMV_FULL7", 0), ("GH_RMV_FULL7", 1)]


@pytest.mark.parametrize("knob,value", KNOBS, ids=[f"{k}={v}" for k, v in KNOBS])
def test_ragged_knobs(gs, oracle_mod, monkeypatch, knob, value):
    """N = 263, k = 4, the wave, with one switch set and asserted through
    knobs(): the moves
    derived from the bases over padded columns, rows staged from the inboxes
    in a partial row block, region and flat dealing of the lane jobs, the
    tile maps when seven of eight tiles are padding, the REMOVE forms on 1/8
    of the grid and on all of it. Parity and the counts every round; the
    final tables are the default engine's."""
    n = 263
    monkeypatch.setenv(knob, str(value))

    def created(eng):
        assert eng.knobs()[knob] == value, eng.knobs()

    trace, final = remove_run(gs, oracle_mod, n, sc.ragged_cfg(4), sc.ragged_wave(n), ROUNDS, on_create=created,
                              per_round=lambda eng, r: check_padding(eng, n, r))
    assert any(s["tombstoned"] for s, _, _ in trace) and any(s["detections"] for s, _, _ in trace)
    assert all(trace[r - 1][1] == 3 for r in HEALTHY), trace  # the switch leaves the nibble path in place
    monkeypatch.delenv(knob)
    assert_final(final, stepwise_wave(gs, oracle_mod, n, 4)[1], f"{knob}={value}")


# ---- 6. the wave in few gh_step calls ---------------------------------------------------------------------

@pytest.mark.parametrize("part", ["fewest", "remove_inside"])
@pytest.mark.parametrize("n", [263, 1000])
def test_ragged_batched_calls(gs, oracle_mod, n, part):
    """The wave in multi-round calls (test_gpu_call_partition.py's helpers):
    `fewest` is the calls 1..7, 8..29, 30..40, `remove_inside` ends a call on
    the REMOVE round d + 1, d read from a stepwise oracle run, so the REMOVE
    round runs inside a call as the looped 1/8-grid form. The tables after
    every call against the oracle, the final ones against the stepwise
    engine's."""
    scen = Scenario(("ragged", n), n, sc.ragged_cfg(4), sc.ragged_wave(n), ROUNDS)
    d = scen.d(oracle_mod)
    assert sc.RAGGED_CRASH < d and d + 1 < sc.RAGGED_REJOIN, d
    seen = []
    final = run_case(gs, oracle_mod, scen, part, at_call_end=remove_inside_hook(scen, oracle_mod, part, seen))
    if part == "remove_inside":
        assert seen == [d + 1], seen
    assert_final(final, stepwise_wave(gs, oracle_mod, n, 4)[1], f"N={n}/{part}")


# ---- 7. census and journal over padded columns ----------------------------------------------------------------

@pytest.mark.parametrize("n", [263, 1000])
def test_ragged_census_journal(gs, oracle_mod, n):
    """gh_census and the journal's census pass (GH_JOURNAL_VIEWS) on the wave:
    census() against the numpy census of the ORACLE's export (census_ref.py)
    after every round -- round 7 (healthy, the table in the tier), the REMOVE
    round and round 40 among them, which are asserted to be -- and journal()
    and journal_rounds() against journal_ref.py fed from the oracle. A padding
    cell counted as listed would show in listed, age_hist or missing_views."""
    cfg, sched = sc.ragged_cfg(4), sc.ragged_wave(n)
    eng = gs.Engine(gs.default_config(n, **cfg))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    try:
        eng.import_state(*sc.full_state(n), 0)
        orc.import_state(*sc.full_state(n), 0)
        eng.journal_enable(jr.VIEWS, 64)
        ref = jr.JournalRef(n, orc.export_state()[2], jr.VIEWS, 64)
        checked, tiered, tomb_rounds = [], [], []
        for r in range(1, ROUNDS + 1):
            if sched.get(r):
                eng.apply_events(sched[r])
                orc.apply_events(sched[r])
            s1, s2 = eng.step(1), orc.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != cpu {s2}"
            hb, ts, alive = orc.export_state()
            want = census_ref(hb, ts, alive, r)
            assert_census_equal(eng.census(), want, f"N={n} round {r}")
            checked.append(r)
            if eng.tier_info()[1] == 1:
                tiered.append(r)
            if s2["tombstoned"]:
                tomb_rounds.append(r)
            ref.observe(r, alive, listed=want.listed, **jr.detection_inputs(orc, s2))
        assert 7 in tiered and tomb_rounds and set(tomb_rounds) <= set(checked) and checked[-1] == ROUNDS == 40
        assert eng.journal_total() == ROUNDS
        jr.assert_journal_equal(eng.journal(), eng.journal_rounds(), ref, f"N={n}")
        compare(eng, orc, ROUNDS)
    finally:
        eng.close()
        orc.close()
