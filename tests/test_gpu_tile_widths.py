"""GPU parity at every tile width gh_config.tile_width takes (8, 16, 32, 64,
128, 256). Almost every kernel is tile-shaped -- k_round and k_seg are
instantiated per TW, round_rb<TW>() sizes the row block, the census, groups
and file passes take their lane shape from d.lgtw / d.tw -- but the rest of the
suite leaves the two defaults (64 without the sender plane, 256 with it) only
in three tests written before the 4-bit tier's nibble path and the later
features existed. Every engine here first asserts knobs()["GH_TILE_W"], on
every shard of a group: a sweep that silently ran at the default would pass
everything else.

Part A: the nibble path at 64- and 128-member tiles. With GH_PLANE=1 an engine
keeps the 4-bit tier from tile_width 64 up (gossiphip.cpp c8), so 64 and 128
run round_block_nib<64|128> -- 4 and 8 16-cell lanes per segment instead of 16,
no split-gather form, ld padded to 8 * TW -- in the healthy
rounds and as the REMOVE-taking form. test_gpu_ragged.py's crash wave, with
victims on both sides of the first and the last tile boundary of that width
(scenarios.width_victims), asserts which variant ran, lane jobs, tier
tombstones and padding cells as it does at 256.

Part B: off the plane at N = 300 (no multiple of 8: a partial last tile and
chunk at every width) the read-only passes -- gh_census, gh_groups, the
journal's GH_JOURNAL_VIEWS pass, gh_vote_scan, gh_lsm, gh_file_audit and
gh_file_select -- after every round against their references fed from the
ORACLE's export, on one engine and on shards; and the smallest case of each
later feature (partitions, lossy control messages, lossy links,
GH_REMOVE_LIST, GH_ORDER_APPEND) through its own module's runner.

Every comparison is equality with the model the feature was built against.
tests/test_tile_width_scenario.py holds the preconditions on the oracle.
Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import groups_ref as gr
import journal_ref as jr
import scenarios as sc
from census_ref import assert_census_equal, census_ref
from file_audit_ref import assert_audit_equal, file_audit_ref, file_select_ref
from oracle import election as el
from test_gpu_call_partition import Scenario, assert_final, remove_inside_hook, run_case
from test_gpu_config_space import make_engine
from test_gpu_counters import append_order_ring_quirk, nibble_from
from test_gpu_parity import compare, run_parity
from test_gpu_ragged import check_padding, is_tier_tombstone, last_running_row, pad_rows, tier_cells
from test_gpu_tier8 import ranged_state, remove_run

pytestmark = pytest.mark.gpu

ROUNDS = sc.RAGGED_ROUNDS
TIER = sc.TIER_WIDTHS                          # part A, and the features' tier cases
OFF_DEFAULT = (8, 16, 32, 128, 256)            # part B's features off the plane (64 is the rest of the suite)
# csrc/round.hip round_rb<TW>(): GH_WG_ROWS_WIDE = 256 rows from TW = 128 up, else GH_WG_CELLS / TW = 16,384 / TW
# within [64, 1,024]: the rows of one k_round workgroup
ROUND_RB = {8: 1024, 16: 1024, 32: 512, 64: 256, 128: 256, 256: 256}
ALIVE = -1  # GH_AVAIL_ALIVE


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in ("GH_PLANE", "GH_C8", "GH_TILE_W", "GH_TMODE", "GH_GX_DIRECT", "GH_QUIRK_ROWS"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def tier_on(monkeypatch):
    monkeypatch.setenv("GH_PLANE", "1")


def assert_width(eng, tw, tier=None):
    """The tile width in effect on the engine, or on every shard of a group;
    `tier`: whether each keeps the plane and the 4-bit tier."""
    for g, kn in enumerate(eng.run("knobs") if hasattr(eng, "engines") else [eng.knobs()]):
        assert kn["GH_TILE_W"] == tw, (g, tw, kn)
        if tier is not None:
            assert (kn["GH_PLANE"], kn["GH_C8"]) == (int(tier), int(tier)), (g, kn)


def created(tw, tier=None):
    return lambda eng: assert_width(eng, tw, tier)


# =============================================================================================
# Part A: the nibble path at TW = 64 and 128
# =============================================================================================

def test_row_block_of_the_tier_widths():
    """check_padding's rows 0, 255, 256 and N - 1 are the rows 0, RB - 1, RB
    and N - 1 of both widths: round_rb<64>() = 16,384 / 64 and round_rb<128>()
    = GH_WG_ROWS_WIDE are 256, as round_rb<256>() is."""
    for tw in TIER:
        rb = ROUND_RB[tw]
        assert rb == 256
        for n in sc.WIDTH_NS:
            assert pad_rows(n) == sorted({0, rb - 1, rb, n - 1})


_WAVES = {}


def width_wave(gs, om, n, k, tw, h=2, r0=0):
    """The wave at (n, k) on one engine of tile width tw from full_state(n, h,
    r0), the victims width_victims(n, tw), one round per call, checked against
    the oracle every round (remove_run: stats, hb, ts, alive, failed set,
    detectors, gh_debug_counts) with the padding cells; kept per case: (trace,
    final export, per-round diagnostics keyed by the round counted from the
    import)."""
    key = (n, k, tw, h, r0)
    if key not in _WAVES:
        victims = sc.width_victims(n, tw)
        probe_rows = [0, last_running_row(n, victims), n - 1]
        diag = {}

        def per_round(eng, r):
            check_padding(eng, n, r)
            tombs = {row: 0 for row in probe_rows}
            for row in probe_rows:
                for c in victims:
                    tombs[row] += bool(is_tier_tombstone(int(tier_cells(eng, row, c & ~7, 8)[c & 7])))
            diag[r - r0] = dict(launched=eng.debug_variant(), tombs=tombs, enc=eng.encoding_info(full=True),
                                tier=eng.tier_info(full=True), jobs=eng.job_info())

        trace, final = remove_run(gs, om, n, dict(sc.ragged_cfg(k), tile_width=tw), sc.shifted_wave(n, r0, victims),
                                  ROUNDS, on_create=created(tw, tier=True), per_round=per_round,
                                  init=sc.full_state(n, hb0=h, ts0=r0), round0=r0)
        _WAVES[key] = (trace, final, diag)
    return _WAVES[key]


def assert_wave_pins(what, n, victims, trace, diag, first=2):
    """What test_ragged_crash_wave asserts: the nibble path (variant 3) ran in
    the healthy rounds first..7 and in every round that made tombstones, its
    REMOVE-taking form (debug_variant 4) in one of them, lane jobs ran, tier
    tombstones stand in the victims' columns of row 0 and of the last running
    row and never in row N - 1 (a victim: its chunks stay escaped while it is
    stopped, and the row it rejoins with never held the others)."""
    rows = [(r, s["detections"], s["tombstoned"], s["released"], var, diag[r]["launched"], jobs, diag[r]["enc"],
             diag[r]["tombs"]) for r, (s, var, jobs) in enumerate(trace, 1)]
    print(f"{what}: (round, detections, tombstoned, released, variant, launched, lane jobs, encoding_info, "
          f"tier tombstones by row)")
    for x in rows:
        print("  ", x)
    assert len(trace) == ROUNDS
    tomb_rounds = [r for r, (s, _, _) in enumerate(trace, 1) if s["tombstoned"] > 0]
    assert tomb_rounds and any(s["detections"] for s, _, _ in trace), rows
    assert all(trace[r - 1][1] == 3 for r in range(first, sc.RAGGED_CRASH)), rows
    assert all(trace[r - 1][1] == 3 for r in tomb_rounds), rows
    assert 4 in {diag[r]["launched"] for r in tomb_rounds}, rows
    assert any(trace[r - 1][2] > 0 for r in range(sc.RAGGED_CRASH, ROUNDS + 1)), rows
    seen = {row: sum(diag[r]["tombs"][row] for r in diag) for row in diag[1]["tombs"]}
    assert seen[0] > 0 and seen[last_running_row(n, victims)] > 0, seen
    assert seen[n - 1] == 0, seen


@pytest.mark.parametrize("k", [3, 4])
@pytest.mark.parametrize("tw", TIER)
@pytest.mark.parametrize("n", sc.WIDTH_NS)
def test_width_crash_wave(gs, oracle_mod, tier_on, n, tw, k):
    """test_ragged_crash_wave at 64- and 128-member tiles, N = 263 (ld 512 and
    1,024: eight tiles, three and five of them padding only) and N = 1,000 (ld
    1,024: 16 and 8 tiles). The victims stand on both sides of the first and of
    the last tile boundary (64 | 128, and 256, 960 | 896), on the first cell of
    the last lane and chunk and on the last cell; they crash at round 8, are
    detected (23 / 24) and REMOVE'd (24 / 25), the last member rejoins at 30.
    Parity, the maintained counts and the padding cells of rows 0, RB - 1, RB
    and N - 1 every round; the variant, lane-job and tombstone pins of
    assert_wave_pins."""
    trace, _, diag = width_wave(gs, oracle_mod, n, k, tw)
    assert_wave_pins(f"N={n} TW={tw} k={k}", n, sc.width_victims(n, tw), trace, diag)


@pytest.mark.parametrize("tw", TIER)
def test_width_counter_offset(gs, oracle_mod, tier_on, tw):
    """The wave at N = 263, k = 4 from the counter offset `f24` (heartbeats and
    rounds through 2^24): the import lies beyond the bases' narrow range, so
    the nibble path is demanded from round 4 on (test_gpu_counters.nibble_from)."""
    n = 263
    h, r0 = sc.COUNTER_OFFSETS["f24"]
    trace, final, diag = width_wave(gs, oracle_mod, n, 4, tw, h, r0)
    assert_wave_pins(f"f24: N={n} TW={tw}", n, sc.width_victims(n, tw), trace, diag, first=nibble_from(h))
    assert final[0].diagonal().max() == h + ROUNDS > 2**24


@pytest.mark.parametrize("tw", TIER)
def test_width_escapes(gs, oracle_mod, tier_on, tw):
    """test_ragged_escapes at N = 263, k = 4: ranged_state's lags, ages and
    tombstones outside the nibbles, so chunks are escaped, the last real chunk
    (7 real cells and one padding cell) among them."""
    n, k = 263, 4
    cfg = dict(fanout=k, seed=0x5EED0110 + k, t_fail=60, t_cleanup=60, tile_width=tw)
    eng = gs.Engine(gs.default_config(n, **cfg))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    esc = []
    try:
        assert_width(eng, tw, tier=True)
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


@pytest.mark.parametrize("part", ["fewest", "remove_inside"])
@pytest.mark.parametrize("tw", TIER)
def test_width_batched_calls(gs, oracle_mod, tier_on, tw, part):
    """test_ragged_batched_calls at N = 263: `fewest` is the calls 1..7,
    8..29, 30..40, `remove_inside` ends a call on the REMOVE round d + 1, which
    then runs inside a call as the looped 1/8-grid form (debug_variant 4). The
    tables after every call against the oracle, the final ones against the
    stepwise engine's of the same width."""
    n = 263
    victims = sc.width_victims(n, tw)
    scen = Scenario(("width", n, tw), n, dict(sc.ragged_cfg(4), tile_width=tw), sc.ragged_wave(n, victims), ROUNDS)
    d = scen.d(oracle_mod)
    assert sc.RAGGED_CRASH < d and d + 1 < sc.RAGGED_REJOIN, d
    seen = []
    final = run_case(gs, oracle_mod, scen, part, on_create=created(tw, tier=True),
                     at_call_end=remove_inside_hook(scen, oracle_mod, part, seen))
    if part == "remove_inside":
        assert seen == [d + 1], seen
    assert_final(final, width_wave(gs, oracle_mod, n, 4, tw)[1], f"TW={tw}/{part}")


@pytest.mark.parametrize("quirk_rows", [0, 1], ids=["rows0", "rows1"])
@pytest.mark.parametrize("tw", TIER)
def test_width_quirk_crash1(gs, oracle_mod, tier_on, monkeypatch, tw, quirk_rows):
    """test_ragged_quirk's crash1 schedule at N = 263: RAGGED_QUIRK's run of
    candidates 254, 255, 256 crosses the last tile boundary of both widths and
    ends on the row's last list entry; the victims never heartbeat, every row
    detects the whole run in round 17 and the quirk skips every second
    candidate. GH_QUIRK_ROWS=0 is the two-sweep pre-pass (k_quirk_sum32 over
    tier chunks), =1 the one-pass row walk. The healthy rounds 2..7 run the
    nibble path."""
    n = 263
    monkeypatch.setenv("GH_QUIRK_ROWS", str(quirk_rows))

    def on_create(eng):
        assert_width(eng, tw, tier=True)
        assert eng.knobs()["GH_QUIRK_ROWS"] == quirk_rows, eng.knobs()

    trace, _ = remove_run(gs, oracle_mod, n, dict(sc.ragged_cfg(4, 1), tile_width=tw),
                          sc.ragged_wave(n, sc.RAGGED_QUIRK[n], crash=1), 21, on_create=on_create,
                          per_round=lambda eng, r: check_padding(eng, n, r))
    det = [r for r, (s, _, _) in enumerate(trace, 1) if s["detections"]]
    assert det[:2] == [17, 18], det
    assert all(trace[r - 1][1] == 3 for r in range(2, 8)), [t[1] for t in trace]


@pytest.mark.parametrize("label,world,layout", sc.WIDTH_SHARDS, ids=[x[0] for x in sc.WIDTH_SHARDS])
@pytest.mark.parametrize("tw", TIER)
def test_width_shards(gs, oracle_mod, tier_on, tw, label, world, layout):
    """test_ragged_shards at N = 263 on 3 column shards (96 columns each: one
    and a half 64-member tiles, less than one of 128) and 2 row shards, the
    victims on both sides of every tile and shard boundary; the whole group's
    table against the oracle every round. Row shards: every shard kept the
    tier and ran the nibble path in the rounds 3..7 (round 2 still fills the
    ghost table's tier)."""
    n = 263
    victims = sc.width_victims(n, tw, world, layout)
    seen = {}

    def per_round(grp, r):
        if layout == 1:
            seen[r] = grp.run("tier_info", full=True)

    trace, _ = remove_run(gs, oracle_mod, n, dict(sc.ragged_cfg(4), tile_width=tw), sc.ragged_wave(n, victims), ROUNDS,
                          world=world, layout=layout, on_create=created(tw, tier=True), per_round=per_round)
    assert any(s["detections"] for s, _, _ in trace) and any(s["tombstoned"] for s, _, _ in trace)
    if layout == 1:
        print(f"{label} TW={tw}: per round, every shard's variant: { {r: [x[3] for x in v] for r, v in seen.items()} }")
        for r in range(3, sc.RAGGED_CRASH):
            for g, (kept, _, _, variant) in enumerate(seen[r]):
                assert kept == 1 and variant == 3, (r, g, seen[r])


# =============================================================================================
# Part B: the read-only passes and the later features at all six widths, off the plane
# =============================================================================================

PASS_ROUNDS, PASS_FILES, PASS_LOG = 30, 200, 64


def audit_from_oracle(eng, orc, hb, alive, observers, what):
    """gh_file_audit and gh_file_select of every observer against
    file_audit_ref.py on the ORACLE's replica table, master list and views."""
    n = orc.n
    rep, ver, _, _ = orc.export_files()
    cand = orc.lsm(0)[0]
    R = rep.shape[1]
    for obs in observers:
        avail = (alive != 0) if obs == ALIVE else (hb[obs] >= 0)
        want = file_audit_ref(rep, ver, avail, n, cand)
        assert_audit_equal(eng.file_audit(obs), want, f"{what} observer {obs}")
        loaded = int(np.argmax(want.load))
        for member, mw in ((-1, R - 1), (loaded, 8), (-1, 0)):
            np.testing.assert_array_equal(eng.file_select(obs, member, mw), file_select_ref(rep, ver, avail, n, member, mw),
                                          err_msg=f"{what} select({obs}, {member}, {mw})")


def run_passes(gs, om, tw, layout="single", rounds=PASS_ROUNDS, cfg_width=None):
    """width_churn at N = 300 from width_state on an engine (or group) of tile
    width tw, compared with the oracle every round; after every round, fed
    from the oracle's export: gh_census, gh_groups, gh_vote_scan, gh_lsm of
    rows 0, 1, a stopped row and N - 1, from round 2 on (files put in round 2)
    gh_file_audit and gh_file_select from row 0, a stopped row and
    GH_AVAIL_ALIVE; at the end the journal (GH_JOURNAL_VIEWS), gh_repair from
    two observers and gh_get_files. Returns what the table went through."""
    n = sc.WIDTH_N
    base, sched = sc.width_churn(n, PASS_ROUNDS)
    cfg = dict(base, max_files=PASS_FILES, tile_width=tw if cfg_width is None else cfg_width)
    eng = make_engine(gs, n, cfg, layout)
    orc = om.Oracle(om.default_config(n, **cfg), threads=8)
    what = f"TW={tw} {layout}"
    rng = np.random.default_rng(tw)
    seen = dict(stopped=0, tombs=0, absent=0, wide=0, detections=0)
    try:
        assert_width(eng, tw, tier=False)
        state = sc.width_state(n)
        eng.import_state(*state, 0)
        orc.import_state(*state, 0)
        wide0 = [e.encoding_info()[0] for e in getattr(eng, "engines", [eng])]
        assert sum(wide0) > 0, wide0  # wide segments from the import on
        eng.journal_enable(jr.VIEWS, PASS_LOG)
        ref = jr.JournalRef(n, state[2], jr.VIEWS, PASS_LOG)
        files = np.arange(0, PASS_FILES, 2, dtype=np.int32)
        for r in range(1, rounds + 1):
            if sched.get(r):
                eng.apply_events(sched[r])
                orc.apply_events(sched[r])
            s1, s2 = eng.step(1), orc.step(1)
            assert s1 == s2, f"{what} round {r}: gpu {s1} != cpu {s2}"
            compare(eng, orc, r)
            hb, ts, alive = orc.export_state()
            msg = f"{what} round {r}"
            want = census_ref(hb, ts, alive, r)
            assert_census_equal(eng.census(), want, msg)
            gr.assert_groups_equal(eng.groups(), gr.groups_ref(hb, alive), msg)
            ref.observe(r, alive, listed=want.listed, **jr.detection_inputs(orc, s2))
            for mv in (np.zeros(n, np.int32), rng.integers(0, n, n).astype(np.int32)):
                for g, e, name in zip(eng.vote_scan(mv), el.vote_scan(hb, mv), ("first", "list_len", "has_master")):
                    np.testing.assert_array_equal(g, e, err_msg=f"{msg} vote_scan {name}")
            stopped = np.flatnonzero(alive == 0)
            probe = [0, 1, n - 1] + [int(x) for x in stopped[:1]]
            for row in probe:
                for x, y, name in zip(eng.lsm(row), orc.lsm(row), ("ids", "hb", "ts")):
                    np.testing.assert_array_equal(x, y, err_msg=f"{msg} lsm({row}) {name}")
            if r == 2:
                for x, y in zip(eng.put(files), orc.put(files)):
                    np.testing.assert_array_equal(x, y, err_msg=f"{msg} put")
            if r >= 2:
                audit_from_oracle(eng, orc, hb, alive, [ALIVE, 0] + [int(x) for x in stopped[:1]], msg)
            run = alive != 0
            col = hb[:, n - 3].astype(np.int64)
            seen["stopped"] += int(len(stopped) > 0)
            seen["tombs"] += int((hb[run] == -2).any())
            seen["absent"] += int((hb[run] == -1).any())
            seen["wide"] += int((col >= 0).any() and col[col >= 0].max() - col[col >= 0].min() > 2**16)
            seen["detections"] += s2["detections"]
        assert eng.journal_total() == rounds
        jr.assert_journal_equal(eng.journal(), eng.journal_rounds(), ref, what)
        for obs in (0, 1):
            assert eng.repair(obs) == orc.repair(obs), f"{what} repair({obs})"
        allf = np.arange(PASS_FILES, dtype=np.int32)
        for x, y in zip(eng.get_files(allf), orc.get_files(allf)):
            np.testing.assert_array_equal(x, y, err_msg=f"{what} get_files")
        audit_from_oracle(eng, orc, hb, alive, [ALIVE, 0], f"{what} after the repairs")
    finally:
        eng.close()
        orc.close()
    return seen


@pytest.mark.parametrize("tw", sc.TILE_WIDTHS)
def test_width_passes(gs, oracle_mod, tw):
    """One engine at every width; 64, the default, is the control. N = 300
    gives ld = 512 (64, 32, 16 and 8 tiles of 8, 16, 32 and 64 members), 1,024
    at 128 and 2,048 at 256 (8 tiles, most of them padding), a last tile of 4,
    12, 12, 44, 44 and 44 members. At tw = 8 a census lane owns a whole tile
    (lgc = 0). The table holds stopped rows, tombstones, absent cells and wide
    segments (asserted on the oracle's export)."""
    seen = run_passes(gs, oracle_mod, tw)
    assert all(v > 0 for v in seen.values()), seen


PASS_SHARDS = [(tw, *s) for tw in (8, 32, 256) for s in sc.WIDTH_SHARDS]


@pytest.mark.parametrize("tw,label,world,layout", PASS_SHARDS, ids=[f"{x[0]}-{x[1]}" for x in PASS_SHARDS])
def test_width_passes_sharded(gs, oracle_mod, tw, label, world, layout):
    """The same on 3 column shards (128 columns each, the last holds 44) and 2
    row shards (150 rows each), at the narrowest width, one between and the
    widest; every rank's answer is compared (ShardGroup checks that they
    agree)."""
    seen = run_passes(gs, oracle_mod, tw, layout=label)
    assert all(v > 0 for v in seen.values()), seen


def test_width_env_override_reaches_shards(gs, oracle_mod, monkeypatch):
    """GH_TILE_W overrides gh_config.tile_width on every shard of a group: the
    configuration asks for 128, every shard reports and runs 16."""
    monkeypatch.setenv("GH_TILE_W", "16")
    seen = run_passes(gs, oracle_mod, 16, layout="cols3", rounds=12, cfg_width=128)
    assert seen["stopped"] > 0 and seen["detections"] > 0, seen


def test_width_refused(gs, monkeypatch):
    """A tile width outside the six is refused by gh_create with GH_EINVAL,
    from the configuration and from GH_TILE_W alike."""
    for tw in (4, 24, 48, 512, -8):
        with pytest.raises(gs.GossipError) as err:
            gs.Engine(gs.default_config(64, tile_width=tw))
        assert err.value.code == gs._abi.GH_EINVAL, tw
    monkeypatch.setenv("GH_TILE_W", "24")
    with pytest.raises(gs.GossipError) as err:
        gs.Engine(gs.default_config(64, tile_width=64))
    assert err.value.code == gs._abi.GH_EINVAL


# ---- the features, each through its own module's runner ------------------------------------------

@pytest.mark.parametrize("tw", OFF_DEFAULT)
@pytest.mark.parametrize("name", ["two16", "pend16"])
def test_width_partition_16bit(gs, name, tw):
    """test_gpu_partition.test_16bit_path: two sides of 43 and 220 members, and
    sides that change while a REMOVE set is pending (recipient bitmaps,
    REMOVE per side), against PartitionModel."""
    import partition_ref as pr
    import test_gpu_partition as tp
    case = tp.CASES[name]
    eng, model = tp.start(gs, case, tile_width=tw), pr.model_of(case)
    try:
        assert_width(eng, tw, tier=False)
        tp.lockstep(eng, model, case)
        assert model.cut > 0 and eng.partition()[0]
    finally:
        eng.close()


@pytest.mark.parametrize("tw", TIER)
def test_width_partition_tier(gs, tier_on, tw):
    """test_gpu_partition.test_nibble_path's nib263_2 (two sides of 163 and
    100, the 1% crash at round 8): the table is in the tier and the nibble
    path ran."""
    import partition_ref as pr
    import test_gpu_partition as tp
    case = tp.CASES["nib263_2"]
    eng, model = tp.start(gs, case, tile_width=tw), pr.model_of(case)
    tier, variants = [], []

    def per_round(r, st):
        tier.append(eng.tier_info()[1])
        variants.append(eng.tier_info(full=True)[3])

    try:
        assert_width(eng, tw, tier=True)
        tp.lockstep(eng, model, case, per_round=per_round)
        print(f"nib263_2 TW={tw}: tier per round {tier}, variants {variants}")
        assert 1 in tier and 3 in variants, (tier, variants)
        assert model.cut > 0
    finally:
        eng.close()


@pytest.mark.parametrize("tw", OFF_DEFAULT)
def test_width_control_loss_16bit(gs, tw):
    """test_gpu_control_loss.test_deaf_mute_16bit (the detector-walk kernel and
    the k_seg ops with drop tallies): member 17 detects everybody and every one
    of its REMOVEs is lost, against ControlLossModel."""
    import test_gpu_control_loss as tc
    case = tc.CASES["deaf16"]
    eng, model = tc.start(gs, case, tile_width=tw)
    try:
        assert_width(eng, tw, tier=False)
        tc.lockstep(eng, model, case)
        st = eng.control_loss_stats()
        assert st["remove_missed"] > 0 and st["leave_sent"] == st["join_sent"] == st["bcast_sent"] == 0
    finally:
        eng.close()


@pytest.mark.parametrize("tw", TIER)
def test_width_control_loss_tier(gs, tier_on, tw):
    """test_gpu_control_loss.test_nibble_path's nib263: the nibble path ran in
    a round that delivered a REMOVE."""
    import test_gpu_control_loss as tc
    case = tc.CASES["nib263"]
    eng, model = tc.start(gs, case, tile_width=tw)
    seen = []
    try:
        assert_width(eng, tw, tier=True)
        tc.lockstep(eng, model, case, per_round=lambda r, st: seen.append(
            (eng.tier_info(full=True)[3], st["tombstoned"] + st["remove_unknown"])))
        print(f"nib263 TW={tw}: (variant, cells a REMOVE reached) per round {seen}")
        assert any(v == 3 and rm > 0 for v, rm in seen), seen
        assert model.ctl["remove_missed"] > 0
    finally:
        eng.close()


LOSS_CASES = [("storm16", 8, False)] + [("nib263", tw, True) for tw in TIER]


@pytest.mark.parametrize("name,tw,tier", LOSS_CASES, ids=[f"{a}-{b}" for a, b, _ in LOSS_CASES])
def test_width_lossy_links(gs, monkeypatch, name, tw, tier):
    """test_gpu_loss: its inbox kernels are not tile-shaped, so off the plane
    the narrowest width alone runs the 16-bit storm; on the tier nib263 (a
    mute and a deaf member, the 1% crash) at both widths, against LossModel."""
    import loss_ref as lr
    import test_gpu_loss as tl
    if tier:
        monkeypatch.setenv("GH_PLANE", "1")
    case = tl.CASES[name]
    eng, model = tl.start(gs, case, tile_width=tw), lr.model_of(case)
    variants = []
    try:
        assert_width(eng, tw, tier=tier)
        eng.set_loss(case["out"], case["inn"])
        total = tl.lockstep([eng], model, case, per_round=lambda r, st: variants.append(eng.tier_info(full=True)[3]))
        assert total["detections"] > 0 and model.loss_stats()[1] > 0
        if tier:
            assert 3 in variants, variants
    finally:
        eng.close()


@pytest.mark.parametrize("tw", OFF_DEFAULT)
def test_width_remove_list(gs, oracle_mod, tw):
    """test_gpu_remove_list.test_churn_remove_list's N = 300 case (the
    reference's REMOVE recipients, column bitmaps) against tablesim's literal
    mode, every round."""
    n, seed = 300, 5
    sched = sc.random_churn(n, 40, seed, p_crash=0.06, p_leave=0.02, p_join=0.05)
    cfg = dict(peer_mode=0, fanout=3, seed=0x3300 + seed, detect_mode=0, t_fail=3, t_cleanup=5, remove_mode=1,
               tile_width=tw)
    eng, orc = run_parity(gs, oracle_mod, cfg, n, 40, sched, init=sc.full_state(n))
    try:
        assert_width(eng, tw, tier=False)
    finally:
        eng.close()
        orc.close()


@pytest.mark.parametrize("tw", OFF_DEFAULT)
def test_width_append_order_ring_quirk(gs, tw):
    """test_gpu_counters' GH_ORDER_APPEND run at N = 64 (ring mode, the quirk
    sweep, from `f24`) against live listsim: 8, 4 and 2 tiles at 8, 16 and 32,
    one partial tile at 128 and 256."""
    append_order_ring_quirk(gs, on_create=created(tw, tier=False), tile_width=tw)
