"""GPU parity of gh_step(h, rounds > 1): the engine runs a batch of rounds in
ONE call, the oracle (oracle/tablesim.c) is stepped round by round with its
counters summed, and after every call the stats, last_round, the full tables,
the failed set, the detectors, the maintained row counts and (where they can
exist) the D7 shadow entries must be equal. bench.py and every real caller
step in batches; the rest of the suite calls step(1), which never reaches

  * the REMOVE round inside a call (q > 0): the looped 1/8-grid IN 6 on the
    side stream instead of the host's full-grid IN 7 (csrc/round.hip k_round),
  * the same with timing on (the fork and join on the launches' own stamps,
    rmv_main off at GH_TMODE=0) while the tables are compared,
  * host state sampled per call (shadow_any, last_nd, busy), arena growth
    between two rounds of one call,
  * shard ranks a round apart (one thread per rank, joined per call only).

Every scenario runs under the partitions PARTS of its rounds into calls; a
call always ends before a round that has events (queued events belong to the
next round run). The detection round d of a scenario is read from a stepwise
oracle run: the first round with detections whose REMOVE round d + 1 makes
tombstones and lies with d - 1 in one stretch without events. Every
precondition is asserted on the oracle, or on the engine's read-only
diagnostics where it concerns the encoding. Run on a MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import scenarios as sc
from test_gpu_config_space import check_shadows, make_engine
from test_gpu_parity import check_counts, compare, shadows_of
from test_oracle_step_batch import call_bounds, staggered_age_state, step_summed, wave

pytestmark = pytest.mark.gpu

NO_SHADOW = np.iinfo(np.int32).min
I32MAX = 2**31 - 1
PARTS = ["fewest", "remove_inside", "detect_last", "ragged", "stepwise"]
RAGGED = [2, 3, 5, 1, 7] + [int(x) for x in np.random.default_rng(0x9A66ED).integers(1, 8, 80)]


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in ("GH_PLANE", "GH_C8", "GH_TMODE", "GH_GX_DIRECT"):
        monkeypatch.delenv(k, raising=False)


# ---- the helper ---------------------------------------------------------------------

def run_partitioned(eng, orc, sched, rounds, cuts, first=1, shadows=False, at_call_end=None):
    """Rounds first..rounds: the engine in one step(k) per call of
    call_bounds(sched, rounds, cuts, first), the oracle round by round with
    its stats summed; after every call the stats, last_round, the tables, the
    failed set and detectors of the call's last round, the maintained counts
    and (shadows) the D7 shadow entries are compared.
    at_call_end(eng, first round, rounds, the oracle's per-round stats) runs
    after the comparison. Returns the engine's final export."""
    n = orc.n
    for r0, k in call_bounds(sched, rounds, cuts, first):
        ev = sched.get(r0, [])
        if ev:
            eng.apply_events(ev)
            orc.apply_events(ev)
        got = eng.step(k)
        want, per = step_summed(orc, k)
        r = r0 + k - 1
        assert got == want, f"call {r0}..{r} ({k} rounds): gpu {got} != cpu, summed {want}"
        assert got["last_round"] == r and got["rounds"] == k and eng.round == r == orc.round
        compare(eng, orc, r)
        if shadows:
            check_shadows(eng, orc, n, f"after the call {r0}..{r}")
        if at_call_end:
            at_call_end(eng, r0, k, per)
    return eng.export_state()


# ---- scenarios, their oracle traces and partitions ------------------------------------

_TRACES, _FINALS, _DIAG = {}, {}, {}


class Scenario:
    """n, configuration, schedule, the rounds r0 + 1 .. last and the state
    imported at r0 (full membership by default); `key` names it in the
    caches of the stepwise oracle trace and the stepwise engine's final export."""

    def __init__(self, key, n, cfg, sched, last, state=None, r0=0, shadows=False):
        self.key, self.n, self.cfg, self.sched, self.last, self.r0, self.shadows = key, n, cfg, sched, last, r0, shadows
        self.state = state if state is not None else sc.full_state(n)

    def oracle(self, om):
        orc = om.Oracle(om.default_config(self.n, **self.cfg), threads=16 if self.n >= 1024 else 8)
        orc.import_state(*self.state, self.r0)
        return orc

    def trace(self, om):
        """{round: the stepwise oracle's stats, "shadows": its shadow entries after the round}"""
        if self.key not in _TRACES:
            orc = self.oracle(om)
            try:
                out = {}
                for r in range(self.r0 + 1, self.last + 1):
                    if self.sched.get(r):
                        orc.apply_events(self.sched[r])
                    out[r] = dict(orc.step(1), shadows=int((orc.debug_shadow() != NO_SHADOW).sum()) if self.shadows else 0)
            finally:
                orc.close()
            _TRACES[self.key] = out
        return _TRACES[self.key]

    def stretch(self, r):
        """first round of the event-free stretch that holds round r"""
        return max([self.r0 + 1] + [e for e in self.sched if e <= r])

    def d(self, om):
        tr = self.trace(om)
        for d in range(self.r0 + 2, self.last):
            if tr[d]["detections"] > 0 and tr[d + 1]["tombstoned"] > 0 and self.stretch(d + 1) <= d - 1:
                return d
        raise AssertionError(f"{self.key}: no detection round with its REMOVE round inside an event-free stretch")

    def cuts(self, om, part):
        first, last = self.r0 + 1, self.last
        if isinstance(part, tuple):  # the rounds after which a call ends, as given
            return part
        if part == "fewest":
            return ()
        if part == "stepwise":
            return tuple(range(first, last + 1))
        if part == "ragged":
            return tuple(int(x) for x in first - 1 + np.cumsum(RAGGED) if x < last)
        d = self.d(om)
        if part == "remove_inside":  # the call stretch(d + 1) .. d + 1
            return (d + 1,)
        assert part == "detect_last"  # .. d, then d + 1 .. the stretch's end
        calls = call_bounds(self.sched, last, (d,), first)
        assert any(a == d + 1 and k > 1 for a, k in calls), (d, calls)
        return (d,)


def run_case(gs, om, scen, part, layout="single", on_create=None, at_call_end=None, before_first=None):
    eng = make_engine(gs, scen.n, scen.cfg, layout)
    orc = None
    try:
        if on_create:
            on_create(eng)
        orc = scen.oracle(om)
        eng.import_state(*scen.state, scen.r0)
        if before_first:
            before_first(eng)
        return run_partitioned(eng, orc, scen.sched, scen.last, scen.cuts(om, part), scen.r0 + 1, scen.shadows,
                               at_call_end)
    finally:
        eng.close()
        if orc:
            orc.close()


def control(gs, om, scen):
    """The stepwise partition on one engine (checked against the oracle after
    every round like any other): its final export, kept per scenario, and per
    round (round, tier_info(full), lane jobs) in _DIAG."""
    if scen.key not in _FINALS:
        diag = []
        _FINALS[scen.key] = run_case(gs, om, scen, "stepwise", at_call_end=lambda eng, r0, k, per: diag.append(
            (r0, eng.tier_info(full=True), eng.job_info()[0])))
        _DIAG[scen.key] = diag
    return _FINALS[scen.key]


def assert_final(final, want, what):
    for x, y, name in zip(final, want, ("hb", "ts", "alive")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: final {name} against the stepwise engine's")


def remove_inside_hook(scen, om, part, seen, tier=True):
    """After the call that ends on d + 1 of the remove_inside partition: the
    REMOVE round ran at q > 0 and made tombstones (oracle); with the tier on
    one engine the REMOVE-taking nibble form ran it (debug_variant 4), which
    inside a call is the looped 1/8-grid IN 6."""
    d = scen.d(om)

    def hook(eng, r0, k, per):
        if part == "remove_inside" and r0 + k - 1 == d + 1:
            assert r0 <= d - 1 and k >= 3, (d, r0, k)
            assert per[-2]["detections"] > 0 and per[-1]["tombstoned"] > 0, per[-2:]
            if tier:
                assert eng.debug_variant() == 4, (eng.debug_variant(), eng.tier_info(full=True))
            seen.append(d + 1)
    return hook


# ---- a. the crash wave on the nibble path, one engine ----------------------------------

WAVE_N, WAVE_ROUNDS = 2048, 36
WAVE_VARIANTS = {"canonical": {}, "quirk": dict(detect_mode=1), "remove_list": dict(remove_mode=1),
                 "t_cleanup20": dict(t_cleanup=20)}


def wave_scenario(variant="canonical"):
    cfg, sched = wave(WAVE_N, **WAVE_VARIANTS[variant])
    return Scenario(("wave", variant), WAVE_N, cfg, sched, WAVE_ROUNDS)


def assert_wave_preconditions(scen, om):
    """(oracle) detection, REMOVE and releases all lie inside the run"""
    tr, d = scen.trace(om), scen.d(om)
    assert d == min(r for r in tr if tr[r]["detections"]), d  # the wave's first detection round
    assert 8 < d < 30 and tr[d + 1]["tombstoned"] > 0
    assert any(tr[r]["released"] for r in range(d + 1, scen.last + 1))
    return d


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("variant", list(WAVE_VARIANTS))
def test_wave_one_engine(gs, oracle_mod, monkeypatch, variant, part):
    """The wave of test_gpu_knobs.wave() (N=2,048, GH_PLANE=1, k=4, T_fail =
    T_cleanup = 16, 1% crash at round 8, a rejoin at 30, 36 rounds; d = 24)
    under every partition: canonical and quirk detection, the reference's
    REMOVE recipients, T_cleanup = 20. remove_inside is the call 8..25, whose
    18th round is the REMOVE round; detect_last the calls 8..24 and 25..29
    (the host's IN 7, then releases at q > 0)."""
    monkeypatch.setenv("GH_PLANE", "1")
    scen = wave_scenario(variant)
    assert_wave_preconditions(scen, oracle_mod)
    seen, ends = [], []

    def at_call_end(eng, r0, k, per):
        remove_inside_hook(scen, oracle_mod, part, seen)(eng, r0, k, per)
        ends.append((r0 + k - 1, eng.tier_info(full=True), eng.job_info()[0]))

    final = run_case(gs, oracle_mod, scen, part, at_call_end=at_call_end)
    assert_final(final, control(gs, oracle_mod, scen), f"{variant}/{part}")
    assert all(t[0] == 1 for _, t, _ in ends), ends  # the tier is kept
    if part == "remove_inside":
        assert seen, ends
    if part == "fewest":
        # the calls 1..7, 8..29, 30..36: the first two left the table in the
        # tier, written by the nibble path
        assert [r for r, _, _ in ends] == [7, 29, 36], ends
        assert all(t[1] == 1 and t[3] == 3 for _, t, _ in ends[:2]), ends
        # job_info tells of a call's last round only, and these three are
        # healthy rounds without a lane job: that lane jobs ran in the rounds
        # in between is what the stepwise engine shows, whose final tables
        # this run has just matched
        diag = _DIAG[scen.key]
        assert sum(j for _, _, j in diag) > 0 and sum(t[3] == 3 for _, t, _ in diag) > WAVE_ROUNDS // 2, diag


# ---- b. the wave with timing on -----------------------------------------------------------

def timed(tmode, rounds_seen):
    """(on_create, before_first, a call-end check): GH_TMODE asserted through
    knobs(), timing on before round 1, read_timing's launches = rounds run so
    far with a growing time"""
    def on_create(eng):
        assert eng.knobs()["GH_TMODE"] == tmode, eng.knobs()

    def before_first(eng):
        eng.set_timing(True)

    def check(eng, r0, k, per):
        ms, launches = eng.read_timing()
        prev_ms, prev_launches = rounds_seen[-1] if rounds_seen else (0.0, 0)
        assert launches == prev_launches + k, (r0, k, launches, prev_launches)
        assert ms > prev_ms, (r0, k, ms, prev_ms)
        rounds_seen.append((ms, launches))
    return on_create, before_first, check


@pytest.mark.parametrize("tmode,part", [(t, p) for t in (0, 1) for p in PARTS[:4]] + [(0, "stepwise")])
def test_wave_timing_on(gs, oracle_mod, monkeypatch, tmode, part):
    """The canonical wave with gh_set_timing on, as the bench runs it:
    GH_TMODE=1 stamps the nibble launch alone (rmv_main as without timing),
    GH_TMODE=0 every launch (rmv_main off: every REMOVE round is the looped
    IN 6, also at q = 0, which the stepwise partition runs). Tables and stats
    as without timing, read_timing() counts every round once."""
    monkeypatch.setenv("GH_PLANE", "1")
    monkeypatch.setenv("GH_TMODE", str(tmode))
    scen = wave_scenario()
    d = assert_wave_preconditions(scen, oracle_mod)
    seen, timings, variants = [], [], {}
    on_create, before_first, check = timed(tmode, timings)

    def at_call_end(eng, r0, k, per):
        remove_inside_hook(scen, oracle_mod, part, seen)(eng, r0, k, per)
        check(eng, r0, k, per)
        variants[r0 + k - 1] = eng.debug_variant()

    final = run_case(gs, oracle_mod, scen, part, on_create=on_create, at_call_end=at_call_end,
                     before_first=before_first)
    monkeypatch.delenv("GH_TMODE")
    assert_final(final, control(gs, oracle_mod, scen), f"timing, GH_TMODE={tmode}, {part}")
    assert timings[-1][1] == WAVE_ROUNDS and timings[-1][0] > 0
    if part == "remove_inside":
        assert seen
    if part == "stepwise":
        assert variants[d + 1] == 4, variants  # the REMOVE round on the nibble path


def test_timing_long_call_regrows_variant_log(gs, oracle_mod, monkeypatch):
    """One healthy call of 4,100 rounds with timing on (GH_TMODE=1): the
    variant log gh_set_timing allocated for 4,096 rounds is reallocated by
    gh_step. N=64: under GH_PLANE=1 the tier is kept at any N (pull, k=4;
    asserted), 64 members give every row 4 distinct peers and the oracle
    17 M cell steps."""
    monkeypatch.setenv("GH_PLANE", "1")
    n, rounds = 64, 4100
    cfg = dict(fanout=4, seed=0x5EED0F30, t_fail=16, t_cleanup=16)
    scen = Scenario(("long", n), n, cfg, {}, rounds)
    timings = []
    on_create, before_first, check = timed(1, timings)

    def created(eng):
        on_create(eng)
        assert eng.tier_info()[0] == 1, eng.tier_info()

    def at_call_end(eng, r0, k, per):
        check(eng, r0, k, per)
        assert k == rounds and sum(s["detections"] for s in per) == 0 and per[-1]["active_rows"] == n
        assert eng.tier_info()[:2] == (1, 1), eng.tier_info(full=True)  # still held in the tier

    run_case(gs, oracle_mod, scen, "fewest", on_create=created, at_call_end=at_call_end, before_first=before_first)
    assert len(timings) == 1 and timings[0][1] == rounds and timings[0][0] > 0


# ---- c. shards, with a plane ------------------------------------------------------------------

SHARD_LAYOUTS = [("rows3", 1), ("rows3", 0), ("cols2", None)]


@pytest.mark.parametrize("part", ["fewest", "remove_inside", "ragged"])
@pytest.mark.parametrize("layout,direct", SHARD_LAYOUTS, ids=["rows3-direct", "rows3-packed", "cols2"])
def test_wave_sharded(gs, oracle_mod, monkeypatch, layout, direct, part):
    """The canonical wave on 3 row shards (ghost planes gathered in place from
    their owners' tables, GH_GX_DIRECT=1, and packed and moved by the
    transport, =0) and on 2 column shards, one thread per rank: inside a call
    nothing but the transport's own ordering keeps a rank's round r + 1 from
    overwriting what another still reads in round r. The whole group's table
    (every shard boundary) against the oracle after every call, and its final
    export against one engine's."""
    monkeypatch.setenv("GH_PLANE", "1")
    if direct is not None:
        monkeypatch.setenv("GH_GX_DIRECT", str(direct))
    scen = wave_scenario()
    assert_wave_preconditions(scen, oracle_mod)
    seen = []

    def on_create(grp):
        kn = grp.knobs()  # (every rank agrees)
        assert kn["GH_PLANE"] == 1 and kn["GH_GX_DIRECT"] == (1 if direct is None else direct), kn
        assert all(t[0] == 1 for t in grp.run("tier_info")), grp.run("tier_info")

    final = run_case(gs, oracle_mod, scen, part, layout=layout, on_create=on_create,
                     at_call_end=remove_inside_hook(scen, oracle_mod, part, seen, tier=False))
    if part == "remove_inside":
        assert seen
    monkeypatch.delenv("GH_GX_DIRECT", raising=False)
    assert_final(final, control(gs, oracle_mod, scen), f"{layout}, direct={direct}, {part}")


# ---- GH_ORDER_APPEND against listsim's recorded run (c: 2 row shards; d: ring, one engine) -------

def golden_d(gold, sched):
    for d in range(2, len(gold)):
        if gold[d - 1]["stats"]["detections"] > 0 and gold[d]["stats"]["tombstoned"] > 0 and \
                max(e for e in sched if e <= d + 1) <= d - 1:
            return d
    raise AssertionError("no detection round with its REMOVE round inside an event-free stretch")


def run_append_golden(gs, case, layout, part):
    """tests/call_partition_golden.py's case on `layout` under `part`: after
    every call the summed counters of its rounds and the last round's record
    (failed set, detectors, alive, hb, ts, every row's list order, the shadow
    entries) as test_introducer_off_zero_append compares them every round."""
    import call_partition_golden as cg
    import list_digest as ld
    n, c, gold, sched = cg.N, cg.CASES[case], cg.load()[case], cg.schedule(case)
    assert len(gold) == cg.ROUNDS and max(x["dual"] for x in gold) > 0 and max(x["reordered"] for x in gold) > 0
    d = golden_d(gold, sched)
    cuts = {"fewest": (), "stepwise": tuple(range(1, cg.ROUNDS + 1)), "remove_inside": (d + 1,), "detect_last": (d,),
            "ragged": tuple(int(x) for x in np.cumsum(RAGGED) if x < cg.ROUNDS)}[part]
    cfg = dict(fanout=3, seed=c["seed"], t_fail=cg.T_FAIL, t_cleanup=cg.T_CLEANUP, introducer=cg.I,
               peer_mode=gs.GH_PEER_RING if c["peer_mode"] == "ring" else gs.GH_PEER_PULL,
               detect_mode=int(c["quirk"]), list_order=gs.GH_ORDER_APPEND)
    calls = call_bounds(sched, cg.ROUNDS, cuts)
    assert max(k for _, k in calls) >= (1 if part == "stepwise" else 3), calls
    if part == "remove_inside":
        assert any(a <= d - 1 and a + k - 1 == d + 1 for a, k in calls), (d, calls)
    if part == "detect_last":
        assert any(a == d + 1 and k > 1 for a, k in calls), (d, calls)
    eng = make_engine(gs, n, cfg, layout)
    try:
        eng.import_state(*sc.full_state(n), 0)
        for r0, k in calls:
            if r0 in sched:
                eng.apply_events(sched[r0])
            st = eng.step(k)
            r = r0 + k - 1
            want = gold[r - 1]
            stats = {f: sum(gold[q - 1]["stats"][f] for q in range(r0, r + 1)) for f in want["stats"]}
            stats["last_round"] = r
            assert st == stats, f"call {r0}..{r}: gpu {st} != listsim, summed {stats}"
            check_counts(eng, r)
            hb, ts, alive = eng.export_state()
            bm = eng.read_failed()
            got = ld.round_record(st, hb, ts, alive, [m for m in range(n) if bm[m >> 5] >> (m & 31) & 1],
                                  eng.read_detectors(), [list(eng.lsm(i)[0]) for i in range(n)],
                                  sc.shadow_view(shadows_of(eng, n), r, cg.T_CLEANUP))
            for key in ("failed", "detectors", "alive", "hb", "ts", "lists", "shadow"):
                assert got[key] == want[key], f"after the call {r0}..{r}, {key}: gpu {got[key]} != listsim {want[key]}"
        return eng.knobs(), eng.run("tier_info") if layout != "single" else [eng.tier_info()]
    finally:
        eng.close()


@pytest.mark.parametrize("part", ["fewest", "remove_inside", "ragged"])
def test_append_rows2_with_plane(gs, monkeypatch, part):
    """GH_ORDER_APPEND on 2 row shards with the plane at N=300 (pull, k=3,
    GH_PLANE=1): the list replicas after list_sync inside a call. The D7 churn
    of test_introducer_off_zero (introducer 157), its event batches 4 rounds
    apart: with one a round every call would be a single round."""
    monkeypatch.setenv("GH_PLANE", "1")
    kn, tiers = run_append_golden(gs, "pull", "rows2", part)
    assert kn["GH_PLANE"] == 1 and all(t[0] == 1 for t in tiers), (kn, tiers)


@pytest.mark.parametrize("part", PARTS)
def test_append_ring_quirk_one_engine(gs, part):
    """GH_ORDER_APPEND in ring mode with the quirk sweep at N=300 on one
    engine (the reference topology; no plane, no tier) against listsim's
    recorded run of the same spread-out churn."""
    kn, tiers = run_append_golden(gs, "ring_quirk", "single", part)
    assert tiers[0][0] == 0, tiers


# ---- d. off the nibble path: ring mode, no plane ---------------------------------------------------

RING_N, RING_R0, RING_GAP = 300, 110, 5
_WARM = {}


def ring_scenario(om, quirk):
    """Ring push at N=300, no plane, T_fail 6 / T_cleanup 8. A ring of 300
    needs ~100 rounds to carry a heartbeat round, so from a synthetic full
    start every far entry times out at once; the start here is what the oracle
    itself holds after 110 rounds with timeouts out of reach (every view
    lagging by its ring distance, every entry fresh). Then 40 rounds of
    sc.random_churn, its batches 5 rounds apart: healthy rounds, a crash
    wave's detection (d = 117), REMOVE, releases, the broken ring's collapse
    and rejoins."""
    cfg = dict(peer_mode=1, fanout=3, seed=0x5EED0F10 + quirk, detect_mode=quirk)
    if quirk not in _WARM:
        w = om.Oracle(om.default_config(RING_N, t_fail=1000, t_cleanup=1000, **cfg), threads=8)
        try:
            w.import_state(*sc.full_state(RING_N), 0)
            st = w.step(RING_R0)
            assert st["detections"] == 0 and st["active_rows"] == RING_N * RING_R0
            _WARM[quirk] = w.export_state()
        finally:
            w.close()
    churn = sc.random_churn(RING_N, 40 // RING_GAP, 0x61 + quirk, p_crash=0.02, p_leave=0.01, p_join=0.05)
    sched = {RING_R0 + (s - 1) * RING_GAP + 1: ev for s, ev in churn.items()}
    return Scenario(("ring", quirk), RING_N, dict(t_fail=6, t_cleanup=8, **cfg), sched, RING_R0 + 40, state=_WARM[quirk],
                    r0=RING_R0)


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("quirk", [0, 1], ids=["canonical", "quirk"])
def test_ring_no_plane(gs, oracle_mod, quirk, part):
    scen = ring_scenario(oracle_mod, quirk)
    tr, d = scen.trace(oracle_mod), scen.d(oracle_mod)
    assert tr[scen.r0 + 1]["active_rows"] > 0.9 * scen.n and tr[scen.r0 + 1]["detections"] == 0  # a healthy start
    assert any(tr[r]["released"] for r in range(d + 1, scen.last + 1))
    seen = []

    def on_create(eng):
        assert eng.plane_info()[0] == 0 and eng.tier_info()[0] == 0

    final = run_case(gs, oracle_mod, scen, part, on_create=on_create,
                     at_call_end=remove_inside_hook(scen, oracle_mod, part, seen, tier=False))
    if part == "remove_inside":
        assert seen
    assert_final(final, control(gs, oracle_mod, scen), f"ring, quirk={quirk}, {part}")


# ---- e. D7 shadow entries across a long call ---------------------------------------------------------

D7_N, D7_I, D7_E, D7_LAST = 300, 157, 10, 40


@pytest.mark.parametrize("peer_mode", [0, 1], ids=["pull", "ring"])
def test_shadows_empty_inside_a_long_call(gs, oracle_mod, peer_mode):
    """sc.rejoin_churn at N=300 with introducer 157 up to round 10, then ONE
    call of the rounds 11..40: the oracle holds shadow entries when the call
    starts and its shadow vector empties inside it, while the engine re-reads
    shadow_any only at the call's end (the introducer's shadow row stays armed
    over rounds without an entry). Stats, tables and shadow entries after
    every call, and the final export against the stepwise engine's."""
    sched = {r: ev for r, ev in sc.rejoin_churn(D7_N, D7_LAST, 0xD7 + peer_mode, introducer=D7_I).items() if r <= D7_E}
    cfg = dict(fanout=3, seed=0x5EED0E10 + peer_mode, t_fail=4, t_cleanup=6, peer_mode=peer_mode, introducer=D7_I)
    scen = Scenario(("d7", peer_mode), D7_N, cfg, sched, D7_LAST, shadows=True)
    tr = scen.trace(oracle_mod)
    assert tr[D7_E]["shadows"] > 0, "no shadow entry when the long call starts"
    gone = min(r for r in range(D7_E + 1, D7_LAST + 1) if tr[r]["shadows"] == 0)
    assert D7_E < gone < D7_LAST - 1 and all(tr[r]["shadows"] == 0 for r in range(gone, D7_LAST + 1)), gone
    calls = []
    final = run_case(gs, oracle_mod, scen, (D7_E,), at_call_end=lambda eng, r0, k, per: calls.append((r0, k)))
    assert calls[-1] == (D7_E + 1, D7_LAST - D7_E), calls
    assert_final(final, control(gs, oracle_mod, scen), f"d7, peer_mode={peer_mode}")


# ---- f. storm and collapse in one call -------------------------------------------------------------

def test_storm_and_collapse_in_one_call(gs, oracle_mod, monkeypatch):
    """The reference's timeouts (T_fail = T_cleanup = 5) from full membership
    at N=2,048, k=4 with the plane: one call of 12 rounds (the bench leg's
    warm-up: the round-6 storm and the round-7 collapse inside it), then one
    of 20 on the collapsed cluster, whose rows no longer run."""
    monkeypatch.setenv("GH_PLANE", "1")
    n = 2048
    scen = Scenario(("collapse",), n, dict(fanout=4, seed=0x5EED0810), {}, 32)
    tr = scen.trace(oracle_mod)
    assert sum(tr[r]["detections"] for r in range(1, 13)) > n and sum(tr[r]["tombstoned"] for r in range(1, 13)) > n
    assert tr[1]["active_rows"] == n and sum(tr[r]["active_rows"] for r in range(13, 33)) < n  # (20 * n when healthy)
    calls = []

    def on_create(eng):
        assert eng.tier_info()[0] == 1

    run_case(gs, oracle_mod, scen, (12,), on_create=on_create, at_call_end=lambda eng, r0, k, per: calls.append((r0, k)))
    assert calls == [(1, 12), (13, 20)]


# ---- g. arena growth inside a call ---------------------------------------------------------------------

ARENA_N, ARENA_CAP, ARENA_STOPPED, ARENA_PER_ROUND = 200, 64, [1, 2, 3], 8


def arena_pair(gs, om, pre):
    """N=200 (64-member tiles, no plane), a 64-slot arena: `pre` rows hold the
    stopped members 1..3 past the narrow age field (31) from the import on,
    8 more rows' entries pass it in every round (one wide segment each: tile
    0 of the row); T_fail = 100, so nothing is detected (oracle, and
    test_oracle_step_batch.test_staggered_ages_detect_nothing)."""
    cfg = dict(fanout=3, seed=0x5EED0F02, t_fail=100, t_cleanup=100, wide_segments=ARENA_CAP)
    state = staggered_age_state(ARENA_N, ARENA_STOPPED, pre, ARENA_PER_ROUND)
    eng = gs.Engine(gs.default_config(ARENA_N, **cfg))
    orc = om.Oracle(om.default_config(ARENA_N, **cfg), threads=8)
    eng.import_state(*state, 0)
    orc.import_state(*state, 0)
    return eng, orc


def test_arena_grows_inside_a_call_busy_start(gs, oracle_mod):
    """A call that starts with more than a quarter of the arena in use checks
    after every round and grows between two rounds of the call: 24 of 64
    slots at the start, 8 more a round, 12 rounds -- 120 wide segments at the
    end, in a grown arena, tables and stats bit-exact."""
    eng, orc = arena_pair(gs, oracle_mod, 24)
    try:
        m0 = eng.memory_info()
        assert m0["wide_cap"] == ARENA_CAP and ARENA_CAP // 4 < m0["wide_used"] <= ARENA_CAP // 2, m0
        ends = []
        run_partitioned(eng, orc, {}, 12, (), at_call_end=lambda e, r0, k, per: ends.append(sum(s["detections"] for s in per)))
        assert ends == [0]
        m1 = eng.memory_info()
        assert m1["wide_used"] > ARENA_CAP and m1["wide_cap"] > ARENA_CAP, (m0, m1)
        assert m1["wide_used"] == m0["wide_used"] + 12 * ARENA_PER_ROUND, (m0, m1)
    finally:
        eng.close()
        orc.close()


def test_arena_climb_inside_a_call_quiet_start(gs, oracle_mod):
    """The same climb from 8 of 64 slots: the call starts with at most a
    quarter in use, so gh_step does not look at the arena between its rounds,
    and round 8 needs 72 slots. The header allows two outcomes: bit-exact
    tables, or GH_ENOMEM with the state refused until a full import (as
    test_arena_overflow_in_a_round_loses_state_loudly); never GH_OK with other
    tables. What happens is GH_ENOMEM (DESIGN.md "GPU parity")."""
    eng, orc = arena_pair(gs, oracle_mod, 8)
    try:
        m0 = eng.memory_info()
        assert m0["wide_cap"] == ARENA_CAP and 0 < m0["wide_used"] <= ARENA_CAP // 4, m0
        want, per = step_summed(orc, 12)
        assert want["detections"] == 0 and want["active_rows"] == 12 * (ARENA_N - len(ARENA_STOPPED))
        st = gs._abi.RoundStats()
        rc = eng.lib.gh_step(eng.h, 12, ctypes.byref(st))
        print(f"quiet start: gh_step(12) returned {rc}, {st.as_dict()}")
        if rc == gs._abi.GH_OK:
            assert st.as_dict() == want
            compare(eng, orc, 12)
            assert eng.memory_info()["wide_used"] == m0["wide_used"] + 12 * ARENA_PER_ROUND
        else:
            assert rc == gs._abi.GH_ENOMEM, rc
            with pytest.raises(gs.GossipError) as ex:
                eng.export_state()
            assert ex.value.code == gs._abi.GH_ENOMEM
            with pytest.raises(gs.GossipError):
                eng.step(1)
            init = sc.full_state(ARENA_N)
            eng.import_state(*init, 0)
            orc.import_state(*init, 0)
            assert eng.step(5) == step_summed(orc, 5)[0]
            compare(eng, orc, 5)
    finally:
        eng.close()
        orc.close()


# ---- h. last_nd after a refused call ---------------------------------------------------------------------

def test_remove_round_after_a_refused_call(gs, oracle_mod, monkeypatch):
    """A call ends on the detection round d; the next is refused with
    GH_ERANGE before any round runs (member 5's own heartbeat is INT32_MAX),
    which leaves the host's |D| of the last round unknown (last_nd = -1);
    member 5 crashes, and the call after that runs the REMOVE round d + 1 at
    q = 0 without the host's IN 7, and five rounds more. N=64 with the tier
    on (GH_PLANE=1 keeps it at any N; asserted, and that the table is held in
    it when the refused call comes), the wave's timeouts (T_cleanup 16: REMOVE
    on the nibble path): member 9 crashes at round 8 and is first detected in
    round d = 24 (oracle)."""
    monkeypatch.setenv("GH_PLANE", "1")
    n, big, crashed = 64, 5, 9
    cfg = dict(fanout=4, seed=0x5EED0F40, t_fail=16, t_cleanup=16)
    sched = {8: [(sc.CRASH, crashed)]}
    probe = Scenario(("refused", "probe"), n, cfg, sched, 32)
    d = probe.d(oracle_mod)  # (heartbeats do not enter the detection rule: the same d with member 5 near INT32_MAX)
    hb, ts, alive = sc.full_state(n, hb0=7)
    hb[:, big] = I32MAX - d - 3
    hb[big, big] = I32MAX - d
    scen = Scenario(("refused", d), n, cfg, sched, d, state=(hb, ts, alive))
    eng = make_engine(gs, n, cfg, "single")
    orc = scen.oracle(oracle_mod)
    try:
        assert eng.tier_info()[0] == 1
        eng.import_state(hb, ts, alive, 0)
        last = []
        run_partitioned(eng, orc, sched, d, (), at_call_end=lambda e, r0, k, per: last.append(per[-1]))
        assert len(last) == 2 and last[-1]["detections"] > 0 and last[-1]["last_round"] == d
        assert eng.export_state()[0][big, big] == I32MAX
        assert eng.tier_info()[:2] == (1, 1), eng.tier_info(full=True)
        rc1, s1 = eng.step_rc(3)
        rc2, s2 = orc.step_rc(3)
        assert rc1 == rc2 == gs._abi.GH_ERANGE and s1 == s2 and s1["rounds"] == 0
        for x in (eng, orc):
            x.apply_events([(sc.CRASH, big)])
        got = eng.step(6)
        want, per = step_summed(orc, 6)
        assert per[0]["tombstoned"] > 0 and per[0]["last_round"] == d + 1, per[0]
        assert got == want, f"gpu {got} != cpu, summed {want}"
        compare(eng, orc, d + 6)
        assert not eng.export_state()[2][big]
    finally:
        eng.close()
        orc.close()
