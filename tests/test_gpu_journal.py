"""The detection journal (gh_journal_*, csrc/journal.hip, DESIGN.md
"Journal") against its numpy definition (tests/journal_ref.py), exactly.

Engine B journals and runs a schedule in multi-round step() calls (split
where events are due: queued events belong to the next round). Engine A, same
configuration, steps one round at a time and feeds the reference from what
the ABI shows after each round: read_failed, read_detectors, alive(), the
round's stats and, for GH_JOURNAL_VIEWS, census().listed. B's journal() and
journal_rounds() must equal the reference, and A's and B's final tables and
summed stats must be equal: journaling changes nothing. Run on a MI355X:
pytest -m gpu."""
import numpy as np
import pytest

import journal_ref as jr
import scenarios as sc

pytestmark = pytest.mark.gpu

SUMMED = ("rounds", "detections", "failed_members", "remove_unknown", "ring_empty", "active_rows", "merged_cells",
          "released", "tombstoned")


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv("GH_PLANE", raising=False)
    monkeypatch.delenv("GH_C8", raising=False)


def alive_of(eng):
    return eng.alive()


def listed_of(eng):
    return eng.census().listed


def chunks(sched, rounds, split):
    """(first round, rounds) of the step() calls: a call ends before every
    round that has events, and after round `split`."""
    cuts = sorted({1, rounds + 1, split + 1} | {r for r in sched if 1 <= r <= rounds})
    return [(a, b - a) for a, b in zip(cuts, cuts[1:])]


def run_journaled(eng, sched, rounds, split):
    """The schedule on a journaling engine in few step() calls; the summed stats."""
    total = dict.fromkeys(SUMMED, 0)
    for r0, k in chunks(sched, rounds, split):
        if sched.get(r0):
            eng.apply_events(sched[r0])
        st = eng.step(k)
        assert st["last_round"] == r0 + k - 1
        for f in SUMMED:
            total[f] += st[f]
    return total


def run_pair(gs, n, cfg, sched, rounds, mode, log_rounds=64, split=7, per_round=None, make=None):
    """A (stepwise, feeds the reference) and B (journals); returns (B's
    journal, B's log, the reference)."""
    make = make or (lambda: gs.Engine(gs.default_config(n, **cfg)))
    a, b = make(), make()
    try:
        for e in (a, b):
            e.import_state(*sc.full_state(n), 0)
        b.journal_enable(mode, log_rounds)
        ref = jr.JournalRef(n, a.alive(), mode, log_rounds)
        stats = jr.drive(a, sched, rounds, ref, alive_of, listed_of, per_round=per_round)
        total = run_journaled(b, sched, rounds, split)
        assert b.journal_total() == rounds
        got, log = b.journal(), b.journal_rounds()
        jr.assert_journal_equal(got, log, ref, f"N={n}")
        assert total == {f: sum(s[f] for s in stats) for f in SUMMED}
        for x, y in zip(a.export_state(), b.export_state()):
            np.testing.assert_array_equal(x, y)
        # the log's detections are the steps' stats.detections, round by round
        want, _ = ref.rounds()
        k = len(want)
        assert log["detections"].tolist() == [s["detections"] for s in stats][rounds - k:]
        assert log["failed"].tolist() == [s["failed_members"] for s in stats][rounds - k:]
    finally:
        a.close()
        b.close()
    return got, log, ref


@pytest.mark.parametrize("mode", [jr.DETECT, jr.VIEWS], ids=["detect", "views"])
def test_journal_clean(gs, monkeypatch, mode):
    """N=1,000 in 1,024 padded columns (a tail wave): two crashes, a rejoin, a
    second crash; three latencies of T_fail, no false positive."""
    monkeypatch.setenv("GH_PLANE", "1")
    s = jr.CLEAN
    got, log, _ = run_pair(gs, s["n"], s["cfg"], s["sched"], s["rounds"], mode)
    assert got.latency_hist[10] == 3 and got.latency_hist.sum() == 3 and not got.fp_rounds.any()
    assert (got.start_round[321], got.stop_round[321], got.first_round[321]) == (20, 26, 36)
    assert {int(e["round"]): (int(e["failed"]), int(e["detections"])) for e in log if e["failed"]} == \
        {13: (2, 11), 36: (1, 2)}
    if mode == jr.VIEWS:
        assert (got.forgotten_round[999], got.forgotten_round[321]) == (14, 37) and got.known_hist[4] == 1
    else:
        assert (got.forgotten_round == -1).all() and (got.known_round == -1).all()
        assert not got.forget_hist.any() and not got.known_hist.any()
        assert (log["stale_views"] == -1).all() and (log["missing_views"] == -1).all()


@pytest.mark.parametrize("mode", [jr.DETECT, jr.VIEWS], ids=["detect", "views"])
def test_journal_storm(gs, monkeypatch, mode):
    """T_fail = 6: false-positive storms, classified. Rounds 7-12 detect
    129 / 7 / 59 / 328 / 433 / 43 members, all but two of round 9 running."""
    monkeypatch.setenv("GH_PLANE", "1")
    s = jr.STORM
    got, log, _ = run_pair(gs, s["n"], s["cfg"], s["sched"], s["rounds"], mode)
    assert log["failed"][6:12].tolist() == [129, 7, 59, 328, 433, 43]
    assert (log["failed"] - log["false_failed"])[6:12].tolist() == [0, 0, 2, 0, 0, 0]
    assert got.fp_rounds.sum() == log["false_failed"].sum() > 0
    assert got.latency_hist[6] == 2 and got.latency_hist.sum() == 2


@pytest.mark.parametrize("extra", [{}, {20: [(sc.CRASH, 900)]}], ids=["churn", "churn+crash"])
def test_journal_tier(gs, monkeypatch, extra):
    """N=2,048, k=4, T_fail=16 in the 4-bit tier (test_census_tier_churn's
    crash / leave / rejoin schedule): the nibble path and its lane jobs under
    the journal's census pass; once more with a crash that stays down and is
    detected (the detection wave's 16-bit rounds)."""
    monkeypatch.setenv("GH_PLANE", "1")
    n = 2048
    cfg = dict(fanout=4, seed=0x5EED0007, t_fail=16, t_cleanup=16)
    sched = {14: [(sc.CRASH, 7), (sc.LEAVE, 1500)], 18: [(sc.JOIN, 1500), (sc.JOIN, 7)], **extra}
    tiers = []
    made = []

    def make():
        made.append(gs.Engine(gs.default_config(n, **cfg)))
        return made[-1]

    got, log, _ = run_pair(gs, n, cfg, sched, 55, jr.VIEWS, make=make,
                           per_round=lambda r: tiers.append(made[0].tier_info()[1]))
    assert tiers[:13] == [1] * 13, tiers  # the table was held in the tier
    assert (got.stop_round[7], got.start_round[7], got.start_round[1500]) == (-1, 18, 18)
    if extra:
        assert 0 in tiers
        assert (got.stop_round[900], got.first_round[900]) == (20, 36) and got.latency_hist[16] == 1


@pytest.mark.parametrize("quirk", [0, 1], ids=["canonical", "quirk"])
def test_journal_defaults_n300(gs, quirk):
    """N=300 with the defaults (no plane, 64-member tiles, T_fail = 5: storms),
    canonical and GH_DETECT_QUIRK detection."""
    n = 300
    cfg = dict(fanout=4, seed=0x5EED0C04, detect_mode=quirk)
    sched = {2: [(sc.CRASH, 17), (sc.CRASH, 200)], 10: [(sc.JOIN, 17)]}
    got, log, _ = run_pair(gs, n, cfg, sched, 20, jr.VIEWS, split=5)
    assert got.latency_hist[4] == 2 and got.latency_hist.sum() == 2  # (from the synthetic start: most rows hold them at ts = 0)
    assert (got.stop_round[200], got.first_round[200]) == (2, 6) and (got.start_round[17], got.last_round[17]) == (10, 6)
    assert log["false_failed"].sum() > 0


SHARD_N, SHARD_ROUNDS = 1024, 25
SHARD_CFG = dict(fanout=4, seed=0x5EED0C05, t_fail=8, t_cleanup=8)
SHARD_SCHED = {3: [(sc.CRASH, 700)]}


@pytest.fixture(scope="module")
def single_journal(gs):
    """One engine on the shard tests' schedule (checked against the reference)."""
    got, log, _ = run_pair(gs, SHARD_N, SHARD_CFG, SHARD_SCHED, SHARD_ROUNDS, jr.VIEWS)
    # 700 is detected at 11 and, after stale gossip re-adds it, again at 20
    assert (got.det_rounds[700], got.first_round[700], got.last_round[700]) == (2, 11, 20)
    assert got.latency_hist[8] == 1 and got.latency_hist.sum() == 1
    return got, log


@pytest.mark.parametrize("world,layout", [(2, 0), (3, 0), (2, 1)], ids=["cols2", "cols3", "rows2"])
def test_journal_sharded(gs, single_journal, world, layout):
    """Column shards (each journals its columns: slices allgathered,
    histograms and log summed on read) and row shards (listed allreduced each
    round): every rank returns one engine's journal."""
    grp = gs.ShardGroup(gs.default_config(SHARD_N, shard_layout=layout, **SHARD_CFG), world)
    try:
        grp.import_state(*sc.full_state(SHARD_N), 0)
        grp.journal_enable(jr.VIEWS, 64)
        run_journaled(grp, SHARD_SCHED, SHARD_ROUNDS, 7)
        got, log = grp.journal(), grp.journal_rounds()
        assert grp.journal_total() == SHARD_ROUNDS
    finally:
        grp.close()
    want, wlog = single_journal
    for f in jr.FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b, err_msg=f"{world} shards, layout {layout}: {f}")
    assert log.dtype == wlog.dtype
    np.testing.assert_array_equal(log, wlog)


def test_journal_ring_wrap(gs):
    """log_rounds = 8 over 40 rounds: n_total = 40, the entries are rounds 33..40."""
    n = 300
    cfg = dict(fanout=4, seed=0x5EED0C04, t_fail=10, t_cleanup=10)
    got, log, ref = run_pair(gs, n, cfg, {3: [(sc.CRASH, 17)], 30: [(sc.CRASH, 18)]}, 40, jr.DETECT, log_rounds=8)
    assert log["round"].tolist() == list(range(33, 41)) and len(ref.log) == 40
    eng = gs.Engine(gs.default_config(n, **cfg))
    try:
        eng.init_full(2, 0, 0)
        eng.journal_enable(jr.DETECT, 8)
        eng.step(5)
        assert eng.journal_rounds()["round"].tolist() == [1, 2, 3, 4, 5]  # not yet wrapped
        eng.step(20)
        assert eng.journal_rounds(cap=3)["round"].tolist() == [23, 24, 25] and eng.journal_total() == 25
        eng.journal_enable(jr.DETECT, 0)  # no log at all
        eng.step(3)
        assert len(eng.journal_rounds()) == 0 and eng.journal_total() == 3
    finally:
        eng.close()


def assert_cleared(j, log, total):
    for f in jr.MEMBER_FIELDS:
        zero = f in ("first_count", "det_rounds", "detectors", "fp_rounds")
        assert (getattr(j, f) == (0 if zero else -1)).all(), f
    for f in jr.HIST_FIELDS:
        assert not getattr(j, f).any(), f
    assert len(log) == 0 and total == 0


def test_journal_clears(gs):
    """Re-enabling, import_state and init_full clear the journal and re-take
    the baseline: a member already stopped then has no stop_round."""
    n = 300
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED0C04, t_fail=10, t_cleanup=10))
    try:
        eng.import_state(*sc.full_state(n), 0)
        eng.journal_enable(jr.VIEWS, 16)
        assert_cleared(eng.journal(), eng.journal_rounds(), eng.journal_total())
        eng.apply_events([(sc.CRASH, 17)])
        eng.step(12)
        j = eng.journal()
        assert (j.stop_round[17], j.first_round[17]) == (1, 11) and eng.journal_total() == 12
        assert j.latency_hist[10] == 1 and j.forgotten_round[17] == 11  # every row detects it in round 11
        eng.journal_enable(jr.VIEWS, 16)
        assert_cleared(eng.journal(), eng.journal_rounds(), eng.journal_total())
        eng.apply_events([(sc.CRASH, 18)])
        eng.step(2)
        j = eng.journal()
        assert (j.stop_round[17], j.stop_round[18]) == (-1, 13)  # 17 stopped before the new baseline
        assert j.forgotten_round[17] == 13 and not j.forget_hist.any()
        hb, ts, alive = eng.export_state()
        eng.import_state(hb, ts, alive, eng.round)
        assert_cleared(eng.journal(), eng.journal_rounds(), eng.journal_total())
        eng.step(1)
        j = eng.journal()
        assert (j.stop_round == -1).all() and eng.journal_rounds()["running"].tolist() == [n - 2]
        eng.init_full(2, 0, 0)
        assert_cleared(eng.journal(), eng.journal_rounds(), eng.journal_total())
        eng.step(1)
        assert eng.journal_rounds()[["round", "running"]].tolist() == [(1, n)]
    finally:
        eng.close()


def test_journal_off_and_bad_modes(gs):
    """Off by default: both reads are refused; so are unknown modes and log
    sizes, and they leave a running journal alone."""
    from gossipsim import _abi
    eng = gs.Engine(gs.default_config(64, fanout=3))
    try:
        eng.init_full(2, 0, 0)
        for call in (eng.journal, eng.journal_rounds, eng.journal_total):
            with pytest.raises(gs.GossipError) as ei:
                call()
            assert ei.value.code == _abi.GH_EINVAL
        eng.journal_enable(jr.DETECT, 4)
        eng.step(2)
        for mode, log_rounds in ((2, 4), (4, 4), (-1, 4), (jr.DETECT, -1), (jr.VIEWS, (1 << 20) + 1)):
            with pytest.raises(gs.GossipError) as ei:
                eng.journal_enable(mode, log_rounds)
            assert ei.value.code == _abi.GH_EINVAL
        assert eng.journal_total() == 2
        eng.journal_enable(jr.OFF)
        with pytest.raises(gs.GossipError):
            eng.journal()
        eng.step(1)  # nothing is journaled, nothing breaks
        eng.journal_enable(jr.VIEWS, 1 << 20)
        eng.step(1)
        assert eng.journal_rounds()["round"].tolist() == [4]
    finally:
        eng.close()


def test_cluster_journal(gs):
    """Cluster (ring push, append order): join all, crash one, tick. The
    journal shows its stop, its first detection and when the last list
    dropped it, as the reference says."""
    n = 64
    cl = gs.Cluster(n, t_fail=5, t_cleanup=5, seed=0x5EED0C07)
    try:
        for i in range(n):
            cl.join(i)
            cl.tick(1)
        cl.tick(4)
        cl.journal_enable(jr.VIEWS, 32)
        eng = cl.engine
        ref = jr.JournalRef(n, eng.alive(), jr.VIEWS, 32)
        cl.crash(9)
        r_crash = eng.round + 1
        for _ in range(12):
            st = cl.tick(1)
            ref.observe(eng.round, eng.alive(), listed=eng.census().listed, **jr.detection_inputs(eng, st))
        j = cl.journal()
        jr.assert_journal_equal(j, cl.journal_rounds(), ref, "cluster")
        assert j.stop_round[9] == r_crash and j.first_round[9] > r_crash and j.first_detector[9] >= 0
        assert j.forgotten_round[9] >= j.first_round[9] and j.forget_hist.sum() == 1 and j.latency_hist.sum() == 1
        assert j.fp_rounds[9] == 0  # (the 64-member ring at T_fail = 5 does detect running members: reported)
    finally:
        cl.engine.close()
