"""GPU parity across the pull fanout range gh_config.fanout takes: k = 1, 2 and
5..8 (scenarios.FANOUTS); the rest of the suite runs k = 3 and 4 almost
everywhere. launch_round (csrc/round.hip) picks k_round<KB = 4> for pull with
k <= 4 and k_round<KB = 8> otherwise, so from k = 5 on the 8-sender
instantiation takes five to eight pull senders per row step out of the inbox
of stride k + 1: the second int4 of s_inb / s_isl, the __ballot(q < cntv)
guarded loads, LEAN_GUARD, the cntv > KB fallback and its own storm variant.
Draws 4..7 come from the second Philox block of the peer draws (k_peers_pull,
k_inbox_bits, k_peers_rows, k_inbox_rows, ensemble.hip); on column shards
their validity bits travel as one byte per receiver, on row shards as
pvf[i * k + q] summed over ranks. Below k = 3 an engine has neither the sender
plane nor the 4-bit tier, dissemination is slow enough for views to leave the
16-bit windows, and at k = 1 the cluster collapses even at T_fail = 16. With
N <= k + 1 every receiver's draws repeat senders.

  a. the crash wave on one engine, k in FANOUTS x N in {263, 1,000}
  b. the N = 300 churn at every tile width
  c. the wave on column and row shards, k = 8 also beside one engine
  d. the mass crash at k = 5 and 8, as the engine chooses and on the storm variant
  e. tiny clusters, N in {2, 3, 5, 8, 9}
  f. the wave far from round 0 (`f24`, and `cap` through its refused round)
  g. lossy links at k = 8 on shards
  h. ensembles at k = 2, 5, 6, 7
  i. GH_ORDER_APPEND at k = 8

Every comparison is equality with the model the feature was built against
(oracle/tablesim.c, loss_ref.LossModel, oracle/listsim.py), after every round:
hb, ts, alive, the failed set, detectors, the round's statistics and
gh_debug_counts. tests/test_fanout_scenario.py holds the preconditions, on the
oracle. Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import ensemble_ref as er
import loss_ref as lr
import scenarios as sc
from test_gpu_config_space import make_engine
from test_gpu_ensemble import check_round, crash_round
from test_gpu_ensemble import make as make_ensemble
from test_gpu_parity import compare, run_parity
from test_gpu_sharded import run_group

pytestmark = pytest.mark.gpu

ROUNDS = sc.RAGGED_ROUNDS
LAYOUTS = {label: (n, world, layout) for label, n, world, layout in sc.FANOUT_SHARDS}


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in ("GH_PLANE", "GH_C8", "GH_TILE_W", "GH_TMODE", "GH_FORCE_STORM", "GH_FORCE_SLOW"):
        monkeypatch.delenv(k, raising=False)


def close(*engines):
    for e in engines:
        e.close()


def lockstep(engines, orc, sched, first, last, per_round=None):
    """Engines (or shard groups) and the oracle one round at a time through
    the rounds first..last; every engine's statistics and tables against the
    oracle's after each. Returns the oracle's statistics."""
    out = []
    for r in range(first, last + 1):
        ev = sched.get(r)
        for e in list(engines) + [orc]:
            if ev:
                e.apply_events(ev)
        want = orc.step(1)
        for x, e in enumerate(engines):
            got = e.step(1)
            assert got == want, f"engine {x}, round {r}: gpu {got} != cpu {want}"
            compare(e, orc, r)
        out.append(want)
        if per_round:
            per_round(r, want)
    return out


# ---- a. the wave on one engine ---------------------------------------------------------------------

@pytest.mark.parametrize("k", sc.FANOUTS)
@pytest.mark.parametrize("n", sc.FANOUT_NS)
def test_fanout_wave(gs, oracle_mod, n, k):
    """tail_members(n) crash at round 8, are detected (24) and REMOVE'd (25),
    the last member joins again at round 30; 40 rounds. From k = 5 on some
    receiver has k valid senders, some five to k - 1, some the same sender
    twice. k = 1 is the collapse: running members detected, REMOVEs of unknown
    members, every row under the guard, lags of 26 and 27 rounds."""
    eng, orc = run_parity(gs, oracle_mod, sc.fanout_cfg(k), n, ROUNDS, sc.fanout_wave(n), init=sc.full_state(n))
    close(eng, orc)


# ---- b. every tile width -----------------------------------------------------------------------------

@pytest.mark.parametrize("k,tw", sc.FANOUT_WIDTHS, ids=[f"k{k}-tw{tw}" for k, tw in sc.FANOUT_WIDTHS])
def test_fanout_tile_widths(gs, oracle_mod, k, tw):
    """width_churn() at N = 300 from width_state() (stopped rows, tombstones,
    absent cells, releases, REMOVEs of unknown members, a column too wide for
    a 16-bit segment), 30 rounds: k = 2, 5 and 8 at all six widths, k = 1 at
    the narrowest and the widest. k_round<KB = 8> is instantiated per width."""
    n, rounds = sc.WIDTH_N, 30
    cfg, sched = sc.fanout_churn(k, tile_width=tw)
    eng, orc = run_parity(gs, oracle_mod, cfg, n, rounds, sched, init=sc.width_state(n))
    try:
        assert eng.knobs()["GH_TILE_W"] == tw, eng.knobs()
    finally:
        close(eng, orc)


# ---- c. shards --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sc.FANOUT_SHARD_KS)
@pytest.mark.parametrize("label", list(LAYOUTS))
def test_fanout_shards(gs, oracle_mod, label, k):
    """The wave on 3 and 8 column shards and on 2 and 3 row shards, a victim
    on each side of every shard boundary; the whole group's table against the
    oracle every round. At k = 8 the validity byte of a column shard's
    receiver uses all eight bits, and some receiver's valid senders stand on
    every shard. k = 8 on cols3 and rows2 runs beside one engine as well."""
    n, world, layout = LAYOUTS[label]
    cfg, sched = sc.fanout_cfg(k), sc.fanout_wave(n, world, layout)
    if k == 8 and label in sc.FANOUT_LOCKSTEP:
        one = make_engine(gs, n, cfg, "single")
        grp = gs.ShardGroup(gs.default_config(n, shard_layout=layout, **cfg), world)
        orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
        try:
            for e in (one, grp, orc):
                e.import_state(*sc.full_state(n), 0)
            stats = lockstep([one, grp], orc, sched, 1, ROUNDS)
            assert sum(s["detections"] for s in stats) > 0 and sum(s["tombstoned"] for s in stats) > 0
        finally:
            close(one, grp, orc)
    else:
        run_group(gs, oracle_mod, world, dict(cfg, shard_layout=layout), n, ROUNDS, sched, init=sc.full_state(n))


# ---- d. storm --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("forced", [False, True], ids=["free", "forced"])
@pytest.mark.parametrize("k", sc.MASS_KS)
def test_fanout_mass_crash(gs, oracle_mod, monkeypatch, k, forced):
    """A quarter of N = 1,000 stops at round 4, T_fail = 6, T_cleanup = 8, 24
    rounds: at k = 5 the detections spread over rounds and take running
    members along, at k = 8 round 10 detects all 250. `free` runs as the
    engine chooses and prints encoding_info(full=True)[2] (1: the storm
    variant) and debug_variant() per round; `forced` sets GH_FORCE_STORM=1, so
    k_round<KB = 8>'s storm variant is certain to run, and asserts that it did,
    in every round. On a MI355X the free run chooses the storm variant itself
    at this size: from round 7 (the first detections) to the end at k = 5,
    where the collapse keeps it there, and in the rounds 10..17 at k = 8 (10 is
    the detection round), the lean variant before and after."""
    if forced:
        monkeypatch.setenv("GH_FORCE_STORM", "1")
    cfg, sched, _ = sc.fanout_mass(k)
    n = sc.MASS_N
    eng = gs.Engine(gs.default_config(n, **cfg))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    seen = []
    try:
        assert eng.knobs()["GH_FORCE_STORM"] == int(forced), eng.knobs()
        for e in (eng, orc):
            e.import_state(*sc.full_state(n), 0)
        stats = lockstep([eng], orc, sched, 1, sc.MASS_ROUNDS,
                         per_round=lambda r, st: seen.append((r, eng.encoding_info(full=True)[2], eng.debug_variant())))
        print(f"mass crash k={k} {'forced' if forced else 'free'}: (round, storm mode, launched variant) {seen}")
        assert sum(s["detections"] for s in stats) >= 250
        if forced:
            assert [(m, v) for _, m, v in seen] == [(1, 1)] * sc.MASS_ROUNDS, seen
    finally:
        close(eng, orc)


# ---- e. tiny clusters ------------------------------------------------------------------------------------------------

def test_fanout_tiny_table(gs, oracle_mod):
    """N in {2, 3, 5, 8, 9} at k = 1 and 8 on one engine, min_members = 2: at
    k = 8 every receiver draws senders more than once from N = 8 down, and
    (u * (n - 1)) >> 32 has one value at N = 2, two at N = 3."""
    for n, k in sc.TINY_TABLE:
        cfg, sched = sc.fanout_tiny(n, k)
        eng, orc = run_parity(gs, oracle_mod, cfg, n, sc.TINY_ROUNDS, sched, init=sc.full_state(n))
        close(eng, orc)


@pytest.mark.parametrize("layout", [0, 1], ids=["cols2", "rows2"])
def test_fanout_tiny_sharded(gs, oracle_mod, layout):
    """N = 9, k = 8 on two column shards (32 columns each: the second shard is
    empty) and on two row shards (5 and 4 rows)."""
    n, k = sc.TINY_SHARDED
    cfg, sched = sc.fanout_tiny(n, k, shard_layout=layout)
    run_group(gs, oracle_mod, 2, cfg, n, sc.TINY_ROUNDS, sched, init=sc.full_state(n))


def test_fanout_tiny_one_tile(gs, oracle_mod):
    """N = 5, k = 8 at tile_width 8 and 256: one tile, mostly padding."""
    n, k, widths = sc.TINY_ONE_TILE
    for tw in widths:
        cfg, sched = sc.fanout_tiny(n, k, tile_width=tw)
        eng, orc = run_parity(gs, oracle_mod, cfg, n, sc.TINY_ROUNDS, sched, init=sc.full_state(n))
        try:
            assert eng.knobs()["GH_TILE_W"] == tw, eng.knobs()
        finally:
            close(eng, orc)


# ---- f. far from round 0 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sc.FANOUT_COUNTER_KS)
@pytest.mark.parametrize("name", ["f24", "cap"])
def test_fanout_counter_offsets(gs, oracle_mod, name, k):
    """The wave at N = 263 from `f24` (heartbeats and rounds through 2^24) and
    from `cap`, 40 calls of one round: on `cap` the own counters reach
    INT32_MAX in round 33, and round 34 and every later one is refused with
    GH_ERANGE on the same call as on the oracle, with the oracle's
    stats["rounds"]."""
    n = 263
    h, r0 = sc.COUNTER_OFFSETS[name]
    cfg, sched = sc.fanout_cfg(k), sc.fanout_wave(n, r0=r0)
    eng = gs.Engine(gs.default_config(n, **cfg))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **cfg), threads=8)
    ran = refused = 0
    try:
        for e in (eng, orc):
            e.import_state(*sc.full_state(n, hb0=h, ts0=r0), r0)
        for r in range(r0 + 1, r0 + ROUNDS + 1):
            if sched.get(r):
                eng.apply_events(sched[r])
                orc.apply_events(sched[r])
            rc, want = orc.step_rc(1)
            got_rc, got = eng.step_rc(1)
            assert (got_rc, got) == (rc, want), f"round {r}: gpu {(got_rc, got)} != cpu {(rc, want)}"
            assert got["rounds"] == want["rounds"] == int(rc == 0)
            if rc == 0:
                assert refused == 0
                ran += 1
                compare(eng, orc, r)
            else:
                assert rc == gs._abi.GH_ERANGE, (r, rc)
                refused += 1
        compare(eng, orc, r0 + ran)
        assert (ran, refused) == ((sc.CAP_ROUNDS, ROUNDS - sc.CAP_ROUNDS) if name == "cap" else (ROUNDS, 0))
        assert eng.export_state()[0].diagonal().max() == h + ran
    finally:
        close(eng, orc)


# ---- g. lossy links on shards at k = 8 --------------------------------------------------------------------------------------

@pytest.mark.parametrize("label", sc.FANOUT_LOCKSTEP)
def test_fanout_lossy_shards(gs, label):
    """test_gpu_loss.CASES["k8"] (N = 520, uniform 0.3, 15 rounds) on 3 column
    shards and 2 row shards against LossModel: the link blocks 4..7 of the
    draws 4..7, k_peers_rows' sent / dropped per draw on the sender's owner;
    loss_stats is the same, global pair on every rank."""
    import test_gpu_loss as tl
    case = tl.CASES["k8"]
    _, world, layout = LAYOUTS[label]
    grp = gs.ShardGroup(gs.default_config(case["n"], shard_layout=layout, **case["cfg"]), world)
    model = lr.model_of(case)

    def per_round(r, st):
        ranks = grp.run("loss_stats")
        assert all(x == model.loss_stats() for x in ranks), (r, ranks, model.loss_stats())

    try:
        grp.import_state(*sc.full_state(case["n"]), 0)
        grp.set_loss(case["out"], case["inn"])
        tl.lockstep([grp], model, case, per_round=per_round)
        assert model.loss_stats()[1] > 0
    finally:
        grp.close()


# ---- h. ensembles -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.FANOUT_ENSEMBLES))
def test_fanout_ensembles(gs, name):
    """One group each at k = 2, 5, 6, 7, two clusters, the first with loss
    (ensemble.hip draws `for blk; 4 * blk < k`): after every round the tables,
    statistics, failed set and detect record against LossModel
    (test_gpu_ensemble.check_round), and tables, statistics, failed set and
    sent / dropped against an Engine of the same seed
    (test_gpu_ensemble.test_engine_parity's loop)."""
    cases = [er.case(*a[:7], seed=a[7]) for a in sc.FANOUT_ENSEMBLES[name]]
    traces = [er.run(er.model(c), c["rounds"], c["crash"]) for c in cases]
    ens, cs = make_ensemble(gs, cases)
    n = cases[0]["n"]
    engines = []
    for c in cs:
        e = gs.Engine(gs.default_config(n, fanout=c["k"], t_fail=c["t_fail"], t_cleanup=c["t_cleanup"], seed=c["seed"]))
        e.import_state(*sc.full_state(n), 0)
        e.set_loss(c["out"], c["inn"])
        engines.append(e)
    sent, dropped = [0] * len(cs), [0] * len(cs)
    try:
        with ens:
            for r in range(1, cases[0]["rounds"] + 1):
                crash_round(ens, cs, r)
                st = ens.step(1)
                check_round(ens, st, traces, r - 1, name)
                hb, ts, alive, _ = ens.export_state()
                failed = ens.failed()
                for b, (c, e) in enumerate(zip(cs, engines)):
                    if c["crash"].get(r):
                        e.apply_events([(gs.GH_EV_CRASH, m) for m in c["crash"][r]])
                    est = e.step(1)
                    assert {f: int(st[f][b]) for f in lr.STATS} == est, (b, r)
                    for x, y in zip((hb[b], ts[b], alive[b]), e.export_state()):
                        assert np.array_equal(x, y), (b, r)
                    assert np.array_equal(failed[b], e.read_failed()), (b, r)
                    s, d = e.loss_stats()
                    assert (int(st["sent"][b]), int(st["dropped"][b])) == (s - sent[b], d - dropped[b]), (b, r)
                    sent[b], dropped[b] = s, d
        assert dropped[0] > 0 and dropped[1] == 0 and min(sent) > 0, (sent, dropped)
    finally:
        close(*engines)


# ---- i. append order ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quirk", [False, True], ids=["canonical", "quirk"])
def test_fanout_append_order(gs, quirk):
    """GH_ORDER_APPEND in pull mode at k = 8, N = 100 against oracle/listsim.py
    as test_gpu_list_order.py does at k = 3: order.hip walks the inbox of
    stride k + 1 in received-list order. Counters, tables, the failed set,
    detectors and every row's gh_lsm order each round."""
    import test_gpu_list_order as lo
    n = sc.APPEND_N
    eng, ls = lo.make_pair(gs, n, "pull", quirk, fanout=sc.APPEND_K, seed=sc.APPEND_SEED, init_full=True)
    try:
        reordered = lo.run_pair(eng, ls, n, sc.APPEND_ROUNDS, sc.fanout_append_churn())
    finally:
        eng.close()
    assert reordered > 0
