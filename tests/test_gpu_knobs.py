"""Parity of every A/B and diagnostic fallback against the oracle. The
environment switches gh_create reads (GH_JOBS_FLAT, GH_QUIRK_ROWS, GH_DNW,
...; include/gossiphip.h gh_debug_knobs) select paths that DESIGN.md's
measurements are taken against and that no default run reaches: the region
form of the lane jobs, the two-sweep quirk pre-pass, IN 6 on a full grid, the
nibble path without its move words or row records, the storm variant and the
per-cell rule everywhere, another grid of the per-cell kernel, other tilings.
Each case sets its switch before the engine is created,
asserts through knobs() that the engine runs with it, and then runs one
workload bit-exact against the oracle, stats and tables every round: a
crash wave (N=2,048, k=4, T_fail = T_cleanup = 16, 1% crash at round 8, one
rejoin at round 30, 36 rounds). Run on a MI355X: pytest -m gpu."""
import pytest

import scenarios as sc
from test_gpu_tier8 import remove_run

pytestmark = pytest.mark.gpu

N, ROUNDS = 2048, 36


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def plane_on(monkeypatch):
    monkeypatch.setenv("GH_PLANE", "1")
    monkeypatch.delenv("GH_C8", raising=False)


def wave(detect_mode=0):
    cfg = dict(fanout=4, seed=0x5EED0D10, t_fail=16, t_cleanup=16, detect_mode=detect_mode)
    crashed = sc.crash_ids(N, 0.01, 0x5EED0D11)
    sched = {8: [(sc.CRASH, int(c)) for c in crashed], 30: [(sc.JOIN, int(crashed[0]))]}
    return cfg, sched


def run_with(gs, oracle_mod, monkeypatch, env, expect, detect_mode=0, world=1, layout=0, on_create=None):
    """The wave with the environment `env`, after asserting that knobs()
    reports `expect` (on every shard: a ShardGroup call checks that the ranks
    agree); returns remove_run's trace."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))

    def created(eng):
        kn = eng.knobs()
        assert {k: kn[k] for k in expect} == expect, kn
        if on_create:
            on_create(eng)

    cfg, sched = wave(detect_mode)
    trace, _ = remove_run(gs, oracle_mod, N, cfg, sched, ROUNDS, world, layout, on_create=created)
    assert any(s["tombstoned"] for s, _, _ in trace) and any(s["detections"] for s, _, _ in trace)
    return trace


def test_knobs_defaults(gs, monkeypatch):
    """What an engine reports with no switch set: the defaults every other
    case departs from (so a case's assertion on knobs() is not vacuous)."""
    from gossipsim import _abi
    for k in _abi.KNOBS:
        if k != "PLANE":
            monkeypatch.delenv("GH_" + k, raising=False)
    eng = gs.Engine(gs.default_config(N, fanout=4, t_fail=16, t_cleanup=16))
    try:
        kn = eng.knobs()
    finally:
        eng.close()
    assert kn == dict(GH_QUIRK_ROWS=1, GH_JOBS_FLAT=1, GH_RMV_FULL7=1, GH_DNW=1, GH_NREC=1, GH_FORCE_SLOW=0,
                      GH_FORCE_STORM=0, GH_ROUND_NT=1, GH_ROUND_TPW=1, GH_SLOW_GRID=768, GH_NIB_RMV=1,
                      GH_GX_DIRECT=1, GH_ROUND_XMAP=1, GH_TMODE=1, GH_PLANE=1, GH_C8=1, GH_TILE_W=256), kn


ONE_ENGINE = [("GH_JOBS_FLAT", 0), ("GH_RMV_FULL7", 0), ("GH_DNW", 0), ("GH_NREC", 0), ("GH_ROUND_NT", 1),
              ("GH_ROUND_NT", 0), ("GH_FORCE_SLOW", 1), ("GH_FORCE_STORM", 1), ("GH_SLOW_GRID", 96)]


@pytest.mark.parametrize("knob,value", ONE_ENGINE, ids=[f"{k}={v}" for k, v in ONE_ENGINE])
def test_knob_one_engine(gs, oracle_mod, monkeypatch, knob, value):
    """One engine, canonical detection, one switch set (GH_ROUND_NT=1 is its
    default, =0 the other leg)."""
    flat = None
    if knob == "GH_JOBS_FLAT":
        # the default first: the region form below is then asked for in a
        # process whose earlier engine ran the flat kernel, and still gets it
        flat = run_with(gs, oracle_mod, monkeypatch, {knob: 1}, {knob: 1})
    trace = run_with(gs, oracle_mod, monkeypatch, {knob: value}, {knob: value})
    if knob == "GH_FORCE_STORM":  # the storm variant in every round
        assert [v for _, v, _ in trace] == [1] * ROUNDS, trace
    elif knob == "GH_FORCE_SLOW":  # every segment by the per-cell rule: no lane jobs
        assert [j for _, _, j in trace] == [0] * ROUNDS, trace
    else:  # the switch leaves the nibble path in place
        assert sum(v == 3 for _, v, _ in trace) >= 30, trace
    if flat is not None:  # both forms do the same lane jobs, round by round
        assert [j for _, _, j in trace] == [j for _, _, j in flat]
        assert sum(j for _, _, j in flat) > 0


@pytest.mark.parametrize("world,layout", [(1, 0), (3, 1)], ids=["engine", "rows3"])
@pytest.mark.parametrize("quirk_rows", [0, 1])
def test_knob_quirk_rows(gs, oracle_mod, monkeypatch, quirk_rows, world, layout):
    """Quirk detection with the two-sweep pre-pass (GH_QUIRK_ROWS=0, its
    segments without escaped chunks skipped) and the one-pass row walk, on
    one engine and on 3 row shards."""
    run_with(gs, oracle_mod, monkeypatch, {"GH_QUIRK_ROWS": quirk_rows}, {"GH_QUIRK_ROWS": quirk_rows}, detect_mode=1,
             world=world, layout=layout)


@pytest.mark.parametrize("world,layout", [(3, 1), (2, 0)], ids=["rows3", "cols2"])
def test_knob_jobs_region_sharded(gs, oracle_mod, monkeypatch, world, layout):
    """The region form of the lane jobs on 3 row shards and 2 column shards."""
    run_with(gs, oracle_mod, monkeypatch, {"GH_JOBS_FLAT": 0}, {"GH_JOBS_FLAT": 0}, world=world, layout=layout)


@pytest.mark.parametrize("tpw", [2, 4])
def test_knob_round_tpw(gs, oracle_mod, monkeypatch, tpw):
    """More than one tile per workgroup turns the 4-bit tier off (the nibble
    path is written for one): the 16-bit variants run the wave."""
    def tier_off(eng):
        assert eng.tier_info()[0] == 0, eng.tier_info()

    trace = run_with(gs, oracle_mod, monkeypatch, {"GH_ROUND_TPW": tpw}, {"GH_ROUND_TPW": tpw, "GH_C8": 0},
                     on_create=tier_off)
    assert {v for _, v, _ in trace} <= {0, 1}, trace
