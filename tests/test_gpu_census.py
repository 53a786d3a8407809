"""gh_census (csrc/census.hip, DESIGN.md "Census"): the device-side
membership census -- per member how many running rows list it or hold it
tombstoned, min / max / sum of the listed heartbeats, the oldest listed age,
and the age histogram -- against the numpy census of the exported state
(tests/census_ref.py), exactly, on every path of the kernel: the 4-bit tier's
nibble walk, its escaped chunks, 16-bit buffers (imports, storm rounds,
engines without plane or tier), wide segments, frozen rows, column padding,
column and row shards. Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import scenarios as sc
from census_ref import assert_census_equal, census_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv("GH_PLANE", raising=False)
    monkeypatch.delenv("GH_C8", raising=False)


def check(eng, msg):
    """The engine's census against the reference census of its own export."""
    got = eng.census()
    hb, ts, alive = eng.export_state()
    assert_census_equal(got, census_ref(hb, ts, alive, eng.round), msg)
    return got


def run_checked(eng, sched, rounds, init, round0=0, per_round=None):
    eng.import_state(*init, round0)
    out = [check(eng, "after import")]
    for r in range(1, rounds + 1):
        if sched.get(r):
            eng.apply_events(sched[r])
        eng.step(1)
        out.append(check(eng, f"round {r}"))
        if per_round:
            per_round(r)
    return out


def test_census_tier_churn(gs, monkeypatch):
    """N=2,048, k=4 pull in the 4-bit tier with the bench's timeouts: a crash
    and a leave (frozen rows, then tier tombstones and the detection wave's
    16-bit storm rounds), both rejoin; 32 row blocks per column, the diagonal
    in every tile. Exact every round, on the tier path and the 16-bit one."""
    monkeypatch.setenv("GH_PLANE", "1")
    n = 2048
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED0007, t_fail=16, t_cleanup=16))
    sched = {14: [(sc.CRASH, 7), (sc.LEAVE, 1500)], 18: [(sc.JOIN, 1500), (sc.JOIN, 7)]}
    tiers = []
    try:
        out = run_checked(eng, sched, 55, sc.full_state(n), per_round=lambda r: tiers.append(eng.tier_info()[1]))
    finally:
        eng.close()
    assert tiers[:13] == [1] * 13 and 0 in tiers, tiers
    assert max(int(c.tombstoned.max()) for c in out) > 0
    # round 15: the two stopped rows have no view, and a member's own entry does not count
    assert out[15].listed[0] == n - 3 and out[15].listed[7] == n - 2


def test_census_padding_and_release(gs, monkeypatch):
    """N=1,000 in 1,024 padded columns: the padding never counts, and a
    crashed member, once detected, tombstoned and released, is a column
    nobody lists (at these timeouts the whole cluster follows it: rows under
    the < 4 guard keep their tombstones)."""
    monkeypatch.setenv("GH_PLANE", "1")
    n, m = 1000, 321
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED0C02, t_fail=6, t_cleanup=6))
    try:
        out = run_checked(eng, {3: [(sc.CRASH, m)]}, 20, sc.full_state(n))
    finally:
        eng.close()
    c = out[-1]
    assert (c.listed[m], c.hb_min[m], c.hb_max[m], c.hb_sum[m], c.age_max[m]) == (0, -1, -1, 0, -1)
    peak = max(int(x.tombstoned[m]) for x in out)
    assert 0 < c.tombstoned[m] < peak  # tombstoned, then released by the rows that still clean
    assert out[3].listed[m] == n - 1 and out[3].listed[0] == n - 2
    assert all(x.age_hist.sum() == x.listed.sum() for x in out)


def escape_state(n, seed, R):
    """test_gpu_tier8.ranged_state (lags 0..40, ages up to 24, views ahead of
    their owners, a few tombstones) with three columns whose heartbeats sit
    at 5,000,000 in a quarter of the rows (wide segments), ages up to 45 in
    every 16th row (past the 16-bit age field) and a few ts in the future."""
    from test_gpu_tier8 import ranged_state
    hb, ts, alive = ranged_state(n, seed)
    rng = np.random.default_rng(seed + 100)
    own = hb.diagonal().copy()
    for c in (100, 555, 900):
        hb[1::4, c] = 5_000_000
    old = np.arange(n) % 16 == 5
    ts[old, :] = (R + 1 - rng.integers(20, 46, (int(old.sum()), n))).astype(np.int32)
    fut = rng.random((n, n)) < 0.0001
    ts[fut] = R + rng.integers(1, 9, int(fut.sum()))
    np.fill_diagonal(hb, own)
    np.fill_diagonal(ts, R)
    return hb, ts, alive


def test_census_escapes_wide_exact(gs, monkeypatch):
    """Lags, ages and heartbeats outside the nibbles and the 16-bit codes:
    the census of the imported 16-bit table (wide segments, ages past the
    last bin, future ts) and of five rounds that escape chunks."""
    monkeypatch.setenv("GH_PLANE", "1")
    n, R = 1024, 40
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED0C03, t_fail=60, t_cleanup=60))
    hb, ts, alive = escape_state(n, 3, R)
    assert (R + 1 - ts.astype(np.int64)).max() == 45 and (ts > R).any()
    esc = []
    try:
        eng.import_state(hb, ts, alive, R)
        assert eng.tier_info()[:2] == (1, 0)  # tiered engine, 16-bit table
        assert eng.encoding_info()[0] > 0     # wide segments
        c = check(eng, "after import")
        assert c.age_max.max() == 45 and c.hb_max[555] == 5_000_000 and c.age_hist[0] > 0
        for r in range(1, 6):
            eng.step(1)
            check(eng, f"round {r}")
            esc.append(eng.tier_info()[2])
    finally:
        eng.close()
    assert max(esc) > 0, esc


def test_census_no_plane_no_tier(gs, monkeypatch):
    """N=300 with the defaults (64-member tiles, no plane, no tier), then the
    plane without the tier (GH_C8=0): the 16-bit walk at both tile widths."""
    n = 300
    cfg = dict(fanout=4, seed=0x5EED0C04)
    sched = {2: [(sc.CRASH, 17)]}
    eng = gs.Engine(gs.default_config(n, **cfg))
    try:
        assert eng.tier_info()[0] == 0 and eng.plane_info()[0] == 0
        a = run_checked(eng, sched, 12, sc.full_state(n))
    finally:
        eng.close()
    monkeypatch.setenv("GH_PLANE", "1")
    monkeypatch.setenv("GH_C8", "0")
    eng = gs.Engine(gs.default_config(n, **cfg))
    try:
        assert eng.tier_info()[0] == 0 and eng.plane_info()[0] == 1
        b = run_checked(eng, sched, 12, sc.full_state(n))
    finally:
        eng.close()
    assert a[1].listed[0] == n - 1 and a[2].listed[0] == n - 2 and a[2].listed[17] == n - 1
    for r, (x, y) in enumerate(zip(a, b)):
        assert_census_equal(x, y, f"round {r}: plane vs none")


SHARD_N, SHARD_ROUNDS = 1024, 25
SHARD_CFG = dict(fanout=4, seed=0x5EED0C05, t_fail=8, t_cleanup=8)
SHARD_SCHED = {3: [(sc.CRASH, 700)]}


@pytest.fixture(scope="module")
def single_census(gs):
    """One engine on the shard tests' schedule: its census after every round."""
    eng = gs.Engine(gs.default_config(SHARD_N, **SHARD_CFG))
    try:
        return run_checked(eng, SHARD_SCHED, SHARD_ROUNDS, sc.full_state(SHARD_N))
    finally:
        eng.close()


@pytest.mark.parametrize("world,layout", [(2, 0), (3, 0), (2, 1)], ids=["cols2", "cols3", "rows2"])
def test_census_sharded(gs, single_census, world, layout):
    """Column shards (the owner's slices allgathered, the bins summed) and
    row shards (partial answers reduced with SUM / MAX): every rank returns
    the census of the group's own export, which is one engine's."""
    grp = gs.ShardGroup(gs.default_config(SHARD_N, shard_layout=layout, **SHARD_CFG), world)
    try:
        out = run_checked(grp, SHARD_SCHED, SHARD_ROUNDS, sc.full_state(SHARD_N))
    finally:
        grp.close()
    assert len(out) == len(single_census)
    for r, (x, y) in enumerate(zip(out, single_census)):
        assert_census_equal(x, y, f"round {r}: {world} shards vs one engine")


def test_census_is_read_only(gs, monkeypatch):
    """A census before and after every step changes no round and no table."""
    monkeypatch.setenv("GH_PLANE", "1")
    n = 1000
    cfg = dict(fanout=4, seed=0x5EED0C02, t_fail=6, t_cleanup=6)
    a, b = gs.Engine(gs.default_config(n, **cfg)), gs.Engine(gs.default_config(n, **cfg))
    try:
        for e in (a, b):
            e.import_state(*sc.full_state(n), 0)
        for r in range(1, 21):
            if r == 3:
                a.apply_events([(sc.CRASH, 321)])
                b.apply_events([(sc.CRASH, 321)])
            b.census()
            sa, sb = a.step(1), b.step(1)
            b.census()
            assert sa == sb, (r, sa, sb)
        for x, y in zip(a.export_state(), b.export_state()):
            np.testing.assert_array_equal(x, y)
        assert a.tier_info() == b.tier_info()
    finally:
        a.close()
        b.close()


def test_cluster_census(gs):
    """Cluster.census() after join / crash / tick (ring push, append order)."""
    n = 64
    cl = gs.Cluster(n, t_fail=5, t_cleanup=5, seed=0x5EED0C07)
    try:
        for i in range(n):
            cl.join(i)
            cl.tick(1)
        cl.tick(4)
        cl.crash(9)
        seen = []
        for _ in range(12):
            cl.tick(1)
            hb, ts, alive = cl.engine.export_state()
            c = cl.census()
            assert_census_equal(c, census_ref(hb, ts, alive, cl.engine.round), f"round {cl.engine.round}")
            seen.append(c)
        # the crash round: 63 running rows, all still listing 9; a member's own entry does not count
        assert seen[0].listed[9] == n - 1 and seen[0].listed[0] == n - 2
    finally:
        cl.engine.close()
