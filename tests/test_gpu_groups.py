"""gh_groups (csrc/groups.hip, DESIGN.md "Groups"): the connected groups of
the running members and the per-row view digests, always against the numpy
reference (tests/groups_ref.py) of the engine's own export_state(), exactly:
crafted graphs on the 16-bit form, the 4-bit tier with escaped chunks on
split, healed and shattered clusters, frozen rows and storm rounds, column and
row shards, ring mode with append order, and that the call is read-only and
allocates nothing before it is first made. `passes` is diagnostic: only >= 1.
Run on a MI355X: pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

import groups_ref as gr
import scenarios as sc

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
    """The engine's groups against the reference groups of its own export."""
    got = eng.groups()
    hb, _, alive = eng.export_state()
    ref = gr.groups_ref(hb, alive)
    gr.assert_groups_equal(got, ref, msg)
    assert got.passes >= 1
    assert sorted(got.sizes().values()) == gr.sizes(ref[0])
    assert got.n_views == gr.n_views(ref[0], ref[1])
    return got


# ---- 1. crafted graphs, 16-bit form, ragged columns --------------------------------------------
def crafted_state(n=263, R=40, seed=5):
    """Known components over a scattered id permutation: a one-way path of 60,
    a star of 40, two cliques of 30 joined by one one-way listing, two
    cliques of 25 that share only stopped members, a stopped row listing
    everybody, a member listing itself alone, a member listing nobody, and a
    one-way ring of the rest: 8 groups."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n)
    hb = np.full((n, n), -1, np.int32)
    alive = np.ones(n, np.uint8)
    path, hub, leaves = ids[0:60], ids[60], ids[61:100]
    A, B, Cq, D = ids[100:130], ids[130:160], ids[160:185], ids[185:210]
    stopped, stale, alone, empty, ring = ids[210:215], ids[215], ids[216], ids[217], ids[218:]
    hb[np.arange(n), np.arange(n)] = 7  # every row lists itself ...
    hb[empty, empty] = -1               # ... but one
    hb[path[:-1], path[1:]] = 9
    hb[leaves, hub] = 9
    for q in (A, B, Cq, D):
        hb[np.ix_(q, q)] = 9
    hb[A[3], B[7]] = 9                  # the single one-way listing that joins A and B
    hb[np.ix_(Cq, stopped)] = 9         # stopped members both cliques list: no bridge
    hb[np.ix_(D, stopped)] = 9
    hb[np.ix_(Cq[::2], D[::3])] = -2    # tombstones: no edge
    alive[stopped] = 0
    hb[stale, :] = 3                    # a stopped row's stale list: no edges
    alive[stale] = 0
    hb[ring, np.roll(ring, -1)] = 9
    # three columns far above their owners' heartbeats in some rows: wide segments
    hb[A[1::2], A[0]] = 5_000_000
    hb[D[::2], D[1]] = 5_000_000
    hb[path[4], path[5]] = 5_000_000
    ts = np.where(hb >= 0, R, np.where(hb == -2, R - 2, 0)).astype(np.int32)
    return hb, ts, alive, 8


def test_groups_crafted_graphs(gs):
    n, R = 263, 40
    hb, ts, alive, want = crafted_state(n, R)
    assert gr.groups_ref(hb, alive)[2] == want
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED6701, t_fail=60, t_cleanup=60))
    try:
        eng.import_state(hb, ts, alive, R)
        assert eng.tier_info()[0] == 0       # the 16-bit form, 263 columns in 512 padded
        assert eng.encoding_info()[0] > 0    # wide segments
        g = check(eng, "crafted")
        assert g.n_groups == want
        assert g.passes >= 2                 # the path does not settle in one pass
        assert (g.group[alive == 0] == -1).all() and (g.digest[alive == 0] == 0).all()
        for r in range(1, 4):                # and as the rounds move it
            eng.step(1)
            check(eng, f"crafted, round {r}")
    finally:
        eng.close()


# ---- 2. the tier form on split, healed and shattered clusters ----------------------------------
def run_split(gs, case, rounds, extra=None):
    """The case on a tiered engine, checked every round: [(Groups, tier_info)]."""
    n = case["n"]
    eng = gs.Engine(gs.default_config(n, **case["cfg"]))
    out = {}
    try:
        eng.import_state(*sc.full_state(n), 0)
        assert eng.tier_info()[0] == 1

        def see(r):
            out[r] = (check(eng, f"round {r}"), eng.tier_info(full=True))
        gr.drive(case, eng, see, rounds)
        if extra:
            extra(eng, see)
    finally:
        eng.close()
    print(f"N={n}: passes per call", sorted({g.passes for g, _ in out.values()}))
    return out


def tier_split_round(out):
    """Among the checked rounds: one with the table current in the tier after
    the nibble path ran, one with escaped chunks written, one with more than
    one group."""
    seen = {r: (ti[1], ti[3], ti[2], g.n_groups) for r, (g, ti) in out.items()}
    print("round: (in tier, variant, escaped chunks, groups)", seen)
    return (any(t == 1 and v == 3 for t, v, _, _ in seen.values()) and any(e > 0 for _, _, e, _ in seen.values())
            and any(n > 1 for _, _, _, n in seen.values()))


def test_groups_tier_case_a(gs, monkeypatch):
    """N=1,000: one group through round 19, the two sides from round 20 on and
    after the heal of round 40; then three far-side members JOIN through the
    introducer and the groups follow the reference."""
    monkeypatch.setenv("GH_PLANE", "1")
    case = gr.CASE_A()
    far = np.flatnonzero(case["side"] == 1)[[0, 100, 299]]

    def rejoin(eng, see):
        eng.apply_events([(sc.JOIN, int(m)) for m in far])
        for r in range(51, 57):
            eng.step(1)
            see(r)
    out = run_split(gs, case, 50, rejoin)
    assert all(out[r][0].n_groups == 1 for r in range(1, 20))
    for r in range(20, 51):
        np.testing.assert_array_equal(out[r][0].group, gr.side_groups(case), err_msg=f"round {r}")
    assert out[18][0].n_views > 100 and out[19][0].n_views > 100
    assert tier_split_round(out), {r: ti for r, (_, ti) in out.items()}


def test_groups_tier_case_b(gs, monkeypatch):
    """N=263 in 512 padded columns of 256-member tiles, three sides."""
    monkeypatch.setenv("GH_PLANE", "1")
    case = gr.CASE_B()
    out = run_split(gs, case, 28)
    for r in range(20, 29):
        np.testing.assert_array_equal(out[r][0].group, gr.side_groups(case), err_msg=f"round {r}")
    assert tier_split_round(out), {r: ti for r, (_, ti) in out.items()}


def test_groups_tier_case_c_shatter(gs, monkeypatch):
    """T_fail = T_cleanup = 6: hundreds of fragments, through round 16."""
    monkeypatch.setenv("GH_PLANE", "1")
    out = run_split(gs, gr.CASE_C(), 16)
    assert out[15][0].n_groups > 200
    assert max(g.passes for g, _ in out.values()) >= 2


# ---- 3. healthy tier start, then frozen rows and storm rounds ----------------------------------
def test_groups_healthy_then_churn(gs, monkeypatch):
    monkeypatch.setenv("GH_PLANE", "1")
    n = 2048
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED0007, t_fail=16, t_cleanup=16))
    sched = {14: [(sc.CRASH, 7), (sc.LEAVE, 1500)], 18: [(sc.JOIN, 1500), (sc.JOIN, 7)]}
    tiers = []
    try:
        eng.import_state(*sc.full_state(n), 0)
        eng.step(12)
        assert eng.tier_info()[1] == 1
        g = check(eng, "round 12")
        assert g.n_groups == 1 and g.n_views == 1 and (g.group == 0).all()
        for r in range(13, 31):
            if sched.get(r):
                eng.apply_events(sched[r])
            eng.step(1)
            g = check(eng, f"round {r}")
            tiers.append(eng.tier_info()[1])
            if r == 14:
                assert g.group[7] == -1 and g.group[1500] == -1 and g.digest[7] == 0
        assert 0 in tiers and 1 in tiers, tiers  # 16-bit storm rounds and tier rounds both checked
    finally:
        eng.close()


# ---- 4. shards: the split comes from the state -------------------------------------------------
SHARD_N, SHARD_ROUNDS = 520, 10
SHARD_STOPPED = [297, 298, 299, 518, 519]


def block_state(n=SHARD_N):
    """Members 0..299 list only each other, 300..519 likewise, and both list
    the five stopped members."""
    hb = np.full((n, n), -1, np.int32)
    hb[:300, :300] = 2
    hb[300:, 300:] = 2
    hb[:, SHARD_STOPPED] = 2
    alive = np.ones(n, np.uint8)
    alive[SHARD_STOPPED] = 0
    return hb, np.zeros((n, n), np.int32), alive


def run_blocks(target):
    target.import_state(*block_state(), 0)
    out = [check(target, "after import")]
    for r in range(1, SHARD_ROUNDS + 1):
        target.step(1)
        out.append(check(target, f"round {r}"))
    assert all(g.n_groups == 2 for g in out)
    return out


def shard_cfg(gs, ring, **kw):
    cfg = dict(fanout=4, seed=0x5EED6704, t_fail=12, t_cleanup=12, **kw)
    if ring:
        cfg.update(peer_mode=gs.GH_PEER_RING, list_order=gs.GH_ORDER_APPEND)
    return gs.default_config(SHARD_N, **cfg)


@pytest.fixture(scope="module")
def single_blocks(gs):
    out = {}
    for ring in (False, True):
        eng = gs.Engine(shard_cfg(gs, ring))
        try:
            out[ring] = run_blocks(eng)
        finally:
            eng.close()
    return out


def test_groups_tier_blocks(gs, monkeypatch):
    """The block state on a tiered engine: after the import's 16-bit table the
    rounds write tier buffers, whose absent nibbles then carry the split."""
    monkeypatch.setenv("GH_PLANE", "1")
    eng = gs.Engine(shard_cfg(gs, False))
    tiers = []
    try:
        eng.import_state(*block_state(), 0)
        assert eng.tier_info()[:2] == (1, 0)
        for r in range(1, SHARD_ROUNDS + 1):
            eng.step(1)
            g = check(eng, f"round {r}")
            assert g.n_groups == 2 and g.n_views == 2
            tiers.append(eng.tier_info(full=True)[1::2])
    finally:
        eng.close()
    assert (1, 3) in tiers, tiers  # current in the tier, written by the nibble path


@pytest.mark.parametrize("world,layout,ring", [(2, 0, False), (3, 0, False), (2, 1, False), (2, 1, True)],
                         ids=["cols2", "cols3", "rows2", "rows2-ring-append"])
def test_groups_sharded(gs, single_blocks, world, layout, ring):
    """Every rank returns the groups of the group's own export, which are one
    engine's, every round; two groups throughout."""
    grp = gs.ShardGroup(shard_cfg(gs, ring, shard_layout=layout), world)
    try:
        out = run_blocks(grp)
    finally:
        grp.close()
    for r, (x, y) in enumerate(zip(out, single_blocks[ring])):
        gr.assert_groups_equal(x, (y.group, y.digest, y.n_groups), f"round {r}: {world} shards vs one engine")


@pytest.mark.parametrize("world,layout", [(2, 0), (3, 0), (2, 1)], ids=["cols2", "cols3", "rows2"])
def test_groups_sharded_crafted(gs, world, layout):
    """The crafted graphs on shards: the one-way path, the star and the ring run
    over a scattered permutation, so their edges cross every column and row
    cut, a member often learns its label from a row that lists it on another
    shard (the column minima's half of the MAX allreduce), and the labels
    need several hook passes, on which all ranks must agree."""
    n, R = 263, 40
    hb, ts, alive, want = crafted_state(n, R)
    cfg = dict(fanout=4, seed=0x5EED6701, t_fail=60, t_cleanup=60)
    one = gs.Engine(gs.default_config(n, **cfg))
    grp = gs.ShardGroup(gs.default_config(n, shard_layout=layout, **cfg), world)
    try:
        one.import_state(hb, ts, alive, R)
        grp.import_state(hb, ts, alive, R)
        for r in range(0, 3):
            if r:
                one.step(1)
                grp.step(1)
            g, y = check(grp, f"crafted on shards, round {r}"), one.groups()
            gr.assert_groups_equal(g, (y.group, y.digest, y.n_groups), f"round {r}: {world} shards vs one engine")
            if r == 0:
                assert g.n_groups == want and g.passes >= 2
    finally:
        one.close()
        grp.close()


# ---- 5. read-only, lazy, NULL outputs ----------------------------------------------------------
def test_groups_read_only_and_lazy(gs, monkeypatch):
    monkeypatch.setenv("GH_PLANE", "1")
    n = 1000
    cfg = dict(fanout=4, seed=0x5EED0C02, t_fail=6, t_cleanup=6)
    a, b = gs.Engine(gs.default_config(n, **cfg)), gs.Engine(gs.default_config(n, **cfg))
    try:
        assert a.memory_info() == b.memory_info()
        for e in (a, b):
            e.import_state(*sc.full_state(n), 0)
            e.apply_events([(sc.CRASH, 321)])
            e.step(8)
            e.census()
        mem = a.memory_info()
        assert mem == b.memory_info()
        b.groups()
        assert b.memory_info() == mem  # tables, arenas and the frozen store are as they were
        assert a.round == b.round
        for x, y in zip(a.export_state(), b.export_state()):
            np.testing.assert_array_equal(x, y)
        for r in range(5):
            b.groups()
            sa, sb = a.step(1), b.step(1)
            assert sa == sb, (r, sa, sb)
            b.groups()
            for x, y in zip(a.export_state(), b.export_state()):
                np.testing.assert_array_equal(x, y)
        assert a.tier_info(full=True) == b.tier_info(full=True) and a.round == b.round
    finally:
        a.close()
        b.close()


def test_groups_null_arguments(gs):
    n = 300
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED6705))
    lib = eng.lib
    try:
        ng, ps = C.c_int64(-1), C.c_int32(-1)
        assert lib.gh_groups(None, None, None, C.byref(ng), C.byref(ps)) == gs._abi.GH_EINVAL
        hb, ts, alive = sc.full_state(n)
        hb[:150, 150:] = -1
        hb[150:, :150] = -1
        alive[[3, 200]] = 0
        eng.import_state(hb, ts, alive, 0)
        ref = gr.groups_ref(hb, alive)
        full = check(eng, "imported halves")
        assert full.n_groups == 2
        group, digest = np.empty(n, np.int32), np.empty(n, np.uint64)
        p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        for g_, d_, n_, p_ in [(None, p(digest), C.byref(ng), C.byref(ps)), (p(group), None, C.byref(ng), C.byref(ps)),
                               (p(group), p(digest), None, C.byref(ps)), (p(group), p(digest), C.byref(ng), None),
                               (None, None, C.byref(ng), C.byref(ps)), (None, None, None, None)]:
            group[:], digest[:], ng.value, ps.value = -7, 7, -1, -1
            assert lib.gh_groups(eng.h, g_, d_, n_, p_) == gs.GH_OK
            if g_ is not None:
                np.testing.assert_array_equal(group, ref[0])
            if d_ is not None:
                np.testing.assert_array_equal(digest, ref[1])
            if n_ is not None:
                assert ng.value == 2
            if p_ is not None:
                assert ps.value >= 1
    finally:
        eng.close()


def test_groups_armed_lossy_journaled(gs):
    """An armed engine with loss, control loss and the journal on still
    answers, and Cluster.groups() lists the groups largest first."""
    n = 200
    eng = gs.Engine(gs.default_config(n, fanout=4, seed=0x5EED6706, t_fail=8, t_cleanup=8))
    try:
        eng.import_state(*sc.full_state(n), 0)
        eng.journal_enable(gs.GH_JOURNAL_VIEWS, 8)
        eng.set_loss(0.05, 0.05)
        eng.set_control_loss(gs.GH_CTL_REMOVE | gs.GH_CTL_LEAVE | gs.GH_CTL_JOIN)
        side = np.zeros(n, np.int32)
        side[120:] = 1
        eng.set_partition(side)
        for r in range(1, 15):
            eng.step(1)
            check(eng, f"round {r}")
    finally:
        eng.close()
    cl = gs.Cluster(40, t_fail=5, t_cleanup=5, seed=0x5EED6707)
    try:
        for i in range(40):
            cl.join(i)
            cl.tick(1)
        cl.crash(9)
        cl.tick(3)
        hb, _, alive = cl.engine.export_state()
        ref = gr.groups_ref(hb, alive)[0]
        got = cl.groups()
        assert [a.size for a in got] == sorted(gr.sizes(ref), reverse=True)
        for a in got:
            assert (ref[a] == a[0]).all() and (np.diff(a) > 0).all()
    finally:
        cl.engine.close()
