"""GPU parity off the defaults of three gh_config fields the rest of the suite
leaves alone -- `introducer` (0 everywhere else), `min_members` (4) and
`replicas` (compared with the oracle at 4 only) -- and with an introducer that
itself crashes, leaves and rejoins. The HIP engine against oracle/tablesim.c
bit for bit every round: counters, hb, ts, alive, failed set, detectors, the
maintained row counts and the D7 shadow entries; placement against or_put /
or_repair / or_get. Every precondition a case relies on (double entries, JOINs
while the introducer is down, empty ring senders, rows on the other side of the
literal 4, ...) is asserted on the oracle's output, never on the engine's.
Run on a MI355X: pytest -m gpu."""
import contextlib

import numpy as np
import pytest

import scenarios as sc
from test_gpu_parity import check_counts, compare, shadows_of
from test_oracle_crosscheck import IntroducerWatch, present_counts, ring_empty_reachable

pytestmark = pytest.mark.gpu

NO_SHADOW = np.iinfo(np.int32).min
ROWS = 1   # GH_LAYOUT_ROWS
N_I, I_OFF = 300, 157  # member 157: past the first 64- and 128-member tile, rank 1 of 3 column shards (128
#                        columns each), rank 1 of 2 and of 3 row shards


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


def make_engine(gs, n, cfg, layout):
    """layout: "single", "cols<G>" or "rows<G>" """
    if layout == "single":
        return gs.Engine(gs.default_config(n, **cfg))
    kind, world = layout[:4], int(layout[4:])
    return gs.ShardGroup(gs.default_config(n, shard_layout=ROWS if kind == "rows" else 0, **cfg), world)


@contextlib.contextmanager
def pair(gs, om, n, cfg, layout, state, r0=0):
    eng = make_engine(gs, n, cfg, layout)
    orc = om.Oracle(om.default_config(n, **cfg), threads=8)
    try:
        eng.import_state(*state, r0)
        orc.import_state(*state, r0)
        yield eng, orc
    finally:
        eng.close()
        orc.close()


def check_shadows(eng, orc, n, what):
    """the engine's shadow entries equal the oracle's, both as an export
    presents a tombstone's ts (scenarios.shadow_view); returns the oracle's"""
    r, tc = orc.round, orc.cfg.t_cleanup
    b = orc.debug_shadow()
    np.testing.assert_array_equal(sc.shadow_view(shadows_of(eng, n), r, tc), sc.shadow_view(b, r, tc),
                                  err_msg=f"shadow entries {what}")
    return b


def run_rounds(eng, orc, n, sched, first, last, per_round=None, every=1):
    """Rounds first..last in lockstep; per_round(r, oracle stats, oracle
    shadow vector) sees the oracle only."""
    for r in range(first, last + 1):
        ev = sched.get(r, [])
        if ev:
            eng.apply_events(ev)
            orc.apply_events(ev)
        s1, s2 = eng.step(1), orc.step(1)
        assert s1 == s2, f"round {r}: gpu {s1} != cpu {s2}"
        compare(eng, orc, r, full=r % every == 0 or r == last or bool(ev))
        sh = check_shadows(eng, orc, n, f"r={r}")
        if per_round:
            per_round(r, s2, sh)


def d7_cfg(peer_mode, **kw):
    return dict(fanout=3, seed=0x5EED0E10 + peer_mode, t_fail=4, t_cleanup=6, peer_mode=peer_mode, **kw)


# ---- a. the introducer is not member 0 -----------------------------------------

@pytest.mark.parametrize("layout", ["single", "cols3", "rows2"])
@pytest.mark.parametrize("peer_mode", [0, 1], ids=["pull", "ring"])
def test_introducer_off_zero(gs, oracle_mod, layout, peer_mode):
    """test_rejoin_while_tombstoned_d7's churn with member 157 as the
    introducer: the shadow row of the lean, nibble and per-cell paths, the
    JOIN / LEAVE event kernels and the JOIN broadcast's ghost row all meet an
    introducer outside tile 0 and owned by rank 1. Double entries occur."""
    n, I = N_I, I_OFF
    sched = sc.rejoin_churn(n, 40, 0xD7 + peer_mode, introducer=I)
    dual = []
    with pair(gs, oracle_mod, n, d7_cfg(peer_mode, introducer=I), layout, sc.full_state(n)) as (eng, orc):
        run_rounds(eng, orc, n, sched, 1, 40, lambda r, st, sh: dual.append(int((sh != NO_SHADOW).sum())))
    assert max(dual) > 0


# ---- b. the introducer stops -----------------------------------------------------

# a crash, a rejoin through itself, a leave and another rejoin
OUTAGE = [(8, sc.CRASH), (11, sc.JOIN), (20, sc.LEAVE), (23, sc.JOIN)]


def reimport_rows(eng, orc, lo, hi, r):
    """gh_import_state of rows [lo, hi) at round r: the oracle's own rows
    with every present heartbeat raised by one."""
    hb, ts, alive = orc.export_state()
    hb, ts, alive = hb[lo:hi].copy(), ts[lo:hi].copy(), alive[lo:hi].copy()
    hb[hb >= 0] += 1
    eng.import_state(hb, ts, alive, r, lo)
    orc.import_state(hb, ts, alive, r, lo)
    compare(eng, orc, r)


@pytest.mark.parametrize("layout", ["single", "cols3", "rows3"])
@pytest.mark.parametrize("peer_mode", [0, 1], ids=["pull", "ring"])
def test_introducer_outage(gs, oracle_mod, layout, peer_mode):
    """The same churn while introducer 157 itself crashes (r=8), rejoins
    through itself (11), leaves (20) and rejoins (23): JOINs that arrive while
    it is down reset their rows and are added nowhere, and its restart drops
    every shadow entry (reset_shadows for a fresh joiner). On 3 row shards
    rank 1 owns it and is the ghost source of the other two. At round 30,
    with shadow entries standing, rows [0, 100) are imported (the introducer's
    lists stay: so do the entries) and then rows [128, 200) (its row is
    rewritten: they go); ten more rounds follow."""
    n, I = N_I, I_OFF
    sched = sc.introducer_outage(sc.rejoin_churn(n, 40, 0xD7 + peer_mode, introducer=I), I, OUTAGE)
    watch = IntroducerWatch(sched, I, listsim=False)
    with pair(gs, oracle_mod, n, d7_cfg(peer_mode, introducer=I), layout, sc.full_state(n)) as (eng, orc):
        run_rounds(eng, orc, n, sched, 1, 30, lambda r, st, sh: watch.observe(orc, r, sh))
        watch.check(2)
        before = orc.debug_shadow()
        assert (before != NO_SHADOW).any()
        reimport_rows(eng, orc, 0, 100, 30)
        after = check_shadows(eng, orc, n, "after an import of rows [0, 100)")
        np.testing.assert_array_equal(after, before)
        reimport_rows(eng, orc, 128, 200, 30)
        after = check_shadows(eng, orc, n, "after an import of rows [128, 200)")
        assert (after == NO_SHADOW).all()
        run_rounds(eng, orc, n, sched, 31, 40)


# ---- d. the nibble path with the shadow row off 0 ---------------------------------

@pytest.mark.parametrize("layout", ["single", "rows2"])
def test_nibble_shadow_row(gs, oracle_mod, monkeypatch, layout):
    """N=2,048, k=4 pull on the 4-bit tier with introducer 1500: members leave
    and rejoin inside the 16-round tombstone window, so the introducer holds
    them twice and shadow_row = 1500 while the tier is current. The nibble
    variant (tier_info 3) runs in a round in which the oracle has shadow
    entries, on every shard."""
    monkeypatch.setenv("GH_PLANE", "1")
    n, I = 2048, 1500
    cfg = dict(fanout=4, seed=0x5EED0E30, t_fail=16, t_cleanup=16, introducer=I)
    sched = {6: [(sc.LEAVE, c) for c in (7, 300, 1499, 1501, 2047)], 8: [(sc.JOIN, c) for c in (7, 300, 1499, 1501, 2047)],
             14: [(sc.LEAVE, c) for c in (63, 64, 1024)], 17: [(sc.JOIN, c) for c in (63, 64, 1024)]}
    nibble_with_shadow = []
    with pair(gs, oracle_mod, n, cfg, layout, sc.full_state(n)) as (eng, orc):
        def per_round(r, st, sh):
            info = eng.run("tier_info", full=True) if layout != "single" else [eng.tier_info(full=True)]
            if (sh != NO_SHADOW).any() and all(x[3] == 3 for x in info):
                nibble_with_shadow.append(r)
        run_rounds(eng, orc, n, sched, 1, 30, per_round)
    assert nibble_with_shadow


# ---- e. min_members off 4 on short lists -------------------------------------------

MM_R0 = 10


def short_run(gs, om, n, layout, peer_mode, quirk, min_members):
    hb, ts, alive = sc.short_list_state(n, 0x51 + min_members, MM_R0, mid=min_members > 4)
    sched = {r + MM_R0 + 1: ev for r, ev in sc.random_churn(n, 19, 0x60 + min_members).items()}
    cfg = dict(fanout=3, seed=0x5EED0E40 + min_members, peer_mode=peer_mode, detect_mode=int(quirk),
               min_members=min_members)
    stats = []
    with pair(gs, om, n, cfg, layout, (hb, ts, alive), MM_R0) as (eng, orc):
        run_rounds(eng, orc, n, sched, MM_R0 + 1, MM_R0 + 20, lambda r, st, sh: stats.append(st))
    L = present_counts(hb)
    assert stats[0]["active_rows"] == int((L >= min_members).sum())  # (no event, no REMOVE in the first round)
    if min_members <= 3:
        assert ((L >= min_members) & (L < 4)).any()
        if peer_mode == 1 and ring_empty_reachable(quirk, min_members):
            assert sum(s["ring_empty"] for s in stats) > 0
    else:
        assert ((L < min_members) & (L >= 4)).any()


@pytest.mark.parametrize("layout,n", [("single", 40), ("single", 300), ("cols3", 300), ("rows2", 300)])
@pytest.mark.parametrize("peer_mode", [0, 1], ids=["pull", "ring"])
@pytest.mark.parametrize("quirk", [False, True], ids=["canonical", "quirk"])
@pytest.mark.parametrize("min_members", [0, 1, 3, 7])
def test_min_members_short_lists(gs, oracle_mod, layout, n, peer_mode, quirk, min_members):
    """short_list_state (lists of length 0 to 3, with and without the row's
    own entry; 4 to 8 too for the threshold 7) imported at round 10, then 20
    rounds of churn, at guard thresholds 0, 1, 3 and 7: the threshold read by
    active_row, k_prologue, k_active_exact and k_active_post, and ring senders
    whose targets coincide, name the sender or do not exist.

    Where ring_empty is counted does not depend on N. One engine and row
    shards take the targets from whole lists (k_ring_fast, the first
    round.hip site) in a round with no flag and no REMOVE pending and a known
    flag count, and count the row (k_ring_select, the second site) otherwise:
    after an import or a write from the host, and while a flag or a REMOVE is
    pending, so in every round with a detection. Column shards always count. A row that empties itself does so by a detection, so
    it is counted at the second site; the rows of length 0 that threshold 0
    lets through every round are counted at the first one in the quiet
    rounds. ring_empty > 0 over the run is asserted on the oracle wherever
    the reference can reach it (test_oracle_crosscheck.ring_empty_reachable:
    not with the quirk sweep above threshold 1)."""
    short_run(gs, oracle_mod, n, layout, peer_mode, quirk, min_members)


@pytest.mark.parametrize("quirk", [False, True], ids=["canonical", "quirk"])
@pytest.mark.parametrize("min_members", [0, 1, 3, 7])
def test_min_members_short_lists_append(gs, min_members, quirk):
    """The same on one engine in ring mode under GH_ORDER_APPEND (the ring of
    order.hip, the third ring_empty site) against listsim's literal lists,
    with test_gpu_list_order's comparison (list order included)."""
    import oracle.listsim as L
    from test_gpu_list_order import APPEND, run_pair
    n, seed = 40, 0x5EED0E50 + min_members
    hb, ts, alive = sc.short_list_state(n, 0x51 + min_members, MM_R0, mid=min_members > 4)
    sched = {r + 1: ev for r, ev in sc.random_churn(n, 19, 0x60 + min_members).items()}  # run_pair counts from 1
    eng = gs.Engine(gs.default_config(n, peer_mode=gs.GH_PEER_RING, detect_mode=int(quirk), seed=seed,
                                      list_order=APPEND, min_members=min_members))
    ls = L.ListSim.from_dense(hb, ts, alive, MM_R0, seed=seed, peer_mode="ring", quirk=quirk, order="append")
    empty = []
    step = ls.step
    ls.step = lambda k=1: empty.append(step(k)) or empty[-1]
    L.MIN_NODES = min_members
    try:
        eng.import_state(hb, ts, alive, MM_R0)
        run_pair(eng, ls, n, 20, sched)
    finally:
        L.MIN_NODES = 4
        eng.close()
    if ring_empty_reachable(quirk, min_members):
        assert sum(s["ring_empty"] for s in empty) > 0


# ---- f. min_members on the fast paths ----------------------------------------------

def guard_rows_state(n, seed, r0, crashed):
    """(hb, ts, alive, low, high): full membership but 32 rows `low` that hold
    4 to 6 members and 32 rows `high` that hold 7 to 9, two of `crashed` among
    them; what such a row does not hold it holds tombstoned at r0, so with a
    long T_cleanup it cannot merge it back and stays short."""
    rng = np.random.default_rng(seed)
    hb = np.full((n, n), r0 + 2, np.int32)
    ts = np.full((n, n), r0, np.int32)
    rows = rng.choice(np.setdiff1d(np.arange(n), crashed), 64, replace=False)
    low, high = rows[:32], rows[32:]
    for k, i in enumerate(rows):
        ln = (4 + k % 3) if k < 32 else (7 + k % 3)
        must = [i] + ([int(c) for c in rng.choice(crashed, 2, replace=False)] if k >= 32 else [])
        rest = rng.choice(np.setdiff1d(np.arange(n), np.concatenate([crashed, [i]])), ln - len(must), replace=False)
        hb[i, :] = -2
        hb[i, must] = r0 + 2
        hb[i, rest] = r0 + 2
    return hb, ts, np.ones(n, np.uint8), low, high


@pytest.mark.parametrize("k", [4, 5])
def test_min_members_fast_paths(gs, oracle_mod, monkeypatch, k):
    """N=2,048 pull on the sender plane at threshold 7: 32 imported rows of
    length 4 to 6 never gossip, 32 of length 7 to 9 do until the REMOVE of a
    small crash wave takes some of them under 7. k=4 runs the nibble path's 4
    senders per row step with the guard rows listed; k=5 the 8-sender step,
    which takes the lean guard. Bit-exact every round."""
    monkeypatch.setenv("GH_PLANE", "1")
    n, r0, mm = 2048, 10, 7
    crashed = np.asarray(sc.crash_ids(n, 8 / n, 0x5EED0E60 + k))
    hb, ts, alive, low, high = guard_rows_state(n, k, r0, crashed)
    cfg = dict(fanout=k, seed=0x5EED0E60 + k, t_fail=6, t_cleanup=20, min_members=mm)
    sched = {r0 + 2: [(sc.CRASH, int(c)) for c in crashed]}
    stats, under = [], []
    with pair(gs, oracle_mod, n, cfg, "single", (hb, ts, alive), r0) as (eng, orc):
        def per_round(r, st, sh):
            stats.append(st)
            L = present_counts(orc.export_state()[0])
            under.append(int((L[high] < mm).sum()))
        run_rounds(eng, orc, n, sched, r0 + 1, r0 + 16, per_round)
    L0 = present_counts(hb)
    assert ((L0[low] >= 4) & (L0[low] < mm)).all() and (L0[high] >= mm).all()
    assert stats[0]["active_rows"] == n - 32
    assert under[0] == 0 and max(under) > 0, under          # rows fell under 7 after the REMOVE
    assert sum(s["failed_members"] for s in stats) >= len(crashed)


def test_min_members_collapse_active_exact(gs, oracle_mod):
    """test_quirk_c2_collapse's N=4,096 at the reference's 5-round timeouts
    with threshold 9: a round detects more than GH_DLIST_MAX (1,024) members,
    so the rows' activity after the REMOVEs is decided by k_active_exact
    against the new threshold."""
    n = 4096
    sched = {8: [(sc.CRASH, c) for c in sc.crash_ids(n, 0.01, 0x5EED0002)]}
    cfg = dict(fanout=3, seed=0x5EED0002, detect_mode=1, min_members=9)
    stats = []
    with pair(gs, oracle_mod, n, cfg, "single", sc.full_state(n)) as (eng, orc):
        run_rounds(eng, orc, n, sched, 1, 12, lambda r, st, sh: stats.append(st), every=3)
    assert max(s["failed_members"] for s in stats) > 1024, [s["failed_members"] for s in stats]


# ---- g. replicas and master at creation ----------------------------------------------

def both(eng, orc, name, *args):
    a, b = getattr(eng, name)(*args), getattr(orc, name)(*args)
    if isinstance(b, tuple):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y, err_msg=name)
    elif isinstance(b, np.ndarray):
        np.testing.assert_array_equal(a, b, err_msg=name)
    else:
        assert a == b, name
    return b


def master_state(n, master, drop, r0=3):
    hb, ts, alive = sc.full_state(n)
    ts[:] = r0
    hb[master, drop] = -1
    ts[master, drop] = 0
    return hb, ts, alive


@pytest.mark.parametrize("layout", ["single", "cols3", "rows3"])
@pytest.mark.parametrize("R", [1, 2, 3, 5, 8])
def test_replicas_and_master_at_creation(gs, oracle_mod, layout, R):
    """N=64, 1,000 file slots, R replicas, master 37 from gh_create on (its
    list alone lacks three members, so candidates drawn from any other row
    differ): 701 puts, every 9th deleted, a 10% crash wave through detection,
    repair from the master and from another detector, gets of every slot and
    100 re-puts, all equal to the oracle's -- replicas, versions, statuses,
    plans and the exported table with its Philox draw counters."""
    n, F, master = 64, 1000, 37
    cfg = dict(max_files=F, replicas=R, master=master, seed=0x5EED0E70 + R, t_fail=4, t_cleanup=4)
    state = master_state(n, master, [5, 21, 50])
    allf = np.arange(F, dtype=np.int32)
    with pair(gs, oracle_mod, n, cfg, layout, state, 3) as (eng, orc):
        rep, ver, st = both(eng, orc, "put", np.arange(701, dtype=np.int32))
        assert (st == gs.GH_OK).all() and not np.isin(rep[:, :R], [5, 21, 50]).any()
        gone = np.arange(0, 701, 9, dtype=np.int32)
        both(eng, orc, "delete_files", gone)
        both(eng, orc, "export_files")
        crashed = sc.crash_ids(n, 0.1, 0x5EED0E70 + R, introducer=master)
        sched = {4: [(sc.CRASH, c) for c in crashed]}
        dets = set()
        run_rounds(eng, orc, n, sched, 4, 12, lambda r, s, sh: dets.update(int(x) for x in orc.read_detectors()))
        other = min(dets - {master})
        plan = both(eng, orc, "repair", master)
        assert len(plan) > 0
        both(eng, orc, "repair", other)
        both(eng, orc, "export_files")
        both(eng, orc, "get_files", allf)
        both(eng, orc, "put", gone[:100])
        both(eng, orc, "get_files", allf)
        both(eng, orc, "export_files")


@pytest.mark.parametrize("R", [1, 2, 3, 5, 8])
def test_replicas_starving(gs, oracle_mod, R):
    """The master's list cut to R members: M - 1 < R candidates can be drawn,
    so every put starves (the starvation test (M - 1) - in_pool < R - len at
    each R); statuses and tables equal the oracle's."""
    n, F, master = 64, 64, 37
    cfg = dict(max_files=F, replicas=R, master=master, seed=0x5EED0E80 + R)
    keep = [master] + [c for c in (3, 11, 29, 40, 41, 58, 63)][: R - 1]
    state = master_state(n, master, [c for c in range(n) if c not in keep])
    with pair(gs, oracle_mod, n, cfg, "single", state, 3) as (eng, orc):
        assert list(orc.lsm(master)[0]) == sorted(keep)
        rep, ver, st = both(eng, orc, "put", np.arange(40, dtype=np.int32))
        assert (st == gs.GH_EPLACEMENT_STARVED).all()
        both(eng, orc, "export_files")
        both(eng, orc, "get_files", np.arange(F, dtype=np.int32))


# ---- h. the Cluster's vote gate ---------------------------------------------------------

def test_cluster_vote_gate_min_members_2(gs, oracle_mod):
    """Cluster(elect=True) with 4 members at min_members = 2: master 0 crashes
    and the 3 members left, whose lists the literal 4 would keep from running,
    vote member 1 in. Round by round against the oracle Tally(min_members=2)
    fed from tablesim's table (which the engine's equals), as
    test_cluster_master_crash_election does at 4."""
    from oracle import election as el
    n, tf = 4, 8
    cfg = dict(seed=0x5EED0E90, t_fail=tf, t_cleanup=tf, peer_mode=gs.GH_PEER_PULL, min_members=2)
    cl = gs.Cluster(n, elect=True, max_files=16, **cfg)
    eng = cl.engine
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, max_files=16, **cfg))
    try:
        eng.import_state(*sc.full_state(n), 0)
        orc.import_state(*sc.full_state(n), 0)
        cl.tick(2)
        orc.step(2)
        cl.crash(0)
        orc.apply_events([(sc.CRASH, 0)])
        tally = el.Tally(n, master=0, min_members=2)
        pending, elected, short_votes = {}, [], 0
        for _ in range(20):
            cl.tick(1)
            orc.step(1)
            r = eng.round
            # a log.Fatal of this round (Fail_recover dialling the dead master) is a crash the Cluster
            # queued after the round; both apply it in the next one
            orc.apply_events([(sc.CRASH, m) for fr, m, _ in cl.fatal if fr == r])
            compare(eng, orc, r)
            hb, _, alive = orc.export_state()
            for m in pending.pop(r, []):
                tally.finish_rebuild(m, int(np.flatnonzero(hb[m] >= 0)[0]))
            first, ln, has = el.vote_scan(hb, tally.mview)
            short_votes += int(((alive != 0) & (ln >= 2) & (ln < 4) & (has == 0)).sum())
            for m in tally.round(alive, first, ln, has, dead=cl.dead):
                elected.append(m)
                pending[r + 2] = pending.get(r + 2, []) + [m]
            np.testing.assert_array_equal(cl.mview, tally.mview, err_msg=f"r={r}")
        assert elected == [1] and short_votes > 0 and not pending  # the oracle's election, by lists shorter than 4
        assert [m for _, m in cl.elections] == [1] and cl.master == 1
    finally:
        eng.close()
        orc.close()


# ---- c. append order with the introducer off 0 -----------------------------------------

@pytest.mark.parametrize("layout", ["single", "rows2"])
@pytest.mark.parametrize("case", ["ring_quirk", "pull"])
def test_introducer_off_zero_append(gs, layout, case):
    """The churn of test_introducer_off_zero under GH_ORDER_APPEND against
    ListSim(order="append", introducer=157): what test_gpu_list_order
    compares every round (counters, hb, ts, alive, failed set, detectors,
    every row's list order) and the shadow entries, through listsim's
    recorded run (tests/list_digest.py: its replay takes a minute at N=300).
    One engine and 2 row shards; ring with the quirk sweep, and pull."""
    import list_digest as ld
    from test_gpu_list_order import APPEND
    n, c, gold = ld.N, ld.CASES[case], ld.load()[case]
    cfg = dict(fanout=3, seed=c["seed"], t_fail=ld.T_FAIL, t_cleanup=ld.T_CLEANUP, introducer=ld.I,
               peer_mode=gs.GH_PEER_RING if c["peer_mode"] == "ring" else gs.GH_PEER_PULL,
               detect_mode=int(c["quirk"]), list_order=APPEND)
    sched = ld.schedule(case)
    assert len(gold) == ld.ROUNDS and max(x["dual"] for x in gold) > 0 and max(x["reordered"] for x in gold) > 0
    eng = make_engine(gs, n, cfg, layout)
    try:
        eng.import_state(*sc.full_state(n), 0)
        for r, want in enumerate(gold, 1):
            if r in sched:
                eng.apply_events(sched[r])
            st = eng.step(1)
            check_counts(eng, r)
            hb, ts, alive = eng.export_state()
            bm = eng.read_failed()
            got = ld.round_record(st, hb, ts, alive, [m for m in range(n) if bm[m >> 5] >> (m & 31) & 1],
                                  eng.read_detectors(), [list(eng.lsm(i)[0]) for i in range(n)],
                                  sc.shadow_view(shadows_of(eng, n), r, ld.T_CLEANUP))
            for key in ("stats", "failed", "detectors", "alive", "hb", "ts", "lists", "shadow"):
                assert got[key] == want[key], f"r={r} {key}: gpu {got[key]} != listsim {want[key]}"
    finally:
        eng.close()
