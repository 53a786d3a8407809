"""Cross-check the two independent CPU restatements of the reference:
oracle/listsim.py (literal Go list semantics) and oracle/tablesim.c (dense
tables), round by round on seeded churn scenarios (SPEC.md)."""
import numpy as np
import pytest

from oracle.listsim import ListSim

import scenarios as sc


def run_pair(om, n, rounds, sched, peer_mode, fanout=3, quirk=False, seed=0x5EED0001,
             init_full=False, t_fail=5, t_cleanup=5, remove="all", per_round=None, introducer=0,
             min_members=4, state=None):
    """`state` = (hb, ts, alive, r0) is imported at round r0 into both (the run
    is then rounds r0 + 1 .. r0 + rounds, `sched` keyed by those)."""
    cfg = om.default_config(n, peer_mode=om.GH_PEER_RING if peer_mode == "ring" else om.GH_PEER_PULL,
                            fanout=fanout, detect_mode=int(quirk), seed=seed, t_fail=t_fail,
                            t_cleanup=t_cleanup, introducer=introducer, min_members=min_members,
                            remove_mode=om.GH_REMOVE_LIST if remove == "list" else om.GH_REMOVE_ALL)
    orc = om.Oracle(cfg)
    kw = dict(seed=seed, peer_mode=peer_mode, fanout=fanout, quirk=quirk, remove=remove, introducer=introducer)
    r0 = 0
    if init_full and state is None:
        state = sc.full_state(n) + (0,)
    if state is not None:
        hb, ts, alive, r0 = state
        orc.import_state(hb, ts, alive, r0)
        ls = ListSim.from_dense(hb, ts, alive, r0, **kw)
    else:
        ls = ListSim(n, **kw)
    import oracle.listsim as L
    L.T_FAIL, L.T_CLEANUP, L.MIN_NODES = t_fail, t_cleanup, min_members
    try:
        for r in range(r0 + 1, r0 + rounds + 1):
            ev = sched.get(r, [])
            if ev:
                orc.apply_events(ev)
                ls.apply_events(ev)
            s1 = orc.step(1)
            s2 = ls.step(1)
            assert s1 == s2, f"round {r}: stats {s1} != {s2}"
            orc.last_stats = s1
            h1, t1, a1 = orc.export_state()
            h2, t2, a2 = ls.dense()
            np.testing.assert_array_equal(a1, a2, err_msg=f"alive r={r}")
            np.testing.assert_array_equal(h1, h2, err_msg=f"hb r={r}")
            np.testing.assert_array_equal(t1, sc.export_view(h2, t2, r, t_cleanup)[1], err_msg=f"ts r={r}")
            bm = orc.read_failed()
            failed = [c for c in range(n) if bm[c >> 5] >> (c & 31) & 1]
            assert failed == ls.last_failed
            assert list(orc.read_detectors()) == ls.last_detectors
            if per_round:
                per_round(orc, ls, r)
    finally:
        L.T_FAIL, L.T_CLEANUP, L.MIN_NODES = 5, 5, 4
    return orc, ls


@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
@pytest.mark.parametrize("quirk", [False, True])
def test_bootstrap_crash_c1(oracle_mod, peer_mode, quirk):
    """BASELINE config 1 shape: 10 joins, member 7 crashes at r=30, to r=60."""
    n = 10
    sched = sc.bootstrap_schedule(n)
    sched.setdefault(30, []).append((sc.CRASH, 7))
    orc, ls = run_pair(oracle_mod, n, 60, sched, peer_mode, quirk=quirk)
    hb, ts, alive = orc.export_state()
    assert alive[7] == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
def test_random_churn(oracle_mod, seed, peer_mode):
    n = 16
    sched = sc.random_churn(n, 50, seed)
    run_pair(oracle_mod, n, 50, sched, peer_mode, fanout=2, init_full=True, seed=0x1000 + seed)


@pytest.mark.parametrize("seed", [4, 5])
def test_random_churn_quirk(oracle_mod, seed):
    n = 14
    sched = sc.random_churn(n, 40, seed, p_crash=0.08)
    run_pair(oracle_mod, n, 40, sched, "ring", init_full=True, quirk=True, seed=0x2000 + seed)


def test_fast_fail_short_cooldown(oracle_mod):
    """T_fail/T_cleanup off their defaults (tombstones survive detection)."""
    n = 12
    sched = sc.random_churn(n, 40, 9, p_crash=0.1)
    run_pair(oracle_mod, n, 40, sched, "pull", fanout=3, init_full=True, t_fail=3, t_cleanup=6)


# ---- the reference's REMOVE recipients (GH_REMOVE_LIST, slave/slave.go:344) ----

@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
@pytest.mark.parametrize("quirk", [False, True])
def test_random_churn_remove_list(oracle_mod, seed, peer_mode, quirk):
    """listsim's literal Remove (recipients = the detector's list right after
    removeMember in the sweep) against tablesim's column-wise form."""
    n = 16
    sched = sc.random_churn(n, 50, seed, p_crash=0.06)
    run_pair(oracle_mod, n, 50, sched, peer_mode, fanout=2, init_full=True, quirk=quirk,
             seed=0x3000 + seed, remove="list")


@pytest.mark.parametrize("quirk", [False, True])
def test_collapse_remove_list(oracle_mod, quirk):
    """The reference's constants at a size where dissemination outruns them
    not: the round-6 detection storm and the collapse, literal recipients."""
    n = 48
    run_pair(oracle_mod, n, 14, {}, "pull", fanout=3, init_full=True, quirk=quirk, seed=0x5EED0002,
             remove="list")


@pytest.mark.parametrize("seed", [7, 8])
def test_bootstrap_churn_remove_list(oracle_mod, seed):
    n = 12
    sched = sc.bootstrap_schedule(n)
    for r, ev in sc.random_churn(n, 50, seed, p_crash=0.05).items():
        sched.setdefault(r + n, []).extend(ev)
    run_pair(oracle_mod, n, 60, sched, "ring", init_full=False, seed=0x4000 + seed, remove="list")


@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
@pytest.mark.parametrize("quirk", [False, True])
@pytest.mark.parametrize("seed", [11, 12])
def test_rejoin_while_tombstoned(oracle_mod, peer_mode, quirk, seed):
    """SPEC D7 under churn: members leave or crash and rejoin while the
    introducer still holds their tombstone, so its list holds them twice
    (MemberList and RecentFailList, slave/slave.go:228-230, 250-255); later
    LEAVEs, REMOVEs and detections meet the double entry
    (:276-286) and cleanFailList releases the old entry (:484-497).
    listsim (the literal lists) = tablesim (the shadow entries) every round,
    and double entries do occur."""
    n = 12
    sched = sc.rejoin_churn(n, 45, seed)
    seen = []

    def per_round(orc, ls, r):
        sh = orc.debug_shadow()
        I = ls.nodes[0]
        dual = sorted(m.addr for m in I.members if any(f.addr == m.addr for f in I.recent_fail))
        assert sorted(np.nonzero(sh != np.iinfo(np.int32).min)[0].tolist()) == dual, (r, sh, dual)
        for f in I.recent_fail:  # the entry's own ts (removeMember kept the Member, :280)
            if f.addr in dual:
                assert sh[f.addr] == f.ts, (r, f.addr, sh[f.addr], f.ts)
        seen.append(len(dual))

    run_pair(oracle_mod, n, 45, sched, peer_mode, quirk=quirk, init_full=True, seed=0x3000 + seed,
             t_fail=4, t_cleanup=6, per_round=per_round)
    assert max(seen) > 0, seen


# ---- off the default introducer and min_members --------------------------------

NO_SHADOW = np.iinfo(np.int32).min


class IntroducerWatch:
    """per_round hook for runs with the introducer off 0 and stopping: the
    shadow entries equal listsim's double entries at the introducer, and the
    preconditions of such a run are recorded, all from the oracle's output:
    double entries per round, JOIN batches that arrived while the introducer
    was down, and its fresh rejoins."""

    def __init__(self, sched, I, listsim=True):
        self.sched, self.I, self.listsim = sched, I, listsim
        self.dual = {}          # round -> number of shadow entries
        self.joins_down = 0     # JOIN batches while the introducer was down
        self.rejoins = []       # rounds in which the stopped introducer rejoined
        self.up = True

    def __call__(self, orc, ls, r):
        I = self.I
        sh = orc.debug_shadow()
        if self.listsim:
            nd = ls.nodes[I]
            dual = sorted(m.addr for m in nd.members if any(f.addr == m.addr for f in nd.recent_fail))
            assert sorted(np.nonzero(sh != NO_SHADOW)[0].tolist()) == dual, (r, sh, dual)
            for f in nd.recent_fail:
                if f.addr in dual:
                    assert sh[f.addr] == f.ts, (r, f.addr, sh[f.addr], f.ts)
        self.observe(orc, r, sh)

    def observe(self, orc, r, sh):
        I = self.I
        joins = [c for kind, c in self.sched.get(r, []) if kind == sc.JOIN]
        if not self.up and joins and I not in joins:
            self.joins_down += 1
        if not self.up and I in joins:
            self.rejoins.append(r)
        self.up = bool(orc.export_state()[2][I])
        self.dual[r] = int((sh != NO_SHADOW).sum())

    def check(self, n_rejoins):
        """the preconditions: double entries occurred, JOINs arrived while the
        introducer was down, and each fresh rejoin emptied a shadow vector
        that was not empty the round before"""
        assert max(self.dual.values()) > 0, self.dual
        assert self.joins_down > 0
        assert len(self.rejoins) == n_rejoins, self.rejoins
        for r in self.rejoins:
            assert self.dual[r] == 0 and self.dual[r - 1] > 0, (r, self.dual)


# (introducer, its stops) at N = 12 over 45 rounds: a crash, a rejoin through
# itself, a leave and another rejoin
OUTAGE_N12 = [(sc.CRASH, 5), (sc.JOIN, 8), (sc.LEAVE, 13), (sc.JOIN, 16)]


def outage_schedule(n, rounds, seed, I, stops=OUTAGE_N12):
    return sc.introducer_outage(sc.rejoin_churn(n, rounds, seed, introducer=I), I,
                                [(r, kind) for kind, r in stops])


@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
@pytest.mark.parametrize("quirk", [False, True])
@pytest.mark.parametrize("I,min_members", [(7, 4), (11, 1), (5, 9), (0, 0)])
def test_introducer_off_zero_with_outages(oracle_mod, peer_mode, quirk, I, min_members):
    """The introducer is member I (first, last, middle), the rejoin churn
    spares it, and it stops itself: it crashes and rejoins through itself,
    then leaves and rejoins; JOINs that arrive while it is down reset their
    rows and are added nowhere; its fresh rejoin drops every RecentFailList
    entry (the shadow vector empties). listsim = tablesim every round at four
    guard thresholds."""
    n = 12
    sched = outage_schedule(n, 45, 12, I)
    watch = IntroducerWatch(sched, I)
    run_pair(oracle_mod, n, 45, sched, peer_mode, quirk=quirk, init_full=True, seed=0x3100 + I,
             t_fail=4, t_cleanup=6, per_round=watch, introducer=I, min_members=min_members)
    watch.check(2)


def present_counts(hb):
    return (np.asarray(hb) >= 0).sum(axis=1)


def ring_empty_reachable(quirk, min_members):
    """An empty ring sender is a row that passes the guard and holds nobody
    after its own sweep. The canonical sweep empties any list of stale
    members without the row's own entry. The quirk sweep (the range over the
    slice that removeMember shifts, slave/slave.go:464-477) reads every other
    entry of a run of candidates, so of L >= 2 stale members at least one
    stays: with it a sender is empty only from a list of length 0 or 1, which
    a threshold of 2 or more never lets through."""
    return min_members <= (1 if quirk else 3)


@pytest.mark.parametrize("peer_mode", ["ring", "pull"])
@pytest.mark.parametrize("quirk", [False, True])
@pytest.mark.parametrize("min_members", [0, 1, 3, 7])
def test_min_members_short_lists(oracle_mod, peer_mode, quirk, min_members):
    """The guard threshold off 4 on lists of length 0 to 3 (and 4 to 8 for
    the threshold above 4): rows shorter than 4 gossip, ring targets
    coincide, name the sender or do not exist (ring_empty). The round after
    the import has no event and no REMOVE in flight, so the rows the guard
    passes are known from the imported lists: the oracle's active_rows is
    that count, and rows on the other side of the literal 4 are among them."""
    n, r0 = 40, 10
    hb, ts, alive = sc.short_list_state(n, 0x51 + min_members, r0, mid=min_members > 4)
    sched = {r + r0 + 1: ev for r, ev in sc.random_churn(n, 19, 0x60 + min_members).items()}
    L = present_counts(hb)
    stats = []

    def per_round(orc, ls, r):
        stats.append(orc.last_stats)

    orc, ls = run_pair(oracle_mod, n, 20, sched, peer_mode, quirk=quirk, seed=0x3200 + min_members,
                       min_members=min_members, state=(hb, ts, alive, r0), per_round=per_round)
    assert r0 + 1 not in sched
    assert stats[0]["active_rows"] == int((L >= min_members).sum())
    if min_members <= 3:
        assert ((L >= min_members) & (L < 4)).any()
        if peer_mode == "ring" and ring_empty_reachable(quirk, min_members):
            assert sum(s["ring_empty"] for s in stats) > 0
    else:
        assert ((L < min_members) & (L >= 4)).any()
