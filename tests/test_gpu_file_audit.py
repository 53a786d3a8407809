"""gh_file_audit / gh_file_select (csrc/files.hip, DESIGN.md "File audit"):
the device-side audit of the master's replica table -- working-replica
histogram, starved placements, per-member load and sole copies -- and the
file selection by holder and working count, against the numpy audit of the
engine's own export (tests/file_audit_ref.py), exactly: every replica count's
kernel, both atomics paths, list order, column and row shards, and as a
prediction of what gh_repair then does. Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import scenarios as sc
from file_audit_ref import assert_audit_equal, file_audit_ref, file_select_ref

pytestmark = pytest.mark.gpu

ALIVE = -1  # GH_AVAIL_ALIVE


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


def table(eng):
    rep, ver, _, _ = eng.export_files()
    return rep, ver


def avail_of(eng, observer):
    """The availability vector as the header defines it, from the exports."""
    if observer == ALIVE:
        return eng.alive() != 0
    return eng.export_state(observer, 1)[0][0] >= 0


def check_audit(eng, observer, msg=""):
    """The engine's audit against the reference audit of its own exports."""
    rep, ver = table(eng)
    cand = eng.lsm(int(eng.cfg.master))[0]
    want = file_audit_ref(rep, ver, avail_of(eng, observer), eng.n, cand)
    got = eng.file_audit(observer)
    assert_audit_equal(got, want, f"{msg} observer {observer}")
    return got


def check_select(eng, observer, member, max_working, caps=(None,)):
    rep, ver = table(eng)
    want = file_select_ref(rep, ver, avail_of(eng, observer), eng.n, member, max_working)
    for cap in caps:
        got = eng.file_select(observer, member, max_working, cap)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, want if cap is None else want[:cap],
                                      err_msg=f"select({observer}, {member}, {max_working}, cap={cap})")
    return want


N, F, PUT = 64, 1000, 701
CRASHED = [int(c) for c in sc.crash_ids(N, 0.1, 0x5EED0F01)]
LIVE = next(i for i in range(1, N) if i not in CRASHED)
# pull gossip that keeps 64 members listed through the wave (k = 3 with T_fail = 5 sheds live members)
STABLE = dict(fanout=4, t_fail=8, t_cleanup=8)
ROUNDS = 14  # the wave is detected in round 9


def churned(make, R, **kw):
    """N = 64, 1,000 slots: 701 files put while the master does not list
    member 63 (so 63 holds nothing), every 9th deleted, then a 10% crash wave
    stepped past detection. `make(cfg)` builds the engine(s); returns them."""
    import gossipsim as g
    cfg = dict(max_files=F, replicas=R, seed=0x5EED0F00 + R, **STABLE)
    cfg.update(kw)
    hb, ts, alive = sc.full_state(N)
    hb[0, 63] = -1
    ts[0, 63] = 0
    engs = make(cfg)
    for e in engs:
        e.import_state(hb, ts, alive, 0)
    for e in engs:
        rep, ver, st = e.put(np.arange(PUT, dtype=np.int32))
        assert (st == g.GH_OK).all()
    for e in engs:
        e.delete_files(np.arange(0, PUT, 9, dtype=np.int32))
        e.apply_events([(sc.CRASH, c) for c in CRASHED])
    stats = [[e.step(1) for _ in range(ROUNDS)] for e in engs]
    assert all(s == stats[0] for s in stats)
    return engs


@pytest.mark.parametrize("R", [1, 4, 8])
def test_small_exact(gs, R):
    """One engine, a slot count that is no multiple of the workgroup: alive
    mode, a live observer (the crashed members gone from its list) and a
    stopped one (its frozen row still lists everybody)."""
    eng, = churned(lambda cfg: [gs.Engine(gs.default_config(N, **cfg))], R)
    try:
        live, stopped = LIVE, CRASHED[0]
        assert len(eng.lsm(live)[0]) == N - len(CRASHED) < len(eng.lsm(stopped)[0]) == N
        a = check_audit(eng, ALIVE)
        assert a.files == PUT - len(range(0, PUT, 9)) and a.load[63] == 0 and a.load.sum() == a.files * R
        assert a.working_hist[:R].sum() > 0 and a.sole.sum() == a.working_hist[1]
        b = check_audit(eng, live)
        np.testing.assert_array_equal(a.working_hist, b.working_hist)  # detection is complete
        c = check_audit(eng, stopped)
        assert c.working_hist[R] == c.files and c.starved == 0 and c.sole.sum() == (c.files if R == 1 else 0)
        loaded = int(np.argmax(a.load))
        for obs in (ALIVE, live, stopped):
            for member in (-1, loaded, 63):
                for mw in sorted({0, 1, R - 1, 8}):
                    want = check_select(eng, obs, member, mw)
                    if member == 63:
                        assert len(want) == 0
        # cap: none written, fewer than the total, more than it
        total = len(check_select(eng, ALIVE, -1, 8, caps=(0, 7, PUT + 5, F)))
        assert total == a.files and len(check_select(eng, ALIVE, loaded, 8, caps=(0, 3, F))) == a.load[loaded]
    finally:
        eng.close()


def lockstep(gs, om, cfg, hb, ts, alive):
    eng = gs.Engine(gs.default_config(N, **cfg))
    orc = om.Oracle(om.default_config(N, **cfg))
    for e in (eng, orc):
        e.import_state(hb, ts, alive, 0)
    f = np.arange(PUT, dtype=np.int32)
    for x, y in zip(eng.put(f), orc.put(f)):
        np.testing.assert_array_equal(x, y)
    return eng, orc


def predicts_repair(gs, eng, orc, o, R):
    """The three identities before repair(o), read-only; returns the plan."""
    before = eng.export_files()
    a = check_audit(eng, o)
    sel = check_select(eng, o, -1, R - 1)
    for x, y in zip(before, eng.export_files()):  # table and draws untouched
        np.testing.assert_array_equal(x, y)
    plan, want = eng.repair(o), orc.repair(o)
    assert plan == want
    return a, sel, plan


def test_predicts_repair(gs, oracle_mod):
    """The audit of observer o says what repair(o) is about to do, engine and
    oracle in lockstep; after repairing from the master's own list what is
    still under-replicated is what starved (here nothing)."""
    R = 4
    cfg = dict(max_files=F, replicas=R, seed=0x5EED0F10, **STABLE)
    eng, orc = lockstep(gs, oracle_mod, cfg, *sc.full_state(N))
    try:
        ev = [(sc.CRASH, c) for c in CRASHED]
        eng.apply_events(ev)
        orc.apply_events(ev)
        for r in range(ROUNDS):
            assert eng.step(1) == orc.step(1), r
        a, sel, plan = predicts_repair(gs, eng, orc, 0, R)
        assert a.working_hist[:R].sum() == len(plan) > 0
        assert a.starved == sum(1 for e in plan if e[3] != gs.GH_OK) == 0
        assert sel.tolist() == [e[0] for e in plan]
        after = check_audit(eng, 0)
        assert after.working_hist[:R].sum() == 0 and after.files == a.files
    finally:
        eng.close()
        orc.close()


def test_predicts_starved_repair(gs, oracle_mod):
    """The master's list cut to 4 members with R = 4: three can be drawn
    (Intn(M - 1)), so a file starves unless its working copies leave enough of
    the three -- a copy on the last candidate takes nothing from them."""
    R = 4
    cfg = dict(max_files=F, replicas=R, seed=0x5EED0F11, **STABLE)
    hb, ts, alive = sc.full_state(N)
    eng, orc = lockstep(gs, oracle_mod, cfg, hb, ts, alive)
    try:
        hb[0, 4:] = -1
        ts[0, 4:] = 0
        for e in (eng, orc):
            e.import_state(hb, ts, alive, 0)
        assert list(eng.lsm(0)[0]) == [0, 1, 2, 3]
        a, sel, plan = predicts_repair(gs, eng, orc, 0, R)
        bad = [e[0] for e in plan if e[3] != gs.GH_OK]
        assert a.working_hist[:R].sum() == len(plan) and sel.tolist() == [e[0] for e in plan]
        assert a.starved == len(bad) and 0 < len(bad) < len(plan)
        # (a sole copy on member 3, the last candidate, was repaired; one on 0 starved)
        rep, _ = table(eng)
        assert all((rep[e[0]] >= 0).sum() == R for e in plan if e[3] == gs.GH_OK and e[1] == 3)
        after = check_audit(eng, 0)
        assert after.working_hist[:R].sum() == len(bad) == after.starved
        np.testing.assert_array_equal(check_select(eng, 0, -1, R - 1), bad)
    finally:
        eng.close()
        orc.close()


def test_quirk_plan_one_entry_audit_counts_all(gs, oracle_mod):
    """GH_DETECT_QUIRK: the plan keeps one entry (SPEC D5), the audit counts
    every file the repair rewrites."""
    R = 4
    cfg = dict(max_files=F, replicas=R, seed=0x5EED0F12, detect_mode=gs.GH_DETECT_QUIRK, **STABLE)
    eng, orc = lockstep(gs, oracle_mod, cfg, *sc.full_state(N))
    try:
        ev = [(sc.CRASH, c) for c in CRASHED]
        eng.apply_events(ev)
        orc.apply_events(ev)
        for r in range(ROUNDS):
            assert eng.step(1) == orc.step(1), r
        a, sel, plan = predicts_repair(gs, eng, orc, 0, R)
        assert len(plan) == 1 and a.working_hist[:R].sum() == len(sel) > 1 and plan[0][0] == sel[-1]
        after = check_audit(eng, 0)
        assert after.working_hist[:R].sum() == a.starved == 0
    finally:
        eng.close()
        orc.close()


def small_cluster(gs, n, files, crash, **kw):
    eng = gs.Engine(gs.default_config(n, max_files=files, seed=0x5EED0F20 + n, fanout=4, **kw))
    eng.init_full(2, 0, 0)
    step = 1 << 18
    for lo in range(0, files, step):
        _, _, st = eng.put(np.arange(lo, min(files, lo + step), dtype=np.int32))
        assert (st == gs.GH_OK).all()
    eng.apply_events([(sc.CRASH, c) for c in crash])
    eng.step(1)
    return eng


@pytest.mark.parametrize("n,files,lds", [(8, 1 << 16, True), (512, 3000, True), (513, 3000, False),
                                         (20000, 5000, False)],
                         ids=["n8-lds", "n512-lds", "n513-global", "n20000-global"])
def test_contention_paths(gs, n, files, lds):
    """Few members under many files (every load / sole atomic on a handful of
    addresses: the workgroups' LDS bins), and member counts past the LDS
    threshold (global atomics), one member crashed so that sole is not 0."""
    assert (n <= 512) == lds  # GH_FA_LDS_N's default
    eng = small_cluster(gs, n, files, [n - 3])
    try:
        a = check_audit(eng, ALIVE, f"N={n}")
        assert a.files == files and a.load.sum() == files * eng.R
        assert a.working_hist[eng.R - 1] == a.load[n - 3] > 0
        check_audit(eng, 0, f"N={n}")
        check_select(eng, ALIVE, n - 3, eng.R - 1, caps=(None, 5))
    finally:
        eng.close()


def test_lds_threshold_knob(gs, monkeypatch):
    """GH_FA_LDS_N=0 sends N = 8 down the global-atomics path: same answer."""
    out = []
    for v in (None, "0"):
        if v is not None:
            monkeypatch.setenv("GH_FA_LDS_N", v)
        eng = small_cluster(gs, 8, 1 << 12, [5])
        try:
            out.append(check_audit(eng, ALIVE))
        finally:
            eng.close()
    assert_audit_equal(out[0], out[1], "LDS bins vs global atomics")


@pytest.mark.parametrize("ordered", ["1", "0"], ids=["two-pass", "host-sort"])
def test_select_many_slots(gs, monkeypatch, ordered):
    """300,001 slots: the ordered selection's workgroups own two chunks of
    256 slots each and the last range is cut short; GH_FS_ORDERED=0 is the
    unordered compaction with the host's sort. Same ascending ids."""
    monkeypatch.setenv("GH_FS_ORDERED", ordered)
    eng = small_cluster(gs, 8, 300001, [5])
    try:
        under = check_select(eng, ALIVE, -1, eng.R - 1, caps=(None, 1000))
        assert len(under) == len(check_select(eng, ALIVE, 5, 8)) > 100000
        assert len(check_select(eng, 0, 2, 0)) == 0 and len(check_select(eng, ALIVE, -1, 8, caps=(0,))) == 300001
    finally:
        eng.close()


def test_list_order_last_candidate(gs):
    """GH_ORDER_APPEND: member 3 leaves and rejoins, so it ends the master's
    list; after three more members leave the list is [0, 4, 5, 3] and the
    three members placement can draw are 0, 4, 5 -- not the three lowest ids.
    `starved` follows the list order, and repair refuses exactly those files."""
    n, R, files = 7, 4, 200
    eng = gs.Engine(gs.default_config(n, max_files=files, replicas=R, seed=0x5EED0F30, fanout=3,
                                      list_order=gs.GH_ORDER_APPEND))
    try:
        eng.import_state(*sc.full_state(n), 0)
        _, _, st = eng.put(np.arange(150, dtype=np.int32))
        assert (st == gs.GH_OK).all()
        eng.apply_events([(sc.LEAVE, 3)])
        eng.step(9)
        eng.apply_events([(sc.JOIN, 3)])
        eng.step(2)
        assert list(eng.lsm(0)[0]) == [0, 1, 2, 4, 5, 6, 3]
        eng.apply_events([(sc.LEAVE, c) for c in (1, 2, 6)])
        eng.step(2)
        cand = list(eng.lsm(0)[0])
        assert cand == [0, 4, 5, 3]
        a = check_audit(eng, 0)
        rep, ver = table(eng)
        by_id = file_audit_ref(rep, ver, avail_of(eng, 0), n, sorted(cand))
        assert 0 < a.starved != by_id.starved  # the order matters here
        check_audit(eng, ALIVE)
        plan = eng.repair(0)
        assert a.starved == sum(1 for e in plan if e[3] != gs.GH_OK) and len(plan) == a.working_hist[:R].sum()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def single_audits(gs):
    """One engine on the shard tests' run: its answers, checked on the way."""
    eng, = churned(lambda cfg: [gs.Engine(gs.default_config(N, **cfg))], 4)
    try:
        return shard_answers(eng)
    finally:
        eng.close()


def shard_answers(eng):
    out = [check_audit(eng, o) for o in (ALIVE, LIVE, CRASHED[0])]
    sel = [check_select(eng, o, m, mw, caps=(None, 4)) for o, m, mw in
           ((ALIVE, -1, 8), (ALIVE, -1, 0), (LIVE, -1, 3), (ALIVE, 7, 1), (CRASHED[0], 7, 8))]
    return out, sel


@pytest.mark.parametrize("world,layout", [(2, 0), (3, 0), (2, 1), (3, 1)], ids=["cols2", "cols3", "rows2", "rows3"])
def test_sharded(gs, single_audits, world, layout):
    """The file table sharded by id over 2 and 3 ranks (1,000 slots and 623
    files, which 3 does not divide; slot counts 500 and 334), on column and
    row shards: every rank returns the same audit and selection (ShardGroup
    checks that), they are one engine's, and the reference's."""
    def make(cfg):
        return [gs.ShardGroup(gs.default_config(N, shard_layout=layout, **cfg), world)]
    grp, = churned(make, 4)
    try:
        out, sel = shard_answers(grp)
    finally:
        grp.close()
    for x, y in zip(out, single_audits[0]):
        assert_audit_equal(x, y, f"{world} shards vs one engine")
    for x, y in zip(sel, single_audits[1]):
        np.testing.assert_array_equal(x, y)


def test_refusals(gs):
    """Bad arguments are refused with GH_EINVAL before anything runs, and the
    engine goes on."""
    def refused(fn, *a):
        with pytest.raises(gs.GossipError) as ei:
            fn(*a)
        assert ei.value.code == gs._abi.GH_EINVAL

    n = 64
    eng = gs.Engine(gs.default_config(n, max_files=0))
    try:
        eng.import_state(*sc.full_state(n), 0)
        refused(eng.file_audit)
        refused(eng.file_select)
        assert eng.step(1)["rounds"] == 1
    finally:
        eng.close()
    eng = gs.Engine(gs.default_config(n, max_files=100))
    try:
        eng.import_state(*sc.full_state(n), 0)
        eng.put(np.arange(50, dtype=np.int32))
        refused(eng.file_audit, n)
        refused(eng.file_audit, -2)
        refused(eng.file_select, n)
        refused(eng.file_select, -2)
        refused(eng.file_select, ALIVE, n)
        refused(eng.file_select, ALIVE, -1, 9)
        refused(eng.file_select, ALIVE, -1, -1)
        assert eng.step(1)["rounds"] == 1
        assert check_audit(eng, ALIVE).files == 50
    finally:
        eng.close()


def test_cluster_store_and_audit(gs):
    """Cluster.store(m) through file_select is what the whole-table read gave,
    after puts, a crash and the tick-driven repair; Cluster.audit() is the
    engine's audit."""
    n, files = 16, 64
    cl = gs.Cluster(n, max_files=files, t_fail=5, t_cleanup=5, seed=0x5EED0F40)
    try:
        for i in range(n):
            cl.join(i)
            cl.tick(1)
        cl.tick(4)
        assert all(p.status == gs.GH_OK for p in cl.put(range(40)))
        cl.delete([3, 4])
        cl.crash(9)
        cl.tick(20)
        assert cl.plans  # a repair pass ran
        f = np.arange(files, dtype=np.int32)
        rep, ver = cl.engine.get_files(f)
        loads = []
        for m in range(n):
            want = f[(ver >= 0) & (rep == m).any(axis=1)].tolist()
            got = cl.store(m)
            assert got == want and all(type(x) is int for x in got), m
            loads.append(len(got))
        a = cl.audit()
        assert_audit_equal(a, check_audit(cl.engine, ALIVE), "Cluster.audit")
        assert a.load.tolist() == loads and a.files == 38
        assert_audit_equal(cl.audit(0), check_audit(cl.engine, 0), "Cluster.audit(0)")
    finally:
        cl.engine.close()
