"""Network partitions (gh_set_partition, SPEC §2 step 6b) on the GPU against
the CPU models of tests/partition_ref.py, bit for bit after every round: hb,
ts, alive, the round's stats, read_failed, read_detectors, partition_stats
and, in append order, every row's list.

Pull mode with crashes runs against the dense numpy model (PartitionModel),
everything with JOIN / LEAVE, ring mode, quirk detection or list order against
the ListSim-based one (PartitionListSim); an armed engine whose members are
all on one side runs against the existing oracles. The scenarios (CASES,
LIST_CASES, HEAL) are checked for non-vacuity on the CPU by
test_partition_ref.py; every pinned literal comes from the models.

The 16-bit two-side case keeps the reference's T = 5: from a full start that
cluster has its round-6 detection storm with or without a split, so the
minority case, which asserts that the majority stays whole, runs with T = 8,
under which the unpartitioned cluster detects nobody.
Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import loss_ref as lr
import partition_ref as pr
import scenarios as sc

pytestmark = pytest.mark.gpu

ROWS = 1  # GH_LAYOUT_ROWS
EINVAL = -1


def _crash(n, seed, at=8):
    return {at: [(sc.CRASH, int(c)) for c in sc.crash_ids(n, 0.01, seed)]}


# Pull-mode scenarios from a full start (PartitionModel); sizes = the members
# of sides 1, 2, ...; the rest, with the introducer, is side 0.
CASES = {
    "two16": pr.pull_case(263, 3, 5, [220], 24, 0x5EED2263),
    "minor16": pr.pull_case(263, 3, 8, [6], 30, 0x5EED2264),
    "nib263_2": pr.pull_case(263, 4, 16, [100], 44, 0x5EED2265, crash=_crash(263, 0x5EED2265)),
    "nib263_3": pr.pull_case(263, 4, 16, [90, 40], 44, 0x5EED2266, crash=_crash(263, 0x5EED2266)),
    "nib1000_2": pr.pull_case(1000, 4, 16, [300], 44, 0x5EED2267, crash=_crash(1000, 0x5EED2267)),
    "nib1000_3": pr.pull_case(1000, 4, 16, [350, 150], 44, 0x5EED2268, crash=_crash(1000, 0x5EED2268)),
    "loss16": pr.pull_case(263, 3, 8, [100], 30, 0x5EED2269, loss=0.1),
    # the sides change again before round 10, while the REMOVE set of round 9
    # (the model's first detections) is pending: its recipients stay those of
    # the sides of round 9
    "pend16": dict(pr.pull_case(263, 3, 8, [100], 24, 0x5EED226A), resplit=(10, pr.sides_of(263, [130], 77))),
}


def _list_case(n, seed, far, rounds, sched, split=2, **kw):
    side = np.zeros(n, np.int32)
    side[list(far)] = 1
    return dict(n=n, seed=seed, side=side, split=split, rounds=rounds, sched=sched, kw=kw)


# PartitionListSim scenarios (T_fail = T_cleanup = 5, ListSim's constants; the
# introducer, member 0, is on side 0): a crash, a leave on each side, a join on
# the introducer's side and one on the far side (its process restarts, nobody
# hears its JOIN). The far side of a ring case is a block of neighbours, so
# that some member is detected by exactly one row of a side.
LIST_CASES = {
    "ring24": _list_case(24, 0x5EED2424, list(range(14, 24)), 30,
                         {3: [(sc.CRASH, 3), (sc.CRASH, 15)], 6: [(sc.LEAVE, 9)], 7: [(sc.LEAVE, 17)],
                          12: [(sc.JOIN, 3)], 14: [(sc.JOIN, 15)]}, peer_mode="ring"),
    "ring48": _list_case(48, 0x5EED2448, list(range(40, 48)), 26,
                         {3: [(sc.CRASH, 6), (sc.CRASH, 42)], 5: [(sc.LEAVE, 21), (sc.LEAVE, 44)],
                          11: [(sc.JOIN, 6), (sc.JOIN, 42)]}, peer_mode="ring"),
    "quirk96": _list_case(96, 0x5EED2496, list(range(40, 96)), 22,
                          {4: [(sc.CRASH, 7), (sc.CRASH, 50)], 9: [(sc.LEAVE, 12), (sc.LEAVE, 60)],
                           13: [(sc.JOIN, 7), (sc.JOIN, 50)]}, peer_mode="pull", fanout=3, quirk=True),
}

# Split at round 3, heal at round 20, far-side members rejoin at round 26.
HEAL = _list_case(48, 0x5EED2C48, list(range(30, 48)), 35,
                  {8: [(sc.CRASH, 5)], 26: [(sc.JOIN, 31), (sc.JOIN, 40), (sc.JOIN, 47)]},
                  split=3, peer_mode="pull", fanout=6)
HEAL["heal"] = 20


def calls(case):
    """The scenario as gh_step calls of at most 5 rounds, a new call wherever
    the sides change or events are queued: [(first round, rounds)]."""
    cuts = sorted({1, case["split"], case["heal"], case["rounds"] + 1, *case["sched"]})
    out = []
    for lo, hi in zip(cuts, cuts[1:]):
        out += [(f, min(5, hi - f)) for f in range(lo, hi, 5)]
    return out


def list_model(case, order="id"):
    return pr.PartitionListSim.from_dense(*sc.full_state(case["n"]), 0, seed=case["seed"], order=order, **case["kw"])


def run_list_model(case, order="id", partitioned=True, per_round=None):
    m = list_model(case, order)
    for r in range(1, case["rounds"] + 1):
        if partitioned and r == case["split"]:
            m.set_partition(case["side"])
        if partitioned and r == case.get("heal"):
            m.set_partition(None)
        if case["sched"].get(r):
            m.apply_events(case["sched"][r])
        st = m.step(1)
        if per_round:
            per_round(m, st)
    return m


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    monkeypatch.delenv("GH_PLANE", raising=False)
    monkeypatch.delenv("GH_C8", raising=False)


def bits(bm, n):
    return [c for c in range(n) if (int(bm[c >> 5]) >> (c & 31)) & 1]


def compare(eng, model, r, what=""):
    """An engine against the pull model after round r."""
    for name, x, y in zip(("hb", "ts", "alive"), eng.export_state(), model.export_state()):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name} after round {r}")
    np.testing.assert_array_equal(eng.read_failed(), model.read_failed(), err_msg=f"{what} failed set, round {r}")
    np.testing.assert_array_equal(np.sort(eng.read_detectors()), model.read_detectors(),
                                  err_msg=f"{what} detectors, round {r}")
    if model.armed:
        assert eng.partition_stats() == model.partition_stats(), f"{what} partition_stats after round {r}"
    if model.out is not None:
        assert eng.loss_stats() == model.loss_stats(), f"{what} loss_stats after round {r}"


def start(gs, case, **cfg_kw):
    eng = gs.Engine(gs.default_config(case["n"], **case["cfg"], **cfg_kw))
    eng.import_state(*sc.full_state(case["n"]), 0)
    if case.get("loss") is not None:
        eng.set_loss(case["loss"], case["loss"])
    return eng


def lockstep(eng, model, case, per_round=None):
    """The engine and the pull model one round at a time, compared after each."""
    for r in range(1, case["rounds"] + 1):
        if r == case["split"]:
            eng.set_partition(case["side"])
            model.set_partition(case["side"])
        if case.get("resplit") and r == case["resplit"][0]:
            assert model.failed().size > 0, "a REMOVE set is pending when the sides change"
            eng.set_partition(case["resplit"][1])
            model.set_partition(case["resplit"][1])
        ev = case["sched"].get(r)
        if ev:
            eng.apply_events(ev)
            model.apply_events(ev)
        want, got = model.step(1), eng.step(1)
        assert got == want, f"round {r}: gpu {got} != model {want}"
        compare(eng, model, r)
        if per_round:
            per_round(r, want)


# ---- 16-bit path ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["two16", "minor16", "pend16"])
def test_16bit_path(gs, name):
    """N=263, k=3 on the 16-bit path: two sides of 43 and 220 members at
    T = 5; a minority of 6 at T = 8 whose majority stays whole; and sides that
    change in the round right after a detection, whose pending REMOVE set keeps
    the recipients of the sides it was detected under (lockstep asserts that
    one is pending)."""
    case = CASES[name]
    eng, model = start(gs, case), pr.model_of(case)
    try:
        assert eng.tier_info()[0] == 0 and eng.partition()[0] is False
        lockstep(eng, model, case)
        assert model.cut > 0
        armed, side = eng.partition()
        assert armed
        np.testing.assert_array_equal(side, case["resplit"][1] if case.get("resplit") else case["side"])
    finally:
        eng.close()


# ---- nibble path ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nib263_2", "nib263_3", "nib1000_2", "nib1000_3"])
def test_nibble_path(gs, monkeypatch, name):
    """GH_PLANE=1, k=4, T=16, 44 rounds in the 4-bit tier: two and three uneven
    sides from round 3 and the 1% crash at round 8. The table is in the tier
    and the nibble path (variant 3) ran."""
    monkeypatch.setenv("GH_PLANE", "1")
    case = CASES[name]
    eng, model = start(gs, case), pr.model_of(case)
    tier, variants = [], []

    def per_round(r, st):
        tier.append(eng.tier_info()[1])
        variants.append(eng.tier_info(full=True)[3])

    try:
        assert eng.tier_info()[0] == 1
        lockstep(eng, model, case, per_round=per_round)
        print(f"{name}: tier per round {tier}, variants {variants}")
        assert 1 in tier, tier
        assert 3 in variants, variants
    finally:
        eng.close()


# ---- one side, against the existing oracles -----------------------------------------
@pytest.mark.parametrize("mode", ["pull", "quirk", "ring"])
def test_one_side_equals_oracle(gs, oracle_mod, mode):
    """An armed engine with every member on side 0 against tablesim, under
    churn: pull canonical, pull quirk and ring. The engine is armed in the round
    right after the first detection, while that REMOVE set is pending (its
    recipients are filled by rule D4 on arming)."""
    n, rounds = 263, 30
    kw = dict(fanout=3, seed=0x5EED2A00 + len(mode), t_fail=3, t_cleanup=5,
              peer_mode=1 if mode == "ring" else 0, detect_mode=1 if mode == "quirk" else 0)
    sched = sc.random_churn(n, rounds, 0x2A + len(mode), p_crash=0.05, p_leave=0.02, p_join=0.05)
    eng = gs.Engine(gs.default_config(n, **kw))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **kw))
    armed_at = None
    try:
        for e in (eng, orc):
            e.import_state(*sc.full_state(n), 0)
        for r in range(1, rounds + 1):
            for e in (eng, orc):
                if sched.get(r):
                    e.apply_events(sched[r])
            s1, s2 = eng.step(1), orc.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != cpu {s2}"
            for name, x, y in zip(("hb", "ts", "alive"), eng.export_state(), orc.export_state()):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} after round {r}")
            np.testing.assert_array_equal(eng.read_failed(), orc.read_failed(), err_msg=f"failed, round {r}")
            np.testing.assert_array_equal(eng.read_detectors(), orc.read_detectors(), err_msg=f"detectors, round {r}")
            if armed_at is None and eng.read_failed().any():
                eng.set_partition(np.zeros(n, np.int32))
                armed_at = r
            if armed_at is not None:
                assert eng.partition_stats() == 0
        assert armed_at is not None and armed_at < rounds - 10, armed_at
    finally:
        eng.close()
        orc.close()


def list_compare(eng, ls, n, r, lists):
    from oracle import listsim as L
    h1, t1, a1 = eng.export_state()
    h2, t2, a2 = ls.dense()
    np.testing.assert_array_equal(a1, a2, err_msg=f"alive r={r}")
    np.testing.assert_array_equal(h1, h2, err_msg=f"hb r={r}")
    np.testing.assert_array_equal(t1, sc.export_view(h2, t2, r, L.T_CLEANUP)[1], err_msg=f"ts r={r}")
    assert bits(eng.read_failed(), n) == ls.last_failed, r
    assert sorted(eng.read_detectors()) == sorted(ls.last_detectors), r
    if ls.armed:
        assert eng.partition_stats() == ls.partition_stats(), r
    if lists:
        assert [list(eng.lsm(i)[0]) for i in range(n)] == [[m.addr for m in nd.members] for nd in ls.nodes], r


def test_one_side_append_order(gs):
    """Append order, ring mode, one side: the armed engine against ListSim,
    the lists too, armed while a REMOVE set is pending."""
    from oracle.listsim import ListSim
    n, rounds = 48, 30
    sched = sc.random_churn(n, rounds, 0x2A48, p_crash=0.05, p_leave=0.03, p_join=0.08)
    eng = gs.Engine(gs.default_config(n, peer_mode=gs.GH_PEER_RING, seed=0x5EED2A48, list_order=gs.GH_ORDER_APPEND))
    ls = ListSim.from_dense(*sc.full_state(n), 0, seed=0x5EED2A48, peer_mode="ring", order="append")
    ls.armed = False
    armed_at = None
    try:
        eng.import_state(*sc.full_state(n), 0)
        for r in range(1, rounds + 1):
            for e in (eng, ls):
                if sched.get(r):
                    e.apply_events(sched[r])
            s1, s2 = eng.step(1), ls.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
            list_compare(eng, ls, n, r, True)
            if armed_at is None and ls.last_failed:
                eng.set_partition(None)
                armed_at = r
            if armed_at is not None:
                assert eng.partition_stats() == 0
        assert armed_at is not None and armed_at < rounds - 10, armed_at
    finally:
        eng.close()


# ---- PartitionListSim cases --------------------------------------------------------
def list_engine(gs, case, order="id"):
    kw = case["kw"]
    eng = gs.Engine(gs.default_config(
        case["n"], seed=case["seed"], fanout=kw.get("fanout", 3),
        peer_mode=gs.GH_PEER_RING if kw["peer_mode"] == "ring" else gs.GH_PEER_PULL,
        detect_mode=gs.GH_DETECT_QUIRK if kw.get("quirk") else gs.GH_DETECT_CANONICAL,
        list_order=gs.GH_ORDER_APPEND if order == "append" else gs.GH_ORDER_ID))
    eng.import_state(*sc.full_state(case["n"]), 0)
    return eng


def list_run(eng, ls, case, lists):
    for r in range(1, case["rounds"] + 1):
        if r == case["split"]:
            eng.set_partition(case["side"])
            ls.set_partition(case["side"])
        if case["sched"].get(r):
            eng.apply_events(case["sched"][r])
            ls.apply_events(case["sched"][r])
        s1, s2 = eng.step(1), ls.step(1)
        assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
        list_compare(eng, ls, case["n"], r, lists)


@pytest.mark.parametrize("order", ["id", "append"])
@pytest.mark.parametrize("name", ["ring24", "ring48"])
def test_ring(gs, name, order):
    """Ring mode in member-ID and in append order (the lists too): a crash, a
    leave on each side, a join on the introducer's side and one on the far
    side."""
    case = LIST_CASES[name]
    eng = list_engine(gs, case, order)
    try:
        list_run(eng, list_model(case, order), case, lists=order == "append")
    finally:
        eng.close()


def test_pull_quirk(gs):
    """Pull mode with quirk detection at N=96, sides of 40 and 56."""
    case = LIST_CASES["quirk96"]
    eng = list_engine(gs, case)
    try:
        list_run(eng, list_model(case), case, lists=False)
    finally:
        eng.close()


# ---- split and heal, call shapes ----------------------------------------------------------
def test_split_and_heal(gs):
    """N=48, pull, k=6: split at round 3, heal at round 20, three far-side
    members rejoin through the introducer at round 26. An engine stepped 5 rounds per call equals one
    stepped a round per call and the model; gh_set_partition zeroes `cut`;
    gh_get_partition returns the array."""
    case = HEAL
    n = case["n"]
    a, b, ls = list_engine(gs, case), list_engine(gs, case), list_model(case)
    try:
        shapes = calls(case)
        assert max(k for _, k in shapes) == 5 and sum(k for _, k in shapes) == case["rounds"]
        for first, k in shapes:
            total = None
            for r in range(first, first + k):
                change = (case["side"],) if r == case["split"] else (None,) if r == case["heal"] else ()
                for e in (a, ls) + ((b,) if r == first else ()):
                    if change:
                        e.set_partition(*change)
                if change:
                    assert r == first, "the sides change at a call boundary"
                    assert a.partition_stats() == b.partition_stats() == 0  # zeroed by every gh_set_partition
                    armed, side = b.partition()
                    assert armed
                    np.testing.assert_array_equal(side, case["side"] if r == case["split"] else np.zeros(n, np.int32))
                ev = case["sched"].get(r)
                if ev:
                    assert r == first, "queued events belong to the call's first round"
                    for e in (a, b, ls):
                        e.apply_events(ev)
                s1, s2 = a.step(1), ls.step(1)
                assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
                list_compare(a, ls, n, r, False)
                total = s2 if total is None else {f: total[f] + s2[f] for f in total}
            got = b.step(k)
            assert {f: got[f] for f in lr.SUMMED} == {f: total[f] for f in lr.SUMMED}, (first, got, total)
            list_compare(b, ls, n, first + k - 1, False)
    finally:
        a.close()
        b.close()


def test_refusals(gs):
    """A side outside [0, GH_PART_SIDES) changes nothing; a GH_REMOVE_LIST
    engine and a ShardGroup refuse; partition_stats refuses before arming. All
    GH_EINVAL."""
    n = 64
    eng = gs.Engine(gs.default_config(n))
    lst = gs.Engine(gs.default_config(n, remove_mode=1))  # GH_REMOVE_LIST
    grp = gs.ShardGroup(gs.default_config(n), 2)
    try:
        with pytest.raises(gs.GossipError) as err:
            eng.partition_stats()
        assert err.value.code == EINVAL
        good = np.arange(n, dtype=np.int32) % gs.GH_PART_SIDES
        for bad in (-1, gs.GH_PART_SIDES, 1 << 20):
            side = good.copy()
            side[n - 1] = bad
            with pytest.raises(gs.GossipError) as err:
                eng.set_partition(side)
            assert err.value.code == EINVAL
            armed, now = eng.partition()
            assert not armed and not now.any()
        eng.set_partition(good)
        side = good.copy()
        side[0] = gs.GH_PART_SIDES
        with pytest.raises(gs.GossipError):
            eng.set_partition(side)
        np.testing.assert_array_equal(eng.partition()[1], good)
        for e in (lst, grp):
            with pytest.raises(gs.GossipError) as err:
                e.set_partition(np.zeros(n, np.int32))
            assert err.value.code == EINVAL
        assert lst.partition()[0] is False
    finally:
        eng.close()
        lst.close()
        grp.close()


def test_cluster_forwards(gs):
    """Cluster.set_partition / partition_stats reach the engine: the ring24
    scenario through the Cluster facade (ring mode, append order, its
    defaults) against the model, the lists too."""
    case = LIST_CASES["ring24"]
    n = case["n"]
    c = gs.Cluster(n, seed=case["seed"])
    ls = list_model(case, "append")
    verb = {sc.CRASH: c.crash, sc.LEAVE: c.leave, sc.JOIN: c.join}
    try:
        c.engine.import_state(*sc.full_state(n), 0)
        with pytest.raises(gs.GossipError):
            c.partition_stats()  # not armed yet
        for r in range(1, case["rounds"] + 1):
            if r == case["split"]:
                c.set_partition(case["side"])
                ls.set_partition(case["side"])
                assert c.partition_stats() == 0 and c.engine.partition()[0]
            for kind, m in case["sched"].get(r, []):
                verb[kind](m)
            if case["sched"].get(r):
                ls.apply_events(case["sched"][r])
            s1, s2 = c.tick(1), ls.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
            list_compare(c.engine, ls, n, r, True)
            if ls.armed:
                assert c.partition_stats() == ls.partition_stats()
        assert ls.cut > 0
    finally:
        c.engine.close()


# ---- loss and partition together -----------------------------------------------------------
def test_loss_and_partition(gs):
    """N=263, k=3, T=8: uniform 0.1 loss on both ends of every link and two
    sides of 163 and 100: a cut
    message is neither sent nor dropped; both counters equal the model's after
    every round."""
    case = CASES["loss16"]
    eng, model = start(gs, case), pr.model_of(case)
    try:
        lockstep(eng, model, case)
        sent, dropped = model.loss_stats()
        assert model.cut > 0 and 0 < dropped < sent
    finally:
        eng.close()


# ---- the journal over a split -----------------------------------------------------------------
def test_journal_over_split(gs):
    """GH_JOURNAL_DETECT over the minority split: the false positives the
    journal counts are the model's detections of running members, per round."""
    case = CASES["minor16"]
    eng = start(gs, case)
    false_failed = []
    model = pr.run_model(case, per_round=lambda m, st: false_failed.append(int(m.alive[m.failed()].sum())))
    try:
        eng.journal_enable(gs.GH_JOURNAL_DETECT, 64)
        eng.step(case["split"] - 1)
        eng.set_partition(case["side"])
        eng.step(case["rounds"] - case["split"] + 1)
        compare(eng, model, case["rounds"])
        log, j = eng.journal_rounds(), eng.journal()
        assert log["false_failed"].tolist() == false_failed
        assert int(j.fp_rounds.sum()) == sum(false_failed) > 0
    finally:
        eng.close()
