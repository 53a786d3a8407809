"""CPU checks of the partition models (tests/partition_ref.py) and of the three
gh_*partition* entry points that need no device.

With one side both models are their originals (tablesim / ListSim), round for
round, stats included; the dense model and the list model agree on a shared
two-side pull scenario; and every scenario the GPU tests run
(test_gpu_partition.py) is non-vacuous in the model alone: messages are cut,
running members are detected, the REMOVE sets include one with no detector on
one side and some on another, one with a single detector on a side that has
other running rows, in ring mode and append order too (T_cleanup <= T_fail everywhere, so a REMOVE wrongly
delivered to that detector would count in remove_unknown) and one with two or
more, and the final tables differ from the unpartitioned run and from the run
that cuts the gossip only (SPEC D9)."""
import ctypes as C

import numpy as np
import pytest

import partition_ref as pr
import scenarios as sc
import test_gpu_partition as tg


# ---- one side ---------------------------------------------------------------
@pytest.mark.parametrize("armed", [False, True], ids=["never", "side0"])
def test_one_side_equals_tablesim(oracle_mod, armed):
    om = oracle_mod
    n, k, t, seed, rounds = 263, 4, 16, 0x5EED2100, 30
    sched = {8: [(sc.CRASH, int(c)) for c in sc.crash_ids(n, 0.01, seed)]}
    orc = om.Oracle(om.default_config(n, fanout=k, t_fail=t, t_cleanup=t, seed=seed))
    mod = pr.PartitionModel(n, k, t, t, seed)
    for e in (orc, mod):
        e.import_state(*sc.full_state(n), 0)
    if armed:
        mod.set_partition(np.full(n, 7))
    for r in range(1, rounds + 1):
        for e in (orc, mod):
            if sched.get(r):
                e.apply_events(sched[r])
        so, sm = orc.step(1), mod.step(1)
        assert so == sm, r
        for x, y in zip(orc.export_state(), mod.export_state()):
            np.testing.assert_array_equal(x, y, err_msg=f"round {r}")
        np.testing.assert_array_equal(orc.read_failed(), mod.read_failed())
        np.testing.assert_array_equal(orc.read_detectors(), mod.read_detectors())
    assert mod.cut == 0 and mod.sets  # (the crashed members were detected)
    orc.close()


@pytest.mark.parametrize("order", ["id", "append"])
@pytest.mark.parametrize("mode,quirk", [("ring", False), ("pull", True)])
def test_one_side_equals_listsim(order, mode, quirk):
    """A join / leave / crash scenario: PartitionListSim on one side is ListSim."""
    from oracle.listsim import ListSim
    n = 24
    kw = dict(seed=0x5EED2124, peer_mode=mode, order=order, quirk=quirk)
    a = ListSim.from_dense(*sc.full_state(n), 0, **kw)
    b = pr.PartitionListSim.from_dense(*sc.full_state(n), 0, **kw)
    b.set_partition(np.full(n, 3))
    sched = {3: [(sc.CRASH, 5), (sc.CRASH, 6)], 14: [(sc.JOIN, 5)], 16: [(sc.LEAVE, 11)], 20: [(sc.JOIN, 6)]}
    for r in range(1, 31):
        for e in (a, b):
            if sched.get(r):
                e.apply_events(sched[r])
        assert a.step(1) == b.step(1), r
        for x, y in zip(a.dense(), b.dense()):
            np.testing.assert_array_equal(x, y, err_msg=f"round {r}")
        assert [[m.addr for m in nd.members] for nd in a.nodes] == [[m.addr for m in nd.members] for nd in b.nodes]
        assert a.last_failed == b.last_failed and a.last_detectors == b.last_detectors
    assert b.cut == 0


# ---- the two models agree ------------------------------------------------------
def test_dense_model_equals_list_model():
    """A two-side pull scenario with crashes at ListSim's T = 5 on both models."""
    from oracle import listsim as L
    n, seed, rounds = 40, 0x5EED2140, 22
    side = pr.sides_of(n, [17], 11)
    sched = {5: [(sc.CRASH, 9), (sc.CRASH, 30)]}
    dm = pr.PartitionModel(n, 3, L.T_FAIL, L.T_CLEANUP, seed)
    dm.import_state(*sc.full_state(n), 0)
    ls = pr.PartitionListSim.from_dense(*sc.full_state(n), 0, seed=seed, peer_mode="pull", fanout=3)
    for r in range(1, rounds + 1):
        for e in (dm, ls):
            if r == 2:
                e.set_partition(side)
            if sched.get(r):
                e.apply_events(sched[r])
        s1, s2 = dm.step(1), ls.step(1)
        assert s1 == s2, r
        hb, ts, alive = ls.dense()
        np.testing.assert_array_equal(dm.export_state()[0], hb, err_msg=f"hb r={r}")
        np.testing.assert_array_equal(dm.export_state()[1], sc.export_view(hb, ts, r, L.T_CLEANUP)[1], err_msg=f"ts r={r}")
        assert dm.failed().tolist() == ls.last_failed and dm.read_detectors().tolist() == sorted(ls.last_detectors)
        assert r < 2 or dm.partition_stats() == ls.partition_stats()
    assert dm.cut > 0 and dm.sets


# ---- the GPU tests' scenarios are non-vacuous in the models -------------------------
def set_kinds(sets):
    """How many REMOVE sets have (no detector on a side while another has
    some, a single detector on a side with other running rows, two or more
    detectors on a side)."""
    none = sum(1 for _, _, cnt, _ in sets if min(cnt.values()) == 0 and max(cnt.values()) > 0)
    one = sum(1 for _, _, cnt, run in sets if any(cnt[s] == 1 and run[s] > 1 for s in cnt))
    many = sum(1 for _, _, cnt, _ in sets if any(v >= 2 for v in cnt.values()))
    return none, one, many


@pytest.mark.parametrize("name", list(tg.CASES))
def test_pull_scenarios_non_vacuous(name):
    case = tg.CASES[name]
    assert case["cfg"]["t_cleanup"] <= case["cfg"]["t_fail"]
    fp = []
    m = pr.run_model(case, per_round=lambda m, st: fp.append(int(m.alive[m.failed()].sum())))
    clean = pr.run_model(case, partitioned=False)
    d9 = pr.run_model(case, gate_control=False)
    assert m.cut > 0 and sum(fp) > 0
    none, one, many = set_kinds(m.sets)
    assert none > 0 and one > 0 and many > 0, (none, one, many)
    assert not np.array_equal(m.hb, clean.hb)
    assert not np.array_equal(m.hb, d9.hb)


def test_pending_set_keeps_its_recipients():
    """pend16: a REMOVE set is pending when the sides change, and delivering it
    by the new sides instead (which SPEC step 6b rules out) gives another
    round and other final tables."""
    case = tg.CASES["pend16"]
    at = case["resplit"][0]
    failed, tomb, late = [], [], []
    m = pr.run_model(case, per_round=lambda m, st: (failed.append(m.failed().size), tomb.append(st["tombstoned"])))
    w = pr.run_model(case, late_recipients=True, per_round=lambda m, st: late.append(st["tombstoned"]))
    assert failed[at - 2] > 0 and not any(failed[:at - 2])  # round at - 1 made the first detections
    assert tomb[:at - 1] == late[:at - 1] and tomb[at - 1] != late[at - 1]
    assert not np.array_equal(m.hb, w.hb)
    assert not np.array_equal(case["side"], case["resplit"][1])


def test_minority_majority_stays_whole():
    """N=263, 6 members on side 1: every running majority row still lists every
    running majority member at the end; with the gossip cut alone (REMOVE to
    every row, SPEC D9) it does not. Unpartitioned, nobody is detected."""
    case = tg.CASES["minor16"]
    assert int((case["side"] == 1).sum()) == 6 and case["n"] == 263
    m = pr.run_model(case)
    d9 = pr.run_model(case, gate_control=False)
    det = []
    pr.run_model(case, partitioned=False, per_round=lambda m, st: det.append(st["detections"]))
    assert sum(det) == 0
    maj = m.alive.astype(bool) & (case["side"] == 0)
    assert maj.sum() == 257
    assert (m.hb[np.ix_(maj, maj)] >= 0).all()
    assert not (d9.hb[np.ix_(maj, maj)] >= 0).all()


@pytest.mark.parametrize("order", ["id", "append"])
@pytest.mark.parametrize("name", list(tg.LIST_CASES) + ["heal"])
def test_list_scenarios_non_vacuous(name, order):
    case = tg.HEAL if name == "heal" else tg.LIST_CASES[name]
    fp, cuts = [], []

    def watch(m, st):
        fp.append(sum(m.nodes[c].alive for c in m.last_failed))
        cuts.append(m.cut)

    m = tg.run_list_model(case, order, per_round=watch)
    clean = tg.run_list_model(case, order, partitioned=False)
    assert max(cuts) > 0 and sum(fp) > 0
    none, one, many = set_kinds([s for s in m.sets if len(s[2]) > 1])
    assert none > 0 and many > 0, (none, one, many)
    assert one > 0, (none, one, many)
    assert not np.array_equal(m.dense()[0], clean.dense()[0])
    side = case["side"]
    kinds = {(kind, int(side[c])) for ev in case["sched"].values() for kind, c in ev}
    if name == "heal":
        # the JOINs of round 26 come from the far side after the heal: the
        # introducer hears them and lists the three
        at26 = tg.run_list_model(dict(case, rounds=26), order)
        assert at26.nodes[0].alive and all(at26.dense()[0][0, c] >= 0 for _, c in case["sched"][26])
        assert all(side[c] == 1 for _, c in case["sched"][26])
    else:
        assert {(sc.LEAVE, 0), (sc.LEAVE, 1), (sc.JOIN, 0), (sc.JOIN, 1)} <= kinds and any(k == sc.CRASH for k, _ in kinds)


# ---- the three entry points without a device --------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gossipsim import _abi
    return _abi.load(), _abi


def test_partition_symbols_exported(lib):
    L, abi = lib
    raw = C.CDLL(str(abi.LIB_PATH))
    bound = {n for n, _, _ in abi.SYMBOLS}
    for name in ("gh_set_partition", "gh_get_partition", "gh_partition_stats"):
        assert hasattr(raw, name) and name in bound
    assert abi.GH_PART_SIDES == pr.SIDES == 64


def test_partition_null_handle(lib):
    L, abi = lib
    a = (C.c_int32 * 8)()
    armed, cut = C.c_int32(7), C.c_int64(7)
    assert L.gh_set_partition(None, a) == abi.GH_EINVAL
    assert L.gh_set_partition(None, None) == abi.GH_EINVAL
    assert L.gh_get_partition(None, C.byref(armed), a) == abi.GH_EINVAL
    assert L.gh_partition_stats(None, C.byref(cut)) == abi.GH_EINVAL
    assert (armed.value, cut.value) == (7, 7)


def test_cluster_refuses_partition_with_elections():
    """Cluster.set_partition / partition_stats raise ValueError with elect=True
    before any engine call (the election's RPCs across a split are not
    modelled)."""
    from gossipsim import Cluster
    c = Cluster.__new__(Cluster)
    c.elect = True
    with pytest.raises(ValueError):
        c.set_partition(np.zeros(8, np.int32))
    with pytest.raises(ValueError):
        c.partition_stats()
