"""CPU checks of the control-loss models (tests/control_loss_ref.py) and of
the three gh_*control_loss* entry points that need no device.

The array form of every draw equals the one-message form; with kinds = 0, loss
off or zero thresholds both models are their parents round for round; the
dense and the list model agree on a shared pull scenario; and every scenario
the GPU tests run (test_gpu_control_loss.py) is non-vacuous on the model alone:
REMOVE pairs are missed and others are not, LEAVE, JOIN and the broadcast each
lose a message and deliver one, and the final tables differ from the same
scenario with kinds = 0. The seeds of the scenarios were chosen so that these
hold; nothing here is pinned to a figure."""
import ctypes as C

import numpy as np
import pytest

import control_loss_ref as cl
import loss_ref as lr
import partition_ref as pr
import scenarios as sc
import test_gpu_control_loss as tg


# ---- the two forms of the draws ----------------------------------------------------
@pytest.mark.parametrize("tag", [cl.TAG_LEAV, cl.TAG_JOIN, cl.TAG_BCST])
def test_event_draws_agree(tag):
    n, seed, r = 97, 0x5EED3001, 13
    rng = np.random.default_rng(tag)
    out, inn = (rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    out[5], inn[6], out[7], inn[8] = lr.ALWAYS, lr.ALWAYS, 0, 0
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    got = cl.ctl_dropped_np(seed, out, inn, tag, a, r, b, a, b)
    some = 0
    for x in range(0, n, 3):
        for y in range(n):
            want = cl.ctl_dropped(seed, out, inn, tag, x, r, y, x, y)
            assert bool(got[x, y]) == want, (x, y)
            some += want
    assert 0 < some < (n // 3 + 1) * n
    assert got[5].all() and got[:, 6].all()
    # the tag is part of the counter
    assert not np.array_equal(got, cl.ctl_dropped_np(seed, out, inn, tag ^ 1, a, r, b, a, b))


def test_remove_draws_agree():
    n, seed, r = 61, 0x5EED3002, 21
    rng = np.random.default_rng(7)
    out, inn = (rng.integers(0, 2 ** 31, n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    out[9], inn[10] = lr.ALWAYS, lr.ALWAYS
    side = np.where(np.arange(n) % 3 == 0, 1, 0)
    for c, dets in ((4, [9]), (30, [1, 9, 12, 40]), (60, list(range(0, 60, 7)))):
        has, got = cl.remove_arrives_np(seed, out, inn, c, r, dets, side)
        for j in range(n):
            E = [i for i in dets if i != j and side[i] == side[j]]
            assert bool(has[j]) == bool(E), (c, j)
            assert bool(got[j]) == any(not cl.remove_dropped(seed, out, inn, c, r, i, j) for i in E), (c, j)
        assert not got[10]
    # another member, another key
    assert cl.remove_key(seed, 4, r) != cl.remove_key(seed, 5, r) != cl.remove_key(seed, 5, r + 1)


# ---- kinds = 0, loss off, zero thresholds: the parents ---------------------------------
@pytest.mark.parametrize("how", ["kinds0", "loss_off", "zero"])
def test_dense_model_equals_parent(how):
    n, k, t, seed, rounds = 263, 3, 8, 0x5EED3100, 30
    side = pr.sides_of(n, [100], 5)
    a, b = pr.PartitionModel(n, k, t, t, seed), cl.ControlLossModel(n, k, t, t, seed)
    for m in (a, b):
        m.import_state(*sc.full_state(n), 0)
        if how == "kinds0":
            m.set_loss(0.2, 0.2)
        elif how == "zero":
            m.set_loss(0.0, 0.0)
    b.set_control_loss(0 if how == "kinds0" else cl.CTL_ALL)
    if how != "kinds0":
        a.set_partition(None)  # (GH_CTL_REMOVE arms)
    for r in range(1, rounds + 1):
        for m in (a, b):
            if r == 3:
                m.set_partition(side)
            if r == 5:
                m.apply_events([(sc.CRASH, 9), (sc.CRASH, 200)])
        assert a.step(1) == b.step(1), r
        for x, y in zip(a.export_state(), b.export_state()):
            np.testing.assert_array_equal(x, y, err_msg=f"round {r}")
        np.testing.assert_array_equal(a.rcv, b.rcv)
        assert a.cut == b.cut and (a.sent, a.dropped) == (b.sent, b.dropped)
    st = b.control_loss_stats()
    assert a.sets and st["remove_missed"] == 0 and (st["remove_pairs"] > 0) == (how == "zero")


@pytest.mark.parametrize("order", ["id", "append"])
@pytest.mark.parametrize("mode,quirk", [("ring", False), ("pull", True)])
@pytest.mark.parametrize("how", ["kinds0", "zero"])
def test_list_model_equals_parents(how, mode, quirk, order):
    """Against PartitionListSim across a split (no gossip loss there: zero
    thresholds / kinds 0 with loss off) and against LossyListSim on one side
    (kinds 0 with loss on)."""
    n = 24
    kw = dict(seed=0x5EED3124, peer_mode=mode, order=order, quirk=quirk)
    side = np.zeros(n, np.int32)
    side[14:] = 1
    sched = {3: [(sc.CRASH, 5), (sc.CRASH, 16)], 8: [(sc.LEAVE, 11), (sc.LEAVE, 20)], 14: [(sc.JOIN, 5)], 18: [(sc.JOIN, 16)]}
    pairs = []
    a, b = pr.PartitionListSim.from_dense(*sc.full_state(n), 0, **kw), cl.ControlLossListSim.from_dense(*sc.full_state(n), 0, **kw)
    if how == "zero":
        b.set_loss(0.0, 0.0)
        b.set_control_loss(cl.CTL_ALL)
    else:
        b.set_control_loss(0)
    pairs.append((a, b, True))
    a, b = lr.LossyListSim.from_dense(*sc.full_state(n), 0, **kw), cl.ControlLossListSim.from_dense(*sc.full_state(n), 0, **kw)
    for m in (a, b):
        m.set_loss(0.3, 0.3)
    b.set_control_loss(0)
    pairs.append((a, b, False))
    for a, b, split in pairs:
        for r in range(1, 31):
            for e in (a, b):
                if split and r == 2:
                    e.set_partition(side)
                if sched.get(r):
                    e.apply_events(sched[r])
            assert a.step(1) == b.step(1), r
            for x, y in zip(a.dense(), b.dense()):
                np.testing.assert_array_equal(x, y, err_msg=f"round {r}")
            assert [[m.addr for m in nd.members] for nd in a.nodes] == [[m.addr for m in nd.members] for nd in b.nodes]
            assert a.last_failed == b.last_failed and a.last_detectors == b.last_detectors
        if split:
            assert a.cut == b.cut > 0
        else:
            assert a.loss_stats() == b.loss_stats() and a.dropped > 0
        st = b.control_loss_stats()
        assert not any(st[f] for f in cl.STATS if f.endswith(("missed", "dropped")))


# ---- the two models agree ------------------------------------------------------------------
def test_dense_model_equals_list_model():
    """A lossy two-side pull scenario with crashes at ListSim's T = 5 and
    GH_CTL_REMOVE on both models, the counters too."""
    from oracle import listsim as L
    n, seed, rounds = 40, 0x5EED3140, 22
    side = pr.sides_of(n, [17], 11)
    sched = {5: [(sc.CRASH, 9), (sc.CRASH, 30)]}
    out, inn = cl.rates(n, 0.3, inn_of={7: 0.9})
    dm = cl.ControlLossModel(n, 3, L.T_FAIL, L.T_CLEANUP, seed)
    dm.import_state(*sc.full_state(n), 0)
    ls = cl.ControlLossListSim.from_dense(*sc.full_state(n), 0, seed=seed, peer_mode="pull", fanout=3)
    for e in (dm, ls):
        e.set_loss(out, inn)
        e.set_control_loss(cl.CTL_REMOVE)
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
        assert dm.partition_stats() == ls.partition_stats() and dm.loss_stats() == ls.loss_stats()
        assert dm.control_loss_stats() == ls.control_loss_stats(), r
    st = dm.control_loss_stats()
    assert dm.cut > 0 and 0 < st["remove_missed"] < st["remove_pairs"]


# ---- the GPU tests' scenarios are non-vacuous on the models -----------------------------------
@pytest.mark.parametrize("name", list(tg.CASES))
def test_pull_scenarios_non_vacuous(name):
    case = tg.CASES[name]
    delivered = []
    m = cl.run_model(case, per_round=lambda m, st: delivered.append(st["tombstoned"] + st["remove_unknown"]))
    z = cl.run_model(case, kinds=0)
    st = m.control_loss_stats()
    assert not np.array_equal(m.hb, z.hb)
    assert sum(1 for t in delivered if t > 0) >= (1 if name == "deaf16" else 3)  # rounds that delivered a REMOVE
    if name == "deaf16":
        # kinds = 0: member 17's reliable REMOVEs empty every list; lossy, the
        # other 262 members still list each other
        oth = np.arange(case["n"]) != tg.DEAF
        assert not (z.hb >= 0).any()
        assert (m.hb[np.ix_(oth, oth)] >= 0).all()
        assert 0 < st["remove_missed"] < st["remove_pairs"]  # (REMOVE(17) itself arrives)
    else:
        assert 0 < st["remove_missed"] < st["remove_pairs"]
        assert int((m.hb == -2).sum() + (m.hb == -1).sum()) < int((z.hb == -2).sum() + (z.hb == -1).sum())
    if case["side"] is not None:
        assert m.cut > 0
        # a REMOVE across the split is no message: some running row has no message of some set
        assert st["remove_pairs"] < sum(sum(run.values()) for _, _, _, run in m.sets)


@pytest.mark.parametrize("name,order", [("ring24", "id"), ("ring24", "append"), ("ring48", "id"), ("ring48", "append"),
                                        ("quirk96", "id")])
def test_list_scenarios_non_vacuous(name, order):
    case = tg.LIST_CASES[name]
    m = tg.run_list_model(case, order)
    z = tg.run_list_model(case, order, kinds=0)
    st = m.control_loss_stats()
    assert 0 < st["remove_missed"] < st["remove_pairs"], st
    for f in ("leave", "join", "bcast"):
        assert 0 < st[f + "_dropped"] < st[f + "_sent"], (f, st)
    assert not np.array_equal(m.dense()[0], z.dense()[0])
    assert m.dropped > 0 and (case["side"] is None or m.cut > 0)
    kinds = {kind for ev in case["sched"].values() for kind, _ in ev}
    assert kinds == {sc.CRASH, sc.LEAVE, sc.JOIN}
    if case["side"] is not None:
        sides = {(kind, int(case["side"][c])) for ev in case["sched"].values() for kind, c in ev}
        assert {(k, s) for k in kinds for s in (0, 1)} <= sides


def test_arming_and_flip_scenarios():
    """What the two deaf-case GPU tests rely on: a REMOVE set is pending well
    before their last round, and with the loss switched off right after the
    round of the detection the other members still keep each other, while
    delivery by the rule in force at delivery (reliable) would not."""
    case = dict(tg.CASES["deaf16"], rounds=16)
    m = cl.model_of(case)
    first = None
    for r in range(1, case["rounds"] + 1):
        if first is None and m.failed().size > 0:
            first = r
            m.set_loss(None, None)
            m.set_control_loss(0)
        m.step(1)
    oth = np.arange(case["n"]) != tg.DEAF
    assert first is not None and first < 12
    assert (m.hb[np.ix_(oth, oth)] >= 0).all()
    z = cl.run_model(case, kinds=0)
    assert not (z.hb[np.ix_(oth, oth)] >= 0).all()


# ---- the three entry points without a device --------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gossipsim import _abi
    return _abi.load(), _abi


def test_control_loss_symbols_exported(lib):
    L, abi = lib
    raw = C.CDLL(str(abi.LIB_PATH))
    bound = {n for n, _, _ in abi.SYMBOLS}
    for name in ("gh_set_control_loss", "gh_get_control_loss", "gh_control_loss_stats"):
        assert hasattr(raw, name) and name in bound
    assert (abi.GH_CTL_REMOVE, abi.GH_CTL_LEAVE, abi.GH_CTL_JOIN) == (cl.CTL_REMOVE, cl.CTL_LEAVE, cl.CTL_JOIN) == (1, 2, 4)
    import gossipsim
    assert gossipsim.CONTROL_LOSS_STATS == cl.STATS


def test_control_loss_null_handle(lib):
    L, abi = lib
    k, out8 = C.c_int32(7), (C.c_int64 * 8)(*([7] * 8))
    assert L.gh_set_control_loss(None, 1) == abi.GH_EINVAL
    assert L.gh_get_control_loss(None, C.byref(k)) == abi.GH_EINVAL
    assert L.gh_control_loss_stats(None, out8) == abi.GH_EINVAL
    assert k.value == 7 and list(out8) == [7] * 8


def test_cluster_refuses_control_loss_with_elections():
    from gossipsim import Cluster
    c = Cluster.__new__(Cluster)
    c.elect = True
    with pytest.raises(ValueError):
        c.set_control_loss(cl.CTL_ALL)
    with pytest.raises(ValueError):
        c.control_loss_stats()


# gh_footprint's create_bytes of the commit before gh_set_control_loss existed, read from its library
FOOTPRINT_263 = 2783718
FOOTPRINT_65536 = 32391242272


def test_footprint_is_the_parents():
    """gh_footprint is a dry walk of gh_create's allocations: the feature
    allocates nothing there, so both figures are those of the commit before it."""
    import gossipsim as gs
    assert gs.footprint(gs.default_config(263, fanout=3))["create_bytes"] == FOOTPRINT_263
    assert gs.footprint(gs.default_config(65536, fanout=4))["create_bytes"] == FOOTPRINT_65536
