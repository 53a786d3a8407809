"""Lossy control messages (gh_set_control_loss, SPEC §2 step 6c) on the GPU
against the CPU models of tests/control_loss_ref.py, bit for bit after every
round: hb, ts, alive, the round's stats, read_failed, read_detectors,
loss_stats, partition_stats, control_loss_stats and, in append order, every
row's list.

Pull mode with crashes runs against the dense numpy model (ControlLossModel),
everything with JOIN / LEAVE, ring mode, quirk detection or list order against
the ListSim-based one (ControlLossListSim); kinds = 0 and zero thresholds run
against the existing oracles. The scenarios (CASES, LIST_CASES) are checked for
non-vacuity on the CPU by test_control_loss_ref.py; every seed was chosen so
that those checks hold on the models, no figure comes from the engine.
Run on a MI355X: pytest -m gpu."""
import ctypes as C

import numpy as np
import pytest

import control_loss_ref as cl
import loss_ref as lr
import scenarios as sc

pytestmark = pytest.mark.gpu

EINVAL = -1
DEAF = 17  # the deaf and mute member of "deaf16"


def _deaf(n):
    out = np.zeros(n, np.uint32)
    out[DEAF] = lr.ALWAYS
    return out, out.copy()


def _far(n, count, seed):
    import partition_ref as pr
    return pr.sides_of(n, [count], seed)


# Pull-mode scenarios from a full start (ControlLossModel).
CASES = {
    # member 17 hears nobody and nobody hears it: it detects everybody, and its
    # REMOVEs are lost with every other message of its
    "deaf16": cl.pull_case(263, 3, 8, 36, 0x5EED3264, *_deaf(263), cl.CTL_REMOVE),
    # 0.2 on both ends of every link, member 40 hears 7 % of what reaches it
    # (a steady source of detections by a single row), 1 % crash at round 8
    "nib263": cl.pull_case(263, 4, 16, 60, 0x5EED3363, *cl.rates(263, 0.2, inn_of={40: 0.93}), cl.CTL_REMOVE,
                           crash=cl.crash_1pct(263, 0x5EED3363)),
    "nib1000": cl.pull_case(1000, 4, 16, 60, 0x5EED36E8, *cl.rates(1000, 0.2, inn_of={40: 0.93}), cl.CTL_REMOVE,
                            crash=cl.crash_1pct(1000, 0x5EED36E8)),
    # the same rates on the 16-bit path across two sides (163 and 100) from round 3
    "sides16": cl.pull_case(263, 4, 16, 44, 0x5EED3365, *cl.rates(263, 0.2, inn_of={40: 0.93}), cl.CTL_ALL,
                            crash=cl.crash_1pct(263, 0x5EED3365), side=_far(263, 100, 0x3365), split=3),
}


def _list_case(n, seed, rounds, sched, far=(), split=2, **kw):
    side = None
    if far:
        side = np.zeros(n, np.int32)
        side[list(far)] = 1
    return dict(n=n, seed=seed, side=side, split=split, rounds=rounds, sched=sched, kw=kw, rate=0.5, kinds=cl.CTL_ALL)


# ControlLossListSim scenarios (T_fail = T_cleanup = 5, ListSim's constants;
# rate 0.5 on both ends of every link, all kinds; the introducer, member 0, is
# on side 0): crashes, leaves and joins on both sides of the split where there
# is one. At this rate the cluster falls apart within a dozen rounds, so the
# events come early, while the lists are long.
LIST_CASES = {
    "ring24": _list_case(24, 0x5EED3428, 18,
                         {2: [(sc.CRASH, 3), (sc.CRASH, 5), (sc.CRASH, 15), (sc.CRASH, 16)],
                          3: [(sc.LEAVE, 9), (sc.LEAVE, 17)], 4: [(sc.JOIN, 3), (sc.JOIN, 15)],
                          5: [(sc.JOIN, 5), (sc.JOIN, 16)], 6: [(sc.LEAVE, 10), (sc.LEAVE, 20), (sc.JOIN, 9)],
                          7: [(sc.JOIN, 3), (sc.JOIN, 17)]}, far=range(14, 24), peer_mode="ring"),
    "ring48": _list_case(48, 0x5EED344E, 18,
                         {2: [(sc.CRASH, 6), (sc.CRASH, 42), (sc.CRASH, 11), (sc.CRASH, 30)],
                          3: [(sc.LEAVE, 21), (sc.LEAVE, 44)], 4: [(sc.JOIN, 6), (sc.JOIN, 42)],
                          5: [(sc.JOIN, 11), (sc.JOIN, 30), (sc.LEAVE, 25)], 6: [(sc.JOIN, 21), (sc.JOIN, 6)],
                          7: [(sc.JOIN, 44), (sc.JOIN, 42)]}, peer_mode="ring"),
    "quirk96": _list_case(96, 0x5EED34A1, 16,
                          {2: [(sc.CRASH, 7), (sc.CRASH, 50), (sc.CRASH, 20), (sc.CRASH, 70)],
                           3: [(sc.LEAVE, 12), (sc.LEAVE, 60)], 4: [(sc.JOIN, 7), (sc.JOIN, 50)],
                           5: [(sc.JOIN, 20), (sc.JOIN, 70), (sc.LEAVE, 13)], 6: [(sc.JOIN, 12), (sc.JOIN, 7)],
                           7: [(sc.JOIN, 60), (sc.JOIN, 20)]}, far=range(40, 96), peer_mode="pull", fanout=3,
                          quirk=True),
}


def list_model(case, order="id", kinds=None):
    m = cl.ControlLossListSim.from_dense(*sc.full_state(case["n"]), 0, seed=case["seed"], order=order, **case["kw"])
    m.set_loss(case["rate"], case["rate"])
    m.set_control_loss(case["kinds"] if kinds is None else kinds)
    return m


def run_list_model(case, order="id", kinds=None, per_round=None):
    m = list_model(case, order, kinds)
    for r in range(1, case["rounds"] + 1):
        if case["side"] is not None and r == case["split"]:
            m.set_partition(case["side"])
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
    assert eng.partition()[0] == model.armed, f"{what} armed after round {r}"
    if model.armed:
        assert eng.partition_stats() == model.partition_stats(), f"{what} partition_stats after round {r}"
    if model.out is not None:
        assert eng.loss_stats() == model.loss_stats(), f"{what} loss_stats after round {r}"
    if model.ctl_called:
        assert eng.control_loss_stats() == model.control_loss_stats(), f"{what} control_loss_stats after round {r}"


def start(gs, case, kinds=None, **cfg_kw):
    """The engine and the model of a pull scenario, loss and kinds set."""
    eng = gs.Engine(gs.default_config(case["n"], **case["cfg"], **cfg_kw))
    eng.import_state(*sc.full_state(case["n"]), 0)
    eng.set_loss(case["out"], case["inn"])
    eng.set_control_loss(case["kinds"] if kinds is None else kinds)
    return eng, cl.model_of(case, kinds)


def lockstep(eng, model, case, per_round=None, before=None):
    """The engine and the pull model one round at a time, compared after each;
    before(r) runs ahead of round r's events."""
    for r in range(1, case["rounds"] + 1):
        if case["side"] is not None and r == case["split"]:
            eng.set_partition(case["side"])
            model.set_partition(case["side"])
        if before:
            before(r)
        ev = case["sched"].get(r)
        if ev:
            eng.apply_events(ev)
            model.apply_events(ev)
        want, got = model.step(1), eng.step(1)
        assert got == want, f"round {r}: gpu {got} != model {want}"
        compare(eng, model, r)
        if per_round:
            per_round(r, want)


# ---- 1. 16-bit path: the deaf and mute member ---------------------------------------
def test_deaf_mute_16bit(gs):
    """N=263, k=3, T=8 on the 16-bit path: member 17 detects everybody, every
    one of its REMOVEs is lost, and the call has armed the engine with every
    member on side 0."""
    case = CASES["deaf16"]
    eng, model = start(gs, case)
    try:
        assert eng.tier_info()[0] == 0
        armed, side = eng.partition()
        assert armed and not side.any() and eng.control_loss() == cl.CTL_REMOVE
        lockstep(eng, model, case)
        st = eng.control_loss_stats()
        assert st["remove_missed"] > 0 and st["leave_sent"] == st["join_sent"] == st["bcast_sent"] == 0
    finally:
        eng.close()


# ---- 2. nibble path ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nib263", "nib1000"])
def test_nibble_path(gs, monkeypatch, name):
    """GH_PLANE=1, k=4, T=16, 60 rounds in the 4-bit tier: the nibble path
    (variant 3) ran in a round that delivered a REMOVE."""
    monkeypatch.setenv("GH_PLANE", "1")
    case = CASES[name]
    eng, model = start(gs, case)
    seen = []

    def per_round(r, st):
        seen.append((eng.tier_info(full=True)[3], st["tombstoned"] + st["remove_unknown"]))

    try:
        assert eng.tier_info()[0] == 1
        lockstep(eng, model, case, per_round=per_round)
        print(f"{name}: (variant, cells a REMOVE reached) per round {seen}")
        assert any(v == 3 and rm > 0 for v, rm in seen), seen
    finally:
        eng.close()


# ---- 3. sides and loss together ------------------------------------------------------------
def test_sides_and_loss(gs):
    """Two sides of 163 and 100 from round 3, all kinds: a message cut by the
    partition is neither drawn nor counted (every counter equals the model's
    after every round)."""
    case = CASES["sides16"]
    eng, model = start(gs, case)
    try:
        lockstep(eng, model, case)
        assert model.cut > 0 and 0 < model.ctl["remove_missed"] < model.ctl["remove_pairs"]
    finally:
        eng.close()


# ---- 4. list cases ---------------------------------------------------------------------------
def list_compare(eng, ls, n, r, lists):
    from oracle import listsim as L
    h1, t1, a1 = eng.export_state()
    h2, t2, a2 = ls.dense()
    np.testing.assert_array_equal(a1, a2, err_msg=f"alive r={r}")
    np.testing.assert_array_equal(h1, h2, err_msg=f"hb r={r}")
    np.testing.assert_array_equal(t1, sc.export_view(h2, t2, r, L.T_CLEANUP)[1], err_msg=f"ts r={r}")
    assert bits(eng.read_failed(), n) == ls.last_failed, r
    assert sorted(eng.read_detectors()) == sorted(ls.last_detectors), r
    assert eng.partition()[0] == ls.armed, r
    if ls.armed:
        assert eng.partition_stats() == ls.partition_stats(), r
    assert eng.loss_stats() == ls.loss_stats(), r
    assert eng.control_loss_stats() == ls.control_loss_stats(), r
    if lists:
        assert [list(eng.lsm(i)[0]) for i in range(n)] == [[m.addr for m in nd.members] for nd in ls.nodes], r


def list_engine(gs, case, order="id"):
    kw = case["kw"]
    eng = gs.Engine(gs.default_config(
        case["n"], seed=case["seed"], fanout=kw.get("fanout", 3),
        peer_mode=gs.GH_PEER_RING if kw["peer_mode"] == "ring" else gs.GH_PEER_PULL,
        detect_mode=gs.GH_DETECT_QUIRK if kw.get("quirk") else gs.GH_DETECT_CANONICAL,
        list_order=gs.GH_ORDER_APPEND if order == "append" else gs.GH_ORDER_ID))
    eng.import_state(*sc.full_state(case["n"]), 0)
    eng.set_loss(case["rate"], case["rate"])
    eng.set_control_loss(case["kinds"])
    return eng


def list_run(eng, ls, case, lists):
    for r in range(1, case["rounds"] + 1):
        if case["side"] is not None and r == case["split"]:
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
    """Ring mode in member-ID and in append order (the lists too), rate 0.5, all
    kinds: ring24 across a split, ring48 on one side."""
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


# ---- 5. identity -------------------------------------------------------------------------------
def test_identity_zero_thresholds(gs, oracle_mod):
    """All kinds with both threshold arrays zero against tablesim under churn
    (crashes, leaves, joins), beside an engine that never made the call: same
    tables, stats, failed sets and detectors. Every message is counted and none
    is dropped. The never-called engine stays unarmed."""
    n, rounds = 263, 30
    kw = dict(fanout=3, seed=0x5EED3A00, t_fail=3, t_cleanup=5)
    sched = sc.random_churn(n, rounds, 0x3A, p_crash=0.05, p_leave=0.02, p_join=0.05)
    eng, never = gs.Engine(gs.default_config(n, **kw)), gs.Engine(gs.default_config(n, **kw))
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **kw))
    try:
        mem0 = never.memory_info()
        for e in (eng, never, orc):
            e.import_state(*sc.full_state(n), 0)
        zero = np.zeros(n, np.uint32)
        eng.set_loss(zero, zero)
        eng.set_control_loss(cl.CTL_ALL)
        assert never.memory_info() == mem0  # (before the churn grows the frozen store)
        for r in range(1, rounds + 1):
            for e in (eng, never, orc):
                if sched.get(r):
                    e.apply_events(sched[r])
            s1, s0, s2 = eng.step(1), never.step(1), orc.step(1)
            assert s1 == s2 == s0, f"round {r}: gpu {s1} / {s0} != cpu {s2}"
            for name, x, z, y in zip(("hb", "ts", "alive"), eng.export_state(), never.export_state(), orc.export_state()):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} after round {r}")
                np.testing.assert_array_equal(z, y, err_msg=f"never-called {name} after round {r}")
            np.testing.assert_array_equal(eng.read_failed(), orc.read_failed(), err_msg=f"failed, round {r}")
            np.testing.assert_array_equal(eng.read_detectors(), orc.read_detectors(), err_msg=f"detectors, round {r}")
        st = eng.control_loss_stats()
        assert st["remove_pairs"] > 0 and st["leave_sent"] > 0 and st["join_sent"] > 0 and st["bcast_sent"] > 0
        assert st["remove_missed"] == st["leave_dropped"] == st["join_dropped"] == st["bcast_dropped"] == 0
        assert never.partition()[0] is False and never.control_loss() == 0
        with pytest.raises(gs.GossipError):
            never.control_loss_stats()
    finally:
        eng.close()
        never.close()
        orc.close()


def test_identity_kinds0_with_loss(gs):
    """kinds = 0 with loss on (0.2 per side) under churn equals an engine with
    the same loss that never made the call, round for round, loss_stats
    included; the call arms nothing and its counters stay zero."""
    n, rounds = 263, 30
    kw = dict(fanout=3, seed=0x5EED3A01, t_fail=3, t_cleanup=5)
    sched = sc.random_churn(n, rounds, 0x3B, p_crash=0.05, p_leave=0.02, p_join=0.05)
    eng, never = gs.Engine(gs.default_config(n, **kw)), gs.Engine(gs.default_config(n, **kw))
    try:
        for e in (eng, never):
            e.import_state(*sc.full_state(n), 0)
            e.set_loss(0.2, 0.2)
        eng.set_control_loss(0)
        for r in range(1, rounds + 1):
            for e in (eng, never):
                if sched.get(r):
                    e.apply_events(sched[r])
            s1, s0 = eng.step(1), never.step(1)
            assert s1 == s0, f"round {r}: {s1} != never called {s0}"
            for name, x, z in zip(("hb", "ts", "alive"), eng.export_state(), never.export_state()):
                np.testing.assert_array_equal(x, z, err_msg=f"{name} after round {r}")
            np.testing.assert_array_equal(eng.read_failed(), never.read_failed(), err_msg=f"failed, round {r}")
            np.testing.assert_array_equal(eng.read_detectors(), never.read_detectors(), err_msg=f"detectors, round {r}")
            assert eng.loss_stats() == never.loss_stats(), r
        assert eng.loss_stats()[1] > 0
        assert not any(eng.control_loss_stats().values()) and eng.partition()[0] is False
    finally:
        eng.close()
        never.close()


def test_identity_listsim_append(gs):
    """Append order, ring mode, all kinds with zero thresholds against ListSim,
    the lists too."""
    from oracle.listsim import ListSim
    n, rounds = 48, 30
    sched = sc.random_churn(n, rounds, 0x3A48, p_crash=0.05, p_leave=0.03, p_join=0.08)
    eng = gs.Engine(gs.default_config(n, peer_mode=gs.GH_PEER_RING, seed=0x5EED3A48, list_order=gs.GH_ORDER_APPEND))
    ls = ListSim.from_dense(*sc.full_state(n), 0, seed=0x5EED3A48, peer_mode="ring", order="append")
    try:
        eng.import_state(*sc.full_state(n), 0)
        eng.set_loss(0.0, 0.0)
        eng.set_control_loss(cl.CTL_ALL)
        for r in range(1, rounds + 1):
            for e in (eng, ls):
                if sched.get(r):
                    e.apply_events(sched[r])
            s1, s2 = eng.step(1), ls.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
            h2, t2, a2 = ls.dense()
            np.testing.assert_array_equal(eng.export_state()[0], h2, err_msg=f"hb r={r}")
            assert [list(eng.lsm(i)[0]) for i in range(n)] == [[m.addr for m in nd.members] for nd in ls.nodes], r
    finally:
        eng.close()


def test_arming_keeps_the_pending_set(gs):
    """gh_set_control_loss(GH_CTL_REMOVE) while a REMOVE set is pending (the
    engine was never armed, loss on with the deaf case's thresholds but no
    kind set before): the set is delivered by rule D4, as the model's."""
    case = dict(CASES["deaf16"], rounds=14)
    eng, model = start(gs, case, kinds=0)
    armed_at = []

    def before(r):
        if not armed_at and model.failed().size > 0:
            assert eng.partition()[0] is False
            eng.set_control_loss(cl.CTL_REMOVE)
            model.set_control_loss(cl.CTL_REMOVE)
            armed_at.append(r)

    try:
        lockstep(eng, model, case, before=before)
        assert armed_at and armed_at[0] < case["rounds"] - 2, armed_at
    finally:
        eng.close()


def test_never_called_engine_is_the_parents(gs):
    """Structure of the off state and of what each call allocates, by
    hipMemGetInfo at N = 8,192 (the bitmaps of arming are 8 MiB each there).
    TOL = 2 MiB is the largest granule hipMalloc rounds a small allocation to
    (a large-page fragment), so "nothing but a small block" is a move of at
    most TOL:
    * a never-called engine with loss on stays unarmed with kinds 0 (the two
      conditions that gate k_ctl_recv, k_bcast_drop and gh_ctl_drop), and its
      gh_set_loss and rounds move free memory by no more than the threshold
      arrays' one small block;
    * GH_CTL_LEAVE | GH_CTL_JOIN costs the counter block alone and arms nothing;
    * GH_CTL_REMOVE then costs what gh_set_partition(NULL) costs a twin engine
      (3 bitmaps of ld * ceil(N / 32) words and the small vectors)."""
    hip = C.CDLL("libamdhip64.so")
    TOL = 2 << 20

    def free():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    n = 8192
    kw = dict(fanout=3, seed=0x5EED3B00, t_fail=8, t_cleanup=8)
    never, ctl, twin = (gs.Engine(gs.default_config(n, **kw)) for _ in range(3))
    try:
        for e in (never, ctl, twin):
            e.init_full(2, 0, 0)
            e.step(2)  # (first launches, code objects loaded)
            e.sync()
        mem0, f0 = never.memory_info(), free()
        never.set_loss(0.1, 0.1)
        never.step(4)
        never.sync()
        d_never = f0 - free()
        assert never.partition()[0] is False and never.control_loss() == 0
        assert never.memory_info() == mem0
        with pytest.raises(gs.GossipError):
            never.control_loss_stats()
        ctl.set_loss(0.1, 0.1)
        f1 = free()
        ctl.set_control_loss(cl.CTL_LEAVE | cl.CTL_JOIN)
        d_events = f1 - free()
        assert ctl.partition()[0] is False
        f2 = free()
        ctl.set_control_loss(cl.CTL_ALL)
        d_remove = f2 - free()
        f3 = free()
        twin.set_partition(None)
        d_part = f3 - free()
        assert ctl.partition()[0] is True
        bitmaps = 3 * n * ((n + 31) // 32) * 4
        print(f"free memory moved by: never called (set_loss + 4 rounds) {d_never}, LEAVE|JOIN {d_events}, "
              f"REMOVE {d_remove}, set_partition(None) {d_part}; the three bitmaps are {bitmaps} bytes")
        assert 0 <= d_never <= TOL
        assert 0 <= d_events <= TOL
        assert d_part >= bitmaps and abs(d_remove - d_part) <= TOL
    finally:
        for e in (never, ctl, twin):
            e.close()


@pytest.mark.parametrize("how", ["import_state", "init_full"])
def test_kinds_persist_across_import_and_init(gs, how):
    """kinds and the thresholds are configuration: set before gh_import_state /
    gh_init_full, they are in force in the rounds after it (the deaf case
    against the model, which gets them after its import)."""
    case = dict(CASES["deaf16"], rounds=14)
    eng = gs.Engine(gs.default_config(case["n"], **case["cfg"]))
    model = cl.model_of(case)
    try:
        eng.set_loss(case["out"], case["inn"])
        eng.set_control_loss(case["kinds"])
        if how == "import_state":
            eng.import_state(*sc.full_state(case["n"]), 0)
        else:
            eng.init_full(2, 0, 0)
        assert eng.control_loss() == case["kinds"] and eng.partition()[0] is True
        lockstep(eng, model, case)
        st = eng.control_loss_stats()
        assert st["remove_missed"] > 0
    finally:
        eng.close()


# ---- 6. a pending set keeps its recipients -------------------------------------------------
def _toggle(e, case, on):
    """Loss and kinds off (nothing is lossy any more), or back to the case's."""
    if on:
        e.set_loss(case["out"], case["inn"])
        e.set_control_loss(case["kinds"])
    else:
        e.set_control_loss(0)
        e.set_loss(None, None)


def toggle_plan(case, limit=2):
    """On the model alone: {round: on / off}, loss and kinds switched off before
    each of `limit` rounds that start with a REMOVE set pending (drawn under
    loss, delivered without) and on again a round later; and the scenario as
    gh_step calls of at most 5 rounds, a new call at every toggle and every
    event batch. Also, per switch-off, how many alive rows the pending set
    misses that rule D4 (what a delivery decided without loss would use)
    reaches."""
    import partition_ref as pr
    model, plan, off, missed = cl.model_of(case), {}, False, []
    for r in range(1, case["rounds"] + 1):
        if off:
            plan[r] = off = False
            _toggle(model, case, True)
        elif model.failed().size > 0 and sum(1 for v in plan.values() if v) < limit:
            plan[r] = off = True
            d4 = pr.PartitionModel._recipients(model, model.last_cand, model.alive.astype(bool))
            missed.append(int((d4 & ~model.rcv & model.alive.astype(bool)[:, None]).sum()))
            _toggle(model, case, False)
        if case["sched"].get(r):
            model.apply_events(case["sched"][r])
        model.step(1)
    cuts = sorted({1, case["rounds"] + 1, *case["sched"], *plan})
    calls = [(f, min(5, hi - f)) for lo, hi in zip(cuts, cuts[1:]) for f in range(lo, hi, 5)]
    return plan, calls, missed


def test_pending_set_and_call_shapes(gs):
    """nib263's rates on the 16-bit path: before each of two rounds that start
    with a REMOVE set pending, loss and kinds are switched off, and on again a
    round later; the set's recipients stay those drawn in the round of the
    detection, as the model's. A second engine runs the same scenario in calls
    of up to 5 rounds and equals the first after each."""
    case = dict(CASES["nib263"], rounds=40)
    plan, calls, missed = toggle_plan(case)
    assert sum(plan.values()) == 2 and min(missed) > 0 and max(k for _, k in calls) == 5 and sum(k for _, k in calls) == case["rounds"]
    a, model = start(gs, case)
    b, _ = start(gs, case)
    try:
        for first, k in calls:
            if first in plan:
                assert model.failed().size > 0 or not plan[first]
                for e in (a, b, model):
                    _toggle(e, case, not plan[first])
            if case["sched"].get(first):
                for e in (a, b, model):
                    e.apply_events(case["sched"][first])
            total = None
            for r in range(first, first + k):
                want, got = model.step(1), a.step(1)
                assert got == want, f"round {r}: gpu {got} != model {want}"
                compare(a, model, r)
                total = want if total is None else {f: total[f] + want[f] for f in total}
            got = b.step(k)
            assert {f: got[f] for f in lr.SUMMED} == {f: total[f] for f in lr.SUMMED}, (first, got, total)
            compare(b, model, first + k - 1, what=f"step({k})")
    finally:
        a.close()
        b.close()


def test_flip_while_pending_is_not_vacuous(gs):
    """The deaf case with the loss switched off right after the round of the
    first detections: the pending set still misses every row (it was drawn in
    the round of the detection), so the other members keep each other."""
    case = dict(CASES["deaf16"], rounds=16)
    eng, model = start(gs, case)
    done = []

    def before(r):
        if not done and model.failed().size > 0:
            for e in (eng, model):
                e.set_loss(None, None)
                e.set_control_loss(0)
            done.append(r)

    try:
        lockstep(eng, model, case, before=before)
        oth = np.arange(case["n"]) != DEAF
        assert done and (model.hb[np.ix_(oth, oth)] >= 0).all()
    finally:
        eng.close()


# ---- 7. refusals ----------------------------------------------------------------------------------
def test_refusals(gs):
    """GH_EINVAL: a 2-shard LOCAL handle, a GH_REMOVE_LIST engine, kinds = 8
    and -1, stats before any call, a NULL handle."""
    from gossipsim import _abi
    n = 64
    eng = gs.Engine(gs.default_config(n))
    lst = gs.Engine(gs.default_config(n, remove_mode=1))  # GH_REMOVE_LIST
    grp = gs.ShardGroup(gs.default_config(n), 2)
    try:
        with pytest.raises(gs.GossipError) as err:
            eng.control_loss_stats()
        assert err.value.code == EINVAL
        for bad in (8, -1):
            with pytest.raises(gs.GossipError) as err:
                eng.set_control_loss(bad)
            assert err.value.code == EINVAL
            assert eng.control_loss() == 0 and eng.partition()[0] is False
        with pytest.raises(gs.GossipError):
            eng.control_loss_stats()  # a refused call is no call
        for e in (lst, grp):
            with pytest.raises(gs.GossipError) as err:
                e.set_control_loss(cl.CTL_REMOVE)
            assert err.value.code == EINVAL
        assert lst.partition()[0] is False
        eng.set_control_loss(cl.CTL_LEAVE | cl.CTL_JOIN)  # arms nothing
        assert eng.partition()[0] is False and eng.control_loss() == 6
        assert not any(eng.control_loss_stats().values())
        L = _abi.load()
        k, out8 = C.c_int32(7), (C.c_int64 * 8)(*([7] * 8))
        assert L.gh_set_control_loss(None, 1) == EINVAL
        assert L.gh_get_control_loss(None, C.byref(k)) == EINVAL
        assert L.gh_control_loss_stats(None, out8) == EINVAL
        assert k.value == 7 and list(out8) == [7] * 8
    finally:
        eng.close()
        lst.close()
        grp.close()


# ---- 8. the Cluster facade ---------------------------------------------------------------------------
def test_cluster_forwards(gs):
    """Cluster.set_control_loss / control_loss_stats reach the engine: ring24
    through the Cluster facade (ring mode, append order, its defaults) against
    the model, the lists too; with elect=True both raise ValueError."""
    case = LIST_CASES["ring24"]
    n = case["n"]
    c = gs.Cluster(n, seed=case["seed"])
    ls = list_model(case, "append")
    verb = {sc.CRASH: c.crash, sc.LEAVE: c.leave, sc.JOIN: c.join}
    try:
        c.engine.import_state(*sc.full_state(n), 0)
        with pytest.raises(gs.GossipError):
            c.control_loss_stats()  # never called yet
        c.set_loss(case["rate"], case["rate"])
        c.set_control_loss(case["kinds"])
        for r in range(1, case["rounds"] + 1):
            if r == case["split"]:
                c.set_partition(case["side"])
                ls.set_partition(case["side"])
            for kind, m in case["sched"].get(r, []):
                verb[kind](m)
            if case["sched"].get(r):
                ls.apply_events(case["sched"][r])
            s1, s2 = c.tick(1), ls.step(1)
            assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
            list_compare(c.engine, ls, n, r, True)
            assert c.control_loss_stats() == ls.control_loss_stats()
    finally:
        c.engine.close()
    e = gs.Cluster.__new__(gs.Cluster)
    e.elect = True
    with pytest.raises(ValueError):
        e.set_control_loss(cl.CTL_ALL)
    with pytest.raises(ValueError):
        e.control_loss_stats()


# ---- 9. the journal ---------------------------------------------------------------------------------------
def test_journal_detect(gs):
    """GH_JOURNAL_DETECT over nib263 (16-bit path) against journal_ref fed from
    the model's exact det_cnt / det_min of every round."""
    import journal_ref as jr
    case = CASES["nib263"]
    eng, model = start(gs, case)
    ref = jr.JournalRef(case["n"], np.ones(case["n"], np.uint8), jr.DETECT, 64)
    try:
        eng.journal_enable(gs.GH_JOURNAL_DETECT, 64)
        for r in range(1, case["rounds"] + 1):
            ev = case["sched"].get(r)
            if ev:
                eng.apply_events(ev)
                model.apply_events(ev)
            want, got = model.step(1), eng.step(1)
            assert got == want, f"round {r}: gpu {got} != model {want}"
            ref.observe(r, model.alive, model.det_cnt, np.where(model.det_cnt > 0, model.det_min, -1).astype(np.int32))
        compare(eng, model, case["rounds"])
        jr.assert_journal_equal(eng.journal(), eng.journal_rounds(), ref)
        assert int(ref.fp_rounds.sum()) > 0
    finally:
        eng.close()
