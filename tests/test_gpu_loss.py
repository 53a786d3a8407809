"""Lossy gossip links (gh_set_loss, SPEC §2 step 6a) on the GPU against the
CPU models of tests/loss_ref.py, bit for bit after every round: hb, ts, alive,
the round's stats, read_failed, read_detectors and loss_stats.

Pull mode runs against the dense numpy model (LossModel), ring mode against
the ListSim-based one (LossyListSim). The scenarios (CASES, RING_CASES) are
checked for non-vacuity on the CPU by test_loss_ref.py: messages are dropped,
the final tables differ from the zero-loss run, and where the docstring says
so a running member is detected; every pinned literal comes from the model.
Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import loss_ref as lr
import scenarios as sc

pytestmark = pytest.mark.gpu

ROWS = 1  # GH_LAYOUT_ROWS


def _crash(n, seed, at=8):
    return {at: [(sc.CRASH, int(c)) for c in sc.crash_ids(n, 0.01, seed)]}


# Pull-mode scenarios from a full start. mute: out = ALWAYS (nobody hears it:
# detected while it runs, REMOVE reaches it and it drops its own entry);
# deaf: in = ALWAYS (it hears nobody, detects everyone at round T_fail + 1 and
# its REMOVEs, which are reliable, empty every list: the cluster collapses, as
# the reference's would). nib*_mute leaves the deaf member out, so that the
# crashed members are detected and cleaned up under loss.
CASES = {
    "storm16": dict(lr.uniform_case(250, 3, 5, 0.25, 30), false_positives=True),
    "nib1000": dict(lr.uniform_case(1000, 4, 16, 0.10, 40, crash=_crash(1000, 0x5EED10A0), mute=321, deaf=777),
                    false_positives=True),
    "nib263": dict(lr.uniform_case(263, 4, 16, 0.10, 40, crash=_crash(263, 0x5EED10A1), mute=130, deaf=262),
                   false_positives=True),
    "nib1000_mute": dict(lr.uniform_case(1000, 4, 16, 0.10, 40, crash=_crash(1000, 0x5EED10A0), mute=321),
                         false_positives=True),
    "k8": lr.uniform_case(520, 8, 5, 0.3, 15),
    "shards": dict(lr.uniform_case(1000, 4, 16, 0.10, 26, crash=_crash(1000, 0x5EED10A2), mute=999),
                   false_positives=True),
}

# Ring-mode scenarios (T_fail = T_cleanup = 5, ListSim's constants): uniform
# loss with a mute and a deaf member, a crash, a rejoin and a leave.
RING_CASES = {
    24: dict(n=24, seed=0x5EED1024, rate=0.2, mute=7, deaf=15, rounds=30,
             sched={4: [(sc.CRASH, 3)], 12: [(sc.JOIN, 3)], 18: [(sc.LEAVE, 20)]}),
    48: dict(n=48, seed=0x5EED1048, rate=0.2, mute=40, deaf=9, rounds=24,
             sched={3: [(sc.CRASH, 47), (sc.CRASH, 24)], 15: [(sc.JOIN, 24)]}),
}


def ring_loss(case):
    n = case["n"]
    out = np.full(n, lr.q32(case["rate"]), np.uint32)
    inn = out.copy()
    out[case["mute"]] = lr.ALWAYS
    inn[case["deaf"]] = lr.ALWAYS
    return out, inn


def ring_model(case, order, lossy=True):
    n = case["n"]
    m = lr.LossyListSim.from_dense(*sc.full_state(n), 0, seed=case["seed"], peer_mode="ring", order=order)
    if lossy:
        m.set_loss(*ring_loss(case))
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
    """Engine (or ShardGroup) against the pull model after round r."""
    for name, x, y in zip(("hb", "ts", "alive"), eng.export_state(), model.export_state()):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name} after round {r}")
    np.testing.assert_array_equal(eng.read_failed(), model.read_failed(), err_msg=f"{what} failed set, round {r}")
    np.testing.assert_array_equal(np.sort(eng.read_detectors()), model.read_detectors(),
                                  err_msg=f"{what} detectors, round {r}")
    if model.out is not None:
        assert eng.loss_stats() == model.loss_stats(), f"{what} loss_stats after round {r}"


def lockstep(engines, model, case, rounds=None, first=1, per_round=None):
    """Engines and the model one round at a time, compared after each."""
    total = dict.fromkeys(lr.SUMMED, 0)
    for r in range(first, (rounds or case["rounds"]) + 1):
        ev = case["sched"].get(r)
        for e in list(engines) + [model]:
            if ev:
                e.apply_events(ev)
        want = model.step(1)
        for x, e in enumerate(engines):
            got = e.step(1)
            assert got == want, f"engine {x}, round {r}: gpu {got} != model {want}"
            compare(e, model, r, f"engine {x}")
        for f in lr.SUMMED:
            total[f] += want[f]
        if per_round:
            per_round(r, want)
    return total


def start(gs, case, **cfg_kw):
    eng = gs.Engine(gs.default_config(case["n"], **case["cfg"], **cfg_kw))
    eng.import_state(*sc.full_state(case["n"]), 0)
    return eng


# ---- zeros --------------------------------------------------------------------
def test_zero_arrays_change_nothing(gs, oracle_mod):
    """N=263, 12 rounds, a crash: an engine with all-zero thresholds, one with
    loss off and tablesim agree on everything; nothing is dropped and `sent`
    is the model's count of valid draws."""
    n, k, t, seed = 263, 3, 5, 0x5EED1263
    case = dict(n=n, cfg=dict(fanout=k, t_fail=t, t_cleanup=t, seed=seed), rounds=12,
                sched={3: [(sc.CRASH, 17), (sc.CRASH, 262)]})
    a, b = start(gs, case), start(gs, case)
    orc = oracle_mod.Oracle(oracle_mod.default_config(n, **case["cfg"]))
    orc.import_state(*sc.full_state(n), 0)
    model = lr.LossModel(n, k, t, t, seed)
    model.import_state(*sc.full_state(n), 0)
    model.set_loss(0.0, 0.0)
    try:
        assert a.loss()[0] is False
        a.set_loss(np.zeros(n, np.uint32), np.zeros(n, np.uint32))
        assert a.loss()[0] is True and b.loss()[0] is False
        for r in range(1, 13):
            ev = case["sched"].get(r)
            for e in (a, b, orc, model):
                if ev:
                    e.apply_events(ev)
            sa, sb, so, sm = a.step(1), b.step(1), orc.step(1), model.step(1)
            assert sa == sb == so == sm, r
            for x, y, z in zip(a.export_state(), b.export_state(), orc.export_state()):
                np.testing.assert_array_equal(x, y, err_msg=f"round {r}")
                np.testing.assert_array_equal(x, z, err_msg=f"round {r}")
            np.testing.assert_array_equal(a.read_failed(), b.read_failed())
            np.testing.assert_array_equal(a.read_failed(), orc.read_failed())
            np.testing.assert_array_equal(a.read_detectors(), b.read_detectors())
            sent, dropped = a.loss_stats()
            assert dropped == 0 and (sent, 0) == model.loss_stats(), r
        assert sent > 0
    finally:
        a.close()
        b.close()
        orc.close()


# ---- one engine, pull mode -------------------------------------------------------
def test_16bit_path_storm(gs):
    """N=250, k=3, T_fail = T_cleanup = 5, uniform 0.25 on both sides, 30
    rounds on the 16-bit path: false-positive storms."""
    case = CASES["storm16"]
    eng, model = start(gs, case), lr.model_of(case)
    try:
        assert eng.tier_info()[0] == 0
        eng.set_loss(case["out"], case["inn"])
        total = lockstep([eng], model, case)
        assert total["detections"] > 0
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["nib1000", "nib263", "nib1000_mute"])
def test_nibble_path(gs, monkeypatch, name):
    """GH_PLANE=1, k=4, T=16, 40 rounds in the 4-bit tier: uniform 0.10, a mute
    member, a deaf one (but in *_mute) and the 1% crash at round 8. The mute
    member is detected while it runs, REMOVE reaches it and it drops its own
    entry. The table is in the tier and the nibble path (variant 3) ran."""
    monkeypatch.setenv("GH_PLANE", "1")
    case = CASES[name]
    mute = int(np.flatnonzero(case["out"] == lr.ALWAYS)[0])
    eng, model = start(gs, case), lr.model_of(case)
    tier, variants, own = [], [], []

    def per_round(r, st):
        tier.append(eng.tier_info()[1])
        variants.append(eng.tier_info(full=True)[3])
        own.append((r, int(mute in model.failed()), int(model.hb[mute, mute])))

    try:
        assert eng.tier_info()[0] == 1
        eng.set_loss(case["out"], case["inn"])
        lockstep([eng], model, case, per_round=per_round)
        print(f"{name}: tier per round {tier}, variants {variants}")
        assert 1 in tier, tier
        assert 3 in variants, variants
        # (the model's table is the engine's, compared above)
        det = [r for r, f, _ in own if f]
        assert det and model.alive[mute], own
        assert any(h < 0 for r, _, h in own if r > det[0]), own
    finally:
        eng.close()


def test_second_peer_block(gs):
    """k=8, N=520, uniform 0.3, 15 rounds: draws 4..7 come from the second
    Philox block of the peer draws, their link blocks are 4..7."""
    case = CASES["k8"]
    eng, model = start(gs, case), lr.model_of(case)
    try:
        eng.set_loss(case["out"], case["inn"])
        lockstep([eng], model, case)
    finally:
        eng.close()


# ---- shards -----------------------------------------------------------------------
@pytest.mark.parametrize("world,layout", [(2, 0), (3, 0), (2, ROWS), (3, ROWS)],
                         ids=["cols2", "cols3", "rows2", "rows3"])
def test_shards(gs, monkeypatch, world, layout):
    """N=1,000 (the last shard's padded tail) over column and row shards, in
    lockstep with one engine and the model; loss_stats is the same, global
    pair on every rank."""
    monkeypatch.setenv("GH_PLANE", "1")
    case = CASES["shards"]
    one = start(gs, case)
    grp = gs.ShardGroup(gs.default_config(case["n"], shard_layout=layout, **case["cfg"]), world)
    model = lr.model_of(case)

    def per_round(r, st):
        ranks = grp.run("loss_stats")
        assert all(x == model.loss_stats() for x in ranks), (r, ranks, model.loss_stats())

    try:
        grp.import_state(*sc.full_state(case["n"]), 0)
        for e in (one, grp):
            e.set_loss(case["out"], case["inn"])
        lockstep([one, grp], model, case, per_round=per_round)
    finally:
        one.close()
        grp.close()


# ---- ring mode -----------------------------------------------------------------------
def ring_compare(eng, ls, n, r, lists):
    from oracle import listsim as L
    h1, t1, a1 = eng.export_state()
    h2, t2, a2 = ls.dense()
    np.testing.assert_array_equal(a1, a2, err_msg=f"alive r={r}")
    np.testing.assert_array_equal(h1, h2, err_msg=f"hb r={r}")
    np.testing.assert_array_equal(t1, sc.export_view(h2, t2, r, L.T_CLEANUP)[1], err_msg=f"ts r={r}")
    assert bits(eng.read_failed(), n) == ls.last_failed, r
    assert sorted(eng.read_detectors()) == sorted(ls.last_detectors), r
    assert eng.loss_stats() == ls.loss_stats(), r
    if lists:
        assert [list(eng.lsm(i)[0]) for i in range(n)] == [[m.addr for m in nd.members] for nd in ls.nodes], r


def ring_run(eng, ls, case, lists=False):
    for r in range(1, case["rounds"] + 1):
        ev = case["sched"].get(r)
        if ev:
            eng.apply_events(ev)
            ls.apply_events(ev)
        s1, s2 = eng.step(1), ls.step(1)
        assert s1 == s2, f"round {r}: gpu {s1} != ref {s2}"
        ring_compare(eng, ls, case["n"], r, lists)


@pytest.mark.parametrize("order", ["id", "append"])
@pytest.mark.parametrize("n", [24, 48])
def test_ring(gs, n, order):
    """Ring mode, one engine in member-ID and in append order, against the
    ListSim-based model (the lists too in append order)."""
    case = RING_CASES[n]
    eng = gs.Engine(gs.default_config(n, peer_mode=gs.GH_PEER_RING, seed=case["seed"],
                                      list_order=gs.GH_ORDER_APPEND if order == "append" else gs.GH_ORDER_ID))
    try:
        eng.import_state(*sc.full_state(n), 0)
        eng.set_loss(*ring_loss(case))
        ring_run(eng, ring_model(case, order), case, lists=order == "append")
    finally:
        eng.close()


def test_ring_row_shards(gs):
    """Ring mode at N=48 over two row shards: every shard builds every inbox,
    rank 0 counts the messages, every rank reports the global counters."""
    case = RING_CASES[48]
    grp = gs.ShardGroup(gs.default_config(48, peer_mode=gs.GH_PEER_RING, seed=case["seed"], shard_layout=ROWS), 2)
    try:
        grp.import_state(*sc.full_state(48), 0)
        grp.set_loss(*ring_loss(case))
        ring_run(grp, ring_model(case, "id"), case)
    finally:
        grp.close()


# ---- call shapes ------------------------------------------------------------------------
def test_call_shapes(gs):
    """step(5) calls against one round per call while the thresholds change
    between calls: off, out only, both sides (raw thresholds), off again, whose
    rounds are the zero-loss model's from that state. gh_set_loss zeroes the
    counters, gh_get_loss returns the arrays, gh_loss_stats refuses with loss
    off."""
    n, k, t, seed = 263, 4, 5, 0x5EED1C5
    case = dict(n=n, cfg=dict(fanout=k, t_fail=t, t_cleanup=t, seed=seed), sched={6: [(sc.CRASH, 100)]})
    rng = np.random.default_rng(5)
    raw_out = rng.integers(0, 1 << 31, n, dtype=np.uint32)
    raw_out[5], raw_out[6] = lr.ALWAYS, 0
    rates_in = rng.random(n) * 0.5
    phases = [None, (0.3, None), (raw_out, rates_in), (None, 0.2), None, None]
    a, b = start(gs, case), start(gs, case)
    model = lr.model_of(case, lossy=False)
    dropped_any = 0
    try:
        for ph, loss in enumerate(phases):
            for e in (a, b, model):
                e.set_loss(*(loss or (None, None)))
            en, o, i = b.loss()
            if loss is None:
                assert not en and not o.any() and not i.any()
                for e in (a, b):
                    with pytest.raises(gs.GossipError) as err:
                        e.loss_stats()
                    assert err.value.code == -1  # GH_EINVAL
            else:
                assert en and a.loss_stats() == b.loss_stats() == (0, 0)  # zeroed by every gh_set_loss
                np.testing.assert_array_equal(o, model.out)
                np.testing.assert_array_equal(i, model.inn)
            first = 5 * ph + 1
            ev = [x for r in range(first, first + 5) for x in case["sched"].get(r, [])]
            if ev:  # (queued events belong to the call's first round)
                assert first in case["sched"]
                b.apply_events(ev)
            total = lockstep([a], model, case, rounds=first + 4, first=first)
            got = b.step(5)
            assert {f: got[f] for f in lr.SUMMED} == total, (ph, got, total)
            compare(b, model, first + 4, "step(5) engine")
            if loss is not None:
                dropped_any += model.loss_stats()[1]
        assert dropped_any > 0
    finally:
        a.close()
        b.close()


# ---- the journal under loss ------------------------------------------------------------------
def test_journal_under_loss(gs):
    """GH_JOURNAL_DETECT over the 16-bit-path storm: the false positives the
    journal counts are the model's detections of running members, per round
    (false_failed) and summed over the members (fp_rounds)."""
    case = CASES["storm16"]
    eng = start(gs, case)
    false_failed = []
    model = lr.run_model(case, True, lambda m, st: false_failed.append(int(m.alive[m.failed()].sum())))
    try:
        eng.set_loss(case["out"], case["inn"])
        eng.journal_enable(gs.GH_JOURNAL_DETECT, 64)
        eng.step(case["rounds"])
        compare(eng, model, case["rounds"])
        log, j = eng.journal_rounds(), eng.journal()
        assert log["false_failed"].tolist() == false_failed
        assert int(j.fp_rounds.sum()) == sum(false_failed) > 0
    finally:
        eng.close()
