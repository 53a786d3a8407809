"""CPU checks of the ensemble modes (gh_ens_config.peer_mode / detect_mode, SPEC
§11): ensemble_modes_ref.ModeModel is pinned against the oracle (tablesim,
lossless) and against loss_ref.LossyListSim (the literal list replay, lossy
ring); the scenarios the GPU tests run reach what they are meant to reach; and
the ABI refuses unknown modes before a device is looked for."""
import ctypes as C

import numpy as np
import pytest

import ensemble_modes_ref as emr
import loss_ref as lr
import scenarios as sc


def oracle_of(n, ring, quirk, t_fail, t_cleanup, min_members, seed):
    from oracle import oracle as om
    return om.Oracle(om.default_config(n, fanout=3, t_fail=t_fail, t_cleanup=t_cleanup, seed=seed,
                                       min_members=min_members, peer_mode=int(ring), detect_mode=int(quirk)))


ORACLE_CASES = [  # (n, t_fail, t_cleanup, min_members, rounds, crashes)
    (10, 5, 5, 4, 30, {3: [4, 5, 6, 7]}),
    (16, 8, 6, 4, 30, {3: [5, 6, 7, 8]}),
    (24, 7, 9, 2, 36, {3: [1, 23], 9: [10, 11]}),
    (33, 16, 9, 4, 36, {3: [1, 32]}),
    (12, 3, 6, 0, 30, {2: [0, 1, 2], 8: [7]}),
    (70, 12, 12, 4, 26, {3: [61, 62, 63, 64, 65, 66]}),
]


@pytest.mark.parametrize("mode", list(emr.MODES))
@pytest.mark.parametrize("cfg", ORACLE_CASES, ids=[f"n{c[0]}m{c[3]}" for c in ORACLE_CASES])
def test_model_equals_oracle_lossless(mode, cfg):
    """Every round: tables, alive, all ten stats and the failed set."""
    ring, quirk = emr.MODES[mode]
    n, t_fail, t_cleanup, mm, rounds, crash = cfg
    seed = 0x5EEDA0 + n
    m = emr.ModeModel(n, 3, t_fail, t_cleanup, seed, mm, ring, quirk)
    o = oracle_of(n, ring, quirk, t_fail, t_cleanup, mm, seed)
    for e in (m, o):
        e.import_state(*sc.full_state(n), 0)
    for r in range(1, rounds + 1):
        if crash.get(r):
            ev = [(lr.CRASH, c) for c in crash[r]]
            m.apply_events(ev)
            o.apply_events(ev)
        assert m.step(1) == o.step(1), r
        for x, y in zip(m.export_state(), o.export_state()):
            assert np.array_equal(x, y), r
        assert np.array_equal(m.read_failed(), o.read_failed()), r
    o.close()


@pytest.mark.parametrize("state_mm", [4, 0])
@pytest.mark.parametrize("mode", list(emr.MODES))
def test_model_equals_oracle_on_the_hub_state(mode, state_mm):
    ring, quirk = emr.MODES[mode]
    n, r0 = 24, 20
    m = emr.ModeModel(n, 3, 5, 5, 0x5EEDB0, state_mm, ring, quirk)
    o = oracle_of(n, ring, quirk, 5, 5, state_mm, 0x5EEDB0)
    for e in (m, o):
        e.import_state(*emr.hub_state(n, r0), r0)
    for r in range(10):
        assert m.step(1) == o.step(1), r
        for x, y in zip(m.export_state(), o.export_state()):
            assert np.array_equal(x, y), r
    o.close()


@pytest.mark.parametrize("quirk", [False, True], ids=["canonical", "quirk"])
@pytest.mark.parametrize("name", ["n10", "n16", "n33"])
def test_model_equals_lossy_listsim(name, quirk):
    """Ring mode with loss on against the literal list replay (its T_fail =
    T_cleanup = 5 and min_members = 4 are constants)."""
    for c0 in emr.GROUPS[name]:
        c = dict(c0, t_fail=5, t_cleanup=5)
        n = c["n"]
        m = emr.model(c, True, quirk)
        ls = lr.LossyListSim.from_dense(*sc.full_state(n), 0, seed=c["seed"], peer_mode="ring", order="id", quirk=quirk)
        ls.set_loss(c["out"], c["inn"])
        for r in range(1, c["rounds"] + 1):
            if c["crash"].get(r):
                ev = [(lr.CRASH, x) for x in c["crash"][r]]
                m.apply_events(ev)
                ls.apply_events(ev)
            assert m.step(1) == ls.step(1), r
            hb, ts, alive = ls.dense()
            got = m.export_state()
            assert np.array_equal(got[0], hb) and np.array_equal(got[2], alive), r
            assert np.array_equal(got[1], sc.export_view(hb, ts, r, 5)[1]), r
            assert m.loss_stats() == ls.loss_stats(), r
        assert m.dropped > 0 or not c["out"].any()


# ---- the GPU scenarios are not vacuous ---------------------------------------------
def totals(name, mode):
    tr, ms = emr.group_models(name, *emr.MODES[mode])
    return {f: sum(emr.total(t, f) for t in tr) for f in emr.FIELDS if f != "last_round"}, ms


@pytest.mark.parametrize("mode", list(emr.MODES))
@pytest.mark.parametrize("name", ["n10", "n16", "n33", "n64", "n100", "n128"])
def test_scenarios_do_something(name, mode):
    tot, _ = totals(name, mode)
    for f in ("detections", "released", "merged_cells", "dropped", "tombstoned", "sent"):
        assert tot[f] > 0, (f, tot)


@pytest.mark.parametrize("mode", list(emr.MODES))
def test_scenarios_reach_remove_unknown(mode):
    assert sum(totals(name, mode)[0]["remove_unknown"] for name in ("n10", "n16", "n33", "n64")) > 0


@pytest.mark.parametrize("name", ["n10", "n16", "n64", "n128"])
def test_quirk_differs_from_canonical(name):
    a, b = emr.group_trace(name, True, False), emr.group_trace(name, True, True)
    assert any(x["stats"] != y["stats"] or not np.array_equal(x["hb"], y["hb"])
               for ta, tb in zip(a, b) for x, y in zip(ta, tb))
    ms = emr.group_models(name, True, True)[1]
    assert sum(m.diag["quirk_skipped"] for m in ms) > 0
    # pull mode: against the canonical pull traces of the same cases
    import ensemble_ref as er
    canon = [er.run(er.model(c), c["rounds"], c["crash"]) for c in emr.GROUPS[name]]
    quirk = emr.group_trace(name, False, True)
    assert any(x["stats"] != y["stats"] for ta, tb in zip(canon, quirk) for x, y in zip(ta, tb))
    assert sum(m.diag["quirk_skipped"] for m in emr.group_models(name, False, True)[1]) > 0


def test_issue_figures_at_n10():
    """Members 4..7 crashed in round 3 at N = 10, ring, lossless, 5 / 5, 40
    rounds: quirk detection makes 13 detections over 7 detection rounds,
    canonical 17 over 6."""
    c = emr.case(10, 3, 5, 5, 0.0, 40, {3: [4, 5, 6, 7]})
    for quirk, want in ((True, (13, 7)), (False, (17, 6))):
        tr = emr.run(emr.model(c, True, quirk), 40, c["crash"])
        det = [rec["stats"]["detections"] for rec in tr]
        assert (sum(det), sum(d > 0 for d in det)) == want


def test_hub_and_tiny_scenarios_reach_the_edges():
    n, r0 = 24, 20
    m = emr.ModeModel(n, 3, 5, 5, 0x5EEDB0, 0, True, True)
    m.import_state(*emr.hub_state(n, r0), r0)
    st = m.step(1)
    assert st["ring_empty"] == 1 and st["detections"] == 0
    assert m.diag["max_senders"] > 8 and m.diag["max_senders"] >= n - 7  # one receiver, more than pull's 8 slots
    assert m.diag["idx_absent"] > 0 and m.diag["short_repeat"] > 0
    m4 = emr.ModeModel(n, 3, 5, 5, 0x5EEDB0, 4, True, False)
    m4.import_state(*emr.hub_state(n, r0), r0)
    assert m4.step(1)["ring_empty"] == 0 and m4.diag["max_senders"] > 8 and m4.diag["idx_absent"] > 0
    for name in ("n3m2", "n2m1"):
        ms = emr.group_models(name, True, True)[1]
        assert sum(x.diag["short_repeat"] for x in ms) > 0, name
    assert sum(emr.total(t, "sent") for t in emr.group_trace("n4", True, False)) > 0


# ---- ABI, without a GPU --------------------------------------------------------------
@pytest.fixture(scope="module")
def abi():
    from conftest import PKG_DIR
    from gossipsim import _abi
    if not _abi.LIB_PATH.exists():
        import subprocess
        subprocess.run(["make", "-s", "-C", str(PKG_DIR)], check=True)
    _abi.load()
    return _abi


def params(abi, b):
    arr = (abi.EnsParams * b)()
    for x in range(b):
        arr[x] = abi.EnsParams(0x5EED0001 + x, 5, 5)
    return arr


def test_config_layout(abi):
    assert C.sizeof(abi.EnsConfig) == 32
    assert [n for n, _ in abi.EnsConfig._fields_][:7] == ["n_members", "n_clusters", "fanout", "min_members", "device",
                                                         "peer_mode", "detect_mode"]
    assert abi.EnsConfig.peer_mode.offset == 20 and abi.EnsConfig.detect_mode.offset == 24
    cfg = abi.EnsConfig(16, 2, 3, 4, 0)  # the five-field form is today's ensemble
    assert (cfg.peer_mode, cfg.detect_mode) == (abi.GH_PEER_PULL, abi.GH_DETECT_CANONICAL)
    assert abi.load().gh_abi_version() == 8


@pytest.mark.parametrize("field,value", [("peer_mode", 2), ("peer_mode", -1), ("detect_mode", 2), ("detect_mode", -1)])
def test_create_refuses_unknown_modes(abi, field, value):
    lib = abi.load()
    cfg = abi.EnsConfig(16, 2, 3, 4, 0)
    setattr(cfg, field, value)
    h = C.c_void_p(0x1234)
    assert lib.gh_ens_create(C.byref(cfg), params(abi, 2), C.byref(h)) == abi.GH_EINVAL
    assert not h.value
    from gossipsim import Ensemble, GossipError
    with pytest.raises(GossipError) as ei:
        Ensemble(16, 2, **{field: value})
    assert ei.value.code == abi.GH_EINVAL


def test_ring_mode_still_validates_fanout(abi):
    lib = abi.load()
    for k in (0, 9):
        cfg = abi.EnsConfig(16, 2, k, 4, 0, abi.GH_PEER_RING, abi.GH_DETECT_QUIRK)
        h = C.c_void_p()
        assert lib.gh_ens_create(C.byref(cfg), params(abi, 2), C.byref(h)) == abi.GH_EINVAL


def test_valid_modes_need_a_device(abi):
    """Without a gfx950 device every valid mode pair fails with GH_ENODEV: no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = abi.load()
    from gossipsim import Ensemble, GossipError
    for pm in (abi.GH_PEER_PULL, abi.GH_PEER_RING):
        for dm in (abi.GH_DETECT_CANONICAL, abi.GH_DETECT_QUIRK):
            cfg = abi.EnsConfig(16, 2, 3, 4, 0, pm, dm)
            cfg.reserved[0] = 77  # (the remaining reserved word is not checked)
            h = C.c_void_p()
            assert lib.gh_ens_create(C.byref(cfg), params(abi, 2), C.byref(h)) == abi.GH_ENODEV
            assert not h.value
            with pytest.raises(GossipError) as ei:
                Ensemble(16, 2, peer_mode=pm, detect_mode=dm)
            assert ei.value.code == abi.GH_ENODEV
