"""CPU checks of the lossy-link models (tests/loss_ref.py) and of the three
gh_*loss* entry points that need no device.

The numpy model with all thresholds zero is tablesim, round for round, stats
included; the ring model with all thresholds zero is ListSim; hit() at its
edges; the vectorised Philox is the pure-Python B(); and every lossy scenario
the GPU tests run (test_gpu_loss.py) is non-vacuous in the model: messages are
dropped, the final tables differ from the zero-loss run, and in the two
false-positive cases a running member is detected."""
import ctypes as C

import numpy as np
import pytest

import loss_ref as lr
import scenarios as sc


def crash_sched(n, seed, at=8):
    return {at: [(sc.CRASH, int(c)) for c in sc.crash_ids(n, 0.01, seed)]}


@pytest.mark.parametrize("n,k,t,crash", [(250, 3, 5, False), (1000, 4, 16, True)], ids=["n250", "n1000_crash"])
def test_zero_thresholds_equal_tablesim(oracle_mod, n, k, t, crash):
    om = oracle_mod
    seed = 0x5EED0100 + n
    rounds = 30 if crash else 20
    sched = crash_sched(n, seed) if crash else {}
    orc = om.Oracle(om.default_config(n, fanout=k, t_fail=t, t_cleanup=t, seed=seed))
    mod = lr.LossModel(n, k, t, t, seed)
    for e in (orc, mod):
        e.import_state(*sc.full_state(n), 0)
    mod.set_loss(np.zeros(n, np.uint32), None)
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
    sent, dropped = mod.loss_stats()
    assert sent > 0 and dropped == 0
    orc.close()


@pytest.mark.parametrize("order", ["id", "append"])
def test_zero_thresholds_equal_listsim(order):
    from oracle.listsim import ListSim
    n = 24
    hb, ts, alive = sc.full_state(n)
    kw = dict(seed=0x5EED0124, peer_mode="ring", order=order)
    a = ListSim.from_dense(hb, ts, alive, 0, **kw)
    b = lr.LossyListSim.from_dense(hb, ts, alive, 0, **kw)
    b.set_loss(None, np.zeros(n, np.uint32))
    sched = {3: [(sc.CRASH, 5), (sc.CRASH, 6)], 14: [(sc.JOIN, 5)], 16: [(sc.LEAVE, 11)]}
    for r in range(1, 31):
        for e in (a, b):
            if sched.get(r):
                e.apply_events(sched[r])
        assert a.step(1) == b.step(1), r
        for x, y in zip(a.dense(), b.dense()):
            np.testing.assert_array_equal(x, y, err_msg=f"round {r}")
        assert [[m.addr for m in nd.members] for nd in a.nodes] == [[m.addr for m in nd.members] for nd in b.nodes]
    sent, dropped = b.loss_stats()
    assert sent > 0 and dropped == 0


def test_hit_edges():
    top = 0xFFFFFFFF
    assert not lr.hit(0, 0) and not lr.hit(0, top)          # 0 never drops
    assert lr.hit(1, 0) and not lr.hit(1, 1) and not lr.hit(1, top)
    assert lr.hit(top, 0) and lr.hit(top, top - 1) and lr.hit(top, top)  # always, the draw 2^32 - 1 included
    assert not lr.hit(top - 1, top - 1) and lr.hit(top - 1, top - 2)
    w = np.array([0, 1, top - 1, top], np.uint64)
    assert lr.hits(np.uint32(0), w).tolist() == [False] * 4
    assert lr.hits(np.uint32(1), w).tolist() == [True, False, False, False]
    assert lr.hits(np.uint32(top), w).tolist() == [True] * 4
    assert (lr.q32(0.0), lr.q32(1.0), lr.q32(0.5), lr.q32(2.0 ** -32)) == (0, top, 1 << 31, 1)


def test_vector_philox_is_B():
    from oracle import philox
    seed = 0x5EED0001_0000BEEF
    a = np.array([0, 1, 7, 999, 65535, 2 ** 32 - 1])[:, None]
    blk = np.arange(8)[None, :]
    w = lr.blocks(seed, a, 37, lr.TAG_LINK, blk)
    for x, av in enumerate(a[:, 0]):
        for b in range(8):
            assert tuple(int(w[j][x, b]) for j in range(4)) == lr.B(seed, int(av), 37, b)
    # ... and the peer draws of the model are oracle.philox.peer
    m = lr.LossModel(263, 8, seed=seed)
    P = m.peers(5)
    for i in (0, 1, 131, 262):
        assert P[i].tolist() == [philox.peer(seed, i, 5, t, 263) for t in range(8)]


# ---- the three entry points without a device --------------------------------
@pytest.fixture(scope="module")
def lib():
    from gossipsim import _abi
    return _abi.load(), _abi


def test_loss_symbols_exported(lib):
    L, abi = lib
    raw = C.CDLL(str(abi.LIB_PATH))
    bound = {n for n, _, _ in abi.SYMBOLS}
    for name in ("gh_set_loss", "gh_get_loss", "gh_loss_stats"):
        assert hasattr(raw, name) and name in bound
    assert (abi.GH_LOSS_NEVER, abi.GH_LOSS_ALWAYS) == (0, 0xFFFFFFFF)


def test_loss_null_handle(lib):
    L, abi = lib
    a = (C.c_uint32 * 8)()
    en, s, d = C.c_int32(7), C.c_int64(7), C.c_int64(7)
    assert L.gh_set_loss(None, a, a) == abi.GH_EINVAL
    assert L.gh_set_loss(None, None, None) == abi.GH_EINVAL
    assert L.gh_get_loss(None, C.byref(en), a, a) == abi.GH_EINVAL
    assert L.gh_loss_stats(None, C.byref(s), C.byref(d)) == abi.GH_EINVAL
    assert (en.value, s.value, d.value) == (7, 7, 7)


# ---- the GPU tests' scenarios are non-vacuous in the model ------------------
def test_scenarios_non_vacuous():
    import test_gpu_loss as tg
    for name, case in tg.CASES.items():
        fp = []

        def watch(m, st):
            fp.append(int(m.alive[m.failed()].sum()))

        lossy = lr.run_model(case, True, watch)
        clean = lr.run_model(case, False)
        sent, dropped = lossy.loss_stats()
        assert 0 < dropped < sent, name
        assert not np.array_equal(lossy.hb, clean.hb), name
        if case.get("false_positives"):
            assert sum(fp) > 0, name


@pytest.mark.parametrize("order", ["id", "append"])
def test_ring_scenarios_non_vacuous(order):
    import test_gpu_loss as tg
    for n, case in tg.RING_CASES.items():
        lossy, clean = tg.ring_model(case, order), tg.ring_model(case, order, lossy=False)
        for r in range(1, case["rounds"] + 1):
            for m in (lossy, clean):
                if case["sched"].get(r):
                    m.apply_events(case["sched"][r])
                m.step(1)
        sent, dropped = lossy.loss_stats()
        assert 0 < dropped < sent, n
        assert not np.array_equal(lossy.dense()[0], clean.dense()[0]), n
