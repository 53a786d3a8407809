"""Cluster ensembles (gh_ens_*, SPEC §11) on the GPU, bit for bit against
loss_ref.LossModel (one model per cluster; tests/ensemble_ref.py holds the
scenarios and their shared traces, test_ensemble_ref.py checks them for
non-vacuity on the CPU) and against the product's own Engine at the same N.
Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import ensemble_ref as er
import loss_ref as lr
import scenarios as sc

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


def make(gs, cases, clusters=None):
    """An ensemble of the cases' clusters (cycled up to `clusters`), started full."""
    b = clusters or len(cases)
    cs = [cases[x % len(cases)] for x in range(b)]
    ens = gs.Ensemble(cs[0]["n"], b, fanout=cs[0]["k"], seeds=[c["seed"] for c in cs],
                      t_fail=[c["t_fail"] for c in cs], t_cleanup=[c["t_cleanup"] for c in cs],
                      min_members=cs[0]["min_members"])
    ens.init_full(2, 0, 0)
    ens.set_loss(np.stack([c["out"] for c in cs]), np.stack([c["inn"] for c in cs]))
    return ens, cs


def crash_round(ens, cs, r):
    for b, c in enumerate(cs):
        if c["crash"].get(r):
            ens.crash(c["crash"][r], cluster=b)


def check_round(ens, st, traces, q, what):
    """The ensemble after round q + 1 of every cluster against traces[b][q]."""
    hb, ts, alive, rnd = ens.export_state()
    failed = ens.failed()
    first, fp = ens.detect()
    for b, tr in enumerate(traces):
        rec = tr[q]
        tag = f"{what} cluster {b} round {rec['round']}"
        assert rnd[b] == rec["round"], tag
        assert np.array_equal(alive[b], rec["alive"]), tag
        assert np.array_equal(hb[b], rec["hb"]), tag
        assert np.array_equal(ts[b], rec["ts"]), tag
        got = {f: int(st[f][b]) for f in er.FIELDS}
        assert got == rec["stats"], tag
        assert np.array_equal(failed[b], rec["failed"]), tag
        assert np.array_equal(first[b], rec["detect"][0]) and np.array_equal(fp[b], rec["detect"][1]), tag


# ---- 1. per-round parity with LossModel (and 6., the detect record) ----------
@pytest.mark.parametrize("name", list(er.GROUPS))
def test_per_round_parity(gs, name):
    cases, traces = er.GROUPS[name], er.group_trace(name)
    ens, cs = make(gs, cases)
    with ens:
        for q in range(cases[0]["rounds"]):
            crash_round(ens, cs, q + 1)
            check_round(ens, ens.step(1), traces, q, name)


# ---- 2. one launch, many rounds ----------------------------------------------
@pytest.mark.parametrize("name", ["n64k3", "n128k4"])
def test_one_launch_equals_single_rounds(gs, name):
    """step(R) once = R x step(1): tables, summed stats, detect record. The
    crashes of the first scheduled round are queued before round 1 in both runs
    (events apply at the next round run), so the reference here is the
    ensemble's own single-round run, itself pinned to LossModel above."""
    cases = er.GROUPS[name]
    rounds = cases[0]["rounds"]
    outs = []
    for chunks in ([1] * rounds, [rounds], [7, rounds - 7]):
        ens, cs = make(gs, cases)
        with ens:
            for b, c in enumerate(cs):
                for ms in c["crash"].values():
                    ens.crash(ms, cluster=b)
            tot = {f: np.zeros(len(cs), np.int64) for f in er.FIELDS}
            for n in chunks:
                st = ens.step(n)
                assert (st["rounds"] == n).all()
                for f in er.FIELDS:
                    tot[f] = st[f] if f == "last_round" else tot[f] + st[f]
            outs.append((ens.export_state(), tot, ens.failed(), ens.detect()))
    # the scenarios did something in this form too (with every crash in round 1 all rows detect at
    # once, so REMOVE finds tombstones already; the pending set still decides who is a sole detector)
    assert outs[0][1]["detections"].sum() > 0 and outs[0][1]["released"].sum() > 0
    assert outs[0][1]["merged_cells"].sum() > 0
    for other in outs[1:]:
        for x, y in zip(outs[0][0], other[0]):
            assert np.array_equal(x, y)
        for f in er.FIELDS:
            assert np.array_equal(outs[0][1][f], other[1][f]), f
        assert np.array_equal(outs[0][2], other[2])
        assert all(np.array_equal(x, y) for x, y in zip(outs[0][3], other[3]))


def test_one_launch_matches_model(gs):
    """The N=64 collapsing scenario with its crashes queued up front, run as one
    step(40), against LossModel run the same way."""
    c = er.COLLAPSE64
    m = er.model(c)
    m.apply_events([(lr.CRASH, x) for ms in c["crash"].values() for x in ms])
    tr = er.run(m, c["rounds"])
    ens, _ = make(gs, [c])
    with ens:
        for ms in c["crash"].values():
            ens.crash(ms)
        st = ens.step(c["rounds"])
        hb, ts, alive, rnd = ens.export_state()
        assert np.array_equal(hb[0], tr[-1]["hb"]) and np.array_equal(ts[0], tr[-1]["ts"])
        assert np.array_equal(alive[0], tr[-1]["alive"]) and rnd[0] == c["rounds"]
        for f in er.FIELDS:
            want = tr[-1]["stats"][f] if f == "last_round" else er.total(tr, f)
            assert int(st[f][0]) == want, f
        first, fp = ens.detect()
        assert np.array_equal(first[0], tr[-1]["detect"][0]) and np.array_equal(fp[0], tr[-1]["detect"][1])
        assert fp.sum() > 0


# ---- 3. parity with the product's own Engine -----------------------------------
def test_engine_parity(gs):
    cases = [er.HEALTHY64, er.COLLAPSE64]
    ens, cs = make(gs, cases)
    engines = []
    for c in cs:
        e = gs.Engine(gs.default_config(64, fanout=c["k"], t_fail=c["t_fail"], t_cleanup=c["t_cleanup"], seed=c["seed"]))
        e.import_state(*sc.full_state(64), 0)
        e.set_loss(c["out"], c["inn"])
        engines.append(e)
    sent = [0, 0]
    dropped = [0, 0]
    with ens:
        for r in range(1, 41):
            crash_round(ens, cs, r)
            st = ens.step(1)
            hb, ts, alive, _ = ens.export_state()
            failed = ens.failed()
            for b, (c, e) in enumerate(zip(cs, engines)):
                if c["crash"].get(r):
                    e.apply_events([(gs.GH_EV_CRASH, m) for m in c["crash"][r]])
                est = e.step(1)
                assert {f: int(st[f][b]) for f in lr.STATS} == est, (b, r)
                for x, y in zip((hb[b], ts[b], alive[b]), e.export_state()):
                    assert np.array_equal(x, y), (b, r)
                assert np.array_equal(failed[b], e.read_failed()), (b, r)
                s, d = e.loss_stats()
                assert (int(st["sent"][b]), int(st["dropped"][b])) == (s - sent[b], d - dropped[b]), (b, r)
                sent[b], dropped[b] = s, d
    for e in engines:
        e.close()
    assert dropped[0] == 3164


# ---- 4. independence and grid reuse ---------------------------------------------
@pytest.mark.parametrize("grid", [None, 7], ids=["resident", "grid7"])
def test_more_clusters_than_the_grid(gs, monkeypatch, grid):
    """B = 600 clusters at N = 16, more than the card has CUs; parameters cycle
    over three sets. Equal parameters give bit-identical clusters, one of each
    set equals LossModel, and the same parameters at B = 1 give the same. A
    CU holds several workgroups of this size, so the card may still take all
    600 at once: the second case caps the grid at 7 workgroups (GH_ENS_GRID),
    each of which then walks 85 or 86 clusters."""
    if grid:
        monkeypatch.setenv("GH_ENS_GRID", str(grid))
    else:
        monkeypatch.delenv("GH_ENS_GRID", raising=False)
    sets = [er.case(16, 3, 5, 5, 0.2, 25, {4: [3]}, seed=0x5EED70),
            er.case(16, 3, 8, 6, 0.05, 25, {2: [0, 15]}, seed=0x5EED71),
            er.case(16, 3, 3, 9, 0.4, 25, seed=0x5EED72, mute=7)]
    rounds = 25

    def run(cases, b):
        ens, cs = make(gs, cases, b)
        with ens:
            tot = None
            for r in range(1, rounds + 1):  # in three launches, the crashes at their rounds
                crash_round(ens, cs, r)
                if r in (1, 2, 4):
                    st = ens.step({1: 1, 2: 2, 4: rounds - 3}[r])
                    tot = st if tot is None else {f: (st[f] if f == "last_round" else tot[f] + st[f]) for f in st}
            return ens.export_state(), tot, ens.detect()

    (hb, ts, alive, rnd), tot, (first, fp) = run(sets, 600)
    assert (rnd == rounds).all()
    for x, c in enumerate(sets):
        same = np.arange(x, 600, 3)
        for arr in (hb, ts, alive, first, fp):
            assert (arr[same] == arr[x]).all(), x
        for f in er.FIELDS:
            assert (tot[f][same] == tot[f][x]).all(), (x, f)
        tr = er.run(er.model(c), rounds, c["crash"])
        assert np.array_equal(hb[x], tr[-1]["hb"]) and np.array_equal(ts[x], tr[-1]["ts"])
        assert np.array_equal(alive[x], tr[-1]["alive"])
        for f in er.FIELDS:
            assert int(tot[f][x]) == (tr[-1]["stats"][f] if f == "last_round" else er.total(tr, f)), (x, f)
        (hb1, ts1, alive1, _), tot1, (first1, fp1) = run([c], 1)
        assert np.array_equal(hb1[0], hb[x]) and np.array_equal(ts1[0], ts[x]) and np.array_equal(alive1[0], alive[x])
        assert np.array_equal(first1[0], first[x]) and np.array_equal(fp1[0], fp[x])
        assert all(int(tot1[f][0]) == int(tot[f][x]) for f in er.FIELDS)
    assert not np.array_equal(hb[0], hb[1]) and not np.array_equal(hb[1], hb[2])


# ---- 5. imported states -----------------------------------------------------------
def test_imported_state(gs):
    n, r0, rounds = 24, 40, 12
    cases = [er.case(n, 3, 6, 6, 0.1, rounds, {r0 + 3: [2]}, seed=0x5EED61),
             er.case(n, 3, 5, 5, 0.1, rounds, seed=0x5EED60),
             er.case(n, 3, 7, 4, 0.2, rounds, {r0 + 2: [23]}, seed=0x5EED62)]
    state = er.imported_state(n, 5, 5, r0)
    full = sc.full_state(n, 30, r0 - 1)
    traces = [er.run(er.model(c, state if b == 1 else full, r0), rounds, c["crash"]) for b, c in enumerate(cases)]
    ens, cs = make(gs, cases)
    with ens:
        ens.init_full(30, r0 - 1, r0)
        ens.step(0)  # (runs nothing)
        ens.import_state(1, *state, r0)
        hb, ts, alive, rnd = ens.export_state(1, 1)
        m = er.model(cases[1], state, r0)
        for x, y in zip((hb[0], ts[0], alive[0]), m.export_state()):
            assert np.array_equal(x, y)
        assert rnd[0] == r0
        for q in range(rounds):
            crash_round(ens, cs, r0 + q + 1)
            check_round(ens, ens.step(1), traces, q, "import")
    assert sum(er.total(traces[1], f) for f in ("released", "detections", "remove_unknown")) > 0


def test_import_clears_pending_and_record(gs):
    """A cluster re-imported mid-run forgets its pending REMOVE set and its
    detect record; its neighbour goes on undisturbed; loss persists."""
    c = er.COLLAPSE64
    ens, cs = make(gs, [c, c])
    with ens:
        for r in range(1, 13):
            crash_round(ens, cs, r)
            ens.step(1)
        assert ens.failed()[0].any() and (ens.detect()[0][0] >= 0).any()
        ens.import_state(0, *sc.full_state(64), 0)
        assert not ens.failed()[0].any() and ens.failed()[1].any()
        first, fp = ens.detect()
        assert (first[0] == -1).all() and (fp[0] == 0).all() and (first[1] >= 0).any()
        tr = er.group_trace("n64k3")[1]
        st = ens.step(1)
        assert {f: int(st[f][0]) for f in er.FIELDS} == tr[0]["stats"]  # round 1 again, the same lossy links
        assert {f: int(st[f][1]) for f in er.FIELDS} == tr[12]["stats"]


# ---- 7. GH_ERANGE and GH_EINVAL on a live handle -------------------------------------
def test_step_refuses_heartbeat_overflow(gs):
    from gossipsim import _abi
    ens = gs.Ensemble(8, 2, t_fail=50, t_cleanup=50)
    with ens:
        ens.init_full(INT32_MAX - 3, 0, 0)
        st = ens.step(2)
        assert (st["rounds"] == 2).all()
        before = ens.export_state()
        assert before[0].max() == INT32_MAX - 1
        with pytest.raises(gs.GossipError) as ei:
            ens.step(5)
        assert ei.value.code == _abi.GH_ERANGE
        for x, y in zip(before, ens.export_state()):
            assert np.array_equal(x, y)
        assert (ens.step(1)["rounds"] == 1).all()  # up to INT32_MAX itself
        assert ens.export_state()[0].max() == INT32_MAX
        with pytest.raises(gs.GossipError) as ei:
            ens.step(1)
        assert ei.value.code == _abi.GH_ERANGE
        hb = np.full((8, 8), 2, np.int32)
        hb[3, 3] = -3
        with pytest.raises(gs.GossipError) as ei:
            ens.import_state(0, hb, np.zeros((8, 8), np.int32), np.ones(8, np.uint8), 0)
        assert ei.value.code == _abi.GH_ERANGE


def test_bad_arguments_on_a_handle(gs):
    from gossipsim import _abi
    ens = gs.Ensemble(8, 3)
    with ens:
        ens.init_full()
        state = sc.full_state(8)
        for bad in (-1, 3):
            with pytest.raises(gs.GossipError) as ei:
                ens.import_state(bad, *state, 0)
            assert ei.value.code == _abi.GH_EINVAL
        for cl in (-2, 3):
            with pytest.raises(gs.GossipError) as ei:
                ens.crash([1], cluster=cl)
            assert ei.value.code == _abi.GH_EINVAL
        for member in (-1, 8):
            with pytest.raises(gs.GossipError) as ei:
                ens.crash([member])
            assert ei.value.code == _abi.GH_EINVAL
        # a JOIN or LEAVE anywhere in the list: refused, and the crash beside it is not queued
        for kind in (gs.GH_EV_JOIN, gs.GH_EV_LEAVE):
            with pytest.raises(gs.GossipError) as ei:
                ens.apply_events([(gs.GH_EV_CRASH, 2), (kind, 3)])
            assert ei.value.code == _abi.GH_EINVAL
        with pytest.raises(gs.GossipError):
            ens.export_state(2, 2)
        with pytest.raises(gs.GossipError) as ei:
            ens.step(-1)
        assert ei.value.code == _abi.GH_EINVAL
        ens.step(1)
        assert ens.export_state()[2].all()  # nobody crashed
