"""The ensemble modes (gh_ens_config.peer_mode / detect_mode, SPEC §11) on the
GPU: ring gossip and quirk detection, bit for bit against
ensemble_modes_ref.ModeModel (pinned to the oracle and to the list replay in
test_ensemble_modes_ref.py, which also shows the scenarios are not vacuous)
and against the product's own Engine in the same modes.
Run on a MI355X: pytest -m gpu."""
import numpy as np
import pytest

import ensemble_modes_ref as emr
import ensemble_ref as er
import loss_ref as lr
import scenarios as sc

pytestmark = pytest.mark.gpu

MODE_IDS = list(emr.MODES)


@pytest.fixture(scope="module")
def gs():
    import gossipsim
    return gossipsim


def make(gs, cases, ring, quirk, clusters=None, full=True):
    """An ensemble of the cases' clusters (cycled up to `clusters`) in the given modes."""
    b = clusters or len(cases)
    cs = [cases[x % len(cases)] for x in range(b)]
    ens = gs.Ensemble(cs[0]["n"], b, fanout=cs[0]["k"], seeds=[c["seed"] for c in cs],
                      t_fail=[c["t_fail"] for c in cs], t_cleanup=[c["t_cleanup"] for c in cs],
                      min_members=cs[0]["min_members"], peer_mode=gs.GH_PEER_RING if ring else gs.GH_PEER_PULL,
                      detect_mode=gs.GH_DETECT_QUIRK if quirk else gs.GH_DETECT_CANONICAL)
    assert (ens.peer_mode, ens.detect_mode) == (int(ring), int(quirk))
    if full:
        ens.init_full(2, 0, 0)
    ens.set_loss(np.stack([c["out"] for c in cs]), np.stack([c["inn"] for c in cs]))
    return ens, cs


def crash_round(ens, cs, r):
    for b, c in enumerate(cs):
        if c["crash"].get(r):
            ens.crash(c["crash"][r], cluster=b)


def check_round(ens, st, traces, q, what):
    """The ensemble after round q + 1 of every cluster against traces[b][q]:
    tables, alive, all 14 stats, the failed bitmap, the detect record."""
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
        got = {f: int(st[f][b]) for f in emr.FIELDS}
        assert got == rec["stats"], tag
        assert np.array_equal(failed[b], rec["failed"]), tag
        assert np.array_equal(first[b], rec["detect"][0]) and np.array_equal(fp[b], rec["detect"][1]), tag


def parity(gs, name, mode):
    ring, quirk = emr.MODES[mode]
    cases, traces = emr.GROUPS[name], emr.group_trace(name, ring, quirk)
    ens, cs = make(gs, cases, ring, quirk)
    with ens:
        for q in range(cases[0]["rounds"]):
            crash_round(ens, cs, q + 1)
            check_round(ens, ens.step(1), traces, q, f"{name} {mode}")


# ---- 1. per-round parity with the model ----------------------------------------------
@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("name", ["n10", "n16", "n33", "n64", "n100", "n128"])
def test_per_round_parity(gs, name, mode):
    parity(gs, name, mode)


# ---- 2. tiny lists ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("name", list(emr.TINY))
def test_tiny_lists(gs, name, mode):
    parity(gs, name, mode)


# ---- 3. the imported hub state ---------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_IDS)
@pytest.mark.parametrize("min_members", [4, 0])
@pytest.mark.parametrize("n", [24, 128])
def test_hub_state(gs, n, min_members, mode):
    """Every row lists {0, 1, 2, itself}: members 0..2 each get about N - 3
    senders in one round; a row without its own entry, an empty row (a
    ring_empty sender at min_members 0), a row of itself alone, a stopped row."""
    ring, quirk = emr.MODES[mode]
    r0, rounds = 20, 9
    cases = [er.case(n, 3, 5, 5, 0.0, rounds, seed=0x5EEDC0, min_members=min_members),
             er.case(n, 3, 4, 6, 0.2, rounds, {r0 + 2: [1]}, seed=0x5EEDC1, min_members=min_members, mute=0, deaf=2)]
    state = emr.hub_state(n, r0)
    models = [emr.model(c, ring, quirk, state, r0) for c in cases]
    traces = [emr.run(m, rounds, c["crash"]) for m, c in zip(models, cases)]
    if ring:
        assert models[0].diag["max_senders"] >= n - 7 and models[0].diag["idx_absent"] > 0
        # (the empty row sends only without the guard; later rounds can empty an active row by detection)
        assert traces[0][0]["stats"]["ring_empty"] == (min_members == 0)
    ens, cs = make(gs, cases, ring, quirk, full=False)
    with ens:
        for b in range(len(cs)):
            ens.import_state(b, *state, r0)
        for q in range(rounds):
            crash_round(ens, cs, r0 + q + 1)
            check_round(ens, ens.step(1), traces, q, f"hub n{n} m{min_members} {mode}")


# ---- 4. parity with the product's own Engine ---------------------------------------------
@pytest.mark.parametrize("mode", ["ring-canonical", "ring-quirk"])
@pytest.mark.parametrize("name,clusters", [("n64", 2), ("n10", 1)], ids=["n64x2", "n10"])
def test_engine_parity(gs, name, clusters, mode):
    ring, quirk = emr.MODES[mode]
    cases = emr.GROUPS[name][1:1 + clusters]
    n, rounds = cases[0]["n"], cases[0]["rounds"]
    ens, cs = make(gs, cases, ring, quirk)
    engines = []
    for c in cs:
        e = gs.Engine(gs.default_config(n, fanout=c["k"], t_fail=c["t_fail"], t_cleanup=c["t_cleanup"], seed=c["seed"],
                                        peer_mode=int(ring), detect_mode=int(quirk)))
        e.import_state(*sc.full_state(n), 0)
        e.set_loss(c["out"], c["inn"])
        engines.append(e)
    sent = [0] * len(cs)
    dropped = [0] * len(cs)
    with ens:
        for r in range(1, rounds + 1):
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
    assert sum(dropped) > 0


# ---- 5. one launch equals single rounds ----------------------------------------------------
@pytest.mark.parametrize("name", ["n64", "n128"])
def test_one_launch_equals_single_rounds(gs, name):
    """Ring / quirk: step(R) once = R x step(1) = step(7) + step(R - 7). Every
    crash is queued before round 1 in all three runs; the single-round run is
    pinned to the model run the same way."""
    cases = emr.GROUPS[name]
    rounds = cases[0]["rounds"]
    outs = []
    for chunks in ([1] * rounds, [rounds], [7, rounds - 7]):
        ens, cs = make(gs, cases, True, True)
        with ens:
            for b, c in enumerate(cs):
                for ms in c["crash"].values():
                    ens.crash(ms, cluster=b)
            tot = {f: np.zeros(len(cs), np.int64) for f in emr.FIELDS}
            for n in chunks:
                st = ens.step(n)
                assert (st["rounds"] == n).all()
                for f in emr.FIELDS:
                    tot[f] = st[f] if f == "last_round" else tot[f] + st[f]
            outs.append((ens.export_state(), tot, ens.failed(), ens.detect()))
    for b, c in enumerate(cases):
        m = emr.model(c, True, True)
        m.apply_events([(lr.CRASH, x) for ms in c["crash"].values() for x in ms])
        tr = emr.run(m, rounds)
        assert np.array_equal(outs[0][0][0][b], tr[-1]["hb"]) and np.array_equal(outs[0][0][1][b], tr[-1]["ts"])
        for f in emr.FIELDS:
            want = tr[-1]["stats"][f] if f == "last_round" else emr.total(tr, f)
            assert int(outs[0][1][f][b]) == want, (b, f)
    assert outs[0][1]["detections"].sum() > 0 and outs[0][1]["merged_cells"].sum() > 0
    for other in outs[1:]:
        for x, y in zip(outs[0][0], other[0]):
            assert np.array_equal(x, y)
        for f in emr.FIELDS:
            assert np.array_equal(outs[0][1][f], other[1][f]), f
        assert np.array_equal(outs[0][2], other[2])
        assert all(np.array_equal(x, y) for x, y in zip(outs[0][3], other[3]))


# ---- 6. more clusters than the grid ----------------------------------------------------------
def test_more_clusters_than_the_grid(gs, monkeypatch):
    """B = 40 ring clusters on 7 workgroups (GH_ENS_GRID): each walks 5 or 6
    clusters; equal parameters give equal clusters and each set equals the model."""
    monkeypatch.setenv("GH_ENS_GRID", "7")
    cases = emr.GROUPS["n16"]
    rounds = cases[0]["rounds"]
    traces = emr.group_trace("n16", True, True)
    ens, cs = make(gs, cases, True, True, clusters=40)
    with ens:
        tot = None
        for r in range(1, rounds + 1):  # in three launches, the crashes at their rounds
            crash_round(ens, cs, r)
            if r in (1, 3, 4):
                st = ens.step({1: 2, 3: 1, 4: rounds - 3}[r])
                tot = st if tot is None else {f: (st[f] if f == "last_round" else tot[f] + st[f]) for f in st}
        hb, ts, alive, rnd = ens.export_state()
        first, fp = ens.detect()
    assert (rnd == rounds).all()
    for x in range(40):
        tr = traces[x % len(cases)]
        assert np.array_equal(hb[x], tr[-1]["hb"]) and np.array_equal(ts[x], tr[-1]["ts"]), x
        assert np.array_equal(alive[x], tr[-1]["alive"]), x
        assert np.array_equal(first[x], tr[-1]["detect"][0]) and np.array_equal(fp[x], tr[-1]["detect"][1]), x
        for f in emr.FIELDS:
            assert int(tot[f][x]) == (tr[-1]["stats"][f] if f == "last_round" else emr.total(tr, f)), (x, f)


# ---- 7. zero modes are today's ensemble -------------------------------------------------------
def test_zero_modes_are_pull_canonical(gs):
    cases, traces = er.GROUPS["n64k3"], er.group_trace("n64k3")
    ens, cs = make(gs, cases, False, False)
    assert (ens.cfg.peer_mode, ens.cfg.detect_mode) == (0, 0)
    with ens:
        for q in range(cases[0]["rounds"]):
            crash_round(ens, cs, q + 1)
            check_round(ens, ens.step(1), traces, q, "zero modes")
