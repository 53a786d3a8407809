"""CPU checks of the ensemble tests' scenarios (tests/ensemble_ref.py) on
loss_ref.LossModel, so that the GPU parity runs of test_gpu_ensemble.py are not
vacuous: the pinned scenarios do what their names say, the scenario set as a
whole exercises every rule of the round, and the imported state holds the
edges it claims. Every literal is the model's."""
import numpy as np

import ensemble_ref as er


def trace_of(c):
    for name, cases in er.GROUPS.items():
        for x, y in enumerate(cases):
            if y is c:
                return er.group_trace(name)[x]
    raise KeyError


def test_healthy64():
    tr = trace_of(er.HEALTHY64)
    first, fp = tr[-1]["detect"]
    assert fp.sum() == 0 and er.total(tr, "false_failed") == 0
    assert {int(m): int(first[m]) for m in np.flatnonzero(first >= 0)} == {1: 15, 63: 15}
    assert er.total(tr, "dropped") == 3164
    assert min(rec["stats"]["active_rows"] for rec in tr) == 62


def test_collapse64():
    tr = trace_of(er.COLLAPSE64)
    assert er.total(tr, "detections") == 119
    assert er.total(tr, "false_failed") == 62 == int(tr[-1]["detect"][1].sum())
    assert er.total(tr, "remove_unknown") == 53
    assert min(rec["stats"]["active_rows"] for rec in tr) == 0


def test_crash128():
    tr = trace_of(er.CRASH128)
    assert [er.total(tr, f) for f in ("detections", "tombstoned", "released", "dropped")] == [19, 1431, 1446, 9253]


def test_small5():
    tr = trace_of(er.SMALL5)
    assert er.total(tr, "remove_unknown") == 4 and er.total(tr, "false_failed") == 4
    assert min(rec["stats"]["active_rows"] for rec in tr) == 1


def test_noloss33():
    tr = trace_of(er.NOLOSS33)
    assert er.total(tr, "dropped") == 0 and er.total(tr, "sent") > 0
    assert er.total(tr, "detections") == 64 and er.total(tr, "remove_unknown") == 93
    assert min(rec["stats"]["active_rows"] for rec in tr) == 0


def test_scenario_set_exercises_every_rule():
    traces = [tr for name in er.GROUPS for tr in er.group_trace(name)]
    for field in ("detections", "remove_unknown", "tombstoned", "released", "false_failed", "false_detections",
                  "dropped", "merged_cells"):
        assert sum(er.total(tr, field) for tr in traces) > 0, field
    # the guard bites: some round has fewer active rows than running ones
    assert any(rec["stats"]["active_rows"] < int(rec["alive"].sum()) for tr in traces for rec in tr)
    # every group's clusters differ from each other (seed, timeouts and loss are read per cluster)
    for name in er.GROUPS:
        a, b = er.group_trace(name)[:2] if len(er.GROUPS[name]) > 1 else (None, None)
        if a is not None and er.GROUPS[name][0]["n"] > 3:
            assert any(not np.array_equal(x["hb"], y["hb"]) or x["stats"] != y["stats"] for x, y in zip(a, b)), name


def test_groups_are_uniform():
    for name, cases in er.GROUPS.items():
        assert len({(c["n"], c["k"], c["rounds"], c["min_members"]) for c in cases}) == 1, name
    assert {c["n"] for cs in er.GROUPS.values() for c in cs} >= {2, 3, 4, 5, 16, 33, 64, 100, 128}
    assert {(c["n"], c["k"]) for cs in er.GROUPS.values() for c in cs} >= {(128, 4), (16, 1), (16, 8)}


def test_imported_state_holds_its_edges():
    t_fail = t_cleanup = 5
    hb, ts, alive = er.imported_state(24, t_fail, t_cleanup, 40)
    present = (hb >= 0).sum(1)
    assert sorted(set(present[:8].tolist())) == [0, 1, 2, 3, 4]
    own = hb[np.arange(24), np.arange(24)] >= 0
    for cnt in (1, 2, 3):  # with and without the row's own entry
        rows = np.flatnonzero(present[:8] == cnt)
        assert own[rows].any() and not own[rows].all(), cnt
    ages = sorted(set((41 - ts[hb == -2]).tolist()))
    assert ages == [t_cleanup - 1, t_cleanup, t_cleanup + 1]
    stale = (hb >= 0) & (ts < 41 - t_fail)
    assert {0, 1, 2} <= set(hb[stale & (alive[:, None] > 0)].tolist())
    assert alive[10] == 0 and alive.sum() == 23
    # the model run on it releases and detects, but never a stale cell with hb <= 1 (members 21, 22)
    c = er.case(24, 3, t_fail, t_cleanup, 0.1, 12, seed=0x5EED60)
    tr = er.run(er.model(c, (hb, ts, alive), 40), 12)
    assert tr[0]["stats"]["released"] > 0 and tr[0]["stats"]["detections"] > 0
    assert tr[0]["stats"]["active_rows"] < int(alive.sum())
    assert [m for m in range(24) if (int(tr[0]["failed"][0]) >> m) & 1] == [23]
