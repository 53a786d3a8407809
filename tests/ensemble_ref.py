"""Scenarios and reference traces of the cluster-ensemble tests (gh_ens_*, SPEC
§11), for the tests only. The reference is loss_ref.LossModel, one model per
cluster: the trace of a case records, after every round, what the ensemble
must show for that cluster. Traces are computed once per process and shared
(test_ensemble_ref.py checks them on the CPU, test_gpu_ensemble.py compares the
GPU against them); nobody writes into a trace."""
from __future__ import annotations

import functools

import numpy as np

import loss_ref as lr
from scenarios import full_state

SEED = 0x5EED47
FIELDS = lr.STATS + ("false_failed", "false_detections", "sent", "dropped")


def case(n, k, t_fail, t_cleanup, rate, rounds, crash=None, seed=SEED, mute=None, deaf=None, min_members=4):
    """A cluster from a full start (hb 2, ts 0, round 0): uniform drop `rate`
    on both sides, optionally one member with out = ALWAYS (mute) and one with
    in = ALWAYS (deaf), crashes {round: [members]}. min_members is the
    ensemble's: the same in every case of a group."""
    out = np.full(n, lr.q32(rate), np.uint32)
    inn = out.copy()
    if mute is not None:
        out[mute] = lr.ALWAYS
    if deaf is not None:
        inn[deaf] = lr.ALWAYS
    return dict(n=n, k=k, t_fail=t_fail, t_cleanup=t_cleanup, seed=seed, out=out, inn=inn, rounds=rounds,
                min_members=min_members,
                crash={int(r): [int(m) for m in ms] for r, ms in (crash or {}).items()})


# The pinned scenarios of the issue (every figure below is the model's).
HEALTHY64 = case(64, 3, 12, 12, 0.25, 40, {3: [1, 63]})
COLLAPSE64 = case(64, 3, 8, 8, 0.25, 40, {3: [1, 63]})
CRASH128 = case(128, 4, 12, 12, 0.3, 40, {4: range(0, 128, 16)})
SMALL5 = case(5, 3, 5, 5, 0.2, 30, {3: [1]})
NOLOSS33 = case(33, 3, 5, 5, 0.0, 30, {3: [1, 32]})

# One ensemble per (N, k): clusters that differ in seed, T_fail, T_cleanup and
# loss. GROUPS[name] = the cases of its clusters (same n, k and rounds).
GROUPS = {
    "n64k3": [HEALTHY64, COLLAPSE64, case(64, 3, 10, 7, 0.15, 40, {5: [0]}, seed=0x5EED48),
              case(64, 3, 12, 12, 0.1, 40, {3: [1, 63]}, seed=0x5EED49, mute=17, deaf=40)],
    "n128k4": [CRASH128, case(128, 4, 9, 14, 0.1, 40, {2: [127]}, seed=0x5EED4A)],
    "n128k3": [case(128, 3, 12, 12, 0.2, 24, {3: [5, 64, 127]}, seed=0x5EED4B)],
    "n100k3": [case(100, 3, 10, 10, 0.2, 24, {3: [7, 99]}, mute=50, deaf=3),
               case(100, 3, 12, 6, 0.05, 24, {6: [98]}, seed=0x5EED4C)],
    "n33k3": [NOLOSS33, case(33, 3, 7, 5, 0.2, 30, {3: [1, 32]}, seed=0x5EED4D)],
    "n5k3": [SMALL5, case(5, 3, 6, 4, 0.1, 30, {8: [4]}, seed=0x5EED4E)],
    "n16k1": [case(16, 1, 5, 5, 0.1, 20, {4: [15]}), case(16, 1, 9, 9, 0.0, 20, seed=0x5EED4F)],
    "n16k8": [case(16, 8, 5, 5, 0.3, 20, {4: [0, 9]}), case(16, 8, 3, 6, 0.5, 20, seed=0x5EED50)],
    "n2k3": [case(2, 3, 5, 5, 0.1, 12), case(2, 3, 5, 5, 0.0, 12, {3: [1]}, seed=0x5EED51)],
    "n3k3": [case(3, 3, 5, 5, 0.1, 12, {3: [0]}), case(3, 3, 2, 2, 0.3, 12, seed=0x5EED52)],
    "n3k3m2": [case(3, 3, 3, 3, 0.3, 16, {9: [2]}, min_members=2),
               case(3, 3, 5, 2, 0.0, 16, {4: [0]}, seed=0x5EED54, min_members=2)],
    "n4k3": [case(4, 3, 5, 5, 0.1, 12, {6: [2]}), case(4, 3, 5, 5, 0.0, 12, seed=0x5EED53)],
}


def model(c, state=None, round_=0):
    """LossModel of case c, from a full start or from `state` = (hb, ts, alive)."""
    m = lr.LossModel(c["n"], c["k"], c["t_fail"], c["t_cleanup"], c["seed"], c["min_members"])
    m.import_state(*(state or full_state(c["n"])), round_)
    m.set_loss(c["out"], c["inn"])
    return m


def run(m, rounds, crash=None):
    """Runs model m for `rounds` rounds (crash = {round: [members]}, by the
    round's tick) and returns the per-round records: dicts of hb, ts, alive
    (as exported), stats (every gh_ens_stats field of that round), failed (the
    bitmap) and detect = (first_round, fp_rounds) so far."""
    n = m.n
    first, fp = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    out = []
    for _ in range(rounds):
        r = m.round + 1
        if crash and crash.get(r):
            m.apply_events([(lr.CRASH, c) for c in crash[r]])
        s0, d0 = m.sent, m.dropped
        st = m.step(1)
        running = m.alive.astype(bool)
        det = m.det_cnt > 0
        st["false_failed"] = int((det & running).sum())
        st["false_detections"] = int(m.det_cnt[running].sum())
        st["sent"], st["dropped"] = m.sent - s0, m.dropped - d0
        fp[det & running] += 1
        first[det & ~running & (first < 0)] = r
        hb, ts, alive = m.export_state()
        out.append(dict(round=r, hb=hb, ts=ts, alive=alive, stats=st, failed=m.read_failed(),
                        detect=(first.copy(), fp.copy())))
    return out


@functools.lru_cache(maxsize=None)
def group_trace(name):
    """The traces of GROUPS[name]'s clusters, [cluster][round]; shared, read-only."""
    return tuple(tuple(run(model(c), c["rounds"], c["crash"])) for c in GROUPS[name])


def total(trace, field):
    return sum(rec["stats"][field] for rec in trace)


def imported_state(n=24, t_fail=5, t_cleanup=5, r0=40):
    """(hb, ts, alive) to import at round r0: rows holding 0, 1, 2 and 3
    present members with and without their own entry (the guard's edge at
    min_members = 4 and below), tombstones aged T_cleanup - 1, T_cleanup and
    T_cleanup + 1 at the next round, cells with hb 0, 1 and 2 aged past T_fail
    (only hb > 1 is detected), a stopped row, and full rows around them."""
    r = r0 + 1  # the first round run
    hb = np.full((n, n), 5, np.int32)
    ts = np.full((n, n), r0 - 1, np.int32)
    alive = np.ones(n, np.uint8)
    few = {0: [], 1: [1], 2: [5], 3: [3, 9], 4: [0, 11], 5: [5, 6, 7], 6: [1, 2, 3], 7: [7, 8, 9, 10]}
    for i, members in few.items():
        hb[i] = -1
        hb[i, members] = 4
    # tombstones whose age at round r is T_cleanup - 1, T_cleanup, T_cleanup + 1 (released only beyond T_cleanup)
    for j, age in enumerate((t_cleanup - 1, t_cleanup, t_cleanup + 1)):
        hb[12 + j, 20] = -2
        ts[12 + j, 20] = r - age
        hb[7, 11 + j] = -2  # and in a row at the guard's edge
        ts[7, 11 + j] = r - age
    # stale entries: hb 0, 1, 2 aged past T_fail
    for j, h in enumerate((0, 1, 2)):
        hb[16, 21 + j] = h
        ts[16, 21 + j] = r - t_fail - 3
        hb[17 + j, 21 + j] = h
        ts[17 + j, 21 + j] = r - t_fail - 1
    alive[10] = 0  # a stopped row keeps its table
    hb[10, :8] = 9
    ts[10, :8] = 3
    return hb, ts, alive
