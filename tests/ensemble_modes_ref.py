"""Reference model, scenarios and traces of the ensemble modes (gh_ens_config's
peer_mode / detect_mode, SPEC §11), for the tests only.

* ModeModel: loss_ref.LossModel (dense numpy, one model per cluster, the same
  gh_* call shapes) with the two modes: ring gossip in member-ID order with the
  ring form of step 6a, and quirk detection (SPEC §4) on the ID-ordered list.
  With both off it runs LossModel's own round. Written as the plain list walk
  of the SPEC, not as the kernel's mask arithmetic. `diag` counts what the
  scenarios are meant to reach (test_ensemble_modes_ref.py asserts on it).
* The scenarios of test_gpu_ensemble_modes.py and their traces, shaped like
  ensemble_ref.py's: GROUPS[name] = the cases of one ensemble's clusters,
  group_trace(name, ring, quirk) = [cluster][round] records, computed once
  per process and shared; nobody writes into a trace."""
from __future__ import annotations

import functools

import numpy as np

import ensemble_ref as er
import loss_ref as lr
from scenarios import full_state

FIELDS = er.FIELDS
MODES = {"ring-canonical": (True, False), "ring-quirk": (True, True), "pull-quirk": (False, True)}


def go_mod(v, m):
    """Go's truncated % and the reference's + len for negatives (slave/slave.go:517-524)."""
    q = abs(v) % m
    q = -q if v < 0 else q
    return q + m if q < 0 else q


class ModeModel(lr.LossModel):
    """SPEC §11: LossModel plus peer_mode ring and detect_mode quirk."""

    def __init__(self, n, fanout=3, t_fail=5, t_cleanup=5, seed=0x5EED0001, min_members=4, ring=False, quirk=False):
        super().__init__(n, fanout, t_fail, t_cleanup, seed, min_members)
        self.ring, self.quirk = bool(ring), bool(quirk)
        self.diag = dict(max_senders=0, idx_absent=0, short_repeat=0, quirk_skipped=0)

    def _quirk_detected(self, row_hb, cand_row):
        """The candidates of one row the skipping sweep detects: in list
        order, even offsets of each run of consecutive candidates, and the
        list's last entry."""
        lst = np.flatnonzero(row_hb >= 0)
        det = np.zeros(self.n, bool)
        off = 0
        prev = False
        for pos, c in enumerate(lst):
            if not cand_row[c]:
                prev = False
                continue
            off = off + 1 if prev else 0
            prev = True
            if off % 2 == 0 or pos == len(lst) - 1:
                det[c] = True
            else:
                self.diag["quirk_skipped"] += 1
        return det

    def _one_round(self, st):
        if not self.ring and not self.quirk:
            return super()._one_round(st)
        n, r = self.n, self.round + 1
        hb, ts = self.hb, self.ts
        for _, c in self.events:  # step 0
            self.alive[c] = 0
        self.events = []
        alive = self.alive.astype(bool)
        rows = np.arange(n)
        # step 1: REMOVE delivery of D_{r-1}
        pend = self.det_cnt > 0
        sole = (self.det_cnt[None, :] == 1) & (self.det_min[None, :] == rows[:, None])
        rm = alive[:, None] & pend[None, :] & ~sole
        st["tombstoned"] += int((rm & (hb >= 0)).sum())
        st["remove_unknown"] += int((rm & (hb == -1)).sum())
        hb[rm & (hb >= 0)] = -2
        # step 2: guard
        active = alive & ((hb >= 0).sum(1) >= self.min_members)
        guard = (alive & ~active)[:, None] & (hb >= 0)
        ts[guard] = r
        st["active_rows"] += int(active.sum())
        # step 3: own heartbeat
        own = active & (hb[rows, rows] >= 0)
        hb[rows[own], rows[own]] += 1
        ts[rows[own], rows[own]] = r
        # step 4: detect
        cand = active[:, None] & (hb > 1) & (ts.astype(np.int64) < r - self.t_fail)
        cand[rows, rows] = False
        if self.quirk:
            for i in np.flatnonzero(cand.any(1)):
                cand[i] = self._quirk_detected(hb[i], cand[i])
        hb[cand] = -2
        self.det_cnt = cand.sum(0).astype(np.int64)
        self.det_min = np.where(self.det_cnt > 0, cand.argmax(0), n).astype(np.int64)
        self.det_any = cand.any(1)
        st["detections"] += int(cand.sum())
        st["failed_members"] += int((self.det_cnt > 0).sum())
        # step 5: clean
        rel = active[:, None] & (hb == -2) & (ts.astype(np.int64) < r - self.t_cleanup)
        hb[rel] = -1
        st["released"] += int(rel.sum())
        # step 6 / 6a: send, lose, merge
        snap = hb.copy()
        m = np.full((n, n), -1, np.int32)
        if self.ring:
            senders = [set() for _ in range(n)]
            for s in np.flatnonzero(active):
                lst = np.flatnonzero(snap[s] >= 0)
                ln = len(lst)
                if ln == 0:
                    st["ring_empty"] += 1
                    continue
                at = np.flatnonzero(lst == s)
                idx = int(at[0]) if len(at) else -1
                self.diag["idx_absent"] += idx < 0
                tg = [int(lst[go_mod(v, ln)]) for v in (idx - 1, idx + 1, idx + 2)]
                if ln < 4 and (len(set(tg)) < 3 or s in tg):
                    self.diag["short_repeat"] += 1
                for q, g in enumerate(tg):
                    if not alive[g]:
                        continue
                    self.sent += 1
                    if self.out is not None and lr.dropped(self.seed, self.out, self.inn, int(s), r, q, int(s), g):
                        self.dropped += 1
                        continue
                    senders[g].add(int(s))
            for g in range(n):
                if senders[g]:
                    self.diag["max_senders"] = max(self.diag["max_senders"], len(senders[g]))
                    m[g] = snap[sorted(senders[g])].max(0)
            m = np.maximum(m, -1)
        elif n >= 2:
            P = self.peers(r)
            msg = alive[:, None] & (alive & active)[P] & (snap[P, rows[:, None]] >= 0)
            keep = msg
            if self.out is not None:
                w = lr.blocks(self.seed, rows[:, None], r, lr.TAG_LINK, np.arange(self.k)[None, :])
                lost = msg & (lr.hits(self.out[P], w[0]) | lr.hits(self.inn[:, None], w[1]))
                self.sent += int(msg.sum())
                self.dropped += int(lost.sum())
                keep = msg & ~lost
            for t in range(self.k):
                m = np.maximum(m, np.where(keep[:, t, None], snap[P[:, t]], -1))
        upd = (hb >= -1) & (m > hb)
        hb[upd] = m[upd]
        ts[upd] = r
        st["merged_cells"] += int(upd.sum())
        self.round = r
        st["rounds"] += 1
        st["last_round"] = r


case = er.case

# One ensemble per name: clusters that differ in seed, timeouts and loss (same
# n, k, rounds, min_members). Each runs in every entry of MODES.
GROUPS = {
    # the reference's own shape (main.go: ten processes, 5 / 5); members 4..7: the issue's quirk figures
    "n10": [case(10, 3, 5, 5, 0.0, 30, {3: [1, 9]}),
            case(10, 3, 5, 5, 0.1, 30, {3: [4, 5, 6, 7]}, seed=0x5EED81),
            case(10, 3, 6, 4, 0.3, 30, {5: [0]}, seed=0x5EED82, mute=2, deaf=7)],
    # adjacent candidates: quirk runs of length 4
    "n16": [case(16, 3, 8, 8, 0.0, 30, {3: [5, 6, 7, 8]}),
            case(16, 3, 8, 8, 0.05, 30, {3: [5, 6, 7, 8]}, seed=0x5EED83),
            case(16, 3, 5, 5, 0.2, 30, {4: [15]}, seed=0x5EED84, mute=3, deaf=12)],
    # ragged in bucket 64
    "n33": [case(33, 3, 16, 9, 0.0, 36, {3: [1, 32]}),
            case(33, 3, 16, 9, 0.1, 36, {3: [1, 32]}, seed=0x5EED85, mute=20, deaf=6),
            case(33, 3, 7, 5, 0.2, 36, {3: [10, 11, 12]}, seed=0x5EED86)],
    "n64": [case(64, 3, 30, 30, 0.05, 40, {3: [1, 63]}),
            case(64, 3, 12, 12, 0.1, 40, {3: [1, 63]}, seed=0x5EED87, mute=17, deaf=40),
            case(64, 3, 8, 6, 0.3, 40, {5: [30, 31, 32, 33]}, seed=0x5EED88)],
    # rows of two waves; T_fail 12: the ring's false-positive cascade from round 13
    "n100": [case(100, 3, 12, 12, 0.1, 24, {3: [7, 99]}, mute=50, deaf=3),
             case(100, 3, 12, 6, 0.0, 24, {6: [98]}, seed=0x5EED89)],
    # ... and a crash wave of six adjacent members across the 64-lane boundary
    "n128": [case(128, 3, 12, 12, 0.1, 24, {3: range(61, 67)}, mute=5, deaf=100),
             case(128, 3, 12, 9, 0.0, 24, {3: range(61, 67)}, seed=0x5EED8A),
             case(128, 3, 6, 6, 0.3, 24, {2: [0, 127]}, seed=0x5EED8B)],
}

# Tiny lists: L < 4, repeated and self targets, negative indices through Go's %.
TINY = {
    "n2": [case(2, 3, 5, 5, 0.1, 12), case(2, 3, 5, 5, 0.0, 12, {3: [1]}, seed=0x5EED91)],
    "n3": [case(3, 3, 5, 5, 0.1, 12, {3: [0]}), case(3, 3, 2, 2, 0.3, 12, seed=0x5EED92)],
    "n4": [case(4, 3, 5, 5, 0.1, 12, {6: [2]}), case(4, 3, 5, 5, 0.0, 12, seed=0x5EED93)],
    "n3m2": [case(3, 3, 3, 3, 0.3, 16, {9: [2]}, min_members=2),
             case(3, 3, 5, 2, 0.0, 16, {4: [0]}, seed=0x5EED94, min_members=2)],
    "n2m1": [case(2, 3, 2, 2, 0.2, 12, {5: [0]}, min_members=1),
             case(2, 3, 5, 5, 0.0, 12, seed=0x5EED95, min_members=1)],
}
GROUPS.update(TINY)


def model(c, ring, quirk, state=None, round_=0):
    """ModeModel of case c, from a full start or from `state` = (hb, ts, alive)."""
    m = ModeModel(c["n"], c["k"], c["t_fail"], c["t_cleanup"], c["seed"], c["min_members"], ring, quirk)
    m.import_state(*(state or full_state(c["n"])), round_)
    m.set_loss(c["out"], c["inn"])
    return m


run = er.run
total = er.total


@functools.lru_cache(maxsize=None)
def group_models(name, ring, quirk):
    """(traces [cluster][round], models after the run) of GROUPS[name] in the given modes."""
    ms = [model(c, ring, quirk) for c in GROUPS[name]]
    return tuple(tuple(run(m, c["rounds"], c["crash"])) for m, c in zip(ms, GROUPS[name])), tuple(ms)


def group_trace(name, ring, quirk):
    """The traces of GROUPS[name]'s clusters, [cluster][round]; shared, read-only."""
    return group_models(name, ring, quirk)[0]


def hub_state(n, r0=20):
    """(hb, ts, alive) to import at round r0, every ts fresh (round r0 + 1
    detects nothing): every row lists {0, 1, 2, itself}, so in ring mode each
    of members 0..2 is the target of about N - 3 senders at once; row 5 lists
    {0, 1, 2, 3} and lacks its own entry (idx = -1), row 6 is empty, row 7 holds only itself, row 8
    is stopped. Rows 0..2 hold three members: under the guard at min_members
    4, senders with L = 3 at min_members 0, where row 6 counts ring_empty."""
    hb = np.full((n, n), -1, np.int32)
    ts = np.full((n, n), r0, np.int32)
    alive = np.ones(n, np.uint8)
    hb[:, :3] = 7
    hb[np.arange(n), np.arange(n)] = 9
    hb[5, 5] = -1
    hb[5, 3] = 7  # (four entries: not under the guard)
    hb[6, :] = -1
    hb[7, :] = -1
    hb[7, 7] = 4
    alive[8] = 0
    return hb, ts, alive
