"""CPU models of network partitions (SPEC.md §2 step 6b, gh_set_partition),
for the tests only.

* PartitionModel: the dense numpy model of SPEC §2 (loss_ref.LossModel: pull
  mode, canonical detection, rule D4, crash events only) with sides: gossip
  between sides is cut and counted, REMOVE(c) goes from each detector to the
  rows of its own side (rule D4 per side, by the sides in force in the round of
  the detection), and lossy links act on what is not cut. `gate_control=False`
  cuts the gossip only and leaves REMOVE to rule D4 over all rows, which is
  what gh_set_loss with rate 1 between the groups gives (SPEC D9): it exists
  for the non-vacuity checks alone.
* PartitionListSim: oracle.listsim.ListSim with reach() in its events and its
  round (ring and pull mode, both list orders, quirk detection, JOIN / LEAVE /
  CRASH), restated here because ListSim has no delivery hook.

With every member on one side both equal their originals (tablesim / ListSim),
which test_partition_ref.py checks."""
from __future__ import annotations

import numpy as np

import loss_ref as lr
from oracle import listsim, philox

SIDES = 64  # GH_PART_SIDES


def check_sides(n, side):
    """int64 [n] sides: None -> zeros; a value outside [0, SIDES) is refused."""
    if side is None:
        return np.zeros(n, np.int64)
    s = np.asarray(side, np.int64)
    assert s.shape == (n,)
    if ((s < 0) | (s >= SIDES)).any():
        raise ValueError("side out of range")
    return s.copy()


class PartitionModel(lr.LossModel):
    def __init__(self, *a, gate_control=True, late_recipients=False, **kw):
        super().__init__(*a, **kw)
        self.gate_control = gate_control
        # late_recipients: REMOVE recipients by the sides in force when the set is
        # DELIVERED, which SPEC step 6b rules out (they are fixed when it is sent);
        # like gate_control=False, for the non-vacuity checks alone
        self.late_recipients = late_recipients
        self.last_cand = None
        self.armed = False
        self.side = np.zeros(self.n, np.int64)
        self.cut = 0
        self.rcv = np.zeros((self.n, self.n), bool)  # [j, c]: row j receives the pending REMOVE(c)
        # per REMOVE set, for the non-vacuity checks: (round of the detection, c,
        # {side: detectors on it}, {side: running rows on it})
        self.sets = []

    def import_state(self, *a, **kw):
        super().import_state(*a, **kw)
        self.rcv[:] = False
        self.last_cand = None

    def set_partition(self, side=None):
        self.side = check_sides(self.n, side)
        self.armed = True
        self.cut = 0

    def partition(self):
        return self.armed, self.side.astype(np.int32)

    def partition_stats(self):
        assert self.armed
        return self.cut

    def _recipients(self, cand, alive):
        """rcv of the round's detections `cand` [i, c] under the sides in force."""
        n, rows = self.n, np.arange(self.n)
        det = cand.any(0)
        rcv = np.zeros((n, n), bool)
        if not det.any():
            return rcv
        side = self.side if self.gate_control else np.zeros(n, np.int64)
        used = np.unique(side)
        cnt = np.zeros((SIDES, n), np.int64)
        low = np.full((SIDES, n), n, np.int64)
        for s in used:
            on = cand & (side == s)[:, None]
            cnt[s] = on.sum(0)
            low[s] = np.where(on, rows[:, None], n).min(0)
        nj, mj = cnt[side], low[side]  # [j, c]
        rcv = (nj > 0) & ~((nj == 1) & (mj == rows[:, None]))
        rcv &= det[None, :]
        for c in np.flatnonzero(det):
            self.sets.append((self.round + 1, int(c), {int(s): int(cnt[s, c]) for s in used},
                              {int(s): int((alive & (side == s)).sum()) for s in used}))
        return rcv

    def _one_round(self, st):
        n, r = self.n, self.round + 1
        hb, ts = self.hb, self.ts
        for _, c in self.events:  # step 0
            self.alive[c] = 0
        self.events = []
        alive = self.alive.astype(bool)
        rows = np.arange(n)
        # step 1: REMOVE delivery of D_{r-1}, to the recipients fixed when it was sent
        if self.late_recipients and self.last_cand is not None:
            keep, self.sets = self.sets, []
            self.rcv = self._recipients(self.last_cand, alive)
            self.sets = keep
        rm = alive[:, None] & self.rcv
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
        hb[cand] = -2
        self.det_cnt = cand.sum(0).astype(np.int64)
        self.det_min = np.where(self.det_cnt > 0, cand.argmax(0), n).astype(np.int64)
        self.det_any = cand.any(1)
        self.rcv = self._recipients(cand, alive)
        self.last_cand = cand
        st["detections"] += int(cand.sum())
        st["failed_members"] += int((self.det_cnt > 0).sum())
        # step 5: clean
        rel = active[:, None] & (hb == -2) & (ts.astype(np.int64) < r - self.t_cleanup)
        hb[rel] = -1
        st["released"] += int(rel.sum())
        # step 6 / 6b / 6a: send, cut, lose, merge
        if n >= 2:
            snap = hb.copy()
            P = self.peers(r)
            msg = alive[:, None] & (alive & active)[P] & (snap[P, rows[:, None]] >= 0)
            cut = msg & (self.side[P] != self.side[:, None])
            self.cut += int(cut.sum())
            msg = msg & ~cut
            keep = msg
            if self.out is not None:
                w = lr.blocks(self.seed, rows[:, None], r, lr.TAG_LINK, np.arange(self.k)[None, :])
                lost = msg & (lr.hits(self.out[P], w[0]) | lr.hits(self.inn[:, None], w[1]))
                self.sent += int(msg.sum())
                self.dropped += int(lost.sum())
                keep = msg & ~lost
            m = np.full((n, n), -1, np.int32)
            for t in range(self.k):
                m = np.maximum(m, np.where(keep[:, t, None], snap[P[:, t]], -1))
            upd = (hb >= -1) & (m > hb)
            hb[upd] = m[upd]
            ts[upd] = r
            st["merged_cells"] += int(upd.sum())
        self.round = r
        st["rounds"] += 1
        st["last_round"] = r


class PartitionListSim(listsim.ListSim):
    """ListSim across a partition: a LEAVE, a JOIN, the introducer's broadcast,
    a gossip message and a REMOVE arrive only where reach(sender, receiver);
    the REMOVE's sides are those of the round of the detection."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        assert self.remove == "all"
        self.armed = False
        self.side = [0] * self.n
        self.pending_side = [0] * self.n  # the sides in force when pending_remove was detected
        self.sets = []
        self.cut = 0

    def set_partition(self, side=None):
        self.side = [int(x) for x in check_sides(self.n, side)]
        self.armed = True
        self.cut = 0

    def partition_stats(self):
        assert self.armed
        return self.cut

    def reach(self, a, b):
        return self.side[a] == self.side[b]

    def _do_events(self, now):
        ev, self.events = self.events, []
        for kind, c in ev:
            if kind == 3:
                self.nodes[c].alive = False
        leavers = []
        for kind, c in ev:
            if kind == 2 and self.nodes[c].alive:
                self.nodes[c].alive = False
                leavers.append(c)
        for c in leavers:
            for m in list(self.nodes[c].members):
                if m.addr == c:
                    continue
                if self.nodes[m.addr].alive and self.reach(c, m.addr):
                    self._remove_at(m.addr, c)
        joiners = [c for kind, c in ev if kind == 1]
        for c in joiners:  # the process starts whatever its side
            nd = self.nodes[c]
            if not nd.alive:
                nd.members, nd.recent_fail = [], []
                nd.alive = True
        I = self.nodes[self.introducer]
        heard = [c for c in joiners if self.reach(c, self.introducer)]
        if heard and I.alive:
            added = 0
            for c in heard:
                if listsim.get_index(c, I.members) == -1:
                    I._append(listsim.Member(c, 0, now))
                    added += 1
            if added:
                msg = I.snapshot()
                for m in msg:
                    rcv = self.nodes[m.addr]
                    if rcv.alive and self.reach(self.introducer, m.addr):
                        self.stats["merged_cells"] += len(rcv.merge(msg, now))

    def _one_round(self):
        r = self.round + 1
        nodes = self.nodes
        self._do_events(r)
        ps = self.pending_side
        for c, dets in sorted(self.pending_remove.items()):
            for j, nd in enumerate(nodes):
                if not nd.alive:
                    continue
                same = [i for i in dets if ps[i] == ps[j]]  # (ascending: the lowest first)
                if not same or same == [j]:
                    continue
                self._remove_at(j, c)
        active = [False] * self.n
        detected_by = {}
        self.last_detectors = []
        for i, nd in enumerate(nodes):
            if not nd.alive:
                continue
            if len(nd.members) < listsim.MIN_NODES:
                for m in nd.members:
                    m.ts = r
                continue
            active[i] = True
            self.stats["active_rows"] += 1
            det = nd.update_member_list(r, self.quirk)
            self.stats["detections"] += len(det)
            for c in det:
                detected_by.setdefault(c, []).append(i)
            if det:
                self.last_detectors.append(i)
        snaps = {i: nodes[i].snapshot() for i in range(self.n) if active[i]}
        inbox = {}
        if self.peer_mode == "ring":
            for s, snap in snaps.items():
                L = len(snap)
                if L == 0:
                    self.stats["ring_empty"] += 1
                    continue
                idx = listsim.get_index(s, snap)
                for v in (idx - 1, idx + 1, idx + 2):
                    tgt = snap[int(listsim._go_mod(v, L))].addr
                    if not nodes[tgt].alive:
                        continue
                    if not self.reach(s, tgt):
                        self.cut += 1
                        continue
                    inbox.setdefault(tgt, []).append(s)
        else:
            for i, nd in enumerate(nodes):
                if not nd.alive:
                    continue
                for t in range(self.k):
                    p = philox.peer(self.seed, i, r, t, self.n)
                    if p in snaps and listsim.get_index(i, snaps[p]) != -1:
                        if not self.reach(p, i):
                            self.cut += 1
                            continue
                        inbox.setdefault(i, []).append(p)
        for i in sorted(inbox):
            changed = set()
            for s in sorted(set(inbox[i])):
                changed |= nodes[i].merge(snaps[s], r)
            self.stats["merged_cells"] += len(changed)
        self.pending_remove = detected_by
        self.pending_recv = {}
        self.pending_side = list(self.side)
        used = sorted(set(self.side))
        for c, dets in detected_by.items():  # (as PartitionModel.sets)
            self.sets.append((r, c, {s: sum(self.side[i] == s for i in dets) for s in used},
                              {s: sum(nd.alive and self.side[i] == s for i, nd in enumerate(nodes)) for s in used}))
        self.last_failed = sorted(detected_by)
        self.stats["failed_members"] += len(detected_by)
        self.round = r
        self.stats["rounds"] += 1
        self.stats["last_round"] = r


# ---- scenarios (shared by the CPU checks of non-vacuity and the GPU parity) --
def sides_of(n, sizes, seed):
    """[n] sides: side s >= 1 gets sizes[s - 1] members drawn by `seed` (the
    introducer, member 0, stays on side 0), everyone else side 0."""
    rng = np.random.default_rng(seed)
    side = np.zeros(n, np.int32)
    pick = rng.permutation(np.arange(1, n))
    at = 0
    for s, k in enumerate(sizes, 1):
        side[pick[at:at + k]] = s
        at += k
    return side


def pull_case(n, k, t, sizes, rounds, seed, split=3, crash=None, loss=None):
    """A pull-mode scenario from a full start: the sides come into force before
    round `split`; optionally a crash schedule and a uniform loss rate."""
    return dict(n=n, cfg=dict(fanout=k, t_fail=t, t_cleanup=t, seed=seed), side=sides_of(n, sizes, seed ^ 0x51DE),
                split=split, rounds=rounds, sched=dict(crash or {}), loss=loss)


def model_of(case, gate_control=True, late_recipients=False):
    from scenarios import full_state
    c = case["cfg"]
    m = PartitionModel(case["n"], c["fanout"], c["t_fail"], c["t_cleanup"], c["seed"], gate_control=gate_control,
                       late_recipients=late_recipients)
    m.import_state(*full_state(case["n"]), 0)
    if case.get("loss") is not None:
        m.set_loss(case["loss"], case["loss"])
    return m


def run_model(case, partitioned=True, gate_control=True, per_round=None, late_recipients=False):
    """The scenario on the model; per_round(model, stats) after every round.
    case["resplit"] = (round, side): a second gh_set_partition before that round."""
    m = model_of(case, gate_control, late_recipients)
    for r in range(1, case["rounds"] + 1):
        if r == case["split"] and partitioned:
            m.set_partition(case["side"])
        if partitioned and case.get("resplit") and r == case["resplit"][0]:
            m.set_partition(case["resplit"][1])
        if case["sched"].get(r):
            m.apply_events(case["sched"][r])
        st = m.step(1)
        if per_round:
            per_round(m, st)
    return m
