"""CPU models of lossy control messages (SPEC.md §2 step 6c, §5;
gh_set_control_loss), for the tests only.

* W() / ctl_dropped() / remove_dropped(): the per-message draws in pure Python
  on oracle.philox; ctl_dropped_np() / remove_arrives_np(): the same over numpy
  arrays (pinned against each other in test_control_loss_ref.py).
* ControlLossModel over partition_ref.PartitionModel: dense, pull mode,
  canonical detection, crash events only; REMOVE per message.
* ControlLossListSim over partition_ref.PartitionListSim: ring and pull mode,
  both list orders, quirk detection, JOIN / LEAVE / CRASH, with the gossip loss
  of loss_ref.LossyListSim on what a partition does not cut.

With kinds = 0, loss off or all thresholds zero both equal their parents, which
test_control_loss_ref.py checks."""
from __future__ import annotations

import numpy as np

import loss_ref as lr
import partition_ref as pr
from oracle import listsim, philox

CTL_REMOVE, CTL_LEAVE, CTL_JOIN = 1, 2, 4
CTL_ALL = 7
TAG_LEAV, TAG_JOIN, TAG_BCST, TAG_CRMV = 0x4C454156, 0x4A4F494E, 0x42435354, 0x43524D56
STATS = ("remove_pairs", "remove_missed", "leave_sent", "leave_dropped", "join_sent", "join_dropped", "bcast_sent",
         "bcast_dropped")


def check_kinds(kinds):
    k = int(kinds)
    if not 0 <= k <= CTL_ALL:
        raise ValueError("kinds outside 0..7")
    return k


# ---- the draws, one message at a time ----------------------------------------
def W(seed, tag, a, r, b):
    """The 4 words of the block of counter (a, r, tag, b) under key `seed`."""
    return philox.philox4x32_10((a, r, tag, b), (seed & philox.MASK, (seed >> 32) & philox.MASK))


def ctl_dropped(seed, out, inn, tag, a, r, b, sender, receiver):
    """The LEAVE / JOIN / broadcast message sender -> receiver drawn by
    W(tag; a, r, b) is lost."""
    w = W(seed, tag, a, r, b)
    return lr.hit(int(out[sender]), w[0]) or lr.hit(int(inn[receiver]), w[1])


def remove_key(seed, c, r):
    w = W(seed, TAG_CRMV, c, r, 0)
    return w[0] | (w[1] << 32)


def remove_dropped(seed, out, inn, c, r, i, j):
    """Detector i's Remove(c) of round r to row j is lost."""
    w = W(remove_key(seed, c, r), TAG_CRMV, i, j, 0)
    return lr.hit(int(out[i]), w[0]) or lr.hit(int(inn[j]), w[1])


# ---- the same over arrays ---------------------------------------------------------
def ctl_dropped_np(seed, out, inn, tag, a, r, b, sender, receiver):
    w = lr.blocks(seed, a, r, tag, b)
    return lr.hits(np.asarray(out)[sender], w[0]) | lr.hits(np.asarray(inn)[receiver], w[1])


def remove_arrives_np(seed, out, inn, c, r, dets, side):
    """For member c detected in round r by the rows `dets` (ascending):
    (has [n], got [n]): row j has a message (E_j(c) non-empty) / one arrived."""
    n = len(out)
    i = np.asarray(dets, np.int64)[:, None]
    j = np.arange(n, dtype=np.int64)[None, :]
    msg = (i != j) & (side[i] == side[j])
    w = lr.blocks(remove_key(seed, c, r), i, j, TAG_CRMV, 0)
    lost = lr.hits(np.asarray(out)[i], w[0]) | lr.hits(np.asarray(inn)[j], w[1])
    return msg.any(0), (msg & ~lost).any(0)


class _Ctl:
    """The gh_*control_loss* call shapes, shared by both models."""

    def _ctl_init(self):
        self.kinds = 0
        self.ctl_called = False
        self.ctl = dict.fromkeys(STATS, 0)

    def set_control_loss(self, kinds):
        k = check_kinds(kinds)
        if (k & CTL_REMOVE) and not self.armed:
            self.set_partition(None)  # arms: every member on side 0, cut = 0
        self.kinds = k
        self.ctl_called = True
        self.ctl = dict.fromkeys(STATS, 0)

    def control_loss(self):
        return self.kinds

    def control_loss_stats(self):
        assert self.ctl_called
        return dict(self.ctl)

    def set_loss(self, out=None, inbound=None):
        super().set_loss(out, inbound)
        self.ctl = dict.fromkeys(STATS, 0)

    def lossy(self, kind):
        return self.out is not None and bool(self.kinds & kind)


class ControlLossModel(_Ctl, pr.PartitionModel):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._ctl_init()

    def _recipients(self, cand, alive):
        rcv = super()._recipients(cand, alive)  # rule D4 per side (and the sets' bookkeeping)
        if not self.lossy(CTL_REMOVE):
            return rcv
        r = self.round + 1
        for c in np.flatnonzero(cand.any(0)):
            has, got = remove_arrives_np(self.seed, self.out, self.inn, int(c), r, np.flatnonzero(cand[:, c]), self.side)
            assert np.array_equal(has, rcv[:, c]), "with nothing dropped the rule is D4 per side"
            rcv[:, c] = got
            self.ctl["remove_pairs"] += int((has & alive).sum())
            self.ctl["remove_missed"] += int((has & alive & ~got).sum())
        return rcv


class ControlLossListSim(_Ctl, pr.PartitionListSim):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._ctl_init()
        self.out = self.inn = None
        self.sent = self.dropped = 0

    # (gossip loss, as loss_ref.LossyListSim)
    def set_loss(self, out=None, inbound=None):
        if out is None and inbound is None:
            self.out = self.inn = None
        else:
            self.out, self.inn = lr._thresholds(self.n, out), lr._thresholds(self.n, inbound)
        self.sent = self.dropped = 0
        self.ctl = dict.fromkeys(STATS, 0)

    def loss_stats(self):
        assert self.out is not None
        return self.sent, self.dropped

    def _arrives(self, a, r, blk, sender, receiver):
        if self.out is None:
            return True
        self.sent += 1
        if lr.dropped(self.seed, self.out, self.inn, a, r, blk, sender, receiver):
            self.dropped += 1
            return False
        return True

    def _ctl_arrives(self, kind, name, tag, a, r, b, sender, receiver):
        """A LEAVE / JOIN / broadcast message that exists: counted and drawn."""
        if not self.lossy(kind):
            return True
        self.ctl[name + "_sent"] += 1
        if ctl_dropped(self.seed, self.out, self.inn, tag, a, r, b, sender, receiver):
            self.ctl[name + "_dropped"] += 1
            return False
        return True

    def _do_events(self, now):
        ev, self.events = self.events, []
        I = self.introducer
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
                j = m.addr
                if j == c or not self.nodes[j].alive or not self.reach(c, j):
                    continue
                if self._ctl_arrives(CTL_LEAVE, "leave", TAG_LEAV, c, now, j, c, j):
                    self._remove_at(j, c)
        joiners = [c for kind, c in ev if kind == 1]
        for c in joiners:  # the process starts whatever happens to its JOIN
            nd = self.nodes[c]
            if not nd.alive:
                nd.members, nd.recent_fail = [], []
                nd.alive = True
        intro = self.nodes[I]
        if not intro.alive:
            return
        heard = [c for c in joiners if self.reach(c, I) and
                 (c == I or self._ctl_arrives(CTL_JOIN, "join", TAG_JOIN, c, now, I, c, I))]
        added = 0
        for c in heard:
            if listsim.get_index(c, intro.members) == -1:
                intro._append(listsim.Member(c, 0, now))
                added += 1
        if added:
            msg = intro.snapshot()
            for m in msg:
                j = m.addr
                if not self.nodes[j].alive or not self.reach(I, j):
                    continue
                if j != I and not self._ctl_arrives(CTL_JOIN, "bcast", TAG_BCST, I, now, j, I, j):
                    continue  # (the introducer's own copy is local: no message)
                self.stats["merged_cells"] += len(self.nodes[j].merge(msg, now))

    def _one_round(self):
        r = self.round + 1
        nodes = self.nodes
        self._do_events(r)
        for c in sorted(self.pending_remove):
            for j in sorted(self.pending_recv[c]):
                if nodes[j].alive:
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
                for q, v in enumerate((idx - 1, idx + 1, idx + 2)):
                    tgt = snap[int(listsim._go_mod(v, L))].addr
                    if not nodes[tgt].alive:
                        continue
                    if not self.reach(s, tgt):
                        self.cut += 1
                        continue
                    if self._arrives(s, r, q, s, tgt):
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
                        if self._arrives(i, r, t, p, i):
                            inbox.setdefault(i, []).append(p)
        for i in sorted(inbox):
            changed = set()
            for s in sorted(set(inbox[i])):
                changed |= nodes[i].merge(snaps[s], r)
            self.stats["merged_cells"] += len(changed)
        # the recipients of D_r, fixed now (sides, thresholds and kinds of round r)
        self.pending_remove = detected_by
        self.pending_recv = {}
        lossy = self.lossy(CTL_REMOVE)
        for c, dets in detected_by.items():
            to = set()
            for j in range(self.n):
                E = [i for i in dets if i != j and self.reach(i, j)]
                if not E:
                    continue
                got = not lossy or any(not remove_dropped(self.seed, self.out, self.inn, c, r, i, j) for i in E)
                if lossy and nodes[j].alive:
                    self.ctl["remove_pairs"] += 1
                    self.ctl["remove_missed"] += not got
                if got:
                    to.add(j)
            self.pending_recv[c] = to
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
def crash_1pct(n, seed, at=8):
    import scenarios as sc
    return {at: [(sc.CRASH, int(c)) for c in sc.crash_ids(n, 0.01, seed)]}


def pull_case(n, k, t, rounds, seed, out, inn, kinds, crash=None, side=None, split=1):
    """A pull-mode scenario from a full start: loss and `kinds` from before
    round 1, optional sides from before round `split`, optional crashes."""
    return dict(n=n, cfg=dict(fanout=k, t_fail=t, t_cleanup=t, seed=seed), out=out, inn=inn, kinds=kinds, rounds=rounds,
                sched=dict(crash or {}), side=side, split=split)


def rates(n, rate, mute=(), deaf=(), inn_of=None):
    out = np.full(n, lr.q32(rate), np.uint32)
    inn = out.copy()
    out[list(mute)] = lr.ALWAYS
    inn[list(deaf)] = lr.ALWAYS
    for m, p in (inn_of or {}).items():
        inn[m] = lr.q32(p)
    return out, inn


def model_of(case, kinds=None):
    from scenarios import full_state
    c = case["cfg"]
    m = ControlLossModel(case["n"], c["fanout"], c["t_fail"], c["t_cleanup"], c["seed"])
    m.import_state(*full_state(case["n"]), 0)
    m.set_loss(case["out"], case["inn"])
    k = case["kinds"] if kinds is None else kinds
    if k is not None and k >= 0:
        m.set_control_loss(k)
    return m


def run_model(case, kinds=None, per_round=None):
    """The scenario on the dense model (kinds: override the case's; -1: the
    call is never made); per_round(model, stats) after every round."""
    m = model_of(case, kinds)
    for r in range(1, case["rounds"] + 1):
        if case["side"] is not None and r == case["split"]:
            m.set_partition(case["side"])
        if case["sched"].get(r):
            m.apply_events(case["sched"][r])
        st = m.step(1)
        if per_round:
            per_round(m, st)
    return m
