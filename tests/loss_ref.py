"""CPU models of lossy gossip links (SPEC.md §2 step 6a, gh_set_loss), for
the tests only.

* B(): the link block in pure Python on oracle.philox.philox4x32_10, and
  blocks(): the same over numpy arrays (pinned against B() in
  test_loss_ref.py).
* LossModel: a dense numpy model of SPEC §2 in pull mode, canonical
  detection, GH_REMOVE_ALL, crash events only, with the gh_* call shapes the
  parity tests use (import_state, apply_events, set_loss, step, export_state,
  read_failed, read_detectors, loss_stats).
* LossyListSim: oracle.listsim.ListSim with its delivery step under loss (ring
  mode, either list order; pull mode too).

With loss off or all thresholds zero both equal their lossless originals
(tablesim / ListSim), which test_loss_ref.py checks."""
from __future__ import annotations

import numpy as np

from oracle import listsim, philox

TAG_LINK = 0x4C494E4B  # 'LINK'
NEVER, ALWAYS = 0, 0xFFFFFFFF
CRASH = 3
STATS = ("rounds", "last_round", "detections", "failed_members", "remove_unknown", "ring_empty", "active_rows",
         "merged_cells", "released", "tombstoned")
SUMMED = tuple(f for f in STATS if f != "last_round")


def q32(p):
    """A drop rate in [0, 1] as a threshold in units of 2^-32."""
    return min(int(round(float(p) * 2.0 ** 32)), ALWAYS)


def hit(thr, w):
    return thr == ALWAYS or w < thr


def B(seed, a, r, blk):
    """The 4 words of the link block of counter (a, r, 'LINK', blk)."""
    return philox.philox4x32_10((a, r, TAG_LINK, blk), (seed & philox.MASK, (seed >> 32) & philox.MASK))


def dropped(seed, out, inn, a, r, blk, sender, receiver):
    """The message sender -> receiver drawn by block B(a, r, blk) is lost."""
    w = B(seed, a, r, blk)
    return hit(int(out[sender]), w[0]) or hit(int(inn[receiver]), w[1])


def blocks(seed, a, b, tag, blk):
    """Philox4x32-10 blocks of counters (a, b, tag, blk) (broadcast arrays)
    under key `seed`: four uint64 arrays holding the 32-bit words."""
    M = np.uint64(philox.MASK)
    S = np.uint64(32)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, np.uint64) & M for x in (a, b, tag, blk)])
    k0, k1 = seed & philox.MASK, (seed >> 32) & philox.MASK
    for rnd in range(10):
        if rnd:
            k0 = (k0 + philox.W0) & philox.MASK
            k1 = (k1 + philox.W1) & philox.MASK
        p0 = np.uint64(philox.M0) * c0
        p1 = np.uint64(philox.M1) * c2
        c0, c1, c2, c3 = ((p1 >> S) ^ c1 ^ np.uint64(k0)) & M, p1 & M, ((p0 >> S) ^ c3 ^ np.uint64(k1)) & M, p0 & M
    return c0, c1, c2, c3


def hits(thr, w):
    thr = np.asarray(thr, np.uint64)
    return (thr == np.uint64(ALWAYS)) | (w < thr)


def _thresholds(n, p):
    """uint32 [n] thresholds: None -> zeros, a float or [n] floats -> q32,
    uint32 arrays as they are (Engine.set_loss's conversion)."""
    if p is None:
        return np.zeros(n, np.uint32)
    a = np.asarray(p)
    if a.dtype == np.uint32:
        return np.broadcast_to(a, (n,)).copy()
    return np.broadcast_to(np.vectorize(q32, otypes=[np.uint32])(a), (n,)).copy()


class LossModel:
    """SPEC §2, dense, pull mode, canonical detection, REMOVE to every alive
    row but a sole detector, crash events only."""

    def __init__(self, n, fanout=3, t_fail=5, t_cleanup=5, seed=0x5EED0001, min_members=4):
        self.n, self.k = n, fanout
        self.t_fail, self.t_cleanup, self.min_members, self.seed = t_fail, t_cleanup, min_members, seed
        self.hb = np.full((n, n), -1, np.int32)
        self.ts = np.zeros((n, n), np.int32)
        self.alive = np.zeros(n, np.uint8)
        self.round = 0
        self.det_cnt = np.zeros(n, np.int64)
        self.det_min = np.full(n, n, np.int64)
        self.det_any = np.zeros(n, bool)
        self.events = []
        self.out = self.inn = None
        self.sent = self.dropped = 0

    # ---- the gh_* call shapes --------------------------------------------
    def import_state(self, hb, ts, alive, round_=0):
        self.hb = np.array(hb, np.int32)
        self.ts = np.array(ts, np.int32)
        self.alive = np.array(alive, np.uint8)
        self.round = round_
        self.det_cnt[:] = 0
        self.det_min[:] = self.n
        self.det_any[:] = False

    def apply_events(self, events):
        assert all(kind == CRASH for kind, _ in events), "the model knows crashes only"
        self.events.extend(events)

    def set_loss(self, out=None, inbound=None):
        if out is None and inbound is None:
            self.out = self.inn = None
        else:
            self.out, self.inn = _thresholds(self.n, out), _thresholds(self.n, inbound)
        self.sent = self.dropped = 0

    def loss_stats(self):
        assert self.out is not None
        return self.sent, self.dropped

    def export_state(self):
        """(hb, ts, alive) as gh_export_state presents them (SPEC §1)."""
        t = self.ts.astype(np.int64)
        t[self.hb == -1] = 0
        if self.t_cleanup < 30:
            now = self.round + 1
            old = (self.hb == -2) & (now - t > self.t_cleanup + 1)
            t[old] = now - (self.t_cleanup + 1)
        return self.hb.copy(), t.astype(np.int32), self.alive.copy()

    def read_failed(self):
        bm = np.zeros((self.n + 31) // 32, np.uint32)
        for c in np.flatnonzero(self.det_cnt > 0):
            bm[c >> 5] |= np.uint32(1 << (c & 31))
        return bm

    def failed(self):
        return np.flatnonzero(self.det_cnt > 0)

    def read_detectors(self):
        return np.flatnonzero(self.det_any).astype(np.int32)

    def step(self, rounds=1):
        st = dict.fromkeys(STATS, 0)
        st["last_round"] = self.round
        for _ in range(rounds):
            self._one_round(st)
        return st

    # ---- one round ---------------------------------------------------------
    def peers(self, r):
        """[n][k] the pull peers of every receiver in round r."""
        n = self.n
        i = np.arange(n, dtype=np.uint64)[:, None]
        t = np.arange(self.k, dtype=np.uint64)[None, :]
        w = blocks(self.seed, i, r, philox.TAG_PEER, t >> np.uint64(2))
        u = np.choose((t & np.uint64(3)).astype(np.int64) + np.zeros((n, 1), np.int64), w)
        q = (u * np.uint64(n - 1)) >> np.uint64(32)
        return (q + (q >= i)).astype(np.int64)

    def _one_round(self, st):
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
        if n >= 2:
            snap = hb.copy()
            P = self.peers(r)
            msg = alive[:, None] & (alive & active)[P] & (snap[P, rows[:, None]] >= 0)
            keep = msg
            if self.out is not None:
                w = blocks(self.seed, rows[:, None], r, TAG_LINK, np.arange(self.k)[None, :])
                lost = msg & (hits(self.out[P], w[0]) | hits(self.inn[:, None], w[1]))
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


class LossyListSim(listsim.ListSim):
    """ListSim whose gossip messages cross lossy links: a ring message (sender
    s, slot q, alive target g) is lost iff hit(out[s], B(s, r, q)[0]) or
    hit(in[g], B(s, r, q)[1]); a valid pull draw t of receiver i from p iff
    hit(out[p], B(i, r, t)[0]) or hit(in[i], B(i, r, t)[1]). Everything else is
    ListSim's round, restated here because it has no delivery hook."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.out = self.inn = None
        self.sent = self.dropped = 0

    def set_loss(self, out=None, inbound=None):
        if out is None and inbound is None:
            self.out = self.inn = None
        else:
            self.out, self.inn = _thresholds(self.n, out), _thresholds(self.n, inbound)
        self.sent = self.dropped = 0

    def loss_stats(self):
        assert self.out is not None
        return self.sent, self.dropped

    def _arrives(self, a, r, blk, sender, receiver):
        if self.out is None:
            return True
        self.sent += 1
        if dropped(self.seed, self.out, self.inn, a, r, blk, sender, receiver):
            self.dropped += 1
            return False
        return True

    def _one_round(self):
        r = self.round + 1
        nodes = self.nodes
        self._do_events(r)
        for c, dets in sorted(self.pending_remove.items()):
            for j, nd in enumerate(nodes):
                if not nd.alive:
                    continue
                if self.remove == "list":
                    if j not in self.pending_recv.get(c, ()):
                        continue
                elif dets == [j]:
                    continue
                self._remove_at(j, c)
        active = [False] * self.n
        detected_by, recv = {}, {}
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
            for c, to in nd.sent.items():
                recv.setdefault(c, set()).update(to)
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
                    if nodes[tgt].alive and self._arrives(s, r, q, s, tgt):
                        inbox.setdefault(tgt, []).append(s)
        else:
            for i, nd in enumerate(nodes):
                if not nd.alive:
                    continue
                for t in range(self.k):
                    p = philox.peer(self.seed, i, r, t, self.n)
                    if p in snaps and listsim.get_index(i, snaps[p]) != -1 and self._arrives(i, r, t, p, i):
                        inbox.setdefault(i, []).append(p)
        for i in sorted(inbox):
            changed = set()
            for s in sorted(set(inbox[i])):
                changed |= nodes[i].merge(snaps[s], r)
            self.stats["merged_cells"] += len(changed)
        self.pending_remove = detected_by
        self.pending_recv = recv
        self.last_failed = sorted(detected_by)
        self.stats["failed_members"] += len(detected_by)
        self.round = r
        self.stats["rounds"] += 1
        self.stats["last_round"] = r


# ---- scenarios (shared by the CPU checks of non-vacuity and the GPU parity) --
def uniform_case(n, k, t, rate, rounds, seed=0x5EED10 + 55, crash=None, mute=None, deaf=None):
    """Configuration + loss arrays of a lossy pull-mode scenario from a full
    start: uniform `rate` on both sides, optionally one member with out =
    ALWAYS (mute), one with in = ALWAYS (deaf) and a crash schedule."""
    out = np.full(n, q32(rate), np.uint32)
    inn = out.copy()
    if mute is not None:
        out[mute] = ALWAYS
    if deaf is not None:
        inn[deaf] = ALWAYS
    return dict(n=n, cfg=dict(fanout=k, t_fail=t, t_cleanup=t, seed=seed), out=out, inn=inn, rounds=rounds,
                sched=dict(crash or {}))


def model_of(case, lossy=True):
    from scenarios import full_state
    c = case["cfg"]
    m = LossModel(case["n"], c["fanout"], c["t_fail"], c["t_cleanup"], c["seed"])
    m.import_state(*full_state(case["n"]), 0)
    if lossy:
        m.set_loss(case["out"], case["inn"])
    return m


def run_model(case, lossy=True, per_round=None):
    """The scenario on the model; per_round(model, stats) after every round.
    Returns the model."""
    m = model_of(case, lossy)
    for r in range(1, case["rounds"] + 1):
        if case["sched"].get(r):
            m.apply_events(case["sched"][r])
        st = m.step(1)
        if per_round:
            per_round(m, st)
    return m
