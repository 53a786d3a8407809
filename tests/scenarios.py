"""Deterministic churn scenarios shared by the CPU (oracle cross-check) and GPU
(parity) tests. A scenario is a list of per-round event batches; engines expose
apply_events(list[(kind, member)]) and step(1)."""
from __future__ import annotations

import numpy as np

from oracle import philox

JOIN, LEAVE, CRASH = 1, 2, 3


def bootstrap_schedule(n, start=1, introducer=0):
    """C1-style start: one member joins per round, the introducer first (it
    joins through itself, slave/slave.go:288 + :228), then the others in ID
    order."""
    order = [introducer] + [c for c in range(n) if c != introducer]
    return {start + k: [(JOIN, c)] for k, c in enumerate(order)}


def random_churn(n, rounds, seed, p_crash=0.04, p_leave=0.02, p_join=0.05, start_full=True, introducer=0):
    """Per-round batches of crash/leave/join events on a seeded stream; the
    introducer is spared."""
    rng = np.random.default_rng(seed)
    alive = np.ones(n, bool) if start_full else np.zeros(n, bool)
    sched = {}
    for r in range(1, rounds + 1):
        ev = []
        for c in range(n):
            if c == introducer:  # keep the introducer alive so joins can happen
                continue
            u = rng.random()
            if alive[c] and u < p_crash:
                ev.append((CRASH, c))
                alive[c] = False
            elif alive[c] and u < p_crash + p_leave:
                ev.append((LEAVE, c))
                alive[c] = False
            elif not alive[c] and u < p_join:
                ev.append((JOIN, c))
                alive[c] = True
        if ev:
            sched[r] = ev
    return sched


def rejoin_churn(n, rounds, seed, p_out=0.06, p_back=0.5, introducer=0):
    """Members leave (or crash) and come back within a few rounds, again and
    again: the introducer (spared here) still holds the tombstone of a member
    when it rejoins, so its list holds the member twice (SPEC D7), and a
    later LEAVE, REMOVE or detection meets that double entry."""
    rng = np.random.default_rng(seed)
    alive = np.ones(n, bool)
    sched = {}
    for r in range(1, rounds + 1):
        ev = []
        for c in range(n):
            if c == introducer:
                continue
            u = rng.random()
            if alive[c] and u < p_out:
                ev.append((LEAVE if rng.random() < 0.6 else CRASH, c))
                alive[c] = False
            elif not alive[c] and u < p_back:
                ev.append((JOIN, c))
                alive[c] = True
        if ev:
            sched[r] = ev
    return sched


def crash_ids(n, frac, seed, introducer=0):
    """BASELINE configs: crash `frac` of N, IDs drawn by Philox(seed, CRASH);
    the introducer/master is excluded."""
    count = max(1, int(round(n * frac)))
    return philox.sample_distinct(seed, philox.TAG_CRASH, count, n, exclude=(introducer,))


def introducer_outage(sched, I, stops):
    """A copy of `sched` with the events `stops` = [(round, kind), ...] added
    for the introducer I itself: it crashes or leaves, JOINs that arrive while
    it is down reset their rows but are added nowhere, and its own JOIN
    restarts it with an empty list (it joins through itself)."""
    out = {r: list(ev) for r, ev in sched.items()}
    for r, kind in stops:
        out.setdefault(r, []).append((kind, I))
    return out


def full_state(n, hb0=2, ts0=0):
    hb = np.full((n, n), hb0, np.int32)
    ts = np.full((n, n), ts0, np.int32)
    alive = np.ones(n, np.uint8)
    return hb, ts, alive


def short_list_state(n, seed, r0, mid=False):
    """(hb, ts, alive), to import at round r0: every member alive and every
    row full (hb r0 + 2, ts r0) but the last 16, whose lists hold 0, 1, 2 and
    3 members, each with and without the row's own entry, twice over (a list
    of length 0 cannot hold its row, so both of its variants are empty). The
    other entries of a short row are drawn by `seed` and were last heard of
    in round 0, so with r0 > T_fail a short row that passes the guard detects
    them at once and may empty itself after the guard. These are the rows the
    min_members guard decides differently below 4, and the ring senders whose
    targets coincide, name the sender itself, or do not exist. With `mid` the
    8 rows before them hold 4, 5, 6 and 8 members in the same way: the rows a
    threshold of 7 decides differently from the literal 4."""
    rng = np.random.default_rng(seed)
    hb = np.full((n, n), r0 + 2, np.int32)
    ts = np.full((n, n), r0, np.int32)
    alive = np.ones(n, np.uint8)
    shapes = [(ln, own) for ln in (0, 1, 2, 3) for own in (True, False)] * 2
    if mid:
        shapes = [(ln, own) for ln in (4, 5, 6, 8) for own in (True, False)] + shapes
    for k, (ln, own) in enumerate(shapes):
        i = n - len(shapes) + k
        others = np.array([c for c in range(n) if c != i])
        own = own and ln > 0
        keep = rng.choice(others, ln - int(own), replace=False)
        hb[i, :] = -1
        ts[i, :] = 0
        hb[i, keep] = r0 + 2  # (ts stays 0: unheard of since round 0)
        if own:
            hb[i, i] = r0 + 2
            ts[i, i] = r0
    return hb, ts, alive


def sole_detector_state(n, world, seed, n_cols=32, p=0.16, t_fail=16, r0=20, lead=0):
    """(hb, ts, alive, det): a state, to import at round r0, in which n_cols
    crashed members c are each known to themselves, to a fraction p of the
    rows (holders) and to one live row det[c] = j whose entry alone is old enough to be
    detected, in round D = r0 + 1 + lead. With T_cleanup <= T_fail j releases
    c at once (and may merge it back from a holder), so in round D + 1
    REMOVE(c) reaches everyone but j (SPEC D4: a sole detector does not
    message itself): j is then the only sender that still carries c, and a
    row that has c absent and pulls from j must end the round with c present
    (unknown REMOVE, then the merge). Everything else is healthy (hb 100,
    ts r0), so nothing but the REMOVE'd lanes needs the per-cell rule in
    round D + 1. `world` only documents which row shards the caller counts
    (sole_detector_cfg is the matching configuration)."""
    rng = np.random.default_rng(seed)
    hb = np.full((n, n), 100, np.int32)
    ts = np.full((n, n), r0, np.int32)
    alive = np.ones(n, np.uint8)
    crashed = rng.choice(np.arange(1, n), n_cols, replace=False)
    alive[crashed] = 0
    live = np.flatnonzero(alive)
    det = {}
    for c in crashed:
        j = int(rng.choice(live))
        keep = rng.random(n) < p
        keep[j] = keep[c] = True  # (c's own, stopped row lists itself: its heartbeat is the column's base)
        hb[~keep, c] = -1
        ts[~keep, c] = 0
        ts[j, c] = r0 - t_fail + lead
        det[int(c)] = j
    return hb, ts, alive, det


def sole_detector_cfg(seed, t_fail=16):
    """Pull mode, canonical detection, T_cleanup = T_fail."""
    return dict(fanout=4, t_fail=t_fail, t_cleanup=t_fail, seed=0x5EED0E00 + seed)


# (world, rng seed, lead, p) of the sole-detector runs at N = SOLE_N, imported
# at round SOLE_R0: test_sole_detector_scenario.py asserts their preconditions
# on the oracle, test_gpu_rows.py runs them on row shards
SOLE_N, SOLE_R0 = 2048, 20
SOLE_CASES = [(2, 1, 0, 0.16), (3, 2, 0, 0.16)]


def tail_members(n, bounds=()):
    """The members whose cells end a piece of the nibble path's geometry at a
    cluster size n that is no multiple of the 256-member tile: the last
    member, the first cell of the last 16-cell lane and of the last 8-cell
    chunk, both sides of the last tile boundary, and both sides of every
    shard boundary in `bounds` (g * ncs of the column layout, g * nrs of the
    row layout). Sorted, distinct, the introducer 0 spared."""
    last = 256 * ((n - 1) // 256)
    ids = {n - 1, 16 * ((n - 1) // 16), 8 * ((n - 1) // 8), last, last - 1}
    for b in bounds:
        ids |= {b - 1, b}
    return sorted(x for x in ids if 0 < x < n)


def shard_bounds(n, world, layout=0):
    """First member of every shard but the first: columns g * ncs with ncs =
    ceil(n / world) rounded up to 32 (layout 0), rows g * nrs with nrs =
    ceil(n / world) (layout 1), as gh_create_sharded lays them out."""
    per = -(-n // world)
    if layout == 0:
        per = -(-per // 32) * 32
    return [g * per for g in range(1, world) if g * per < n]


# The ragged-N runs (test_ragged_scenario.py asserts their preconditions on
# the oracle, test_gpu_ragged.py runs them): the sizes, each with another
# tail against the 256-member tile, the 16-cell lane and the 8-cell chunk,
RAGGED_NS = (250, 263, 520, 1000, 2049)
RAGGED_ROUNDS, RAGGED_CRASH, RAGGED_REJOIN = 40, 8, 30
# ... (label, n, world, layout) of the sharded runs (layout 1: row shards),
RAGGED_SHARDS = [("cols2", 263, 2, 0), ("cols3", 263, 3, 0), ("cols8_n250", 250, 8, 0),
                 ("rows2", 263, 2, 1), ("rows3", 263, 3, 1), ("rows3_n1000", 1000, 3, 1)]
# ... and the quirk-detection victims: runs of candidates that end on the
# row's last list entry, across the 2,048-cell window edge at N = 2,049.
# Crashed at round 8 like the wave, each is first detected by the few rows
# that pulled from it in its last round, one candidate per row, so no choice
# of victims makes quirk detection differ from canonical; crashed at round 1,
# before their first heartbeat, every row holds them at ts 0 and detects the
# whole run in round 17, where the quirk skips every second candidate.
RAGGED_QUIRK = {263: [254, 255, 256, 261, 262], 2049: [2046, 2047, 2048]}
RAGGED_QUIRK_CRASH = (8, 1)


def ragged_cfg(k=4, detect_mode=0):
    return dict(fanout=k, seed=0x5EED0C10, t_fail=16, t_cleanup=16, detect_mode=detect_mode)


def ragged_wave(n, victims=None, rejoin=True, crash=RAGGED_CRASH):
    """`victims` (tail_members(n) by default) crash at round 8; with `rejoin`
    the last member joins again at round 30, after its REMOVE: its column's
    base jump makes lane jobs of the last, partial lane."""
    victims = tail_members(n) if victims is None else victims
    sched = {crash: [(CRASH, int(c)) for c in victims]}
    if rejoin:
        sched[RAGGED_REJOIN] = [(JOIN, n - 1)]
    return sched


# The tile-width runs (test_tile_width_scenario.py asserts their preconditions
# on the oracle, test_gpu_tile_widths.py runs them): every value
# gh_config.tile_width takes, and the two below the plane's default of 256 at
# which an engine with the sender plane still keeps the 4-bit tier.
TILE_WIDTHS = (8, 16, 32, 64, 128, 256)
TIER_WIDTHS = (64, 128)
WIDTH_NS = (263, 1000)  # the wave's sizes at TIER_WIDTHS
WIDTH_N = 300           # the 16-bit form's size: no multiple of 8, a partial last tile at every width
# ... (label, world, layout) of the sharded runs at N = 263 and at WIDTH_N
WIDTH_SHARDS = [("cols3", 3, 0), ("rows2", 2, 1)]


def tile_bounds(n, tw):
    """First member of the second and of the last tile of `tw` members (64 and
    256 at n = 263, tw = 64; 128 and 896 at n = 1,000, tw = 128)."""
    return sorted(b for b in {tw, tw * ((n - 1) // tw)} if 0 < b < n)


def width_victims(n, tw, world=1, layout=0):
    """tail_members(n) with both sides of the first and of the last tile
    boundary of width `tw` and of every shard boundary."""
    return tail_members(n, tile_bounds(n, tw) + (shard_bounds(n, world, layout) if world > 1 else []))


def width_churn(n=WIDTH_N, rounds=30):
    """(cfg, sched) of the 16-bit form's run at every tile width: seeded churn
    under short timeouts (stopped rows, tombstones, absent cells, releases)."""
    cfg = dict(fanout=3, seed=0x5EED7100, t_fail=4, t_cleanup=6)
    return cfg, random_churn(n, rounds, 0x7101, p_crash=0.04, p_leave=0.02, p_join=0.05)


def width_state(n=WIDTH_N, hb0=2):
    """full_state(n) with one column whose heartbeat stands millions above its
    owner's in every fourth row: wide segments in a 16-bit table from the
    import on (test_gpu_census.escape_state)."""
    hb, ts, alive = full_state(n, hb0=hb0)
    hb[1::4, n - 3] = 5_000_000
    hb[n - 3, n - 3] = hb0
    return hb, ts, alive


# The counter-offset runs (test_counter_scenario.py asserts their
# preconditions on the oracle, test_gpu_counters.py runs them): name ->
# (H, R0). A run starts from full_state(n, hb0=H, ts0=R0) imported at round
# R0 and runs shifted_wave(n, R0): the ragged wave far from round 0. The
# 4-bit tier's per-column base is the owner's heartbeat - 1000 (gh_internal.h
# GH_BASE_LAG), so `base0` takes it through 0; `top` ends with every own
# counter at INT32_MAX - 3; on `cap` the own counters reach INT32_MAX in
# round 33 and round 34 is refused (GH_ERANGE).
I32MAX = 2**31 - 1
COUNTER_OFFSETS = {
    "base0": (985, 0),
    "round985": (2, 985),
    "i16": (2**15 - 12, 2**15 - 14),
    "u16": (2**16 - 12, 2**16 - 14),
    "f24": (2**24 - 12, 2**24 - 14),
    "p30": (2**30, 2**30),
    "hb30": (2**30, 0),
    "round30": (2, 2**30),
    "top": (I32MAX - 43, 7),
    "cap": (I32MAX - 33, 2**24),
}
CAP_ROUNDS = 33  # the rounds `cap` runs before the refusal
# heartbeat u16 with round f24: the N = 2,048 case beside `cap`
COUNTER_MIXED = (2**16 - 12, 2**24 - 14)
STAGGERED_OWN = (2, 990, 2**16 - 6, 2**24 - 6, 2**30, I32MAX - 60)


def counter_state(n, name):
    """(hb, ts, alive, R0) of COUNTER_OFFSETS[name]"""
    h, r0 = COUNTER_OFFSETS[name]
    return full_state(n, hb0=h, ts0=r0) + (r0,)


def shifted_wave(n, r0, victims=None, rejoin=True, crash=RAGGED_CRASH):
    """ragged_wave with its rounds moved by r0"""
    return {r0 + r: ev for r, ev in ragged_wave(n, victims, rejoin, crash).items()}


def staggered_state(n, r0, seed):
    """(hb, ts, alive), to import at round r0: every member running, its own
    counter drawn from STAGGERED_OWN, every view of it lagging by 0..3 (never
    below heartbeat 0) and 0..3 rounds old. Neighbouring columns of one
    8-cell chunk and one 16-cell lane then have bases billions apart; only the
    INT32_MAX - 60 columns reach the cap, 60 rounds on."""
    rng = np.random.default_rng(seed)
    own = np.asarray(STAGGERED_OWN, np.int64)[rng.integers(0, len(STAGGERED_OWN), n)]
    hb = np.maximum(own[None, :] - rng.integers(0, 4, (n, n)), 0)
    ts = r0 - rng.integers(0, 4, (n, n)).astype(np.int64)
    np.fill_diagonal(hb, own)
    np.fill_diagonal(ts, r0)
    return hb.astype(np.int32), ts.astype(np.int32), np.ones(n, np.uint8)


# The fanout runs (test_fanout_scenario.py asserts their preconditions on the
# oracle and on loss_ref.LossModel.peers, test_gpu_fanout.py runs them): every
# value gh_config.fanout takes but the 3 and 4 of the rest of the suite. k >= 5
# takes the 8-sender instantiation of the round kernel and draws 4..7 from the
# second Philox block; k < 3 has neither the sender plane nor the 4-bit tier.
FANOUTS = (1, 2, 5, 6, 7, 8)
FANOUT_NS = (263, 1000)            # the wave's sizes on one engine
FANOUT_COLLAPSE = 1                # the fanout at which the wave's cluster collapses at T_fail = 16
FANOUT_SHARD_KS = (1, 2, 5, 8)
# ... (label, n, world, layout) of the sharded waves
FANOUT_SHARDS = [("cols3", 263, 3, 0), ("cols8", 250, 8, 0), ("rows2", 263, 2, 1), ("rows3", 263, 3, 1)]
FANOUT_LOCKSTEP = ("cols3", "rows2")   # k = 8 also beside one engine
# ... (k, tile width) of the N = WIDTH_N churn
FANOUT_WIDTHS = [(k, tw) for k in (2, 5, 8) for tw in TILE_WIDTHS] + [(1, 8), (1, 256)]
FANOUT_CHURN_KS = (1, 2, 5, 8)
FANOUT_COUNTER_KS = (2, 8)         # the wave far from round 0: from `f24`, and `cap` through its refusal
FANOUT_SEED = 0x5EED0F00
# the seed of fanout k is FANOUT_SEED + 16 * FANOUT_SEED_STEP[k] + k: the first
# step at which every precondition of test_fanout_scenario.py holds (at k = 8
# the sharded inbox shapes need a receiver that draws three crashed senders in
# its second Philox block, at k = 1 cols8's 233 survivors must all fall under
# the guard in one round)
FANOUT_SEED_STEP = {1: 1, 2: 0, 5: 0, 6: 0, 7: 0, 8: 5}


def fanout_cfg(k, t=16, **kw):
    """ragged_cfg's shape at fanout k, T_fail = T_cleanup = t, on the fanout
    runs' own seeds; `kw` adds to or overrides the configuration."""
    return dict(dict(fanout=k, seed=FANOUT_SEED + 16 * FANOUT_SEED_STEP[k] + k, t_fail=t, t_cleanup=t), **kw)


def fanout_victims(n, world=1, layout=0):
    """tail_members(n), on shards with both sides of every shard boundary."""
    return tail_members(n, shard_bounds(n, world, layout) if world > 1 else ())


def fanout_wave(n, world=1, layout=0, r0=0):
    """ragged_wave of fanout_victims (crash at round 8, the last member joins
    again at round 30), its rounds moved by r0."""
    return shifted_wave(n, r0, fanout_victims(n, world, layout))


def fanout_churn(k, **kw):
    """(cfg, sched) of width_churn() at fanout k."""
    cfg, sched = width_churn()
    return dict(cfg, fanout=k, **kw), sched


# The mass crash: a quarter of N = 1,000 stops at round 4 under short
# timeouts, 24 rounds; at k = 5 the detections spread over rounds, at k = 8
# one round detects every victim.
MASS_N, MASS_T_FAIL, MASS_T_CLEANUP, MASS_FRAC, MASS_CRASH, MASS_ROUNDS = 1000, 6, 8, 0.25, 4, 24
MASS_KS = (5, 8)
MASS_SEED_STEP = {5: 0, 8: 0}      # as FANOUT_SEED_STEP, for the mass crash's own preconditions


def fanout_mass(k):
    """(cfg, sched, victims) of the mass crash at fanout k."""
    cfg = fanout_cfg(k, t_fail=MASS_T_FAIL, t_cleanup=MASS_T_CLEANUP, seed=FANOUT_SEED + 16 * MASS_SEED_STEP[k] + k)
    victims = crash_ids(MASS_N, MASS_FRAC, cfg["seed"])
    return cfg, {MASS_CRASH: [(CRASH, int(c)) for c in victims]}, victims


# The tiny clusters: (n, k) with N <= k + 1 at k = 8 (every receiver's draws
# repeat senders from N <= 8 down), min_members = 2, T_fail = T_cleanup = 5,
# the last member crashes at round 6.
TINY_NS, TINY_KS = (2, 3, 5, 8, 9), (1, 8)
TINY_TABLE = [(n, k) for k in TINY_KS for n in TINY_NS]
TINY_T, TINY_CRASH, TINY_ROUNDS = 5, 6, 20
TINY_SHARDED = (9, 8)              # (n, k) on two column shards and on two row shards
TINY_ONE_TILE = (5, 8, (8, 256))   # (n, k, tile widths): one tile, mostly padding


def fanout_tiny(n, k, **kw):
    """(cfg, sched) of a tiny cluster."""
    return fanout_cfg(k, TINY_T, min_members=2, **kw), {TINY_CRASH: [(CRASH, n - 1)]}


# Ensembles at the fanouts ensemble_ref.GROUPS leaves out: name -> the
# arguments of ensemble_ref.case for its two clusters (n, k, t_fail, t_cleanup,
# rate, rounds, crash, seed); the second cluster of every group has no loss.
FANOUT_ENSEMBLES = {
    "n16k2": [(16, 2, 8, 8, 0.2, 24, {4: [15]}, 0x5EED0F52), (16, 2, 9, 6, 0.0, 24, {3: [0, 7]}, 0x5EED0F53)],
    "n33k5": [(33, 5, 5, 5, 0.3, 24, {4: [1, 32]}, 0x5EED0F55), (33, 5, 4, 6, 0.0, 24, {6: [16]}, 0x5EED0F56)],
    "n64k6": [(64, 6, 5, 5, 0.3, 24, {4: [0, 63]}, 0x5EED0F57), (64, 6, 6, 4, 0.0, 24, {5: [31, 32]}, 0x5EED0F58)],
    "n128k7": [(128, 7, 5, 5, 0.3, 20, {4: [5, 64, 127]}, 0x5EED0F59), (128, 7, 4, 7, 0.0, 20, {3: [127]}, 0x5EED0F5A)],
}

# GH_ORDER_APPEND at k = 8: N = 100 in pull mode from a full start against
# oracle/listsim.py (its T_fail = T_cleanup = 5), seeded churn with re-adds.
APPEND_N, APPEND_K, APPEND_ROUNDS, APPEND_SEED = 100, 8, 30, 0x5EED0F80


def fanout_append_churn():
    return random_churn(APPEND_N, APPEND_ROUNDS, 0xF81, p_crash=0.03, p_leave=0.02, p_join=0.08)


def masked(hb, ts):
    """ts of absent cells carries no meaning in the list model (listsim keeps
    no Member for them); compare it only where hb != -1."""
    t = ts.copy()
    t[hb == -1] = 0
    return hb, t


def export_view(hb, ts, round_, t_cleanup):
    """A dense (hb, ts) state as gh_export_state / or_export_state present it
    (SPEC.md §1): ts 0 for absent cells, and with T_cleanup < 30 a tombstone
    older than T_cleanup + 1 rounds at exactly T_cleanup + 1 rounds (round_ =
    last completed)."""
    t = ts.astype(np.int64).copy()
    t[hb == -1] = 0
    if t_cleanup < 30:
        now = round_ + 1
        old = (hb == -2) & (now - t > t_cleanup + 1)
        t[old] = now - (t_cleanup + 1)
    return hb, t.astype(np.int32)


def shadow_view(sh, round_, t_cleanup):
    """D7 shadow entries (the ts of the introducer's RecentFailList entry
    beside a present member, INT32_MIN for none) as export_view presents a
    tombstone's ts: the engine keeps a tombstone's age saturated at
    T_cleanup + 1 rounds, which is all cleanFailList (slave/slave.go:490) can
    tell, and an introducer whose list is under the guard threshold never
    cleans, so its entries do grow older than that."""
    none = np.iinfo(np.int32).min
    t = np.asarray(sh).astype(np.int64)
    if t_cleanup < 30:
        now = round_ + 1
        old = (t != none) & (now - t > t_cleanup + 1)
        t[old] = now - (t_cleanup + 1)
    return t.astype(np.int32)
