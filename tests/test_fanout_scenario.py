"""Preconditions of the fanout runs of tests/test_gpu_fanout.py (scenarios.py
FANOUTS, fanout_cfg, fanout_victims and what follows them), on the CPU oracle
and on loss_ref.LossModel.peers (the Python restatement of the peer draws)
alone, in the style of test_ragged_scenario.py. The GPU module compares the
engine with the oracle at k = 1, 2 and 5..8; that only reaches the code it is
after -- the round kernel's 8-sender instantiation with five to eight senders
per row step, draws 4..7 of the second Philox block on shards, the collapse
at k = 1, clusters with N <= k + 1 -- if the reference run goes through those
states. Every condition is on the inputs (they keep the GPU tests from passing
vacuously), none is a tolerance, none is asserted on the engine."""
import numpy as np
import pytest

import ensemble_ref as er
import loss_ref as lr
import scenarios as sc
from test_ragged_scenario import failed_of

ROUNDS = sc.RAGGED_ROUNDS
LAG_MAX = 11                     # csrc/gh_internal.h c4_enc: the 4-bit tier's window
BEFORE_REJOIN = sc.RAGGED_REJOIN - 1
HEALTHY = [k for k in sc.FANOUTS if k != sc.FANOUT_COLLAPSE]

_TRACES = {}


def wave_trace(om, n, cfg, sched, rounds=ROUNDS, hb0=2, r0=0, init=None):
    """The schedule on the oracle from full_state(n, hb0, r0) (or `init`)
    imported at round r0, `sched` keyed by the rounds r0 + 1 ..: per round a
    dict of the stats, the failed set, the largest lag of a running row's view
    of a running member, alive and the present cells (hb >= 0) after the round.
    A round the oracle refuses (GH_ERANGE) ends the trace. Kept per case."""
    key = (n, tuple(sorted(cfg.items())), tuple(sorted((r, tuple(ev)) for r, ev in sched.items())), rounds, hb0, r0,
           init is None)
    if key in _TRACES:
        return _TRACES[key]
    orc = om.Oracle(om.default_config(n, **cfg), threads=8)
    out = []
    try:
        orc.import_state(*(init or sc.full_state(n, hb0=hb0, ts0=r0)), r0)
        for r in range(r0 + 1, r0 + rounds + 1):
            if sched.get(r):
                orc.apply_events(sched[r])
            rc, st = orc.step_rc(1)
            if rc != 0:
                assert rc == om.GH_ERANGE and st["rounds"] == 0, (r, rc, st)
                break
            hb, ts, alive = orc.export_state()
            run = alive != 0
            own = hb.diagonal().astype(np.int64)
            views = run[:, None] & run[None, :] & (hb >= 0)
            out.append(dict(st=st, failed=failed_of(orc), lag=int(np.where(views, own[None, :] - hb, 0).max()),
                            alive=run, present=hb >= 0, tombs=int((hb[run] == -2).sum()),
                            absent=int((hb[run] == -1).sum())))
    finally:
        orc.close()
    _TRACES[key] = out
    return out


def detection_rounds(trace):
    return [r for r, x in enumerate(trace, 1) if x["failed"]]


def assert_healthy_wave(trace, n, victims, what):
    """Every victim detected before the rejoin, tombstones the round after the
    first detection, releases later, no REMOVE of an unknown member, every
    running row active in every round, and nobody but a victim detected."""
    assert len(trace) == ROUNDS, (what, len(trace))
    det = detection_rounds(trace)
    seen = set().union(*(x["failed"] for x in trace[:BEFORE_REJOIN]))
    assert set(victims) <= seen, (what, sorted(set(victims) - seen))
    assert set().union(*(x["failed"] for x in trace)) <= set(victims), what
    d = det[0]
    assert sc.RAGGED_CRASH < d < sc.RAGGED_REJOIN, (what, det)
    tomb = [r for r, x in enumerate(trace, 1) if x["st"]["tombstoned"] > 0]
    assert d + 1 in tomb, (what, det, tomb)
    tombstoned = sum(x["st"]["tombstoned"] for x in trace)
    released = sum(x["st"]["released"] for x in trace[d:])
    assert released > 0, what
    assert all(x["st"]["remove_unknown"] == 0 for x in trace), what
    assert all(x["st"]["active_rows"] >= n - len(victims) for x in trace), what
    lag = max(x["lag"] for x in trace)
    print(f"{what}: victims {list(victims)}, detection {det}, REMOVE {tomb}, tombstoned {tombstoned}, released "
          f"{released}, max lag {lag}")
    return det


def assert_collapse(trace, n, victims, what):
    """k = 1: running members are detected, REMOVEs reach rows that never knew
    the member, some round has no active row, and the views leave the 4-bit
    tier's window."""
    assert len(trace) == ROUNDS, (what, len(trace))
    false_pos = set().union(*(x["failed"] for x in trace)) - set(victims)
    det = sum(x["st"]["detections"] for x in trace)
    unknown = sum(x["st"]["remove_unknown"] for x in trace)
    empty = [r for r, x in enumerate(trace, 1) if x["st"]["active_rows"] == 0]
    lag = max(x["lag"] for x in trace)
    print(f"{what}: victims {list(victims)}, detections {det}, running members detected {len(false_pos)}, "
          f"remove_unknown {unknown}, rounds without an active row {empty}, max lag {lag}")
    assert false_pos and unknown > 0 and empty and lag > LAG_MAX, what


# ---- the wave: one engine and shards --------------------------------------------------------

def test_fanout_tables():
    """The tables the GPU module is parametrised by."""
    assert sc.FANOUTS == (1, 2, 5, 6, 7, 8) and not set(sc.FANOUTS) & {3, 4}
    assert len(sc.FANOUT_WIDTHS) == 20 and {tw for k, tw in sc.FANOUT_WIDTHS if k == 1} == {8, 256}
    for k in (2, 5, 8):
        assert [tw for kk, tw in sc.FANOUT_WIDTHS if kk == k] == list(sc.TILE_WIDTHS)
    assert len({sc.fanout_cfg(k)["seed"] for k in sc.FANOUTS}) == len(sc.FANOUTS)
    assert sc.fanout_cfg(5) == dict(fanout=5, seed=sc.fanout_cfg(5)["seed"], t_fail=16, t_cleanup=16)
    assert sc.fanout_cfg(8, 5, min_members=2)["min_members"] == 2 and sc.fanout_cfg(8, 5)["t_cleanup"] == 5
    for label, n, world, layout in sc.FANOUT_SHARDS:
        bounds, victims = sc.shard_bounds(n, world, layout), sc.fanout_victims(n, world, layout)
        assert len(bounds) == world - 1, (label, bounds)
        assert all(b - 1 in victims and b in victims for b in bounds), (label, bounds, victims)
        assert set(sc.tail_members(n)) <= set(victims)
    assert sc.fanout_victims(263) == sc.tail_members(263)
    assert set(sc.FANOUT_LOCKSTEP) <= {x[0] for x in sc.FANOUT_SHARDS}
    assert all(n <= k + 1 for n, k in sc.TINY_TABLE if k == 8) and sc.TINY_SHARDED in sc.TINY_TABLE
    assert sc.TINY_ONE_TILE[:2] in sc.TINY_TABLE


@pytest.mark.parametrize("k", sc.FANOUTS)
@pytest.mark.parametrize("n", sc.FANOUT_NS)
def test_fanout_wave_preconditions(oracle_mod, n, k):
    """tail_members(n) crash at round 8, the last joins again at round 30: a
    healthy run at k = 2 and 5..8, the collapse at k = 1."""
    victims = sc.fanout_victims(n)
    trace = wave_trace(oracle_mod, n, sc.fanout_cfg(k), sc.fanout_wave(n))
    if k == sc.FANOUT_COLLAPSE:
        assert_collapse(trace, n, victims, f"N={n} k={k}")
    else:
        assert_healthy_wave(trace, n, victims, f"N={n} k={k}")


@pytest.mark.parametrize("k", sc.FANOUT_SHARD_KS)
@pytest.mark.parametrize("label,n,world,layout", sc.FANOUT_SHARDS, ids=[x[0] for x in sc.FANOUT_SHARDS])
def test_fanout_shard_wave_preconditions(oracle_mod, label, n, world, layout, k):
    """The sharded waves: the victims also stand on both sides of every shard
    boundary of that layout."""
    victims = sc.fanout_victims(n, world, layout)
    trace = wave_trace(oracle_mod, n, sc.fanout_cfg(k), sc.fanout_wave(n, world, layout))
    if k == sc.FANOUT_COLLAPSE:
        assert_collapse(trace, n, victims, f"{label}: N={n} k={k}")
    else:
        assert_healthy_wave(trace, n, victims, f"{label}: N={n} k={k}")


# ---- the inbox shapes --------------------------------------------------------------------------

def valid_draws(trace, n, k, seed, r, state0=None):
    """(peers [n][k], valid [n][k]) of round r <= BEFORE_REJOIN of a healthy
    wave: draw t of receiver i is a message (round.hip k_peers_pull; SPEC §2
    step 6) iff i runs, the sender runs and is active, and the sender's
    snapshot holds i. In these rounds every running row is active
    (assert_healthy_wave: active_rows >= N - |victims|), nobody but a victim is
    ever detected, and no event but the crash has happened, so a sender's
    snapshot holds a running receiver iff its row held it after round r - 1."""
    assert 1 <= r <= BEFORE_REJOIN
    peers = lr.LossModel(n, k, seed=seed).peers(r)
    alive = trace[r - 1]["alive"]
    held = trace[r - 2]["present"] if r > 1 else np.ones((n, n), bool)
    assert trace[r - 1]["st"]["active_rows"] == int(alive.sum())
    rows = np.arange(n)[:, None]
    return peers, alive[:, None] & alive[peers] & held[peers, rows]


def shard_size(n, world, layout):
    """Members per shard: columns ceil(n / world) rounded up to 32, rows ceil(n / world)."""
    per = -(-n // world)
    return -(-per // 32) * 32 if layout == 0 else per


def inbox_shapes(trace, n, k, seed, world=1, layout=0):
    """Over the rounds 1..BEFORE_REJOIN: how many (round, receiver) pairs have
    exactly k valid senders, between 5 and k - 1, a sender twice among the
    valid draws, valid senders on min(k, world) shards, and one valid draw in
    the second block (draws 4..k - 1), and valid draws in the first block only."""
    seen = dict(full=0, five_to_k1=0, twice=0, all_ranks=0, lone_second=0, no_second=0)
    per = shard_size(n, world, layout)
    for r in range(1, BEFORE_REJOIN + 1):
        peers, ok = valid_draws(trace, n, k, seed, r)
        cnt = ok.sum(1)
        seen["full"] += int((cnt == k).sum())
        seen["five_to_k1"] += int(((cnt >= 5) & (cnt <= k - 1)).sum())
        for i in np.flatnonzero(cnt >= 2):
            s = peers[i][ok[i]]
            seen["twice"] += int(len(set(s.tolist())) < len(s))
            seen["all_ranks"] += int(len(set((s // per).tolist())) == min(k, world))
        second = ok[:, 4:].sum(1)
        seen["lone_second"] += int((second == 1).sum())
        seen["no_second"] += int(((second == 0) & (cnt > 0)).sum())
    return seen


@pytest.mark.parametrize("k", [k for k in sc.FANOUTS if k >= 5])
@pytest.mark.parametrize("n", sc.FANOUT_NS)
def test_fanout_inbox_shapes(oracle_mod, n, k):
    """k >= 5 on one engine: some receiver has exactly k valid senders (the
    whole second int4 of s_inb / s_isl), some between 5 and k - 1 (from k = 6
    on: no such count exists at k = 5), some the same sender twice."""
    cfg = sc.fanout_cfg(k)
    trace = wave_trace(oracle_mod, n, cfg, sc.fanout_wave(n))
    seen = inbox_shapes(trace, n, k, cfg["seed"])
    print(f"N={n} k={k}: (round, receiver) pairs over the rounds 1..{BEFORE_REJOIN}: {seen}")
    assert seen["full"] > 0 and seen["twice"] > 0, seen
    assert seen["five_to_k1"] > 0 or k == 5, seen


@pytest.mark.parametrize("k", [k for k in sc.FANOUT_SHARD_KS if k >= 5])
@pytest.mark.parametrize("label,n,world,layout", sc.FANOUT_SHARDS, ids=[x[0] for x in sc.FANOUT_SHARDS])
def test_fanout_shard_inbox_shapes(oracle_mod, label, n, world, layout, k):
    """k = 5 and 8 on shards, additionally: some receiver's valid senders
    stand on every shard (on k of them where k < world: 5 of cols8's 8), and
    some draw q >= 4 is the only valid draw of its receiver's second block.
    At k = 8 that takes three crashed senders among the draws 4..7 (the seed
    is chosen for it, scenarios.FANOUT_SEED_STEP); at k = 5 the block holds
    draw 4 alone, so there a receiver whose draw 4 is the crashed one (valid
    draws in the first block only) is asked for as well."""
    cfg = sc.fanout_cfg(k)
    trace = wave_trace(oracle_mod, n, cfg, sc.fanout_wave(n, world, layout))
    seen = inbox_shapes(trace, n, k, cfg["seed"], world, layout)
    print(f"{label}: N={n} k={k}: (round, receiver) pairs over the rounds 1..{BEFORE_REJOIN}: {seen}")
    assert seen["full"] > 0 and seen["twice"] > 0 and (seen["five_to_k1"] > 0 or k == 5), seen
    assert seen["all_ranks"] > 0 and seen["lone_second"] > 0, seen
    assert seen["no_second"] > 0 or k != 5, seen


# ---- the churn at N = 300 -------------------------------------------------------------------------

@pytest.mark.parametrize("k", sc.FANOUT_CHURN_KS)
def test_fanout_churn_preconditions(oracle_mod, k):
    """width_churn() from width_state() at fanout 1, 2, 5 and 8 (the run of
    every tile width): the table holds stopped rows, tombstones in running rows
    and absent cells in at least half of the rounds; detections, REMOVEs,
    releases and REMOVEs of unknown members all happen."""
    n, rounds = sc.WIDTH_N, 30
    cfg, sched = sc.fanout_churn(k)
    assert cfg["fanout"] == k and cfg["seed"] == sc.width_churn()[0]["seed"]
    trace = wave_trace(oracle_mod, n, cfg, sched, rounds, init=sc.width_state(n))
    assert len(trace) == rounds
    seen = dict(stopped=sum(int((~x["alive"]).any()) for x in trace), tombs=sum(int(x["tombs"] > 0) for x in trace),
                absent=sum(int(x["absent"] > 0) for x in trace))
    tot = {f: sum(x["st"][f] for x in trace) for f in ("detections", "tombstoned", "released", "remove_unknown")}
    print(f"N={n} churn k={k}: rounds with (stopped rows, tombstones, absent cells) {seen}, totals {tot}")
    assert all(v >= rounds // 2 for v in seen.values()), seen
    assert all(v > 0 for v in tot.values()), tot


# ---- the mass crash -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sc.MASS_KS)
def test_fanout_mass_crash_preconditions(oracle_mod, k):
    """A quarter of N = 1,000 stops at round 4, T_fail = 6, T_cleanup = 8: at
    k = 5 the detections spread over at least three rounds and include running
    members, at k = 8 one round detects all 250 victims."""
    cfg, sched, victims = sc.fanout_mass(k)
    assert len(victims) == 250 and len(set(victims)) == 250 and 0 not in victims
    trace = wave_trace(oracle_mod, sc.MASS_N, cfg, sched, sc.MASS_ROUNDS)
    assert len(trace) == sc.MASS_ROUNDS
    per_round = {r: (len(x["failed"]), x["st"]["detections"]) for r, x in enumerate(trace, 1) if x["failed"]}
    false_pos = set().union(*(x["failed"] for x in trace)) - set(victims)
    print(f"mass crash k={k}: (failed members, detections) by round {per_round}, running members detected "
          f"{len(false_pos)}")
    assert set(victims) <= set().union(*(x["failed"] for x in trace))
    if k == 5:
        assert len(per_round) >= 3 and false_pos, per_round
    else:
        assert any(set(victims) <= x["failed"] for x in trace), per_round


# ---- tiny clusters -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", sc.TINY_TABLE)
def test_fanout_tiny_preconditions(oracle_mod, n, k):
    """N in {2, 3, 5, 8, 9} at k = 1 and 8, min_members = 2, T = 5, the last
    member crashes at round 6: it is detected; at k = 8 cells merge in every
    round before the crash, and from N = 8 down (k > N - 1) every receiver
    draws some sender twice in every round ((u * (n - 1)) >> 32 takes N - 1
    values)."""
    cfg, sched = sc.fanout_tiny(n, k)
    assert cfg["min_members"] == 2 and sched == {sc.TINY_CRASH: [(sc.CRASH, n - 1)]}
    trace = wave_trace(oracle_mod, n, cfg, sched, sc.TINY_ROUNDS)
    assert len(trace) == sc.TINY_ROUNDS
    det = [r for r, x in enumerate(trace, 1) if n - 1 in x["failed"]]
    merged = [x["st"]["merged_cells"] for x in trace]
    print(f"tiny N={n} k={k}: the victim detected in {det}, merged cells per round {merged}")
    # (the crash takes effect before round 6's detection step; at k = 1 some row's view of the member is
    # already T rounds old by then, at k = 8 every view is fresh and the detection waits for round 6 + T)
    assert any(d >= sc.TINY_CRASH for d in det), det
    assert k == 1 or det[0] >= sc.TINY_CRASH + sc.TINY_T, det
    if k == 8:
        assert all(m > 0 for m in merged[:sc.TINY_CRASH - 1]), merged
        model = lr.LossModel(n, k, seed=cfg["seed"])
        for r in range(1, sc.TINY_ROUNDS + 1):
            peers = model.peers(r)
            assert ((peers >= 0) & (peers < n) & (peers != np.arange(n)[:, None])).all()
            distinct = [len(set(row.tolist())) for row in peers]
            assert n > 8 or all(d < k for d in distinct), (r, distinct)
            assert all(d <= n - 1 for d in distinct), (r, distinct)


# ---- far from round 0 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", sc.FANOUT_COUNTER_KS)
@pytest.mark.parametrize("name", ["f24", "cap"])
def test_fanout_counter_preconditions(oracle_mod, name, k):
    """The wave at N = 263, k = 2 and 8 from the counter offsets `f24` (the
    whole healthy wave, heartbeats and rounds through 2^24) and `cap` (33
    rounds run, the 34th is refused with every own counter at INT32_MAX; the
    detections lie inside)."""
    n = 263
    h, r0 = sc.COUNTER_OFFSETS[name]
    victims = sc.fanout_victims(n)
    trace = wave_trace(oracle_mod, n, sc.fanout_cfg(k), sc.fanout_wave(n, r0=r0), ROUNDS, hb0=h, r0=r0)
    if name == "f24":
        assert_healthy_wave(trace, n, victims, f"f24: N={n} k={k}")
        assert h + ROUNDS > 2**24 > h and r0 + ROUNDS > 2**24 > r0
    else:
        assert len(trace) == sc.CAP_ROUNDS and h + sc.CAP_ROUNDS == sc.I32MAX
        det = detection_rounds(trace)
        print(f"cap: N={n} k={k}: {len(trace)} rounds run, detection {det}")
        assert det and set(victims) <= set().union(*(x["failed"] for x in trace))
        assert any(x["st"]["tombstoned"] > 0 for x in trace)


# ---- lossy links at k = 8 on shards ---------------------------------------------------------------------------

@pytest.mark.parametrize("label", sc.FANOUT_LOCKSTEP)
def test_fanout_lossy_shards_preconditions(label):
    """test_gpu_loss.CASES["k8"] (N = 520, rate 0.3, 15 rounds) on cols3 and
    rows2: on the model, messages of the draws 4..7 are sent and dropped, by
    senders of every shard (k_peers_rows counts them on the sender's owner)."""
    import test_gpu_loss as tl
    case = tl.CASES["k8"]
    n, k = case["n"], case["cfg"]["fanout"]
    assert (n, k, case["rounds"]) == (520, 8, 15)
    world, layout = next((w, lay) for lb, _, w, lay in sc.FANOUT_SHARDS if lb == label)
    per = shard_size(n, world, layout)
    sent = np.zeros((world, k), np.int64)
    lost = np.zeros((world, k), np.int64)

    def per_round(m, st):
        # the round's messages once more, from the state the round left: the senders' snapshots are
        # not kept, so count the draws alone (every running receiver's draw of a running sender)
        r = m.round
        peers = m.peers(r)
        run = m.alive.astype(bool)
        ok = run[:, None] & run[peers]
        w = lr.blocks(m.seed, np.arange(n)[:, None], r, lr.TAG_LINK, np.arange(k)[None, :])
        drop = ok & (lr.hits(m.out[peers], w[0]) | lr.hits(m.inn[:, None], w[1]))
        for q in range(k):
            np.add.at(sent[:, q], peers[ok[:, q], q] // per, 1)
            np.add.at(lost[:, q], peers[drop[:, q], q] // per, 1)

    m = lr.run_model(case, True, per_round)
    total_sent, total_dropped = m.loss_stats()
    print(f"k8 on {label}: sent {total_sent}, dropped {total_dropped}; draws of running senders by (shard, draw) "
          f"{sent.tolist()}, of them lost {lost.tolist()}")
    assert total_dropped > 0 and total_sent > total_dropped
    assert (sent[:, 4:] > 0).all() and (lost[:, 4:] > 0).all(), (sent, lost)


# ---- ensembles ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.FANOUT_ENSEMBLES))
def test_fanout_ensemble_preconditions(name):
    """One group each at k = 2, 5, 6, 7 (ensemble_ref.GROUPS has 1, 3, 4, 8):
    two clusters of one size between 16 and 128, the first with loss; on
    LossModel both detect their victims, the lossy one drops messages."""
    cases = [er.case(*a[:7], seed=a[7]) for a in sc.FANOUT_ENSEMBLES[name]]
    assert len(cases) == 2 and 16 <= cases[0]["n"] <= 128
    assert len({(c["n"], c["k"], c["rounds"], c["min_members"]) for c in cases}) == 1
    assert cases[0]["k"] in (2, 5, 6, 7) and name not in er.GROUPS
    for b, c in enumerate(cases):
        tr = er.run(er.model(c), c["rounds"], c["crash"])
        crashed = {x for ms in c["crash"].values() for x in ms}
        found = {x for x in crashed if tr[-1]["detect"][0][x] > 0}
        fig = {f: er.total(tr, f) for f in ("detections", "tombstoned", "released", "merged_cells", "sent", "dropped")}
        print(f"{name} cluster {b}: victims detected {sorted(found)} of {sorted(crashed)}, {fig}")
        assert found == crashed and fig["merged_cells"] > 0 and fig["sent"] > 0
        assert (fig["dropped"] > 0) == (b == 0), fig


# ---- append order ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quirk", [False, True], ids=["canonical", "quirk"])
def test_fanout_append_preconditions(quirk):
    """GH_ORDER_APPEND at k = 8, N = 100 in pull mode on oracle/listsim.py:
    members are detected and re-added, the lists leave ID order, and receivers
    hold five to eight senders in received-list order."""
    from oracle.listsim import ListSim
    n, k = sc.APPEND_N, sc.APPEND_K
    sched = sc.fanout_append_churn()
    ls = ListSim.from_dense(*sc.full_state(n), 0, seed=sc.APPEND_SEED, peer_mode="pull", fanout=k, quirk=quirk,
                            order="append")
    reordered = detections = 0
    for r in range(1, sc.APPEND_ROUNDS + 1):
        if sched.get(r):
            ls.apply_events(sched[r])
        st = ls.step(1)
        detections += st["detections"]
        reordered = max(reordered, sum(1 for nd in ls.nodes if [m.addr for m in nd.members] != sorted(m.addr for m in nd.members)))
    joins = sum(kind == sc.JOIN for ev in sched.values() for kind, _ in ev)
    print(f"append k={k} {'quirk' if quirk else 'canonical'}: detections {detections}, rows out of ID order {reordered}, "
          f"joins {joins}")
    assert detections > 0 and reordered > 0 and joins > 0
