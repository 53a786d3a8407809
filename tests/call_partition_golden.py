"""Recorded listsim runs for tests/test_gpu_call_partition.py's GH_ORDER_APPEND
cases, in the records of tests/list_digest.py (its replay of 40 rounds at
N=300 takes a minute per case): the D7 churn of
test_gpu_config_space.test_introducer_off_zero with introducer 157, its event
batches GAP rounds apart instead of one a round, so that a gh_step call can
hold several rounds between two of them (a call ends before every round that
has events).

    python tests/call_partition_golden.py   # rewrites tests/golden/call_partition_append.json

tests/test_oracle_step_batch.py replays the first rounds of every case on the
CPU against the file."""
import json
import pathlib
import sys

HERE = pathlib.Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "call_partition_append.json"

N, I, ROUNDS, GAP, T_FAIL, T_CLEANUP = 300, 157, 40, 4, 4, 6
CASES = {"ring_quirk": dict(peer_mode="ring", quirk=True, seed=0x5EED0F21, churn=0xD8),
         "pull": dict(peer_mode="pull", quirk=False, seed=0x5EED0F20, churn=0xD7)}


def spread(sched, gap):
    """Batch s of `sched` (s = 1, 2, ...) in round (s - 1) * gap + 1."""
    return {(s - 1) * gap + 1: ev for s, ev in sched.items()}


def schedule(case):
    import scenarios as sc
    return spread(sc.rejoin_churn(N, ROUNDS // GAP, CASES[case]["churn"], introducer=I), GAP)


def replay(case, rounds):
    """listsim's records of the first `rounds` rounds of a case"""
    import list_digest as ld
    import oracle.listsim as L
    import scenarios as sc
    c = CASES[case]
    sched = schedule(case)
    hb, ts, alive = sc.full_state(N)
    ls = L.ListSim.from_dense(hb, ts, alive, 0, seed=c["seed"], peer_mode=c["peer_mode"], fanout=3,
                              quirk=c["quirk"], order="append", introducer=I)
    out = []
    L.T_FAIL, L.T_CLEANUP = T_FAIL, T_CLEANUP
    try:
        for r in range(1, rounds + 1):
            if r in sched:
                ls.apply_events(sched[r])
            st = ls.step(1)
            h, t, a = ls.dense()
            out.append(ld.round_record(st, h, sc.export_view(h, t, r, T_CLEANUP)[1], a, ls.last_failed,
                                       ls.last_detectors, [[m.addr for m in nd.members] for nd in ls.nodes],
                                       sc.shadow_view(ld.listsim_shadow(ls, I), r, T_CLEANUP)))
    finally:
        L.T_FAIL, L.T_CLEANUP = 5, 5
    return out


def load():
    return json.loads(GOLDEN.read_text())


if __name__ == "__main__":
    sys.path[:0] = [str(HERE.parent), str(HERE)]
    GOLDEN.parent.mkdir(exist_ok=True)
    GOLDEN.write_text(json.dumps({case: replay(case, ROUNDS) for case in CASES}, indent=0) + "\n")
