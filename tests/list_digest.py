"""Recorded listsim runs for GPU tests whose literal-list reference is too
slow to replay in the suite (oracle/listsim.py is O(N^2) Python per round: a
minute at N=300): per round the counters, failed set and detectors in plain
and SHA-256 digests of hb, ts (as exported), alive, every row's list order and
the introducer's double entries (the D7 shadow vector, as scenarios.shadow_view
presents it).

    python tests/list_digest.py        # rewrites tests/golden/append_introducer157.json

tests/test_list_digest.py replays the first rounds of every case on the CPU
against the file; tests/test_gpu_config_space.py compares the engine with it."""
import hashlib
import json
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "append_introducer157.json"
NO_SHADOW = np.iinfo(np.int32).min

# the churn of test_gpu_config_space.test_introducer_off_zero under GH_ORDER_APPEND
N, I, ROUNDS, T_FAIL, T_CLEANUP = 300, 157, 40, 4, 6
CASES = {"ring_quirk": dict(peer_mode="ring", quirk=True, seed=0x5EED0E21, churn=0xD8),
         "pull": dict(peer_mode="pull", quirk=False, seed=0x5EED0E20, churn=0xD7)}


def _h(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()[:32]


def round_record(stats, hb, ts, alive, failed, detectors, lists, shadow):
    """One round's record; ts as gh_export_state presents it."""
    flat = np.concatenate([np.asarray([len(x)] + list(x), np.int32) for x in lists])
    return dict(stats={k: int(v) for k, v in stats.items()}, failed=[int(c) for c in failed],
                detectors=sorted(int(c) for c in detectors), hb=_h(hb, np.int32), ts=_h(ts, np.int32),
                alive=_h(alive, np.uint8), lists=_h(flat, np.int32), shadow=_h(shadow, np.int32),
                dual=int((np.asarray(shadow) != NO_SHADOW).sum()),
                reordered=sum(1 for x in lists if list(x) != sorted(x)))


def listsim_shadow(ls, introducer):
    nd = ls.nodes[introducer]
    out = np.full(ls.n, NO_SHADOW, np.int32)
    present = {m.addr for m in nd.members}
    for f in nd.recent_fail:
        if f.addr in present:
            out[f.addr] = f.ts
    return out


def schedule(case):
    import scenarios as sc
    return sc.rejoin_churn(N, ROUNDS, CASES[case]["churn"], introducer=I)


def replay(case, rounds):
    """listsim's records of the first `rounds` rounds of a case"""
    import scenarios as sc
    import oracle.listsim as L
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
            out.append(round_record(st, h, sc.export_view(h, t, r, T_CLEANUP)[1], a, ls.last_failed,
                                    ls.last_detectors, [[m.addr for m in nd.members] for nd in ls.nodes],
                                    sc.shadow_view(listsim_shadow(ls, I), r, T_CLEANUP)))
    finally:
        L.T_FAIL, L.T_CLEANUP = 5, 5
    return out


def load():
    return json.loads(GOLDEN.read_text())


if __name__ == "__main__":
    sys.path[:0] = [str(HERE.parent), str(HERE)]
    GOLDEN.parent.mkdir(exist_ok=True)
    GOLDEN.write_text(json.dumps({case: replay(case, ROUNDS) for case in CASES}, indent=0) + "\n")
