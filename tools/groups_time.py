"""Times gh_groups beside gh_census and k_round on one engine in one run
(DESIGN.md "Groups"): the bench's headline workload (N=65,536, k=4 pull, seed
0x5EED0003, T_fail = T_cleanup = 16, full start), 12 warm-up rounds, then the
minimum and median wall time of 20 groups() calls and of 20 census() calls,
each after a sync(), and k_round's average launch time (set_timing /
read_timing) over 20 rounds of the same engine. A second leg splits the
cluster even / odd (set_partition) and times both calls again after 20 and
after 40 rounds, off the healthy path. --host-n N (0: skip) times the host alternative once at
that size: export_state() plus the numpy reference (tests/groups_ref.py).
Prints one JSON line.

    python tools/groups_time.py [--n N] [--calls 20] [--rounds 20] [--host-n 16384]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

REPO = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "p2p-file-system-with-gossip-detect-failure-management_amd")]

import numpy as np  # noqa: E402

import gossipsim as gs  # noqa: E402


def timed(eng, call, calls):
    call()  # (the first call allocates)
    ms, out = [], None
    for _ in range(calls):
        eng.sync()
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_min": round(min(ms), 4), "ms_median": round(statistics.median(ms), 4), "calls": calls}, out


def leg(eng, calls):
    g_t, g = timed(eng, eng.groups, calls)
    c_t, _ = timed(eng, eng.census, calls)
    tier = eng.tier_info(full=True)
    return {"groups": g_t, "census": c_t, "groups_over_census": round(g_t["ms_median"] / c_t["ms_median"], 3),
            "passes": g.passes, "n_groups": g.n_groups, "n_views": g.n_views,
            "sizes_largest": sorted(g.sizes().values(), reverse=True)[:4], "table_in_tier": tier[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--fanout", type=int, default=4)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0003)
    ap.add_argument("--t-fail", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-n", type=int, default=16384)
    args = ap.parse_args()
    n = args.n
    cfg = dict(fanout=args.fanout, seed=args.seed, t_fail=args.t_fail, t_cleanup=args.t_fail, max_files=0)
    res = {"workload": f"N={n}, k={args.fanout} pull, T_fail=T_cleanup={args.t_fail}, full start, "
                       f"{args.warmup} warm-up rounds"}
    eng = gs.Engine(gs.default_config(n, **cfg))
    try:
        eng.init_full(2, 0, 0)
        eng.step(args.warmup)
        res["healthy"] = leg(eng, args.calls)
        eng.set_timing(True)
        eng.step(args.rounds)
        kern_ms, launches = eng.read_timing()
        eng.set_timing(False)
        res["k_round_ms_avg"] = round(kern_ms / max(launches, 1), 4)
        res["k_round_launches"] = launches
        eng.set_partition(np.arange(n, dtype=np.int32) & 1)
        eng.step(args.rounds)
        res["split_even_odd"] = dict(leg(eng, args.calls), rounds_split=args.rounds, round=eng.round)
        eng.step(args.rounds)  # (by now the sides have dropped each other)
        res["split_even_odd_later"] = dict(leg(eng, args.calls), rounds_split=2 * args.rounds, round=eng.round)
    finally:
        eng.close()
    if args.host_n:
        sys.path.insert(0, str(REPO / "tests"))
        from groups_ref import groups_ref
        m = args.host_n
        eng = gs.Engine(gs.default_config(m, **cfg))
        try:
            eng.init_full(2, 0, 0)
            eng.step(args.warmup)
            eng.sync()
            t0 = time.perf_counter()
            hb, _, alive = eng.export_state()
            t1 = time.perf_counter()
            ref = groups_ref(hb, alive)
            t2 = time.perf_counter()
            g = eng.groups()
            assert np.array_equal(g.group, ref[0]) and np.array_equal(g.digest, ref[1])
            res["host_alternative"] = {"n": m, "export_state_ms": round((t1 - t0) * 1e3, 1),
                                       "groups_ref_ms": round((t2 - t1) * 1e3, 1), "n_groups": ref[2]}
        finally:
            eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
