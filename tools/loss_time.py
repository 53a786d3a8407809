"""Times what lossy links (gh_set_loss, DESIGN.md "Lossy links") cost a round:
the bench's headline workload (N=65,536, k=4 pull, seed 0x5EED0003, T_fail =
T_cleanup = 16, full start), 12 warm-up rounds, then `reps` times the wall time
of one step(rounds) call after a sync(). Four legs, one process each, one
after the other on one box:

    parent   the parent commit's package (--parent-pkg: a checkout of it, built)
    off      this tree, loss off
    zeros    this tree, loss enabled with all-zero thresholds
    loss10   this tree, uniform 0.10 on both sides

Prints one JSON line with the per-leg lists and medians (ms per round), the
footprint of both trees and, for the lossy leg, the counters.

    python tools/loss_time.py [--parent-pkg DIR] [--n N] [--rounds 20] [--reps 5]
    python tools/loss_time.py --leg off          (one leg, as the driver runs it)
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

REPO = pathlib.Path(__file__).resolve().parents[1]
PKG = REPO / "p2p-file-system-with-gossip-detect-failure-management_amd"
LEGS = ("parent", "off", "zeros", "loss10")


def run_leg(args):
    sys.path[:0] = [str(args.pkg or PKG)]
    import gossipsim as gs
    n = args.n
    cfg = gs.default_config(n, fanout=args.fanout, seed=args.seed, t_fail=args.t_fail, t_cleanup=args.t_fail,
                            max_files=0)
    out = {"footprint": gs.footprint(cfg)["create_bytes"]}
    eng = gs.Engine(cfg)
    try:
        eng.init_full(2, 0, 0)
        eng.step(args.warmup)
        if args.leg == "zeros":
            eng.set_loss(0.0, 0.0)
        elif args.leg == "loss10":
            eng.set_loss(0.10, 0.10)
        eng.step(2)  # (first launches outside the timed calls)
        ms = []
        for _ in range(args.reps):
            eng.sync()
            t0 = time.perf_counter()
            eng.step(args.rounds)
            ms.append(round((time.perf_counter() - t0) * 1e3 / args.rounds, 4))
        out["ms_per_round"] = ms
        out["tier"] = list(eng.tier_info(full=True))
        if args.leg in ("zeros", "loss10"):
            out["sent"], out["dropped"] = eng.loss_stats()
    finally:
        eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--fanout", type=int, default=4)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0003)
    ap.add_argument("--t-fail", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-pkg", type=pathlib.Path, default=None)
    ap.add_argument("--leg", choices=LEGS, default=None)
    ap.add_argument("--pkg", type=pathlib.Path, default=None)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    res = {}
    for leg in LEGS:
        if leg == "parent" and args.parent_pkg is None:
            continue
        cmd = [sys.executable, __file__, "--leg", leg, "--n", str(args.n), "--fanout", str(args.fanout),
               "--seed", hex(args.seed), "--t-fail", str(args.t_fail), "--warmup", str(args.warmup),
               "--rounds", str(args.rounds), "--reps", str(args.reps)]
        if leg == "parent":
            cmd += ["--pkg", str(args.parent_pkg)]
        p = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
        res[leg] = json.loads(p.stdout.strip().splitlines()[-1])
    med = {k: round(statistics.median(v["ms_per_round"]), 4) for k, v in res.items()}
    print(json.dumps({
        "workload": f"N={args.n}, k={args.fanout} pull, T_fail=T_cleanup={args.t_fail}, full start, "
                    f"{args.warmup} warm-up rounds, step({args.rounds}) x {args.reps} per leg, one process per leg, "
                    f"in turn",
        "ms_per_round_median": med,
        "ms_per_round_all": {k: v["ms_per_round"] for k, v in res.items()},
        "spread_ms": {k: round(max(v["ms_per_round"]) - min(v["ms_per_round"]), 4) for k, v in res.items()},
        "create_bytes": {k: v["footprint"] for k, v in res.items()},
        "tier_info": {k: v["tier"] for k, v in res.items()},
        "loss_stats": {k: [v["sent"], v["dropped"]] for k, v in res.items() if "sent" in v},
    }))


if __name__ == "__main__":
    main()
