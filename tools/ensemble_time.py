#!/usr/bin/env python3
"""Times cluster ensembles (gossipsim.Ensemble, SPEC §11) against the same job
done with one Engine per cluster, in one process on one MI355X, and writes one
JSON file (DESIGN.md "Ensemble" quotes profiles/ensemble_time.json).

The job: B clusters of N members, k = 3, T_fail = T_cleanup = 12, drop rate 0.1
on both sides, from a full start, ROUNDS rounds each.
  ensemble  one Ensemble of B clusters, one step(ROUNDS) call: the host clock
            around the call (gh_ens_step returns after the device is done).
            Warmed up by one untimed call; every repeat starts from init_full.
  engines   one Engine per cluster, each stepped ROUNDS rounds in one gh_step
            call (the host clock around it; gh_step blocks until done), one
            after the other: what a sweep does today. Engines of one N cost
            the same whatever the seed, so ENGINES of them are timed per N and
            the job's time is B times their mean (stated in the output).
--peer-mode ring / --detect-mode quirk time the ensemble in those modes
(gh_ens_config.peer_mode / detect_mode) against Engines created in the same
modes; --t-fail sets T_fail = T_cleanup of the job (a ring needs more than the
pull default to hold together). DESIGN.md quotes
profiles/ensemble_modes_time.json for them.
cluster-rounds per second = B * ROUNDS / seconds. No GPU: the script fails."""
import argparse
import json
import pathlib
import statistics
import sys
import time

REPO = pathlib.Path(__file__).resolve().parents[1]
for p in (REPO, REPO / "p2p-file-system-with-gossip-detect-failure-management_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

import gossipsim as gs  # noqa: E402

K, T, RATE = 3, 12, 0.1
PEER = dict(pull=gs.GH_PEER_PULL, ring=gs.GH_PEER_RING)
DETECT = dict(canonical=gs.GH_DETECT_CANONICAL, quirk=gs.GH_DETECT_QUIRK)


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), repeats=len(xs))


def time_ensemble(n, b, rounds, repeats, t=T, modes=None):
    seeds = 0x5EED9000 + np.arange(b, dtype=np.uint64)
    with gs.Ensemble(n, b, fanout=K, seeds=seeds, t_fail=t, t_cleanup=t, **(modes or {})) as ens:
        ens.set_loss(RATE, RATE)
        ens.init_full()
        ens.step(rounds)  # warm-up: code object load, first launch
        secs, st = [], None
        for _ in range(repeats):
            ens.init_full()
            t0 = time.perf_counter()
            st = ens.step(rounds)
            secs.append(time.perf_counter() - t0)
        assert (st["rounds"] == rounds).all()
        return secs, {f: int(st[f].sum()) for f in ("detections", "merged_cells", "sent", "dropped", "active_rows")}


def time_engines(n, engines, rounds, t=T, modes=None):
    secs = []
    for x in range(engines):
        eng = gs.Engine(gs.default_config(n, fanout=K, t_fail=t, t_cleanup=t, seed=0x5EED9000 + x, **(modes or {})))
        eng.set_loss(RATE, RATE)
        eng.init_full()
        eng.step(min(rounds, 100))  # warm-up
        eng.init_full()
        t0 = time.perf_counter()
        st = eng.step(rounds)
        secs.append(time.perf_counter() - t0)
        assert st["rounds"] == rounds
        eng.close()
    return secs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(REPO / "profiles" / "ensemble_time.json"))
    ap.add_argument("--rounds", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", type=int, default=8)
    ap.add_argument("--members", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--clusters", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--peer-mode", choices=list(PEER), default="pull")
    ap.add_argument("--detect-mode", choices=list(DETECT), default="canonical")
    ap.add_argument("--t-fail", type=int, default=T, help="T_fail = T_cleanup of the job")
    a = ap.parse_args()
    # (the default job passes no mode at all: the call it always made)
    modes = {}
    if a.peer_mode != "pull":
        modes["peer_mode"] = PEER[a.peer_mode]
    if a.detect_mode != "canonical":
        modes["detect_mode"] = DETECT[a.detect_mode]
    job = dict(k=K, t_fail=a.t_fail, t_cleanup=a.t_fail, rate=RATE, rounds=a.rounds, start="init_full(2, 0, 0)")
    if modes:
        job.update(peer_mode=a.peer_mode, detect_mode=a.detect_mode)
    out = dict(job=job,
               method="host clock around the blocking step call; ensemble: one warm-up call, then `repeats` timed calls "
                      "each from init_full; engines: `engines` Engines per N timed one after the other, the job's "
                      "time taken as B x their mean",
               rows=[])
    for n in a.members:
        es = time_engines(n, a.engines, a.rounds, a.t_fail, modes)
        eng_rate = a.rounds / statistics.mean(es)
        for b in a.clusters:
            secs, work = time_ensemble(n, b, a.rounds, a.repeats, a.t_fail, modes)
            rate = [b * a.rounds / s for s in secs]
            row = dict(n=n, clusters=b, ensemble_seconds=spread(secs), ensemble_cluster_rounds_per_s=spread(rate),
                       engine_seconds_per_cluster=spread(es), engine_cluster_rounds_per_s=eng_rate,
                       engines_job_seconds=b * statistics.mean(es),
                       speedup=statistics.median(rate) / eng_rate, ensemble_work=work)
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
