"""The ownership census at scale: on a 65,536-node simulation,
in two states --

  converged:   20 churn rounds, no faults;
  checkpoint:  §10's (20 churn rounds, then 1 % of the nodes fail-stop and 30
               more rounds run, so that rings differ) --

the device time (HIP events) and wall time of a census (ownership(); the
median of 1 + --repeat fresh ones, a round before each), of a cached read,
and of ownership_at() for 2^24 key hashes; the measures found (those of the
first fresh census, and measure[0] of every one); the per-round time of the same process; the expected backward-walk steps per
arc (n / a view's ring size, averaged over the claimant views); and the
brute-force bound N x intervals lookups at the route rate §10 measured.
Writes profiles/ownership/ownership_bench.json and prints it.

usage: python tools/ownership_bench.py [--nodes N] [--keys K] [--seed S]   (GPU box)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ringpop_amd  # noqa: E402

ROUTE_RATE = 7.0e9  # lookups/s: route_uniform at this size


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def other_ms(S):
    return S.kernel_times()["other"][0]


def state(S, n, keys, rounds_ms, repeat):
    S.sync()
    S.enable_timing(True, stages=["other"])
    # the very first call also builds the server -> point index and loads the kernels' code
    own0, first_wall = timed(S.ownership)
    first_dev = other_ms(S)
    _, cached_wall = timed(S.ownership)
    at, at_first_wall = timed(lambda: S.ownership_at(keys))
    d0 = other_ms(S)
    at2, at_wall = timed(lambda: S.ownership_at(keys))
    at_dev = other_ms(S) - d0
    assert np.array_equal(at, at2)
    # a fresh census after one more round, everything resident
    _, round_wall = timed(lambda: (S.round(churn=False), S.sync()))
    d0 = other_ms(S)
    own, wall = timed(S.ownership)
    dev = other_ms(S) - d0
    # ... and `repeat` more of them, a round before each (nothing cached)
    ring = S.view_counts()[:, 5].astype(np.float64)
    devs, walls, orphaned = [dev], [wall], [own["measure"][0]]
    for _ in range(repeat):
        S.round(churn=False)
        S.sync()
        d0 = other_ms(S)
        again, wall = timed(S.ownership)
        devs.append(other_ms(S) - d0)
        walls.append(wall)
        orphaned.append(again["measure"][0])
    claimant = own["claimed"] > 0
    arcs = int(own["intervals"])  # (an upper bound: one arc per present own point of every claimant view)
    return {
        "census": {"first_wall_ms": round(first_wall, 2), "first_device_ms": round(first_dev, 3),
                   "wall_ms": round(float(np.median(walls)), 2), "device_ms": round(float(np.median(devs)), 3),
                   "device_ms_all": [round(d, 3) for d in devs], "wall_ms_all": [round(w, 2) for w in walls],
                   "cached_wall_ms": round(cached_wall, 3)},
        "ownership_at": {"keys": int(len(keys)), "first_wall_ms": round(at_first_wall, 2), "wall_ms": round(at_wall, 2),
                         "device_ms": round(at_dev, 3), "keys_per_s_device": round(len(keys) / (at_dev * 1e-3), 1)},
        "round_ms_same_process": {"mean_of_run": round(rounds_ms, 3), "one_more_round_wall": round(round_wall, 3)},
        "before_the_extra_round": {k: own0[k] for k in ("measure", "claimants", "max_claims", "max_claims_hash")},
        "orphaned_per_census": orphaned,
        "measure": own["measure"], "claimants": own["claimants"], "intervals": own["intervals"],
        "max_claims": own["max_claims"], "max_claims_hash": own["max_claims_hash"],
        "claimed_min_max_of_claimants": [int(own["claimed"][claimant].min()), int(own["claimed"][claimant].max())],
        "ring_servers_min_max_of_claimants": [int(ring[claimant].min()), int(ring[claimant].max())],
        "expected_walk_steps_per_arc": round(float((n / ring[claimant]).mean()), 4),
        "arcs_upper_bound": arcs,
        "brute_force_bound_s": round(n * own["intervals"] / ROUTE_RATE, 1),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--keys", type=int, default=1 << 24)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=8, help="fresh censuses after the first, a round before each")
    p.add_argument("--arena-entries", type=int, default=3 << 30,
                   help="checkpoint: message arena (the default one fills a few fault rounds later; DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ownership", "ownership_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    keys = np.random.default_rng(11).integers(0, 1 << 32, size=args.keys, dtype=np.uint64).astype(np.uint32)
    out = {"tool": "ownership_bench", "nodes": n, "churn_k": k, "route_rate_lookups_per_s": ROUTE_RATE}

    if args.only != "checkpoint":
        S = ringpop_amd.Sim(n, args.seed, churn_k=k)
        S.run(2, churn=True)
        S.sync()
        _, ms = timed(lambda: (S.run(args.churn_rounds - 2, churn=True), S.sync()))
        out["converged"] = state(S, n, keys, ms / (args.churn_rounds - 2), args.repeat)
        S.close()
    if args.only == "converged":
        return finish(out, args.out)

    # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds (§10)
    failed = [(i * n) // k + 1 for i in range(k)]
    S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed}, arena_entries=args.arena_entries)
    S.run(args.churn_rounds, churn=True)
    S.sync()
    _, ms = timed(lambda: (S.run(args.fault_rounds, churn=True), S.sync()))
    out["checkpoint"] = dict(state(S, n, keys, ms / args.fault_rounds, args.repeat), failed=len(failed),
                             rounds=args.churn_rounds + args.fault_rounds)
    S.close()
    return finish(out, args.out)


def finish(out, path):
    try:
        out["commit"] = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                       cwd=ROOT).stdout.strip() or None
    except OSError:
        out["commit"] = None
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
