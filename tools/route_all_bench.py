"""Multi-key requests at scale: on a 65,536-node simulation, in
tools/route_n_bench.py's two states --

  converged:   20 churn rounds, no faults;
  checkpoint:  20 churn rounds, then 1 % of the nodes fail-stop and 30 more
               rounds run, so that rings differ --

the device time (HIP events) of route_all_uniform(seed, --keys / K, K) for K =
8, 64 and 256 (the median of --repeat, a round before each) and beside it, in
the same process and at the same instant, route_uniform of --keys requests:
ns per key against route_uniform's ns per request is what a caller weighs
between K single routes and one multi-key route.  Writes
profiles/route_all/route_all_bench.json and prints it.

usage: python tools/route_all_bench.py [--nodes N] [--keys T] [--seed S]   (GPU box)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ringpop_amd  # noqa: E402

KS = (8, 64, 256)
REQ_SEED = 11


def other_ms(S):
    return S.kernel_times()["other"][0]


def state(S, keys, repeat):
    """Every figure is the median over `repeat` instants, a round before each; at one instant every call sees the
    same rings and the same key draws."""
    S.sync()
    S.enable_timing(True, stages=["other"])
    S.route_uniform(REQ_SEED, 256)  # (the tables, the kernels' code)
    for K in KS:
        S.route_all_uniform(REQ_SEED, 4, K)
    calls = {"route_uniform": lambda: S.route_uniform(REQ_SEED, keys)}
    calls.update({str(K): (lambda K=K: S.route_all_uniform(REQ_SEED, keys // K, K)) for K in KS})
    devs, first = {k: [] for k in calls}, {}
    for _ in range(repeat):
        S.round(churn=False)
        S.ring_checksums()  # (the rings' checksums are the "checksum" stage's: not in the figures)
        got = {}
        for k, f in calls.items():
            S.sync()
            d0 = other_ms(S)
            got[k] = f()
            devs[k].append(other_ms(S) - d0)
        for K in KS:  # (every key is drawn and looked up once, whatever K)
            assert got[str(K)]["keys"] + got[str(K)]["entry_dead"] * K == keys, (K, got[str(K)])
        first = first or got

    def figure(k):
        ms = float(np.median(devs[k]))
        return {"device_ms": round(ms, 3), "device_ms_all": [round(d, 3) for d in devs[k]],
                "ns_per_key": round(ms * 1e6 / keys, 4), "stats_first_instant": first[k]}

    out = {"keys": keys, "route_uniform": figure("route_uniform"), "route_all_uniform": {str(K): figure(str(K)) for K in KS}}
    one = out["route_uniform"]["device_ms"]
    out["ratio_per_key_to_route_uniform"] = {str(K): round(out["route_all_uniform"][str(K)]["device_ms"] / one, 3)
                                             for K in KS}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--keys", type=int, default=1 << 24, help="keys in total of every call (a multiple of 256)")
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=9, help="computations per figure, a round before each")
    p.add_argument("--arena-entries", type=int, default=3 << 30, help="checkpoint: message arena (DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_all", "route_all_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    out = {"tool": "route_all_bench", "nodes": n, "churn_k": k, "repeat": args.repeat}

    if args.only != "checkpoint":
        S = ringpop_amd.Sim(n, args.seed, churn_k=k)
        S.run(args.churn_rounds, churn=True)
        out["converged"] = state(S, args.keys, args.repeat)
        S.close()
    if args.only != "converged":
        # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds (§10)
        failed = [(i * n) // k + 1 for i in range(k)]
        S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed},
                            arena_entries=args.arena_entries)
        S.run(args.churn_rounds + args.fault_rounds, churn=True)
        out["checkpoint"] = dict(state(S, args.keys, args.repeat), failed=len(failed),
                                 rounds=args.churn_rounds + args.fault_rounds)
        S.close()
    try:
        out["commit"] = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                       cwd=ROOT).stdout.strip() or None
    except OSError:
        out["commit"] = None
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
