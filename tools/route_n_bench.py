"""Replicated requests at scale: on a 65,536-node simulation,
in the censuses' two states (tools/holders_bench.py) --

  converged:   20 churn rounds, no faults;
  checkpoint:  20 churn rounds, then 1 % of the nodes fail-stop and 30 more
               rounds run, so that rings differ --

the device time (HIP events) of route_n_uniform(R, seed, --requests) for R = 1,
3 and 8 (the median of --repeat, a round before each) and beside it, in the
same process and for the same requests, route_uniform: the reference point at
R = 1; for R > 1 it is the cost per slot against R = 1's.  The R = 1 counts are
compared with route_uniform's outside the timed spans.  Writes
profiles/route_n/route_n_bench.json and prints it.

usage: python tools/route_n_bench.py [--nodes N] [--requests K] [--seed S]   (GPU box)"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ringpop_amd  # noqa: E402

RS = (1, 3, 8)
REQ_SEED = 11


def other_ms(S):
    return S.kernel_times()["other"][0]


def state(S, count, repeat):
    """Every figure is the median over `repeat` instants, a round before each; at one instant route_uniform and
    route_n_uniform at every R see the same rings and the same requests."""
    S.sync()
    S.enable_timing(True, stages=["other"])
    S.route_uniform(REQ_SEED, 256), S.route_n_uniform(3, REQ_SEED, 256)  # (the tables, the kernels' code)
    calls = {"route_uniform": lambda: S.route_uniform(REQ_SEED, count)}
    calls.update({str(R): (lambda R=R: S.route_n_uniform(R, REQ_SEED, count)) for R in RS})
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
        one, st = got["route_uniform"], got["1"]
        assert all(st[k] == one[k] for k in S.ROUTE_OUTCOMES) and st["misplaced"] == one["misrouted"], (st, one)
        first = first or got

    def figure(k):
        ms = float(np.median(devs[k]))
        t = {"device_ms": round(ms, 3), "device_ms_all": [round(d, 3) for d in devs[k]],
             "ns_per_request": round(ms * 1e6 / count, 3), "stats_first_instant": first[k]}
        if k != "route_uniform":
            t["ns_per_slot"] = round(ms * 1e6 / first[k]["slots"], 3)
        return t

    out = {"requests": count, "route_uniform": figure("route_uniform"), "route_n_uniform": {str(R): figure(str(R)) for R in RS}}
    r = out["route_n_uniform"]
    out["ratio_route_n_1_to_route_uniform"] = round(r["1"]["device_ms"] / out["route_uniform"]["device_ms"], 3)
    out["ratio_per_slot_to_R1"] = {str(R): round(r[str(R)]["ns_per_slot"] / r["1"]["ns_per_slot"], 3) for R in RS[1:]}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--requests", type=int, default=1 << 24)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=9, help="computations per figure, a round before each")
    p.add_argument("--arena-entries", type=int, default=3 << 30, help="checkpoint: message arena (DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_n", "route_n_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    out = {"tool": "route_n_bench", "nodes": n, "churn_k": k, "repeat": args.repeat}

    if args.only != "checkpoint":
        S = ringpop_amd.Sim(n, args.seed, churn_k=k)
        S.run(args.churn_rounds, churn=True)
        out["converged"] = state(S, args.requests, args.repeat)
        S.close()
    if args.only != "converged":
        # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds (§10)
        failed = [(i * n) // k + 1 for i in range(k)]
        S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed},
                            arena_entries=args.arena_entries)
        S.run(args.churn_rounds + args.fault_rounds, churn=True)
        out["checkpoint"] = dict(state(S, args.requests, args.repeat), failed=len(failed),
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
