"""Ownership movement at scale: on a 65,536-node simulation --

  converged:   20 churn rounds, no faults: the device time (HIP events) and
               wall time of a snapshot and of a comparison of the previous
               snapshot with "now" (the median of --repeat, a round before
               each), and the plain census' beside them;
  checkpoint:  §10's (20 churn rounds, then 1 % of the nodes fail-stop and 30
               more rounds run): a snapshot before the fail-stops against
               "now" after the drain, the stats printed;
  restart:     1 % of the nodes leave gracefully per round for --waves rounds
               (each rejoins --away rounds later): a snapshot per round, and
               the movement of every round against the one before.

Writes profiles/movement/movement_bench.json and prints it.

usage: python tools/movement_bench.py [--nodes N] [--only STATE] [--out FILE]   (GPU box)"""
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

STATS = ("transition", "same_set", "handed_off", "gained", "lost", "gainers", "losers", "max_gained",
         "max_gained_node", "max_lost", "max_lost_node", "max_turnover", "max_turnover_hash", "from_clock", "to_clock",
         "intervals")


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def other(S):
    return S.kernel_times()["other"]


def device(S, f):
    """(result, device ms, timed spans, wall ms) of f()."""
    ms0, n0 = other(S)
    out, wall = timed(f)
    ms1, n1 = other(S)
    return out, ms1 - ms0, n1 - n0, wall


def stats(m):
    return {k: m[k] for k in STATS}


def med(xs):
    return round(float(np.median(xs)), 3)


def converged(args, n, k):
    S = ringpop_amd.Sim(n, args.seed, churn_k=k)
    S.run(args.churn_rounds, churn=True)
    S.sync()
    S.enable_timing(True, stages=["other"])
    prev = S.ownership_snapshot()  # (also builds the server -> point index and loads the kernels' code)
    S.ownership_moved(prev)
    rows = {"census": [], "snapshot": [], "moved_now": [], "moved_cached": [], "moved_two_snapshots": []}
    walls = {key: [] for key in rows}
    moved = None
    for _ in range(args.repeat):
        S.round(churn=False)
        S.sync()
        _, ms, _, wall = device(S, S.ownership)  # the plain census: no arcs recorded
        rows["census"].append(ms); walls["census"].append(wall)
        S.round(churn=False)
        S.sync()
        snap, ms, spans, wall = device(S, S.ownership_snapshot)  # a recording census and the copies
        assert spans == 2
        rows["snapshot"].append(ms); walls["snapshot"].append(wall)
        S.round(churn=False)
        S.sync()
        moved, ms, spans, wall = device(S, lambda: S.ownership_moved(prev))  # a recording census and a comparison
        assert spans == 2
        rows["moved_now"].append(ms); walls["moved_now"].append(wall)
        _, ms, spans, wall = device(S, lambda: S.ownership_moved(prev))  # the comparison alone
        assert spans == 1
        rows["moved_cached"].append(ms); walls["moved_cached"].append(wall)
        _, ms, spans, wall = device(S, lambda: S.ownership_moved(prev, snap))
        assert spans == 1
        rows["moved_two_snapshots"].append(ms); walls["moved_two_snapshots"].append(wall)
        prev.close()
        prev = snap
    prev.close()
    S.close()
    return {"device_ms": {key: med(v) for key, v in rows.items()},
            "device_ms_all": {key: [round(x, 3) for x in v] for key, v in rows.items()},
            "wall_ms": {key: med(v) for key, v in walls.items()}, "last_moved_now": stats(moved)}


def checkpoint(args, n, k):
    failed = [(i * n) // k + 1 for i in range(k)]
    S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed}, arena_entries=args.arena_entries)
    S.run(args.churn_rounds, churn=True)
    S.sync()
    S.enable_timing(True, stages=["other"])
    before = S.ownership_snapshot()
    claimed = S.ownership()["claimed"]
    S.run(args.fault_rounds, churn=True)
    S.sync()
    moved, ms, _, wall = device(S, lambda: S.ownership_moved(before))
    _, ms2, _, _ = device(S, lambda: S.ownership_moved(before))
    out = {"failed": len(failed), "rounds": args.churn_rounds + args.fault_rounds, "stats": stats(moved),
           "failed_nodes_claimed_before": int(claimed[failed].astype(object).sum()),
           "failed_nodes_lost": int(moved["lost_by"][failed].astype(object).sum()),
           "device_ms_with_census": round(ms, 3), "device_ms_comparison": round(ms2, 3), "wall_ms": round(wall, 2)}
    before.close()
    S.close()
    return out


def restart(args, n, k):
    per = max(1, n // 100)
    mul = 7919 if n % 7919 else 7907
    leaves, rejoins = {}, {}
    for w in range(args.waves):
        ids = sorted({((w * per + j) * mul + 1) % n for j in range(per)})
        leaves[args.churn_rounds + w] = ids
        rejoins[args.churn_rounds + w + args.away] = ids
    S = ringpop_amd.Sim(n, args.seed, churn_k=k, leaves=leaves, rejoins=rejoins, arena_entries=args.arena_entries)
    S.run(args.churn_rounds, churn=True)
    S.sync()
    S.enable_timing(True, stages=["other"])
    first = prev = S.ownership_snapshot()
    rows = []
    for _ in range(args.waves):
        S.round(churn=False)
        m, ms, _, _ = device(S, lambda: S.ownership_moved(prev))
        snap = S.ownership_snapshot()  # (the arcs are the cached ones: the copies only)
        rows.append({"clock": m["to_clock"], "gained": m["gained"], "lost": m["lost"],
                     "gainers": m["gainers"], "losers": m["losers"], "handed_off": m["handed_off"],
                     "same_set": m["same_set"], "orphaned": m["transition"][1][0] + m["transition"][2][0],
                     "device_ms": round(ms, 3)})
        if prev is not first:
            prev.close()
        prev = snap
    whole = S.ownership_moved(first, prev)
    out = {"leavers_per_round": per, "waves": args.waves, "away": args.away, "per_round": rows,
           "first_to_last": stats(whole)}
    first.close()
    prev.close()
    S.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=9)
    p.add_argument("--waves", type=int, default=20)
    p.add_argument("--away", type=int, default=30)
    p.add_argument("--arena-entries", type=int, default=3 << 30,
                   help="checkpoint, restart: message arena (the default one fills during fault rounds; DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint", "restart"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "movement", "movement_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    out = {"tool": "movement_bench", "nodes": n, "churn_k": k}
    for name, f in (("converged", converged), ("checkpoint", checkpoint), ("restart", restart)):
        if args.only in (None, name):
            out[name] = f(args, n, k)
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
