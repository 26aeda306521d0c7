"""The holders query at scale: on a 65,536-node simulation, in
the censuses' two states (tools/replication_bench.py) --

  converged:   20 churn rounds, no faults;
  checkpoint:  20 churn rounds, then 1 % of the nodes fail-stop and 30 more
               rounds run, so that rings differ --

the device time (HIP events) and wall time of holders_at(R, keys, cap 16) for
R = 1, 3 and 8 over --keys random key hashes and of holders_at(3) for a single
key (the median of --repeat, a round before each); and beside it, in the same
process, what it replaces: ring_lookup_n(v, keys, 3) for --views evenly spread
views v, whose sum is scaled to all n views (labelled so: the n launches are
not run, and the host loop that looks for v in its rows is not counted).  The
counts are compared with replication_at's outside the timed spans.  Writes
profiles/holders/holders_bench.json and prints it.

usage: python tools/holders_bench.py [--nodes N] [--keys K] [--seed S]   (GPU box)"""
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

RS = (1, 3, 8)
CAP = 16


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def other_ms(S):
    return S.kernel_times()["other"][0]


def fresh(S, f, repeat):
    """Device and wall ms of f() `repeat` times, a round before each; the last result."""
    devs, walls = [], []
    for _ in range(repeat):
        S.round(churn=False)
        S.sync()
        d0 = other_ms(S)
        got, wall = timed(f)
        devs.append(other_ms(S) - d0)
        walls.append(wall)
    return got, {"device_ms": round(float(np.median(devs)), 3), "wall_ms": round(float(np.median(walls)), 2),
                 "device_ms_all": [round(d, 3) for d in devs]}


def state(S, keys, views, repeat):
    n = S.n
    S.sync()
    S.enable_timing(True, stages=["other"])
    S.holders_at(3, keys[:256]), S.ring_lookup_n(0, keys[:256], 3)  # (the tables, the kernels' code)
    out = {"keys": len(keys), "cap": CAP, "holders_at": {}}
    for R in RS:
        (rows, counts), t = fresh(S, lambda: S.holders_at(R, keys, CAP), repeat)
        assert np.array_equal(counts, S.replication_at(R, keys))
        assert ((rows >= 0).sum(axis=1) == np.minimum(counts, CAP)).all()
        t["us_per_key_device"] = round(t["device_ms"] * 1e3 / len(keys), 3)
        t["holders_min_max"] = [int(counts.min()), int(counts.max())]
        out["holders_at"][str(R)] = t
    _, out["holders_at_3_single_key"] = fresh(S, lambda: S.holders_at(3, keys[:1], CAP), repeat)
    # what it replaces: one launch and two copies per view, here for `views` of the n
    vs = [(i * n) // views for i in range(views)]

    def per_view():
        for v in vs:
            S.ring_lookup_n(v, keys, 3)

    _, t = fresh(S, per_view, repeat)
    scale = n / views
    out["ring_lookup_n_3_per_view"] = dict(t, views_run=views, scaled_to_views=n,
                                           device_ms_scaled=round(t["device_ms"] * scale, 1),
                                           wall_ms_scaled=round(t["wall_ms"] * scale, 1))
    three = out["holders_at"]["3"]
    out["ratio_scaled_per_view_to_holders_at_3"] = {
        "device": round(t["device_ms"] * scale / three["device_ms"], 1),
        "wall": round(t["wall_ms"] * scale / three["wall_ms"], 1)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--keys", type=int, default=4096)
    p.add_argument("--views", type=int, default=64, help="views the per-view yardstick runs (scaled to all)")
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=9, help="computations per figure, a round before each")
    p.add_argument("--arena-entries", type=int, default=3 << 30, help="checkpoint: message arena (DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "holders", "holders_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    keys = np.random.default_rng(11).integers(0, 1 << 32, size=args.keys, dtype=np.uint64).astype(np.uint32)
    out = {"tool": "holders_bench", "nodes": n, "churn_k": k, "repeat": args.repeat}

    if args.only != "checkpoint":
        S = ringpop_amd.Sim(n, args.seed, churn_k=k)
        S.run(args.churn_rounds, churn=True)
        out["converged"] = state(S, keys, args.views, args.repeat)
        S.close()
    if args.only != "converged":
        # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds (§10)
        failed = [(i * n) // k + 1 for i in range(k)]
        S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed},
                            arena_entries=args.arena_entries)
        S.run(args.churn_rounds + args.fault_rounds, churn=True)
        out["checkpoint"] = dict(state(S, keys, args.views, args.repeat), failed=len(failed),
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
