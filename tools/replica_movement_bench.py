"""Replica-set movement at scale: on a 65,536-node simulation,
for R = 1, 3 and 8, in tools/movement_bench.py's two states --

  converged:   20 churn rounds, no faults: a snapshot, a comparison of the
               previous snapshot with "now" with and without the recording
               census, one of two snapshots, and moved_at for --keys key
               hashes (device time from HIP events and wall time, the median
               of --repeat, a round before each), the plain census beside them;
  checkpoint:  §10's (20 churn rounds, then 1 % of the nodes fail-stop and 30
               more rounds run): a snapshot before the fail-stops against
               "now" after the drain, the same figures and the stats.

Writes profiles/replica_movement/replica_movement_bench.json and prints it.

usage: python tools/replica_movement_bench.py [--nodes N] [--only STATE] [--out FILE]   (GPU box)"""
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
ARRAYS = ("gained_by", "lost_by")


def device(S, f):
    """(result, device ms, timed spans, wall ms) of f()."""
    ms0, n0 = S.kernel_times()["other"]
    t0 = time.perf_counter()
    out = f()
    wall = (time.perf_counter() - t0) * 1e3
    ms1, n1 = S.kernel_times()["other"]
    return out, ms1 - ms0, n1 - n0, wall


def stats(m):
    return {k: v for k, v in m.items() if k not in ARRAYS}


def measure(S, frm, R, keys, repeat, step):
    """The figures for one R against snapshot `frm`: `step` makes the state new before each fresh computation."""
    rows = {k: [] for k in ("census", "snapshot", "moved_now", "moved_cached", "moved_two_snapshots", "moved_at")}
    walls = {k: [] for k in rows}

    def take(name, f, spans=None):
        out, ms, n, wall = device(S, f)
        assert spans is None or n == spans, (name, n, spans)
        rows[name].append(ms)
        walls[name].append(wall)
        return out

    moved = None
    for _ in range(repeat):
        step()
        take("census", lambda: S.replication(R), 1)  # the plain census: no arcs recorded
        step()
        snap = take("snapshot", lambda: S.replication_snapshot(R), 2)  # a recording census and the copies
        step()
        moved = take("moved_now", lambda: S.replication_moved(frm), 2)  # a recording census and a comparison
        take("moved_cached", lambda: S.replication_moved(frm), 1)  # the comparison alone
        take("moved_two_snapshots", lambda: S.replication_moved(frm, snap), 1)
        take("moved_at", lambda: S.replication_moved_at(frm, None, keys), 1)
        snap.close()
    med = lambda v: round(float(np.median(v)), 3)  # noqa: E731
    return {"device_ms": {k: med(v) for k, v in rows.items()},
            "device_ms_all": {k: [round(x, 3) for x in v] for k, v in rows.items()},
            "wall_ms": {k: med(v) for k, v in walls.items()}, "last_moved_now": stats(moved)}


def run(S, args, keys, before):
    """`before`: {R: snapshot} to compare against, or None: a snapshot of the state as it is."""
    S.sync()
    S.enable_timing(True, stages=["other"])

    def step():
        S.round(churn=False)
        S.sync()

    out = {}
    for R in RS:
        frm = before[R] if before else S.replication_snapshot(R)
        S.replication_moved(frm), S.replication_moved_at(frm, None, keys[:256])  # (the buffers, the kernels' code)
        out[str(R)] = measure(S, frm, R, keys, args.repeat, step)
        frm.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--keys", type=int, default=4096)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=9)
    p.add_argument("--arena-entries", type=int, default=3 << 30,
                   help="checkpoint: message arena (the default one fills during fault rounds; DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "replica_movement", "replica_movement_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    keys = np.random.default_rng(11).integers(0, 1 << 32, size=args.keys, dtype=np.uint64).astype(np.uint32)
    out = {"tool": "replica_movement_bench", "nodes": n, "churn_k": k, "keys": args.keys, "repeat": args.repeat}
    if args.only != "checkpoint":
        S = ringpop_amd.Sim(n, args.seed, churn_k=k)
        S.run(args.churn_rounds, churn=True)
        out["converged"] = run(S, args, keys, None)
        S.close()
    if args.only != "converged":
        failed = [(i * n) // k + 1 for i in range(k)]
        S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed}, arena_entries=args.arena_entries)
        S.run(args.churn_rounds, churn=True)
        before = {R: S.replication_snapshot(R) for R in RS}
        S.run(args.fault_rounds, churn=True)
        out["checkpoint"] = dict(run(S, args, keys, before), failed=len(failed), rounds=args.churn_rounds + args.fault_rounds)
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
