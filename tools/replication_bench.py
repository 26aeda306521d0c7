"""The replica-set census at scale: on a 65,536-node
simulation, in the ownership census' two states (tools/ownership_bench.py) --

  converged:   20 churn rounds, no faults;
  checkpoint:  20 churn rounds, then 1 % of the nodes fail-stop and 30 more
               rounds run, so that rings differ --

the device time (HIP events) and wall time of replication(R) for R = 1, 2, 3,
5 and 8 (the median of --repeat fresh ones, a round before each), and of the
ownership census in the same process on the same states, the yardstick; the
arc kernel's walk steps per arc; a cached read; replication_at(3) for 2^24 key
hashes; ring_lookup_n(0, keys, 3) beside ring_lookup(0, keys) (wall: both copy
their keys in and their results out); and the measures found at R = 3, at the
checkpoint also after every --drain-step further rounds until nothing is
under-replicated.  Writes profiles/replication/replication_bench.json and
prints it.

usage: python tools/replication_bench.py [--nodes N] [--keys K] [--seed S]   (GPU box)"""
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

RS = (1, 2, 3, 5, 8)
SHOWN = ("measure", "under", "exact", "over", "claimants", "max_claims", "min_claims")


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def other_ms(S):
    return S.kernel_times()["other"][0]


def fresh(S, f, repeat):
    """Device and wall ms of f() computed afresh `repeat` times, a round before each; the last result."""
    devs, walls, under = [], [], []
    for _ in range(repeat):
        S.round(churn=False)
        S.sync()
        d0 = other_ms(S)
        got, wall = timed(f)
        devs.append(other_ms(S) - d0)
        walls.append(wall)
        under.append(S.replication(3)["under"])  # (the state each one was computed in; outside the timed span)
    return got, {"device_ms": round(float(np.median(devs)), 3), "wall_ms": round(float(np.median(walls)), 2),
                 "device_ms_all": [round(d, 3) for d in devs], "under_r3_all": under}


def state(S, keys, repeat):
    S.sync()
    S.enable_timing(True, stages=["other"])
    S.ownership(), S.replication(3), S.ring_lookup_n(0, keys[:1024], 3)  # (the index, the buffers, the kernels' code)
    out = {"replication": {}}
    _, out["ownership"] = fresh(S, S.ownership, repeat)
    for R in RS:
        got, t = fresh(S, lambda: S.replication(R), repeat)
        t["ratio_to_ownership_device"] = round(t["device_ms"] / out["ownership"]["device_ms"], 3)
        t["walk_steps_per_arc"] = round(got["walk_steps"] / max(got["arcs"], 1), 4)
        t["arcs"] = got["arcs"]
        out["replication"][str(R)] = t
    three = S.replication(3)
    _, out["cached_wall_ms"] = timed(lambda: S.replication(3))
    d0 = other_ms(S)
    _, wall = timed(lambda: S.replication_at(3, keys))
    out["replication_at"] = {"keys": len(keys), "device_ms": round(other_ms(S) - d0, 3), "wall_ms": round(wall, 2)}
    d0 = other_ms(S)
    (owners, counts), wall = timed(lambda: S.ring_lookup_n(0, keys, 3))
    out["ring_lookup_n_3"] = {"keys": len(keys), "device_ms": round(other_ms(S) - d0, 3), "wall_ms": round(wall, 2)}
    first, wall = timed(lambda: S.ring_lookup(0, keys))
    out["ring_lookup"] = {"keys": len(keys), "wall_ms": round(wall, 2)}
    assert np.array_equal(owners[:, 0], first) and (counts == 3).all()
    out["at_r3"] = {k: three[k] for k in SHOWN}
    out["under_share_r3"] = three["under"] / 2.0 ** 32
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--keys", type=int, default=1 << 24)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--repeat", type=int, default=9, help="fresh computations per figure, a round before each")
    p.add_argument("--drain-step", type=int, default=5)
    p.add_argument("--drain-max", type=int, default=60)
    p.add_argument("--arena-entries", type=int, default=3 << 30, help="checkpoint: message arena (DESIGN.md §11)")
    p.add_argument("--only", choices=("converged", "checkpoint"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "replication", "replication_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    keys = np.random.default_rng(11).integers(0, 1 << 32, size=args.keys, dtype=np.uint64).astype(np.uint32)
    out = {"tool": "replication_bench", "nodes": n, "churn_k": k, "repeat": args.repeat}

    if args.only != "checkpoint":
        S = ringpop_amd.Sim(n, args.seed, churn_k=k)
        S.run(args.churn_rounds, churn=True)
        out["converged"] = state(S, keys, args.repeat)
        S.close()
    if args.only != "converged":
        # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds (§10)
        failed = [(i * n) // k + 1 for i in range(k)]
        S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed},
                            arena_entries=args.arena_entries)
        S.run(args.churn_rounds + args.fault_rounds, churn=True)
        # (the measures first: the timings below run further rounds)
        rounds = args.churn_rounds + args.fault_rounds
        at = S.replication(3)
        drain = [{"after_round": rounds, **{k2: at[k2] for k2 in SHOWN}}]
        out["checkpoint"] = dict(state(S, keys, args.repeat), failed=len(failed), rounds=rounds)
        rounds += (1 + len(RS)) * args.repeat
        while True:
            at = S.replication(3)
            drain.append({"after_round": rounds, **{k2: at[k2] for k2 in SHOWN}})
            if not at["under"] or rounds >= args.drain_max + args.churn_rounds + args.fault_rounds:
                break
            S.run(args.drain_step, churn=False)
            rounds += args.drain_step
        out["checkpoint"]["drain_r3"] = drain
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
