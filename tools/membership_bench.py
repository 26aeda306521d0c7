"""The membership census at scale: on one shard, at --nodes
(65,536, then 32,768), in two states --

  churn:      --churn-rounds churn rounds, no faults;
  failstop:   the same, then 1 % of the nodes fail-stop and --fault-rounds more
              rounds run, so that 1 % of the rows are no viewers' and the
              columns hold suspect and faulty cells --

the device time (HIP events, the "other" stage) and wall time of
rp_sim_membership, the median of --repeat calls with a round before each:

  columns:  seen, top and at_top only -- the column pass and the combine (the
            entry point skips the row pass when neither stats nor behind is
            asked for);
  full:     Sim.membership() -- both passes and the two folds;
  rows:     full - columns, the row pass and the one-wave finish.

Beside them the floor of one pass: viewers x n cells x 16 B (a lane reads 8
bytes of each cell, the lines moved are the cells') over this box's streaming
read rate, measured by rp_calibrate in the same process before the cluster is
built (§6.11).  One JSON line per (nodes, state), appended to --out.

usage: python tools/membership_bench.py [--nodes N ...] [--seed S]   (GPU box)"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ringpop_amd  # noqa: E402
from ringpop_amd._lib import check, lib, ptr  # noqa: E402

CAL_BYTES = 16 << 30  # (bench.py's box_ceiling: 64x the Infinity Cache)
STATS = ("viewers", "agreed", "cells_behind", "laggards", "undetected", "suspected_dead", "false_suspect", "false_faulty")


def stream16_bytes_per_s():
    v = (ctypes.c_double * 5)()
    check(lib().rp_calibrate(CAL_BYTES, v, 5))
    return v[3] * 16


def fresh(S, f, repeat):
    """Device and wall ms of f() `repeat` times, a round before each."""
    devs, walls = [], []
    for _ in range(repeat):
        S.round(churn=False)
        S.sync()
        d0 = S.kernel_times()["other"][0]
        t0 = time.perf_counter()
        f()
        walls.append((time.perf_counter() - t0) * 1e3)
        devs.append(S.kernel_times()["other"][0] - d0)
    return {"device_ms": round(float(np.median(devs)), 3), "wall_ms": round(float(np.median(walls)), 2),
            "device_ms_all": [round(d, 3) for d in devs]}


def state(S, rate, repeat):
    n = S.n
    seen, top, at = np.zeros((n, 5), dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)

    def columns():
        check(lib().rp_sim_membership(S._h, None, ptr(seen), ptr(top), ptr(at), None, n))

    S.sync()
    S.enable_timing(True, stages=["other"])
    got = S.membership()  # (the tables, the buffers, the kernels' code)
    columns()
    assert np.array_equal(seen, got["seen"]) and np.array_equal(at, got["at_top"])
    out = {"columns": fresh(S, columns, repeat), "full": fresh(S, S.membership, repeat)}
    floor = got["viewers"] * n * 16 / rate * 1e3
    col, rows = out["columns"]["device_ms"], round(out["full"]["device_ms"] - out["columns"]["device_ms"], 3)
    out.update(rows_device_ms=rows, floor_ms_per_pass=round(floor, 3), columns_over_floor=round(col / floor, 2),
               rows_over_floor=round(rows / floor, 2), pass_bytes=got["viewers"] * n * 16,
               columns_GBps=round(got["viewers"] * n * 16 / col / 1e6, 1),
               rows_GBps=round(got["viewers"] * n * 16 / rows / 1e6, 1), stats={k: got[k] for k in STATS})
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, nargs="+", default=[65536, 32768])
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=5)
    p.add_argument("--fault-rounds", type=int, default=12)
    p.add_argument("--repeat", type=int, default=7, help="calls per figure, a round before each")
    p.add_argument("--arena-entries", type=int, default=3 << 30, help="failstop: message arena (DESIGN.md §11)")
    p.add_argument("--only", choices=("churn", "failstop"), default=None, help="one state only")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "membership", "membership_bench.jsonl"))
    args = p.parse_args()
    rate = stream16_bytes_per_s()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in args.nodes:
        k = -(-n // 100)
        for name in ("churn", "failstop"):
            if args.only not in (None, name):
                continue
            if name == "churn":
                S, rounds = ringpop_amd.Sim(n, args.seed, churn_k=k), args.churn_rounds
            else:
                # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds (§10)
                failed = [(i * n) // k + 1 for i in range(k)]
                S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed},
                                    arena_entries=args.arena_entries)
                rounds = args.churn_rounds + args.fault_rounds
            S.run(rounds, churn=True)
            line = dict({"tool": "membership_bench", "nodes": n, "shards": 1, "state": name, "rounds": rounds,
                         "repeat": args.repeat, "stream16_GBps": round(rate / 1e9, 1)}, **state(S, rate, args.repeat))
            S.close()
            text = json.dumps(line)
            with open(args.out, "a") as f:
                f.write(text + "\n")
            print(text, flush=True)


if __name__ == "__main__":
    main()
