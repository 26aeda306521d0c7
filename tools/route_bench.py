"""Request routing at scale: on a config-4-shaped simulation
(65,536 nodes, 20 churn rounds, then 1 % of the nodes fail-stop and 30 more
rounds run, so that rings differ) one JSON line with

  (a) ring_checksums() of all views: wall time and device time (HIP events);
  (b) the membership checksums() of all views, same process, same rounds
      (and, in a second simulation of the same rounds, on the wave path);
  (c) route_uniform() of 2^24 requests: requests/s and the statistics;
  (d) for scale, Sim.ring_lookup(v, 2^24 hashes) of one view: keys/s.

usage: python tools/route_bench.py [--nodes N] [--requests R] [--seed S]   (GPU box)"""
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


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--requests", type=int, default=1 << 24)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--fault-rounds", type=int, default=30)
    p.add_argument("--no-wave-b", action="store_true", help="skip the second simulation that times (b) on the wave path")
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    # 1 % of the nodes, evenly spread, fail-stop at the first round after the churn rounds
    failed = [(i * n) // k + 1 for i in range(k)]
    S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed})
    S.run(args.churn_rounds + args.fault_rounds, churn=True)
    S.sync()
    live = np.ones(n, dtype=bool)
    live[failed] = False

    # (a) every view's ring checksum; the first call also loads the kernel's
    # code, so a second, forced recomputation (a round in between) is timed too
    S.enable_timing(True, stages=["checksum"])
    rcs, a_first_ms = timed(S.ring_checksums)
    a_first_dev = S.kernel_times()["checksum"][0]
    _, a_cached_ms = timed(S.ring_checksums)
    # (b) every view's membership checksum, right after the same rounds
    cs, b_ms = timed(S.checksums)
    _, b_again_ms = timed(S.checksums)
    # (c) 2^24 requests drawn on the device
    S.enable_timing(True, stages=["other"])
    stats, c_first_ms = timed(lambda: S.route_uniform(11, args.requests))
    c_first_dev = S.kernel_times()["other"][0]
    stats2, c_ms = timed(lambda: S.route_uniform(11, args.requests))
    c_dev = S.kernel_times()["other"][0] - c_first_dev
    assert stats2 == stats
    # (d) the one-view lookup of as many hashes (H2D, k_view_lookup, D2H)
    keys = np.random.default_rng(11).integers(0, 1 << 32, size=args.requests, dtype=np.uint64).astype(np.uint32)
    S.ring_lookup(0, keys[:1024])
    _, d_ms = timed(lambda: S.ring_lookup(0, keys))
    # a fresh recomputation of (a) after one more round, the kernel's code resident
    S.round(churn=True)
    S.sync()
    S.enable_timing(True, stages=["checksum"])
    _, a_ms = timed(S.ring_checksums)
    a_dev = S.kernel_times()["checksum"][0]
    S.close()
    # (b) again on the wave path (one wave per view, as (a) is): a second
    # simulation of the same rounds whose many-view lists never take the
    # lane-per-view kernel
    b_wave_ms = None
    if not args.no_wave_b:
        W = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed}, ck_lane_min=0xFFFFFFFF)
        W.run(args.churn_rounds + args.fault_rounds, churn=True)
        W.sync()
        csw, b_wave_ms = timed(W.checksums)
        assert np.array_equal(csw[live], cs[live])
        W.close()

    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                cwd=ROOT).stdout.strip() or None
    except OSError:
        commit = None
    print(json.dumps({
        "tool": "route_bench", "commit": commit, "nodes": n, "churn_k": k, "failed": len(failed),
        "rounds": args.churn_rounds + args.fault_rounds + 1, "requests": args.requests,
        "a_ring_checksums": {"first_wall_ms": round(a_first_ms, 2), "first_device_ms": round(a_first_dev, 2),
                             "wall_ms": round(a_ms, 2), "device_ms": round(a_dev, 2),
                             "cached_wall_ms": round(a_cached_ms, 3),
                             "distinct_live": int(len(np.unique(rcs[live])))},
        "b_membership_checksums": {"wall_ms": round(b_ms, 2), "again_wall_ms": round(b_again_ms, 2),
                                   "wave_path_wall_ms": None if b_wave_ms is None else round(b_wave_ms, 2),
                                   "distinct_live": int(len(np.unique(cs[live])))},
        "c_route_uniform": {"first_wall_ms": round(c_first_ms, 2), "wall_ms": round(c_ms, 2),
                            "device_ms": round(c_dev, 2),
                            "requests_per_s": round(args.requests / (c_ms * 1e-3), 1), "stats": stats},
        "d_ring_lookup_one_view": {"wall_ms": round(d_ms, 2), "keys_per_s": round(args.requests / (d_ms * 1e-3), 1)},
    }))


if __name__ == "__main__":
    main()
