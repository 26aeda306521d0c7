"""Ring checksums of all views, one view per wave against one view per lane
(DESIGN.md §22): for each cluster size, on (a) a converged cluster after 20
churn rounds and (b) §10's checkpoint (20 churn rounds, 1 % of the nodes
fail-stop, 30 more rounds: nearly all rings distinct), the device time (HIP
events) of Sim.ring_checksums() with the path forced to the wave kernel and
to the lane kernel.  The two alternate: a warm-up call each, then five timed
repeats each.  Setting the path before every call marks the cached checksums
stale, so every call recomputes, and both paths hash the same rings; one more
round runs before the warm-up pair only (at (b)'s checkpoint with 65,536
nodes a few further single rounds fill the simulation's message arena).  The
two result arrays are compared after every pair.  One JSON line per size and
kind, and a last line with the crossover: the smallest size from which the lane
path's slowest repeat beats the wave path's fastest on both kinds.

usage: python tools/ring_ck_bench.py [--nodes N ...] [--out FILE]   (GPU box)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ringpop_amd  # noqa: E402

WAVE, LANE = 0xFFFFFFFF, 1
REPEATS = 5


def bench(n, seed, kind):
    k = -(-n // 100)
    failed = [(i * n) // k + 1 for i in range(k)]
    S = ringpop_amd.Sim(n, seed, churn_k=k, failures={20: failed} if kind == "b" else None)
    S.run(20 if kind == "a" else 50, churn=True)
    S.sync()
    S.enable_timing(True, stages=["checksum"])
    times = {WAVE: [], LANE: []}
    S.round(churn=True)
    for rep in range(REPEATS + 1):  # (the first pair warms up)
        got = {}
        for path in (WAVE, LANE):
            S.ring_checksum_lanes(path)
            before = S.kernel_times()["checksum"][0]
            got[path] = S.ring_checksums()
            if rep:
                times[path].append(S.kernel_times()["checksum"][0] - before)
        assert np.array_equal(got[WAVE], got[LANE]), (n, kind, rep)
    distinct = int(len(np.unique(got[LANE])))
    counts = S.ring_checksum_counts()
    assert counts["wave_views"] == counts["lane_views"] == (REPEATS + 1) * n
    # the string bytes hashed (20-byte blocks = bytes / 20) from the views' rings
    alen = np.array([len(a) for a in S.addresses()], dtype=np.int64) if n <= 8192 else None
    S.close()
    w, l = times[WAVE], times[LANE]
    return {"tool": "ring_ck_bench", "nodes": n, "kind": kind, "distinct_checksums": distinct,
            "wave_ms": [round(x, 3) for x in w], "lane_ms": [round(x, 3) for x in l],
            "wave_min_ms": round(min(w), 3), "lane_max_ms": round(max(l), 3),
            "lane_wins": bool(max(l) < min(w)), "in_ring_bytes": n * n,
            "mean_address_bytes": None if alen is None else round(float(alen.mean()), 2)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, nargs="+", default=[4096, 8192, 16384, 32768, 65536])
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ringck", "ring_ck_bench.json"))
    args = p.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []
    with open(args.out, "w") as f:
        for n in sorted(args.nodes):
            for kind in ("a", "b"):
                rows.append(bench(n, args.seed, kind))
                print(json.dumps(rows[-1]), flush=True)
                f.write(json.dumps(rows[-1]) + "\n")
                f.flush()
        wins = {n: all(r["lane_wins"] for r in rows if r["nodes"] == n) for n in sorted(args.nodes)}
        sizes = sorted(wins)
        cross = next((n for i, n in enumerate(sizes) if all(wins[m] for m in sizes[i:])), None)
        last = {"tool": "ring_ck_bench", "crossover_nodes": cross, "lane_wins_by_nodes": wins}
        print(json.dumps(last), flush=True)
        f.write(json.dumps(last) + "\n")


if __name__ == "__main__":
    main()
