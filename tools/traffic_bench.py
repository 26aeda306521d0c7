"""Request traffic at scale: one JSON document with

  (a) on route_bench's checkpoint (65,536 nodes, 20 churn rounds, then 1 % of
      the nodes fail-stop) 30 rounds of Traffic.run() with 2^20 uniform
      requests per round: the per-clock rows (the availability curve), device
      ms per poll and per submit (HIP events), the peak pending count, and the
      wall time per round beside Sim.run() of the same rounds -- in this
      process and, with --parent-lib, in a child process on another build of
      the library (the parent commit's) --; then one full ring checksum
      recomputation, to say how much of a run() round it is; before it,
      --more-rounds further rounds of run() (default 0; untimed), for the rows
      past the suspicion timeouts -- at 65,536 nodes the simulation needs a
      larger message arena (Sim(arena_entries=...)) than the default for them;
  (b) 2^24 uniform requests submitted into a converged cluster (nothing fails,
      nothing is appended) beside route_uniform() of as many, five repeats
      each: wall and device ranges.

usage: python tools/traffic_bench.py [--parent-lib PATH] [--commit ID] [--out FILE]   (GPU box)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, (time.perf_counter() - t0) * 1e3


def checkpoint(args):
    import ringpop_amd
    n, k = args.nodes, -(-args.nodes // 100)
    failed = [(i * n) // k + 1 for i in range(k)]
    S = ringpop_amd.Sim(n, args.seed, churn_k=k, failures={args.churn_rounds: failed})
    S.run(args.churn_rounds, churn=True)
    S.sync()
    return S, len(failed)


def plain_rounds(args):
    """Sim.run() of the measured rounds from the checkpoint: wall ms per round."""
    S, _ = checkpoint(args)
    _, ms = timed(lambda: (S.run(args.rounds, churn=True), S.sync()))
    S.close()
    return ms / args.rounds


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--churn-rounds", type=int, default=20)
    p.add_argument("--rounds", type=int, default=30)
    p.add_argument("--more-rounds", type=int, default=0)
    p.add_argument("--commit", help="recorded in the document (default: git's HEAD, where there is a repository)")
    p.add_argument("--per-round", type=int, default=1 << 20)
    p.add_argument("--requests", type=int, default=1 << 24)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--parent-lib", help="another build of the library: Sim.run() of the same rounds in a child process")
    p.add_argument("--plain-only", action="store_true", help="(the child) print the plain rounds' ms per round")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "traffic", "traffic_bench.json"))
    args = p.parse_args()
    if args.plain_only:
        print(json.dumps({"plain_ms_per_round": plain_rounds(args)}))
        return
    import ringpop_amd

    # (a) the availability curve through a mass failure
    S, nfailed = checkpoint(args)
    # (run() presizes for what is pending plus 24 batches: twice that covers the second run() below)
    T = S.traffic(capacity=args.per_round * 48 + 1024, timing=True)
    _, run_ms = timed(lambda: (T.run(args.rounds, args.per_round, 11), S.sync()))
    times = T.times()
    stats, by = T.stats()
    rows = T.history(args.churn_rounds, args.rounds + 1)
    pending = T.pending_count()
    # on through the suspicion timeouts and the convergence that follows (not timed)
    if args.more_rounds:
        T.run(args.more_rounds, args.per_round, 11)
        S.sync()
    more_stats, more_by = T.stats()
    more_rows = T.history(args.churn_rounds + args.rounds + 1, args.more_rounds)
    more_pending, more_peak = T.pending_count(), T.times()["peak_pending"]
    # one forced ring checksum recomputation, the kernel's code resident
    S.round(churn=True)
    S.sync()
    S.enable_timing(True, stages=["checksum"])
    _, rck_ms = timed(S.ring_checksums)
    rck_dev = S.kernel_times()["checksum"][0]
    T.close()
    S.close()
    plain_here = plain_rounds(args)
    plain_parent = None
    if args.parent_lib:
        env = dict(os.environ, RINGPOP_HIP_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--nodes", str(args.nodes), "--seed",
               str(args.seed), "--churn-rounds", str(args.churn_rounds), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(r.stdout + r.stderr)
        plain_parent = json.loads(r.stdout.strip().splitlines()[-1])["plain_ms_per_round"]
    a = {"nodes": args.nodes, "failed": nfailed, "checkpoint_rounds": args.churn_rounds, "rounds": args.rounds,
         "per_round": args.per_round, "run_wall_ms_per_round": round(run_ms / args.rounds, 3),
         "plain_run_wall_ms_per_round": round(plain_here, 3),
         "plain_run_wall_ms_per_round_parent_lib": None if plain_parent is None else round(plain_parent, 3),
         "poll_device_ms": round(times["poll_ms"] / max(times["polls"], 1), 3), "polls": times["polls"],
         "submit_device_ms": round(times["submit_ms"] / max(times["submits"], 1), 3), "submits": times["submits"],
         "peak_pending": times["peak_pending"], "pending_at_end": pending,
         "ring_checksums_wall_ms": round(rck_ms, 2), "ring_checksums_device_ms": round(rck_dev, 2),
         "ring_checksum_share_of_run_round": round(rck_dev / (run_ms / args.rounds), 3),
         "stats": stats, "by_retries": by, "rows_from_clock": args.churn_rounds, "rows": rows,
         "recovery": {"rounds": args.more_rounds, "rows_from_clock": args.churn_rounds + args.rounds + 1,
                      "pending_at_end": more_pending, "peak_pending": more_peak, "stats": more_stats,
                      "by_retries": more_by, "rows": more_rows}}

    # (b) 2^24 requests into a converged cluster, beside k_route
    C = ringpop_amd.Sim(args.nodes, args.seed)
    C.run(1, churn=False)
    C.sync()
    U = C.traffic(capacity=args.requests, timing=True)
    C.enable_timing(True, stages=["other"])
    C.route_uniform(11, 1024)  # (kernel code, routing tables, ring checksums)
    U.submit_uniform(11, 0, 1024)
    sub_wall, sub_dev, route_wall, route_dev = [], [], [], []
    for _ in range(args.repeats):
        d0 = U.times()["submit_ms"]
        _, w = timed(lambda: U.submit_uniform(11, 0, args.requests))
        sub_wall.append(round(w, 3))
        sub_dev.append(round(U.times()["submit_ms"] - d0, 3))
        d0 = C.kernel_times()["other"][0]
        rs, w = timed(lambda: C.route_uniform(11, args.requests))
        route_wall.append(round(w, 3))
        route_dev.append(round(C.kernel_times()["other"][0] - d0, 3))
    ustats, _ = U.stats()
    assert U.pending_count() == 0 and ustats["failed"] == 0 and ustats["retry_scheduled"] == 0
    assert rs["local"] + rs["delivered"] == args.requests
    b = {"nodes": args.nodes, "requests": args.requests, "repeats": args.repeats,
         "submit_uniform_wall_ms": sub_wall, "submit_uniform_device_ms": sub_dev,
         "route_uniform_wall_ms": route_wall, "route_uniform_device_ms": route_dev,
         "submitted": ustats["submitted"], "delivered": ustats["delivered"], "local": ustats["local"]}
    U.close()
    C.close()

    commit = args.commit
    try:
        commit = commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                          cwd=ROOT).stdout.strip() or None
    except OSError:
        pass
    doc = {"tool": "traffic_bench", "commit": commit, "a_mass_failure_run": a, "b_converged_submit_vs_route": b}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in a.items() if k not in ("rows", "by_retries", "recovery")}))
    print(json.dumps({k: v for k, v in a["recovery"].items() if k != "rows"}))
    print(json.dumps(b))


if __name__ == "__main__":
    main()
