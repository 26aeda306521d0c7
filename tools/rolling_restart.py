"""A rolling restart at scale: one JSON document.

After --warm rounds of churn, --frac of the nodes leave gracefully per round
for --waves rounds, each rejoining --away rounds later (rp_sim_leave /
rp_sim_rejoin); the run goes on until every live, gossiping view agrees again.

  baseline   the same rounds with no events scheduled, same process: wall ms
             per round (Sim.round, so each round ends with a host read)
  restart    the events: wall ms per round, the rounds' counts, the first
             converged round after the last rejoin
  traffic    (--per-round > 0) the events again under Traffic.run with
             --per-round uniform requests per round: the per-clock rows (the
             availability curve: finals that reached an owner / submitted)

A run that stops on a device error (a full message arena, say) reports the
round and the error instead of the rest.

usage: python tools/rolling_restart.py [--nodes N] [--out FILE]   (GPU box)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def schedule(args):
    """{round: [ids]} for the leaves and the rejoins: wave w takes the next
    `per` ids of a fixed permutation of the nodes (odd multiplier mod n)."""
    n, per = args.nodes, max(1, int(args.nodes * args.frac))
    mul = 7919 if n % 7919 else 7907
    leaves, rejoins = {}, {}
    for w in range(args.waves):
        ids = sorted({((w * per + j) * mul + 1) % n for j in range(per)})
        leaves[args.warm + w] = ids
        rejoins[args.warm + w + args.away] = ids
    return leaves, rejoins


def drive(S, args, last_event, label):
    """Rounds until reconvergence (or --max-rounds): per-round wall ms and counts."""
    import ringpop_amd
    rows, stop = [], None
    try:
        for r in range(args.max_rounds):
            t0 = time.perf_counter()
            o = S.round(churn=r < args.warm)
            ms = (time.perf_counter() - t0) * 1e3
            rows.append({"round": r, "ms": round(ms, 3), "evaluated": o["evaluated"], "applied": o["applied"],
                         "full_syncs": o["full_syncs"], "messages": o["messages"], "waves": o["waves"],
                         "converged": bool(o["converged"])})
            if r > last_event and o["converged"]:
                break
    except ringpop_amd.RingpopError as e:
        stop = {"round": len(rows), "error": str(e)}
    print(label, "rounds", len(rows), "stopped" if stop else "done", file=sys.stderr, flush=True)
    return rows, stop


def mean(xs):
    return round(sum(xs) / len(xs), 3) if xs else None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--warm", type=int, default=20, help="rounds of churn before the first leave")
    p.add_argument("--frac", type=float, default=0.01, help="share of the nodes that leaves per round")
    p.add_argument("--waves", type=int, default=20, help="rounds with leaves")
    p.add_argument("--away", type=int, default=30, help="rounds between a node's leave and its rejoin")
    p.add_argument("--max-rounds", type=int, default=200)
    p.add_argument("--per-round", type=int, default=1 << 16, help="traffic: requests per round (0: skip)")
    p.add_argument("--arena-entries", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import ringpop_amd
    n, k = args.nodes, -(-args.nodes // 100)
    leaves, rejoins = schedule(args)
    first, last = args.warm, args.warm + args.waves - 1 + args.away
    doc = {"nodes": n, "churn_per_round": k, "warm": args.warm, "leavers_per_round": len(leaves[first]),
           "waves": args.waves, "away": args.away, "first_leave": first, "last_rejoin": last}
    kw = dict(churn_k=k, arena_entries=args.arena_entries)

    S = ringpop_amd.Sim(n, args.seed, **kw, leaves=leaves, rejoins=rejoins)
    rows, stop = drive(S, args, last, "restart")
    S.close()
    conv = [r["round"] for r in rows if r["round"] > last and r["converged"]]
    window = [r["ms"] for r in rows if first <= r["round"] <= last]
    doc["restart"] = {"rounds": rows, "stopped": stop, "reconverged_at": conv[0] if conv else None,
                      "rounds_to_reconverge": conv[0] - last if conv else None,
                      "ms_per_round_event_window": mean(window), "ms_per_round_max": max(window) if window else None,
                      "ms_per_round_warm": mean([r["ms"] for r in rows if 5 <= r["round"] < first])}

    # the same rounds with nothing scheduled (as many as the restart ran)
    B = ringpop_amd.Sim(n, args.seed, **kw)
    base = []
    for r in range(len(rows)):
        t0 = time.perf_counter()
        B.round(churn=r < args.warm)
        base.append(round((time.perf_counter() - t0) * 1e3, 3))
    B.close()
    doc["baseline"] = {"ms": base, "ms_per_round_event_window": mean(base[first:last + 1]),
                       "ms_per_round_warm": mean(base[5:first])}

    if args.per_round and not stop:
        S = ringpop_amd.Sim(n, args.seed, **kw, leaves=leaves, rejoins=rejoins)
        # (run() reserves a worst case: every request of the schedule's 23 rounds + 1 pending)
        T = S.traffic(capacity=max(1 << 20, 32 * args.per_round))
        total = len(rows)
        try:
            T.run(args.warm, args.per_round, 11, churn=True)
            T.run(total - args.warm, args.per_round, 11, churn=False)
            for _ in range(20):  # the retries still pending
                S.round(churn=False)
                T.poll()
            hist = T.history(1, total + 20)
            curve = []
            for c, h in enumerate(hist, start=1):
                done = h["local"] + h["delivered"] + h["rerouted_local"] + h["failed"] + h["entry_dead"]
                curve.append({"clock": c, "finals": done, "served": h["local"] + h["delivered"] + h["rerouted_local"],
                              "failed": h["failed"], "checksums_differ": h["checksums_differ"],
                              "send_unreachable": h["send_unreachable"], "retry_scheduled": h["retry_scheduled"],
                              "retry_succeeded": h["retry_succeeded"], "misrouted": h["misrouted"]})
            st, by = T.stats()
            doc["traffic"] = {"per_round": args.per_round, "stats": st, "by_retries": by, "curve": curve,
                              "pending_at_end": T.pending_count()}
        except ringpop_amd.RingpopError as e:
            doc["traffic"] = {"error": str(e)}
        T.close()
        S.close()

    text = json.dumps(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    r = doc["restart"]
    print(json.dumps({k2: v for k2, v in doc.items() if k2 not in ("restart", "baseline", "traffic")}))
    print("restart: ms/round warm %s, event window %s (max %s); baseline warm %s, window %s; reconverged at %s (%s rounds "
          "after the last rejoin); stopped: %s" % (r["ms_per_round_warm"], r["ms_per_round_event_window"],
                                                    r["ms_per_round_max"], doc["baseline"]["ms_per_round_warm"],
                                                    doc["baseline"]["ms_per_round_event_window"], r["reconverged_at"],
                                                    r["rounds_to_reconverge"], r["stopped"]))
    if "traffic" in doc and "stats" in doc["traffic"]:
        print("traffic:", doc["traffic"]["stats"])


if __name__ == "__main__":
    main()
