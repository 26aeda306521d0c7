"""Multi-key request traffic at scale: on a 65,536-node
simulation in tools/rolling_restart.py's setting (1 % of the nodes leave per
round from round 20 on, each away for 30 rounds), --rounds rounds in --

  submit   Traffic_all.submit_uniform(seed, first, --keys / K, K) for K = 8 and
           64 beside Sim.route_all_uniform of the same requests at the same
           instant: ns per key of each.  Two submits come first (code, tables,
           the arenas' growth); each timed one draws new requests.
  poll     the same --requests single-key requests through Sim.traffic and,
           one key a request, through Sim.traffic_all (max_retries 8, schedule
           {1}: every pending send is due at every clock), then rounds with a
           poll of each: ms per poll and ns per pending send at equal pending
           sends; the same for a K = 8 tracker.

Every figure is a host clock around a call that ends in a device synchronise,
with the ring checksums of the instant computed before (Sim.ring_checksums), so
that no call pays for them: the median and the range over --repeat.  Writes
profiles/traffic_all/traffic_all_bench.json and prints it.

usage: python tools/traffic_all_bench.py [--nodes N] [--keys T]   (GPU box)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ringpop_amd  # noqa: E402
from tools.rolling_restart import schedule  # noqa: E402

REQ_SEED = 11


def clocked(S, f):
    S.sync()
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def figure(ms, units):
    med = float(np.median(ms))
    return {"ms": round(med, 3), "ms_range": [round(min(ms), 3), round(max(ms), 3)], "units": int(units),
            "ns_per_unit": round(med * 1e6 / units, 3) if units else None}


def submit(S, keys, repeat):
    out = {}
    S.ring_checksums()
    for K in (8, 64):
        count = keys // K
        T = S.traffic_all(capacity=1 << 22, key_capacity=1 << 26)
        for w in range(2):
            T.submit_uniform(REQ_SEED, w * count, count, K)
        S.route_all_uniform(REQ_SEED, count, K)
        sub, one = [], []
        for r in range(repeat):
            sub.append(clocked(S, lambda: T.submit_uniform(REQ_SEED, (2 + r) * count, count, K)))
            one.append(clocked(S, lambda: S.route_all_uniform(REQ_SEED, count, K)))
        st = T.stats()[0]
        out[str(K)] = {"submit_uniform": figure(sub, keys), "route_all_uniform": figure(one, keys),
                       "ratio": round(float(np.median(sub) / np.median(one)), 3), "open_sends": len(T.pending()[0]),
                       "sends": st["sends"], "requests": st["requests"]}
        T.close()
    return out


def poll(S, requests, repeat):
    cfg = dict(max_retries=8, schedule=(1,), capacity=1 << 23)
    Ta, Tb, Tc = S.traffic(**cfg), S.traffic_all(**cfg), S.traffic_all(key_capacity=1 << 26, **cfg)
    Ta.submit_uniform(REQ_SEED, 0, requests)
    Tb.submit_uniform(REQ_SEED, 0, requests, 1)
    Tc.submit_uniform(REQ_SEED, 0, requests // 8, 8)
    rows = []
    for r in range(repeat + 1):  # (the first round's polls load the code: left out)
        S.round(churn=False)
        S.ring_checksums()
        before = (Ta.pending_count(), len(Tb.pending()[0]), len(Tc.pending()[0]))
        ms = (clocked(S, Ta.poll), clocked(S, Tb.poll), clocked(S, Tc.poll))
        if r:
            rows.append({"pending_sends": before, "ms": [round(x, 3) for x in ms],
                         "ns_per_pending_send": [round(x * 1e6 / max(p, 1), 2) for x, p in zip(ms, before)]})
        assert before[0] == before[1], before
    sa, sb = Ta.stats()[0], Tb.stats()[0]
    assert all(sa[k] == sb[k] for k in ("delivered", "failed", "proxied", "retry_attempted")), (sa, sb)
    for T in (Ta, Tb, Tc):
        T.close()
    return {"trackers": ["rp_traffic", "rp_traffic_all K=1", "rp_traffic_all K=8"], "polls": rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=65536)
    p.add_argument("--seed", type=int, default=2024)
    p.add_argument("--warm", type=int, default=20)
    p.add_argument("--frac", type=float, default=0.01)
    p.add_argument("--waves", type=int, default=20)
    p.add_argument("--away", type=int, default=30)
    p.add_argument("--rounds", type=int, default=30, help="rounds before the measurements: inside the event window")
    p.add_argument("--keys", type=int, default=1 << 22, help="keys of every submit (a multiple of 64)")
    p.add_argument("--requests", type=int, default=1 << 22, help="single-key requests of the poll comparison")
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--arena-entries", type=int, default=3 << 30, help="message arena (DESIGN.md §11): the event window fills it")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "traffic_all", "traffic_all_bench.json"))
    args = p.parse_args()
    n, k = args.nodes, -(-args.nodes // 100)
    leaves, rejoins = schedule(args)
    S = ringpop_amd.Sim(n, args.seed, churn_k=k, leaves=leaves, rejoins=rejoins, arena_entries=args.arena_entries)
    for r in range(args.rounds):
        S.round(churn=r < args.warm)
    out = {"tool": "traffic_all_bench", "nodes": n, "rounds": args.rounds, "leavers_per_round": len(leaves[args.warm]),
           "repeat": args.repeat, "submit": submit(S, args.keys, args.repeat)}
    out["poll"] = poll(S, args.requests, args.repeat)
    S.close()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
