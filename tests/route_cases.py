"""Request routing (rp_sim_route): the scenarios, the request generator and the
expectation, restated from the CPU oracle alone.

The expectation uses three oracle calls -- Sim.ring_lookup(v, h),
Sim.info(v)["ring_checksum"] and Sim.info(v)["dead"] -- and the partition
window; everything is integer-exact."""
import functools

import numpy as np

import oracle

OUTCOMES = ("local", "delivered", "checksums_differ", "unreachable", "entry_dead")
LOCAL, DELIVERED, CHECKSUMS_DIFFER, UNREACHABLE, ENTRY_DEAD = range(5)
COUNTS = OUTCOMES + ("misrouted",)

SIM_SEED, REQ_SEED, REQUESTS = 7, 11, 1500

# name -> (n, Sim keywords, rounds, the counts that must occur over its checkpoints)
SCENARIOS = {
    # one full chunk of 64 members and a partial one; rings diverge in rounds 28-34
    "failstop": (96, {"failures": {2: [5, 40, 41, 95]}}, 45, COUNTS),
    # the window closes at the route after round 40 (the next round's clock)
    "partition": (64, {"partition": {"start": 1, "end": 40, "split": 20}}, 50,
                  tuple(k for k in COUNTS if k != "entry_dead")),
    # colliding replica hashes: the coll_owner path
    "shift": (32, {"replica_hash_shift": 20, "failures": {1: [3]}}, 40, COUNTS),
}

_G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def splitmix64_finalise(z):
    """Plain-Python splitmix64 finaliser (the header's constants)."""
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def request(seed, i, n):
    """Request i of rp_sim_route_uniform, in plain Python: (entry, key_hash)."""
    r = splitmix64_finalise(seed + (i + 1) * _G)
    return ((r >> 32) * n) >> 32, r & 0xFFFFFFFF


def requests(seed, count, n):
    """The first `count` requests as numpy arrays (entries, key_hashes)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(count, dtype=np.uint64) + np.uint64(1)) * np.uint64(_G)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    entries = (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.uint32)
    return entries, (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def cut(partition, clock, a, b):
    return bool(partition) and partition["split"] > 0 and partition["start"] <= clock < partition["end"] and \
        ((a < partition["split"]) != (b < partition["split"]))


def expect(cpu, clock, partition, entries, keys):
    """The routing table of the issue, from the oracle `cpu` after `clock`
    rounds: (dests, outcomes, owner_agrees, stats, ring checksums)."""
    n = cpu.n
    info = [cpu.info(v) for v in range(n)]
    dead = [i["dead"] != 0 for i in info]
    rcs = [i["ring_checksum"] for i in info]
    m = len(entries)
    dests = np.full(m, -1, dtype=np.int32)
    outcomes = np.zeros(m, dtype=np.uint8)
    agrees = np.zeros(m, dtype=np.uint8)
    for i, (e, h) in enumerate(zip(entries.tolist(), keys.tolist())):
        if dead[e]:
            outcomes[i] = ENTRY_DEAD
            continue
        d = cpu.ring_lookup(e, h)
        if d < 0 or d == e:  # (an empty ring: lookup falls back to whoami)
            outcomes[i], dests[i] = LOCAL, e
            continue
        dests[i] = d
        if dead[d] or cut(partition, clock, e, d):
            outcomes[i] = UNREACHABLE
            continue
        outcomes[i] = CHECKSUMS_DIFFER if rcs[e] != rcs[d] else DELIVERED
        agrees[i] = 1 if cpu.ring_lookup(d, h) == d else 0
    stats = {k: int((outcomes == c).sum()) for c, k in enumerate(OUTCOMES)}
    stats["requests"] = m
    stats["misrouted"] = int((((outcomes == DELIVERED) | (outcomes == CHECKSUMS_DIFFER)) & (agrees == 0)).sum())
    return dests, outcomes, agrees, stats, np.array(rcs, dtype=np.uint32)


def sim_kwargs(name):
    return dict(SCENARIOS[name][1])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The scenario on the oracle (seed 7, churn on), routed after every round
    with the 1,500 requests of seed 11: a list, entry r - 1 = expect() after
    round r.  Computed once and shared; callers must not modify it."""
    n, kw, rounds, _ = SCENARIOS[name]
    cpu = oracle.Sim(n, SIM_SEED, **kw)
    entries, keys = requests(REQ_SEED, REQUESTS, n)
    out = []
    for r in range(1, rounds + 1):
        cpu.round(churn=True)
        out.append(expect(cpu, r, kw.get("partition"), entries, keys))
    cpu.close()
    return out
