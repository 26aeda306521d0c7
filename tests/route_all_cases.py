"""Multi-key requests (rp_sim_route_all): the batches and the
expectation, restated in plain Python from the CPU oracle alone --
Sim.ring_lookup(v, h), Sim.info(v)["ring_checksum"], Sim.info(v)["dead"] and
route_cases.cut -- over route_cases' scenarios; everything is integer-exact."""
import functools

import numpy as np

import oracle
import ownership_cases as oc
import route_cases as rc

EMPTY, NO_GROUP = 255, 0xFFFF
ARRAYS = ("key_group", "key_agrees", "group_dest", "group_outcome", "group_keys", "group_agree", "fanout", "worst")
# clocks inside and after each scenario's divergence window
CHECKPOINTS = {"failstop": (29, 31, 45), "partition": (30, 40, 46), "shift": (27, 28, 40)}
# one fixed-K batch per code path: every lane count, the chunk boundary, one key past it, the cap
KS = (1, 8, 9, 16, 32, 33, 64, 65, 128, 256)
COUNT = 203  # requests of a fixed-K batch: no multiple of the 8, 4 or 2 requests of a wave
RAGGED = (0, 1, 7, 63, 64, 65, 255, 256)


def uniform_batch(n, count, K, seed=rc.REQ_SEED):
    """rp_sim_route_all_uniform's requests: (entries, offsets, key_hashes)."""
    e, h = rc.requests(seed, count * K, n)
    return e[::K].copy(), np.arange(count + 1, dtype=np.uint64) * np.uint64(K), h


def ragged_batch(n, addresses, shift=0):
    """RAGGED five times over and a last request without keys; nodes 5 and 3 (fail-stopped in two scenarios) enter
    with 7 and 63 keys; half the keys lie on, just below and just above ring points and at both ends of the space."""
    ks = np.array(RAGGED * 5 + (0,), dtype=np.uint64)
    off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(ks, dtype=np.uint64)])
    T = int(off[-1])
    e, h = rc.requests(rc.REQ_SEED + 1, T, n)
    q = oc.queries(oc.boundaries(addresses, shift))
    h[:T // 2] = q[np.linspace(0, len(q) - 1, T // 2).astype(np.int64)]
    h[T // 2] = 0
    e = e[np.minimum(off[:-1], T - 1).astype(np.int64)]
    e[2], e[3] = 5, 3
    return e, off, h


def stats_of(r, entries, offsets):
    """rp_route_all_stats from the result arrays."""
    K = np.diff(offsets).astype(np.int64)
    live = r["worst"] != rc.ENTRY_DEAD
    req = np.repeat(np.arange(len(K)), K)  # (a key's, and a group slot's, request)
    klive = live[req]
    koc = r["group_outcome"][offsets[:-1].astype(np.int64)[req][klive] + r["key_group"][klive]]
    goc, sent = r["group_outcome"], (r["group_outcome"] == 1) | (r["group_outcome"] == 2)
    f = r["fanout"][live].astype(np.int64)
    return {"requests": len(K), "entry_dead": int((~live).sum()), "empty": int((live & (K == 0)).sum()),
            "keys": int(klive.sum()), "groups": int((goc != EMPTY).sum()),
            "group_outcome": np.bincount(goc[goc != EMPTY], minlength=4).tolist(),
            "key_outcome": np.bincount(koc, minlength=4).tolist(),
            "misrouted_keys": int(((koc == 1) | (koc == 2)).sum() - r["key_agrees"].sum()),
            "split_groups": int((sent & (r["group_agree"] > 0) & (r["group_agree"] < r["group_keys"])).sum()),
            "worst_hist": np.bincount(r["worst"][live], minlength=4).tolist(),
            "fanout_hist": np.bincount([int(x).bit_length() for x in f], minlength=10).tolist(),
            "max_fanout": int(r["fanout"].max(initial=0))}


def expect(cpu, clock, partition, entries, offsets, keys):
    """The issue's definition for the oracle `cpu` after `clock` rounds: a dict of ARRAYS and "stats"."""
    info = [cpu.info(v) for v in range(cpu.n)]
    dead, rcs = [i["dead"] != 0 for i in info], [i["ring_checksum"] for i in info]
    look = functools.lru_cache(maxsize=None)(cpu.ring_lookup)
    T, m, h = len(keys), len(entries), keys.tolist()
    r = {"key_group": np.full(T, NO_GROUP, np.uint16), "key_agrees": np.zeros(T, np.uint8),
         "group_dest": np.full(T, -1, np.int32), "group_outcome": np.full(T, EMPTY, np.uint8),
         "group_keys": np.zeros(T, np.uint16), "group_agree": np.zeros(T, np.uint16),
         "fanout": np.zeros(m, np.uint16), "worst": np.zeros(m, np.uint8)}
    for i, e in enumerate(entries.tolist()):
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        if dead[e]:
            r["worst"][i] = rc.ENTRY_DEAD
            continue
        groups = {}  # owner -> rank: insertion order is first appearance (_.groupBy, then Object.keys)
        for k in range(lo, hi):
            d = look(e, h[k])
            r["key_group"][k] = groups.setdefault(e if d < 0 else d, len(groups))
        for d, j in groups.items():
            member = np.flatnonzero(r["key_group"][lo:hi] == j) + lo
            if d == e:
                oc_ = rc.LOCAL
            elif dead[d] or rc.cut(partition, clock, e, d):
                oc_ = rc.UNREACHABLE
            else:
                oc_ = rc.CHECKSUMS_DIFFER if rcs[e] != rcs[d] else rc.DELIVERED
                for k in member.tolist():
                    r["key_agrees"][k] = 1 if look(d, h[k]) == d else 0
            r["group_dest"][lo + j], r["group_outcome"][lo + j], r["group_keys"][lo + j] = d, oc_, len(member)
            r["group_agree"][lo + j] = r["key_agrees"][member].sum()
            r["worst"][i] = max(r["worst"][i], oc_)
        r["fanout"][i] = len(groups)
    r["stats"] = stats_of(r, entries, offsets)
    return r


def batches(n, addresses, shift=0):
    """name -> (entries, offsets, key_hashes): the fixed-K batches and the ragged one."""
    b = {K: uniform_batch(n, COUNT, K) for K in KS}
    b["ragged"] = ragged_batch(n, addresses, shift)
    return b


@functools.lru_cache(maxsize=None)
def expected(name):
    """The scenario on the oracle (seed 7, churn on): {clock: {batch: expect()}} at its CHECKPOINTS, and the batches.
    Computed once and shared; callers must not modify it."""
    n, kw, _, _ = rc.SCENARIOS[name]
    cpu = oracle.Sim(n, rc.SIM_SEED, **kw)
    bs = batches(n, [cpu.address(v) for v in range(n)], kw.get("replica_hash_shift", 0))
    out = {}
    for r in range(1, max(CHECKPOINTS[name]) + 1):
        cpu.round(churn=True)
        if r in CHECKPOINTS[name]:
            out[r] = {b: expect(cpu, r, kw.get("partition"), *x) for b, x in bs.items()}
    cpu.close()
    return out, bs
