"""The ownership census (rp_sim_ownership / rp_sim_ownership_at):
the scenarios and the expectation, restated from the CPU oracle alone.

The boundaries are the sorted distinct replica hashes of every address.  Node
v with info(v)["dead"] == 0 claims the interval that ends at boundary b iff
ring_lookup(v, b) is v, or negative (an empty ring: lookup falls back to
whoami).  Everything is integer-exact."""
import functools

import numpy as np

import oracle

SIM_SEED = 7
REPLICAS = 100
SPACE = 1 << 32

# name -> (n, Sim keywords, rounds, (first, last) round of the window compared at every round)
SCENARIOS = {
    "failstop": (48, {"failures": {2: [5, 20, 21, 47]}}, 45, (26, 36)),
    "partition": (64, {"partition": {"start": 1, "end": 40, "split": 20}}, 50, (26, 36)),
    # colliding replica hashes: the coll_owner path, replicas of one server on one point
    "shift": (32, {"replica_hash_shift": 20, "failures": {1: [3]}}, 40, (26, 30)),
    # every round, and before the first
    "join": (40, {"joins": [(3, 7, [0, 1]), (3, 33, [2]), (6, 12, [7])]}, 14, (0, 14)),
}


def checkpoints(name):
    """The clocks (rounds run so far) a scenario is compared at."""
    _, _, rounds, (w0, w1) = SCENARIOS[name]
    return [r for r in range(0 if w0 == 0 else 1, rounds + 1) if r % 3 == 0 or w0 <= r <= w1]


def boundaries(addresses, shift=0):
    """The sorted distinct replica hashes farmhash32(address + str(i)), i < 100."""
    h = oracle.farmhash32_batch([a + str(i) for a in addresses for i in range(REPLICAS)]).astype(np.uint32)
    if shift:
        h = (h >> np.uint32(shift)) << np.uint32(shift)
    return np.unique(h)


def lengths(b):
    """Interval i >= 1 is (b[i-1], b[i]]; interval 0 wraps."""
    ln = np.empty(len(b), dtype=np.uint64)
    ln[1:] = np.diff(b.astype(np.uint64))
    ln[0] = int(b[0]) + SPACE - int(b[-1])
    assert int(ln.sum()) == SPACE
    return ln


def census(b, rows):
    """The results of the issue's definition from rows = an iterable of
    (v, claim[v, :]) over the claimants (claim[v, i]: node v claims interval
    i), read once; `n` entries of claimed come from the caller."""
    ln = lengths(b)
    claims = np.zeros(len(b), dtype=np.uint32)
    claimed = {}
    for v, row in rows:
        claims += row
        claimed[v] = int(ln[row].sum())
    cls = np.minimum(claims, 7)
    first = int(np.argmax(claims))  # (the first index of the maximum)
    return {"measure": [int(ln[cls == k].sum()) for k in range(8)],
            "exact": {int(k): int(ln[claims == k].sum()) for k in np.unique(claims)},
            "claimants": len(claimed), "intervals": len(b), "max_claims": int(claims[first]),
            "max_claims_hash": int(b[first]), "claimed_by": claimed, "claims": claims}


def finish(e, n):
    by = e.pop("claimed_by")
    e["claimed"] = np.array([by.get(v, 0) for v in range(n)], dtype=np.uint64)
    return e


def queries(b):
    """Key hashes around every boundary, and both ends of the hash space."""
    return np.concatenate([b, b - np.uint32(1), b + np.uint32(1), np.array([0, SPACE - 1], dtype=np.uint32)])


def claims_at(b, claims, hashes):
    """claims of the interval each hash falls in: the first boundary >= h, else interval 0."""
    i = np.searchsorted(b, hashes, side="left")
    return claims[np.where(i == len(b), 0, i)]


def expect(cpu, b):
    n, look, bl = cpu.n, cpu.ring_lookup, b.tolist()
    dead = [cpu.info(v)["dead"] for v in range(n)]
    e = finish(census(b, ((v, np.array([o == v or o < 0 for o in (look(v, h) for h in bl)], dtype=bool))
                          for v in range(n) if dead[v] == 0)), n)
    e["dead"] = dead
    return e


def brute_force(S, b):
    """The same from a device simulation's own per-view lookup kernel
    (Sim.ring_lookup over every claimant view, `dead` from Sim.info): the
    yardstick where the oracle has no model."""
    n = S.n
    dead = [S.info(v)["dead"] for v in range(n)]

    def rows():
        for v in range(n):
            if dead[v] == 0:
                o = S.ring_lookup(v, b)
                yield v, (o == v) | (o < 0)

    e = finish(census(b, rows()), n)
    e["dead"] = dead
    return e


@functools.lru_cache(maxsize=None)
def expected(name):
    """The scenario on the oracle (seed 7, churn on): (boundaries, {clock:
    expect()}) at checkpoints(name).  Computed once and shared by every test
    and shard count; callers must not modify it."""
    n, kw, rounds, _ = SCENARIOS[name]
    cpu = oracle.Sim(n, SIM_SEED, **kw)
    b = boundaries([cpu.address(v) for v in range(n)], kw.get("replica_hash_shift", 0))
    want, out = set(checkpoints(name)), {}
    if 0 in want:
        out[0] = expect(cpu, b)
    for r in range(1, rounds + 1):
        cpu.round(churn=True)
        if r in want:
            out[r] = expect(cpu, b)
    cpu.close()
    return b, out
