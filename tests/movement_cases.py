"""Ownership movement between two instants (rp_sim_ownership_moved; DESIGN.md
§15): the clocks, the pairs and the expectation, restated from the CPU oracle
alone.

A claimant's claim row at a clock is, per boundary b (ownership_cases), whether
ring_lookup(v, b) is v or negative; a node that is no claimant has the empty
row.  Node v gains what its row holds at `to` and not at `from` and loses the
reverse; every stats field, gained[] and lost[] follow with numpy.  Everything
is integer-exact."""
import functools

import numpy as np

import oracle
import ownership_cases as oc

SPACE = oc.SPACE

# the clocks (rounds run so far) each scenario of ownership_cases.SCENARIOS is snapshotted at
CLOCKS = {
    "failstop": [1, 3, 27, 30, 33, 45],
    "partition": [1, 30, 39, 42, 45, 50],
    "shift": [1, 20, 28, 40],
    "join": [0, 3, 4, 7, 14],
}
# one pair of each scenario the other way round
REVERSED = {"failstop": (30, 27), "partition": (42, 39), "shift": (28, 20), "join": (4, 3)}

SCALARS = ("same_set", "handed_off", "gained", "lost", "gainers", "losers", "max_gained", "max_gained_node", "max_lost",
           "max_lost_node", "max_turnover", "max_turnover_hash", "from_clock", "to_clock", "intervals")


def pairs(name):
    """Consecutive clocks, first -> last, and one pair reversed."""
    c = CLOCKS[name]
    return list(zip(c[:-1], c[1:])) + [(c[0], c[-1]), REVERSED[name]]


def unpacked(row, npts):
    return np.unpackbits(row, count=npts).astype(bool)


def movement(b, frm, to, n, from_clock, to_clock):
    """The issue's definitions from two {claimant: bit-packed claim row} maps."""
    ln, npts = oc.lengths(b), len(b)
    g, l, cf, ct = (np.zeros(npts, dtype=np.int64) for _ in range(4))
    gained, lost = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    none = np.zeros(npts, dtype=bool)
    for v in range(n):
        rf = unpacked(frm[v], npts) if v in frm else none
        rt = unpacked(to[v], npts) if v in to else none
        gv, lv = rt & ~rf, rf & ~rt
        g += gv
        l += lv
        cf += rf
        ct += rt
        gained[v], lost[v] = int(ln[gv].sum()), int(ln[lv].sum())
    assert np.array_equal(ct, cf + g - l)
    a, c = np.minimum(cf, 2), np.minimum(ct, 2)
    turnover = g + l
    first = int(np.argmax(turnover))  # (the first index of the maximum)
    moved = bool(turnover[first])
    e = {"transition": [[int(ln[(a == i) & (c == j)].sum()) for j in range(3)] for i in range(3)],
         "same_set": int(ln[turnover == 0].sum()),
         "handed_off": int(ln[(cf == 1) & (ct == 1) & (g == 1) & (l == 1)].sum()),
         "gained": sum(int(x) for x in gained), "lost": sum(int(x) for x in lost),
         "gainers": int(np.count_nonzero(gained)), "losers": int(np.count_nonzero(lost)),
         "max_gained": int(gained.max()), "max_gained_node": int(np.argmax(gained)),
         "max_lost": int(lost.max()), "max_lost_node": int(np.argmax(lost)),
         "max_turnover": int(turnover[first]), "max_turnover_hash": int(b[first]) if moved else 0,
         "from_clock": from_clock, "to_clock": to_clock, "intervals": npts,
         "gained_by": gained, "lost_by": lost}
    assert sum(sum(r) for r in e["transition"]) == SPACE
    return e


def oracle_rows(cpu, b):
    n, look, bl = cpu.n, cpu.ring_lookup, b.tolist()
    return {v: np.packbits(np.array([o == v or o < 0 for o in (look(v, h) for h in bl)], dtype=bool))
            for v in range(n) if cpu.info(v)["dead"] == 0}


def device_rows(S, b):
    """The brute force: the same rows from a device simulation's own per-view
    lookup kernel (Sim.ring_lookup), where the oracle has no model."""
    out = {}
    for v in range(S.n):
        if S.info(v)["dead"] == 0:
            o = S.ring_lookup(v, b)
            out[v] = np.packbits((o == v) | (o < 0))
    return out


def claimed(b, rows, n):
    ln = oc.lengths(b)
    return np.array([int(ln[unpacked(rows[v], len(b))].sum()) if v in rows else 0 for v in range(n)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The scenario on the oracle (seed 7, churn on): (boundaries, {(from, to):
    movement()} for pairs(name), {clock: claimed[]}).  Computed once and shared;
    callers must not modify it."""
    n, kw, rounds, _ = oc.SCENARIOS[name]
    cpu = oracle.Sim(n, oc.SIM_SEED, **kw)
    b = oc.boundaries([cpu.address(v) for v in range(n)], kw.get("replica_hash_shift", 0))
    want, rows = set(CLOCKS[name]), {}
    if 0 in want:
        rows[0] = oracle_rows(cpu, b)
    for r in range(1, rounds + 1):
        cpu.round(churn=True)
        if r in want:
            rows[r] = oracle_rows(cpu, b)
    cpu.close()
    return (b, {(f, t): movement(b, rows[f], rows[t], n, f, t) for f, t in pairs(name)},
            {r: claimed(b, rows[r], n) for r in rows})
