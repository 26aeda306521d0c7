"""The replica-set census (rp_sim_replication): the plain
reference over the ownership census' scenarios (tests/ownership_cases.py).

For a claimant v, L[i] = ring_lookup(v, b[i]) over all boundaries b.  Read
cyclically from index i, the owners in order of first appearance are
lookupN_v for interval i: absent points only repeat the next present owner.
v holds interval i at R iff v is among the first R of them, or L[i] < 0 (an
empty ring: RingPop.lookupN returns [whoami]).  Everything is integer-exact."""
import functools

import numpy as np

import oracle
import ownership_cases as oc

RS = (1, 2, 3, 8)


def preference(L, n):
    """(lists [len(L), n], counts): per interval the first n distinct owners,
    unused slots -1.  A step loop over the runs of equal owners (a walk sees
    a run as one owner), every start at once, until each list is full or holds
    every owner of the ring."""
    L = np.asarray(L, dtype=np.int64)
    npts = len(L)
    if n == 0 or L[0] < 0:
        return np.full((npts, n), -1, dtype=np.int32), np.zeros(npts, dtype=np.int32)
    start = np.flatnonzero(L != np.roll(L, 1))
    if start.size == 0:
        start = np.zeros(1, dtype=np.int64)
    r = L[start]
    m, full = len(r), min(n, len(np.unique(r)))
    lists, cnt, at = np.full((m, n), -1, dtype=np.int32), np.zeros(m, dtype=np.int64), np.arange(m)
    for s in range(m):
        cur = r[(at + s) % m]
        new = (cnt < full) & ~(lists == cur[:, None]).any(axis=1)
        lists[new, cnt[new]] = cur[new]
        cnt[new] += 1
        if (cnt >= full).all():
            break
    run_of = (np.searchsorted(start, np.arange(npts), side="right") - 1) % m  # (before the first start: the last run)
    return lists[run_of], cnt[run_of].astype(np.int32)


def census(b, n, rows, R):
    """The issue's definition from rows = {claimant v: preference(L_v, >= R)[0], or None for an empty ring}."""
    ln = oc.lengths(b)
    claims, held = np.zeros(len(b), dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    for v, pref in rows.items():
        h = np.ones(len(b), dtype=bool) if pref is None else (pref[:, :R] == v).any(axis=1)
        claims += h
        held[v] = int(ln[h].sum())
    cls, hi, lo = np.minimum(claims, 15), int(np.argmax(claims)), int(np.argmin(claims))  # (the first index of each)
    return {"measure": [int(ln[cls == k].sum()) for k in range(16)], "replicas": R, "claimants": len(rows),
            "intervals": len(b), "under": int(ln[claims < R].sum()), "exact": int(ln[claims == R].sum()),
            "over": int(ln[claims > R].sum()), "max_claims": int(claims[hi]), "max_claims_hash": int(b[hi]),
            "min_claims": int(claims[lo]), "min_claims_hash": int(b[lo]), "held": held, "claims": claims}


def expect(S, b, rs=RS, device=False):
    """{R: census} of a simulation as it stands: the oracle's, or (device) a
    device simulation's through its existing per-view lookup kernel, the
    brute force where the oracle has no model.  L is computed once per view."""
    look = S.ring_lookup
    rows = {}
    for v in range(S.n):
        if S.info(v)["dead"] == 0:
            L = look(v, b) if device else np.array([look(v, h) for h in b.tolist()])
            rows[v] = None if L[0] < 0 else preference(L, max(rs))[0]
    return {R: census(b, S.n, rows, R) for R in rs}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The scenario on the oracle (seed 7, churn on): (boundaries, {clock: {R:
    census}}) at oc.checkpoints(name).  Computed once; callers must not modify it."""
    n, kw, rounds, _ = oc.SCENARIOS[name]
    cpu = oracle.Sim(n, oc.SIM_SEED, **kw)
    b = oc.boundaries([cpu.address(v) for v in range(n)], kw.get("replica_hash_shift", 0))
    want, out = set(oc.checkpoints(name)), {}
    for r in range(rounds + 1):
        if r:
            cpu.round(churn=True)
        if r in want:
            out[r] = expect(cpu, b)
    cpu.close()
    return b, out
