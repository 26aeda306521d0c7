"""The ownership census on the GPU (rp_sim_ownership / rp_sim_ownership_at):
every stats field, every node's claimed measure and the claim counts around
every ring point against the expectation restated from the CPU oracle
(tests/ownership_cases.py) on 1, 2 and 4 in-process shards; against a brute
force through the existing per-view lookup kernel where the oracle has no
model (graceful leave and rejoin, sparse views set directly, 2,048 nodes);
the cache; the argument checks; the ranks of a loop cluster."""
import ctypes
import threading

import numpy as np
import pytest

import oracle
import ownership_cases as oc

pytestmark = pytest.mark.gpu

STATS = ("measure", "claimants", "intervals", "max_claims", "max_claims_hash")
ALL = 1 << 32


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def check(S, b, want, where, queries=None):
    got = S.ownership()
    for k in STATS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    assert got["claimed"].dtype == np.uint64
    bad = np.flatnonzero(got["claimed"] != want["claimed"])
    assert bad.size == 0, (where, "claimed", bad[:8], got["claimed"][bad[:8]], want["claimed"][bad[:8]])
    assert sum(got["measure"]) == ALL, where
    q = oc.queries(b) if queries is None else queries
    at = S.ownership_at(q)
    assert at.dtype == np.uint32
    bad = np.flatnonzero(at != oc.claims_at(b, want["claims"], q))
    assert bad.size == 0, (where, "ownership_at", q[bad[:8]], at[bad[:8]])
    return got


def device_boundaries(S, shift=0):
    return oc.boundaries([S.address(v) for v in range(S.n)], shift)


@pytest.mark.parametrize("shards", [1, 2, 4])
@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_ownership_matches_oracle(rp, name, shards):
    n, kw, rounds, _ = oc.SCENARIOS[name]
    b, want = oc.expected(name)
    S = rp.Sim(n, oc.SIM_SEED, **kw, shards=shards)
    q = oc.queries(b)
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        if r in want:
            check(S, b, want[r], (name, shards, r), q)
    S.close()


def test_ownership_through_leave_and_rejoin(rp):
    """Node 9 leaves at round 5 and rejoins at round 22: from the leave on it
    claims nothing, its keys are orphaned until the others drop it, and the
    census equals the brute force every round until every key has one owner."""
    n, leaver = 64, 9
    S = rp.Sim(n, oc.SIM_SEED, leaves={5: [leaver]}, rejoins={22: [leaver]})
    b = device_boundaries(S)
    orphaned = agreed_after_rejoin = False
    for r in range(1, 61):
        S.round(churn=True)
        got = check(S, b, oc.brute_force(S, b), ("leave", r), b)
        if 6 <= r <= 22:
            assert got["claimed"][leaver] == 0 and got["claimants"] == n, r
        if r == 6:
            assert got["measure"][0] > 0
            orphaned = True
        if r > 23 and got["claimed"][leaver] > 0 and got["measure"][1] == ALL:
            agreed_after_rejoin = True
            break
    assert orphaned and agreed_after_rejoin
    S.close()


def test_ownership_of_sparse_views(rp):
    """Views set directly, 40 nodes: every node's ring holds itself and two
    others (arcs of about 13 points: the wave-cooperative walk, one wrapping
    arc per view); node 39 knows only itself (everything, without a walk).
    rp_sim_set_views refuses a view whose own entry is not alive, so the
    empty ring -- which claims everything by lookup's fallback to whoami --
    comes from node 39's graceful leave in the first round (a node that
    gossips needs a pingable member, so it is the only such node)."""
    n = 40
    st = np.full((n, n), 3, dtype=np.int32)  # faulty: known, not in the ring
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    for v in range(39):
        st[v, [v, (v + 7) % 39, (v + 19) % 39]] = 1
    st[39, 39] = 1
    S = rp.Sim(n, 3, views=(st, inc), leaves={0: [39]})
    assert [S.info(v)["ring_servers"] for v in (0, 38, 39)] == [3, 3, 1]
    b = device_boundaries(S)
    got = check(S, b, oc.brute_force(S, b), "sparse")
    assert got["claimed"][39] == ALL and got["claimants"] == n
    assert got["measure"][0] == got["measure"][1] == 0 and got["max_claims"] > 2
    assert all(0 < int(c) < ALL for c in got["claimed"][:39])
    S.round(churn=False)
    assert S.info(39)["ring_servers"] == 0 and S.info(39)["dead"] == 0
    got = check(S, b, oc.brute_force(S, b), "sparse, after the leave")
    assert got["claimed"][39] == ALL and got["claimants"] == n
    S.close()


def test_ownership_at_2048_nodes(rp):
    """204,800 points: 100 scan tiles of 2,048 intervals, two steps of the
    64-tile partial scan, diverged views (20 fail-stops, declared faulty by
    some views and not by others) against 4.2e8 brute-force lookups."""
    n = 2048
    failed = list(range(50, 2048, 100))
    assert len(failed) == 20
    S = rp.Sim(n, oc.SIM_SEED, failures={3: failed})
    S.run(3, churn=True)
    S.run(30, churn=False)
    b = device_boundaries(S)
    assert len(b) > 64 * 2048
    want = oc.brute_force(S, b)
    assert want["claimants"] == n - 20 and want["measure"][0] > 0 and want["measure"][1] > 0
    rng = np.random.default_rng(5)
    q = np.concatenate([b[:: 7], b[:: 11] + np.uint32(1), rng.integers(0, ALL, 4096, dtype=np.uint64).astype(np.uint32),
                        np.array([0, ALL - 1], dtype=np.uint32)])
    check(S, b, want, "n2048", q)
    S.close()


def test_ownership_cache_tracks_changes(rp):
    n, kw, _, _ = oc.SCENARIOS["failstop"]
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    cpu = oracle.Sim(n, oc.SIM_SEED, **kw)
    b = oc.boundaries([cpu.address(v) for v in range(n)])
    for _ in range(30):
        S.round(churn=True)
        cpu.round(churn=True)
    first = check(S, b, oc.expect(cpu, b), "round 30")
    again = check(S, b, oc.expect(cpu, b), "round 30 again")  # (no call between: the cached counts)
    assert again["measure"] == first["measure"] and np.array_equal(again["claimed"], first["claimed"])
    S.round(churn=True)
    cpu.round(churn=True)
    second = check(S, b, oc.expect(cpu, b), "round 31")
    assert second["measure"] != first["measure"]
    # node 0 learns that member m is faulty: its ring, and only its, changes.  m owns the point before
    # one of node 0's own, so node 0 now claims that interval too (m, alive, still does)
    owners = [cpu.ring_lookup(0, h) for h in b.tolist()]
    m = next(owners[i - 1] for i in range(1, len(b)) if owners[i] == 0 and owners[i - 1] not in [0] + kw["failures"][2])
    _, inc = S.view(0)
    row = [[m, 3, int(inc[m]), 0, int(inc[0])]]
    assert S.update(0, row) == 1 and cpu.update(0, row) == 1
    third = check(S, b, oc.expect(cpu, b), "update")
    assert np.flatnonzero(third["claimed"] != second["claimed"]).tolist() == [0]
    assert third["measure"] != second["measure"] and third["measure"][2] > second["measure"][2]
    S.close()
    cpu.close()


def test_ownership_arguments(rp):
    from ringpop_amd._lib import OwnershipStats, lib, ptr
    n = 32
    S = rp.Sim(n, oc.SIM_SEED)
    S.run(2, churn=True)
    st = OwnershipStats()
    short = np.full(n - 1, 77, dtype=np.uint64)
    assert lib().rp_sim_ownership(S._h, ctypes.byref(st), ptr(short), n - 1) == -1  # RP_ERR_INVALID
    assert (short == 77).all() and list(st.measure) == [0] * 8
    assert lib().rp_sim_ownership(S._h, ctypes.byref(st), None, 0) == 0  # claimed = NULL
    full = S.ownership()
    assert st.as_dict() == {k: full[k] for k in STATS}
    assert list(st.reserved) == [0] * 4 and sum(st.measure) == ALL and st.claimants == n
    assert S.ownership_at(np.zeros(0, dtype=np.uint32)).size == 0
    S.close()


def test_ownership_on_loop_ranks(rp):
    """A rank of a loop cluster holds its own nodes' views only: unsupported."""
    from ringpop_amd.sim import Loop
    G, n, rounds = 2, 64, 3
    loop = Loop(G)
    sims = [rp.Sim(n, oc.SIM_SEED, shards=G, rank=r, loop=loop) for r in range(G)]
    errors = []

    def rank_main(r):
        try:
            for _ in range(rounds):
                sims[r].round(churn=True)
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append((r, repr(e)))

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for S in sims:
        for call in (S.ownership, lambda: S.ownership_at(np.arange(4, dtype=np.uint32))):
            with pytest.raises(rp.RingpopError) as ei:
                call()
            assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
    for S in sims:
        S.close()
    loop.close()
