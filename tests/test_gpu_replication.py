"""The replica-set census and the per-view lookupN on the GPU
(rp_sim_replication / rp_sim_replication_at / rp_sim_ring_lookup_n) against the
plain reference of tests/replication_cases.py: restated from the CPU oracle on
1 and 4 in-process shards, and from the existing per-view lookup kernel where
the oracle has no model (sparse views, a graceful leave, 512 nodes)."""
import ctypes
import threading

import numpy as np
import pytest

import ownership_cases as oc
import replication_cases as rc

pytestmark = pytest.mark.gpu

STATS = ("measure", "replicas", "claimants", "intervals", "under", "exact", "over", "max_claims", "max_claims_hash",
         "min_claims", "min_claims_hash")
ALL = 1 << 32


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def check(S, b, want, where, q):
    got = S.replication(want["replicas"])
    for k in STATS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    bad = np.flatnonzero(got["held"] != want["held"])
    assert bad.size == 0, (where, "held", bad[:8], got["held"][bad[:8]], want["held"][bad[:8]])
    assert sum(got["measure"]) == got["under"] + got["exact"] + got["over"] == ALL, where
    at = S.replication_at(want["replicas"], q)
    bad = np.flatnonzero(at != oc.claims_at(b, want["claims"], q))
    assert at.dtype == np.uint32 and bad.size == 0, (where, "replication_at", q[bad[:8]], at[bad[:8]])
    if want["replicas"] == 1:  # by construction: the ownership census
        own = S.ownership()
        assert got["measure"][:7] + [sum(got["measure"][7:])] == own["measure"], where
        assert all(got[k] == own[k] for k in ("claimants", "intervals", "max_claims", "max_claims_hash")), where
        assert np.array_equal(got["held"], own["claimed"]) and np.array_equal(at, S.ownership_at(q)), where
    return got


def check_lookup_n(S, b, where):
    """Lists, order, counts and padding of every node's lookupN around every boundary."""
    q = oc.queries(b)
    at = np.searchsorted(b, q, side="left") % len(b)
    for v in range(S.n):
        pref, cnt = rc.preference(S.ring_lookup(v, b), 16)
        for n in (0, 1, 2, 3, 4, 16):
            owners, counts = S.ring_lookup_n(v, q, n)
            assert owners.shape == (len(q), n) and owners.dtype == counts.dtype == np.int32
            assert np.array_equal(owners, pref[at, :n]) and np.array_equal(counts, np.minimum(cnt[at], n)), (where, v, n)


def sparse_sim(rp):
    """test_ownership_of_sparse_views' cluster: 40 nodes, rings of three servers, node 39 alone."""
    n = 40
    st = np.full((n, n), 3, dtype=np.int32)
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    for v in range(39):
        st[v, [v, (v + 7) % 39, (v + 19) % 39]] = 1
    st[39, 39] = 1
    return rp.Sim(n, 3, views=(st, inc), leaves={0: [39]})


def test_ring_lookup_n_with_collisions(rp):
    n, kw, _, _ = oc.SCENARIOS["shift"]
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(10, churn=True)
    check_lookup_n(S, oc.boundaries([S.address(v) for v in range(n)], kw["replica_hash_shift"]), "shift")
    S.close()


def test_sparse_views(rp):
    """R = 2 takes the cooperative walk; R = 3 is the ring size: every member
    of a ring holds everything; R = 4 exceeds it.  Node 39 alone, then empty."""
    S = sparse_sim(rp)
    b = oc.boundaries([S.address(v) for v in range(S.n)])
    for when in ("alone", "empty"):
        check_lookup_n(S, b, when)
        want = rc.expect(S, b, (2, 3, 4), device=True)
        for R in (2, 3, 4):
            got = check(S, b, want[R], (when, R), oc.queries(b))
            assert got["held"][39] == ALL and got["claimants"] == S.n
            assert R == 2 or (got["held"] == ALL).all()
        S.round(churn=False)
    assert S.info(39)["ring_servers"] == 0
    S.close()


@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_replication_matches_oracle(rp, name, shards):
    n, kw, rounds, _ = oc.SCENARIOS[name]
    b, want = rc.expected(name)
    S = rp.Sim(n, oc.SIM_SEED, **kw, shards=shards)
    q = oc.queries(b)
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        for R in rc.RS if r in want else ():
            check(S, b, want[r][R], (name, shards, r, R), q)
    S.close()


def test_replication_at_512_nodes(rp):
    """51,200 points: 25 scan tiles with non-zero tile bases, views diverged over 10 fail-stops."""
    n = 512
    S = rp.Sim(n, oc.SIM_SEED, failures={3: list(range(20, 512, 50))[:10]})
    S.run(3, churn=True)
    S.run(24, churn=False)
    b = oc.boundaries([S.address(v) for v in range(n)])
    want = rc.expect(S, b, (3,), device=True)[3]
    assert len(b) > 24 * 2048 and want["claimants"] == n - 10 and want["under"] > 0 and want["exact"] > 0
    check(S, b, want, "n512", oc.queries(b))
    S.close()


def test_replication_through_leave_and_rejoin(rp):
    n, leaver = 64, 9
    S = rp.Sim(n, oc.SIM_SEED, leaves={5: [leaver]}, rejoins={22: [leaver]})
    b = oc.boundaries([S.address(v) for v in range(n)])
    S.run(5, churn=True)
    under = agreed = False
    for r in range(6, 61):
        S.round(churn=True)
        got = check(S, b, rc.expect(S, b, (2,), device=True)[2], ("leave", r), b)
        under |= got["under"] > 0
        if r <= 22:
            assert got["held"][leaver] == 0 and got["claimants"] == n, r
        elif got["exact"] == ALL and got["held"][leaver] > 0:
            agreed = True
            break
    assert under and agreed
    S.close()


def test_replication_cache_and_arguments(rp):
    from ringpop_amd._lib import ReplicationStats, lib, ptr
    n, kw, _, _ = oc.SCENARIOS["failstop"]
    b, want = rc.expected("failstop")
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(30, churn=True)
    q = oc.queries(b)
    three = check(S, b, want[30][3], "round 30", q)
    again = S.replication(3)  # (cached: the walk's work is the first run's, and the result)
    assert all(again[k] == three[k] for k in STATS + ("walk_steps", "arcs")) and three["arcs"] > 0
    check(S, b, want[30][2], "another R", q)
    check(S, b, want[30][3], "and back", q)
    S.round(churn=True)
    check(S, b, want[31][3], "round 31", q)
    assert np.array_equal(S.replication_at(8, q), oc.claims_at(b, want[31][8]["claims"], q))  # (computes R = 8 itself)
    _, inc = S.view(0)
    m = next(v for v in range(1, n) if v not in kw["failures"][2])
    assert S.update(0, [[m, 3, int(inc[m]), 0, int(inc[0])]]) == 1  # node 0's ring loses m: only its view changes
    now = check(S, b, rc.expect(S, b, (3,), device=True)[3], "update", q)
    assert np.flatnonzero(now["held"] != want[31][3]["held"]).tolist() == [0]
    st, short, keys, out = ReplicationStats(), np.full(n - 1, 77, dtype=np.uint64), q[:4].copy(), np.zeros(64, np.int32)
    call = lib().rp_sim_replication
    assert call(S._h, 3, ctypes.byref(st), ptr(short), n - 1) == -1 and (short == 77).all() and sum(st.measure) == 0
    assert call(S._h, 0, ctypes.byref(st), None, 0) == call(S._h, 9, ctypes.byref(st), None, 0) == -1  # RP_ERR_INVALID
    assert call(S._h, 3, ctypes.byref(st), None, 0) == 0 and st.as_dict() == {k: now[k] for k in st.as_dict()}
    assert list(st.reserved) == [0] * 4
    for bad_n in (-1, 17):
        assert lib().rp_sim_ring_lookup_n(S._h, 0, ptr(keys), 4, bad_n, ptr(out), ptr(out)) == -1
    assert lib().rp_sim_ring_lookup_n(S._h, n, ptr(keys), 4, 3, ptr(out), ptr(out)) == -1
    S.close()


def test_replication_on_loop_ranks(rp):
    """A rank of a loop cluster holds its own nodes' views only: unsupported."""
    from ringpop_amd.sim import Loop
    G, n = 2, 64
    loop = Loop(G)
    sims = [rp.Sim(n, oc.SIM_SEED, shards=G, rank=r, loop=loop) for r in range(G)]
    th = [threading.Thread(target=S.run, args=(3,), kwargs={"churn": True}) for S in sims]
    for t in th:
        t.start()
    for t in th:
        t.join()
    keys = np.arange(4, dtype=np.uint32)
    for S in sims:
        for call in (lambda: S.replication(3), lambda: S.replication_at(3, keys), lambda: S.ring_lookup_n(0, keys, 3)):
            with pytest.raises(rp.RingpopError) as ei:
                call()
            assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
    for S in sims:
        S.close()
    loop.close()
