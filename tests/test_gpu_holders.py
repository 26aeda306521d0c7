"""The holders query on the GPU (rp_sim_holders_at) against the
plain restatement used for the replica-set census: for every claimant v,
L = ring_lookup(v, b) over all boundaries b (the per-view kernel, pinned to the
oracle) and pref = preference(L, 8); v holds interval i at R iff L[0] < 0 or
v is in pref[i, :R].  A key falls in interval searchsorted(b, q, "left")."""
import threading

import numpy as np
import pytest

import ownership_cases as oc
import replication_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def reference(S, b):
    """hold(R) -> bool [intervals, n] of the simulation as it stands; L is computed once per view."""
    looks = {v: S.ring_lookup(v, b) for v in range(S.n) if S.info(v)["dead"] == 0}
    prefs = {v: None if L[0] < 0 else rc.preference(L, 8)[0] for v, L in looks.items()}  # (None: an empty ring)

    def hold(R):
        H = np.zeros((len(b), S.n), dtype=bool)
        for v, pref in prefs.items():
            H[:, v] = True if pref is None else (pref[:, :R] == v).any(axis=1)
        return H
    return hold


def check(S, b, hold, R, q, where):
    H = hold(R)[np.searchsorted(b, q, side="left") % len(b)]
    want = np.sort(np.where(H, np.arange(S.n), S.n), axis=1)
    want[want == S.n] = -1
    got, counts = S.holders_at(R, q, cap=S.n)
    assert got.dtype == np.int32 and counts.dtype == np.uint32 and got.shape == (len(q), S.n), where
    bad = np.flatnonzero((got != want).any(axis=1) | (counts != H.sum(axis=1)))
    assert bad.size == 0, (where, q[bad[:4]], got[bad[:4]], want[bad[:4]], counts[bad[:4]])
    assert np.array_equal(counts, S.replication_at(R, q)), where
    assert R != 1 or np.array_equal(counts, S.ownership_at(q)), where
    return got, counts


@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_holders_in_scenarios(rp, name, shards):
    """48, 32 and 40 nodes: a ragged tile; 64: a whole one; on 4 shards a tile's lanes span shards."""
    n, kw, rounds, _ = oc.SCENARIOS[name]
    S = rp.Sim(n, oc.SIM_SEED, **kw, shards=shards)
    b = oc.boundaries([S.address(v) for v in range(n)], kw.get("replica_hash_shift", 0))
    q = oc.queries(b)
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        if r in oc.checkpoints(name):
            hold = reference(S, b)
            for R in rc.RS:
                check(S, b, hold, R, q, (name, shards, r, R))
    S.close()


@pytest.mark.parametrize("shards", [1, 4])
def test_holders_over_several_tiles(rp, shards):
    """200 nodes: tiles of 64, 64, 64 and 8 views, diverged over ten fail-stops.
    Views that differ only in the dead nodes they still list never give a key
    more than R holders (the view that has dropped them all has exactly R live
    ones, every other a subset): fail-stops alone left no key with more than 3
    here (2,862 intervals below, 17,138 at 3).  A node that joins two rounds
    before the end, known to few views yet, supplies those."""
    n = 200
    S = rp.Sim(n, oc.SIM_SEED, failures={3: list(range(7, 200, 19))[:10]}, joins=[(25, 150, [0, 1])], shards=shards)
    S.run(3, churn=True)
    S.run(24, churn=False)
    b = oc.boundaries([S.address(v) for v in range(n)])
    hold = reference(S, b)
    per_key = hold(3).sum(axis=1)
    print("intervals with fewer than, exactly and more than 3 holders:",
          (per_key < 3).sum(), (per_key == 3).sum(), (per_key > 3).sum())
    assert (per_key < 3).any() and (per_key == 3).any() and (per_key > 3).any()
    check(S, b, hold, 3, oc.queries(b), ("n200", shards))
    S.close()


def test_holders_in_sparse_views(rp):
    """test_gpu_replication's sparse cluster: 40 nodes, rings of three servers,
    node 39 alone and, a round later, with an empty ring.  R = 2 takes the
    cooperative walk; from R = 3 on every member of a ring holds everything."""
    n = 40
    st = np.full((n, n), 3, dtype=np.int32)
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    for v in range(39):
        st[v, [v, (v + 7) % 39, (v + 19) % 39]] = 1
    st[39, 39] = 1
    S = rp.Sim(n, 3, views=(st, inc), leaves={0: [39]})
    b = oc.boundaries([S.address(v) for v in range(n)])
    for when in ("alone", "empty"):
        hold = reference(S, b)
        for R in (2, 3, 4):
            got, counts = check(S, b, hold, R, oc.queries(b), (when, R))
            assert (got == 39).any(axis=1).all(), (when, R)
            assert R == 2 or (counts == n).all(), (when, R)
        S.round(churn=False)
    assert S.info(39)["ring_servers"] == 0
    S.close()


@pytest.fixture(scope="module")
def failstop(rp):
    n, kw, _, _ = oc.SCENARIOS["failstop"]
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(30, churn=True)
    b = oc.boundaries([S.address(v) for v in range(n)])
    yield S, b, reference(S, b)
    S.close()


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_holders_cap(failstop, cap):
    from ringpop_amd._lib import lib, ptr
    S, b, hold = failstop
    q = oc.queries(b)
    full, counts = check(S, b, hold, 3, q, "cap = n")
    got, c = S.holders_at(3, q, cap=cap)
    assert got.shape == (len(q), cap) and np.array_equal(got, full[:, :cap]) and np.array_equal(c, counts)
    c = np.zeros(len(q), dtype=np.uint32)
    assert lib().rp_sim_holders_at(S._h, 3, ptr(q), len(q), 5, None, ptr(c)) == 0 and np.array_equal(c, counts)


def test_holders_of_more_than_one_chunk(failstop):
    S, b, hold = failstop
    q = np.concatenate([np.random.default_rng(5).integers(0, 1 << 32, size=70000, dtype=np.uint64).astype(np.uint32),
                        oc.queries(b)])
    check(S, b, hold, 2, q, "70,000 keys")


def test_holders_arguments_and_isolation(rp, failstop):
    from ringpop_amd._lib import lib, ptr
    S, b, _ = failstop
    q, c, out = oc.queries(b), np.full(4, 77, dtype=np.uint32), np.full((4, 4), 77, dtype=np.int32)
    call = lib().rp_sim_holders_at
    for bad in (0, 9):
        assert call(S._h, bad, ptr(q), 4, 4, ptr(out), ptr(c)) == -1  # RP_ERR_INVALID
    assert call(None, 3, ptr(q), 4, 4, ptr(out), ptr(c)) == call(S._h, 3, None, 4, 4, ptr(out), ptr(c)) == -1
    assert call(S._h, 3, ptr(q), 4, 4, ptr(out), None) == -1 and (c == 77).all() and (out == 77).all()
    assert call(S._h, 3, None, 0, 4, None, None) == 0
    # the censuses' caches stay: no span is timed for the second replication(3)
    S.enable_timing(True, stages=["other"])
    before = S.replication(3), S.ownership()
    spans = S.kernel_times()["other"][1]
    S.holders_at(3, q)
    assert S.kernel_times()["other"][1] == spans + 2  # (one chunk: k_hold_mask and k_hold_list)
    after = S.replication(3), S.ownership()
    assert S.kernel_times()["other"][1] == spans + 2
    for x, y in zip(before, after):
        assert all(np.array_equal(x[k], y[k]) for k in x)
    S.enable_timing(False)
    # a rank of a loop cluster holds its own nodes' views only
    from ringpop_amd.sim import Loop
    loop = Loop(2)
    sims = [rp.Sim(64, oc.SIM_SEED, shards=2, rank=r, loop=loop) for r in range(2)]
    th = [threading.Thread(target=X.run, args=(3,), kwargs={"churn": True}) for X in sims]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for X in sims:
        with pytest.raises(rp.RingpopError) as ei:
            X.holders_at(3, q[:4])
        assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
        X.close()
    loop.close()
