"""Replicated requests on the GPU (rp_sim_route_n / rp_sim_route_n_uniform;
DESIGN.md §18) against a plain restatement of the definition built only from
entry points that are pinned to the oracle elsewhere: Sim.ring_lookup_n per
distinct entry (the entry's list), Sim.holders_at with cap = n (who believes
it holds a key), Sim.info(v)["dead"], Sim.ring_checksums and route_cases.cut."""
import ctypes
import threading

import numpy as np
import pytest

import ownership_cases as oc
import replication_cases as rpc
import route_cases as rc

pytestmark = pytest.mark.gpu

EMPTY = 255
# clocks inside and after each scenario's divergence window (failstop: rings differ in rounds 28-34; partition: from
# round 27 on, the window closes at 40; shift: rounds 27-28)
CHECKPOINTS = {"failstop": (29, 31, 45), "partition": (30, 40, 46), "shift": (27, 28, 40)}


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def restate(S, R, e, h, partition=None):
    """(dests, outcomes, holds, acks, stats) of the definition, for the simulation as it stands."""
    n, m, clock = S.n, len(e), S.rounds()
    dead = np.array([S.info(v)["dead"] != 0 for v in range(n)])
    rcs = S.ring_checksums()
    live = ~dead[e]
    L, c = np.full((m, R), -1, dtype=np.int32), np.zeros(m, dtype=np.int64)
    for v in np.unique(e[live]).tolist():
        at = np.flatnonzero(e == v)
        L[at], c[at] = S.ring_lookup_n(v, h[at], R)
    empty = live & (c == 0)  # an empty ring, or servers that own no point: [whoami]
    L[empty, 0], c[empty] = e[empty], 1
    uk, inv = np.unique(h, return_inverse=True)
    rows, _ = S.holders_at(R, uk, cap=n)
    believes = np.zeros((len(uk), n + 1), dtype=bool)  # (the rows' -1 lands in column n)
    believes[np.arange(len(uk))[:, None], rows] = True
    slot = live[:, None] & (np.arange(R) < c[:, None])
    d, E = np.where(slot, L, 0), e[:, None].astype(np.int64)
    local = slot & (d == E)
    unr = slot & ~local & (dead[d] | rc.cut(partition, clock, E, d))
    sent = slot & ~local & ~unr
    out = np.full((m, R), EMPTY, dtype=np.uint8)
    out[~live, 0] = rc.ENTRY_DEAD
    out[local], out[unr] = rc.LOCAL, rc.UNREACHABLE
    out[sent] = np.where(rcs[E] != rcs[d], rc.CHECKSUMS_DIFFER, rc.DELIVERED)[sent]
    holds = local | (sent & believes[inv.reshape(-1, 1), d])
    acks, strict = ((out <= 2) & holds).sum(axis=1), ((out <= 1) & holds).sum(axis=1)
    stats = {"requests": m, "entry_dead": int((~live).sum()), "slots": int(slot.sum()),
             "misplaced": int((sent & ~holds).sum()), "short_lists": int((live & (c < R)).sum()),
             "acks_hist": np.bincount(acks[live], minlength=9).tolist(),
             "strict_hist": np.bincount(strict[live], minlength=9).tolist()}
    stats.update({k: int((out == i).sum()) for i, k in enumerate(rc.OUTCOMES[:4])})
    return np.where(slot, L, -1).astype(np.int32), out, holds.astype(np.uint8), acks.astype(np.uint8), stats


def compare(got, want, where):
    for k, what in enumerate(("dests", "outcomes", "holds", "acks")):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, what)
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))
        assert bad.size == 0, (where, what, bad[:4], got[k][bad[:4]], want[k][bad[:4]])
    print(where, want[4])
    assert got[4] == want[4], (where, got[4], want[4])


def requests_at_points(S, shift=0):
    """route_cases' 1,500 requests, then keys on, just below and just above every point and at both ends of the
    hash space from three fixed entries; the length is no multiple of 8."""
    n = S.n
    q = oc.queries(oc.boundaries([S.address(v) for v in range(n)], shift))
    e, h = rc.requests(rc.REQ_SEED, rc.REQUESTS, n)
    e = np.concatenate([e] + [np.full(len(q), v, dtype=np.uint32) for v in (1, n // 2, n - 2)])
    h = np.concatenate([h, q, q, q])
    m = len(e) // 8 * 8 - 3
    return e[:m], h[:m]


@pytest.mark.parametrize("R", rpc.RS)
@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("name", list(rc.SCENARIOS))
def test_route_n_in_scenarios(rp, name, shards, R):
    n, kw, _, must = rc.SCENARIOS[name]
    S = rp.Sim(n, rc.SIM_SEED, **kw, shards=shards)
    e, h = requests_at_points(S, kw.get("replica_hash_shift", 0))
    total, fewer, full = dict.fromkeys(must + ("misplaced",), 0), False, False
    for r in CHECKPOINTS[name]:
        S.run(r - S.rounds(), churn=True)
        want = restate(S, R, e, h, kw.get("partition"))
        got = S.route_n(R, e, h)
        compare(got, want, (name, shards, R, r))
        for k in total:
            total[k] += want[4]["misplaced" if k == "misrouted" else k]
        fewer, full = fewer or bool((want[3] < R).any()), full or bool((want[3] == R).any())
        if R == 1:
            dests, outcomes, agrees, _ = S.route(e, h)
            assert np.array_equal(got[0][:, 0], dests) and np.array_equal(got[1][:, 0], outcomes)
            assert np.array_equal(got[2][:, 0], np.where(outcomes == rc.LOCAL, 1, agrees))
    S.close()
    # the expectation itself covers what the scenario is for
    assert all(total.values()) and fewer and full, (total, fewer, full)


@pytest.mark.parametrize("R", [2, 3, 4])
def test_route_n_in_sparse_views(rp, R):
    """test_gpu_holders' sparse cluster: 40 nodes, rings of three servers, node 39 alone and, a round later,
    with an empty ring.  Three servers' points are one in thirteen: lists and walks leave the window."""
    n = 40
    st = np.full((n, n), 3, dtype=np.int32)
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    for v in range(39):
        st[v, [v, (v + 7) % 39, (v + 19) % 39]] = 1
    st[39, 39] = 1
    S = rp.Sim(n, 3, views=(st, inc), leaves={0: [39]})
    h = oc.queries(oc.boundaries([S.address(v) for v in range(n)]))[:-3]
    e = (np.arange(len(h)) % n).astype(np.uint32)
    for when in ("alone", "empty"):
        want = restate(S, R, e, h)
        got = S.route_n(R, e, h)
        compare(got, want, (when, R))
        own = e == 39  # (a list of one: short at every R here)
        assert (R < 4 or want[4]["short_lists"] > own.sum()) and want[4]["slots"] > want[4]["requests"]
        assert (got[0][own, 0] == 39).all() and (got[0][own, 1:] == -1).all() and (got[3][own] == 1).all()
        assert (got[1][own, 0] == rc.LOCAL).all() and (got[1][own, 1:] == EMPTY).all()
        S.round(churn=False)
    assert S.info(39)["ring_servers"] == 0
    S.close()


@pytest.fixture(scope="module")
def failstop(rp):
    n, kw, _, _ = rc.SCENARIOS["failstop"]
    S = rp.Sim(n, rc.SIM_SEED, **kw)
    S.run(29, churn=True)
    yield S
    S.close()


@pytest.mark.parametrize("R", [1, 3])
def test_route_n_uniform_equals_host_generated_requests(failstop, R):
    S, count = failstop, 70_003
    want = S.route_n(R, *rc.requests(rc.REQ_SEED, count, S.n))[4]
    assert want["requests"] == count and want["misplaced"] > 0 and want["entry_dead"] > 0
    assert sum(want["acks_hist"]) == sum(want["strict_hist"]) == count - want["entry_dead"]
    assert S.route_n_uniform(R, rc.REQ_SEED, count) == want
    if R == 1:
        one = S.route_uniform(rc.REQ_SEED, count)
        assert all(want[k] == one[k] for k in rc.OUTCOMES) and want["misplaced"] == one["misrouted"]


def test_route_n_arguments_and_isolation(rp, failstop):
    from ringpop_amd._lib import RouteNStats, lib, ptr
    S = failstop
    e, h = rc.requests(rc.REQ_SEED, 21, S.n)
    d, o, hl, a = (np.full(21 * 3, 77, dtype=t) for t in (np.int32, np.uint8, np.uint8, np.uint8))
    st, call = RouteNStats(), lib().rp_sim_route_n
    outs = (ptr(d), ptr(o), ptr(hl), ptr(a), ctypes.byref(st))
    far = e.copy()
    far[20] = S.n
    for bad in ((S._h, 0, ptr(e), ptr(h), 21), (S._h, 9, ptr(e), ptr(h), 21), (None, 3, ptr(e), ptr(h), 21),
                (S._h, 3, None, ptr(h), 21), (S._h, 3, ptr(e), None, 21), (S._h, 3, ptr(far), ptr(h), 21)):
        assert call(*bad, *outs) == -1  # RP_ERR_INVALID
    assert lib().rp_sim_route_n_uniform(S._h, 9, 1, 21, ctypes.byref(st)) == -1
    assert all((x == 77).all() for x in (d, o, hl, a))
    assert call(S._h, 3, None, None, 0, *outs) == 0 and all((x == 77).all() for x in (d, o, hl, a))
    want = S.route_n(3, e, h)
    assert call(S._h, 3, ptr(e), ptr(h), 21, None, None, None, None, ctypes.byref(st)) == 0 and st.as_dict() == want[4]
    assert call(S._h, 3, ptr(e), ptr(h), 21, *outs[:4], None) == 0 and np.array_equal(d.reshape(21, 3), want[0])
    # the censuses' caches stay: no span is timed for the second replication(3)
    S.enable_timing(True, stages=["other"])
    before = S.replication(3), S.ownership()
    spans = S.kernel_times()["other"][1]
    S.route_n(3, e, h)
    assert S.kernel_times()["other"][1] == spans + 1  # (one launch)
    after = S.replication(3), S.ownership()
    assert S.kernel_times()["other"][1] == spans + 1
    for x, y in zip(before, after):
        assert all(np.array_equal(x[k], y[k]) for k in x)
    S.enable_timing(False)
    # a rank of a loop cluster holds its own nodes' views only
    from ringpop_amd.sim import Loop
    loop = Loop(2)
    sims = [rp.Sim(64, rc.SIM_SEED, shards=2, rank=r, loop=loop) for r in range(2)]
    th = [threading.Thread(target=X.run, args=(3,), kwargs={"churn": True}) for X in sims]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for X in sims:
        for use in (lambda: X.route_n(3, e[:4] % 64, h[:4]), lambda: X.route_n_uniform(3, 1, 16)):
            with pytest.raises(rp.RingpopError) as ei:
                use()
            assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
        X.close()
    loop.close()
