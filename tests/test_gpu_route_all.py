"""Multi-key requests on the GPU (rp_sim_route_all / rp_sim_route_all_uniform;
DESIGN.md §21) against the plain restatement of the definition from the CPU
oracle (tests/route_all_cases.py): every output array and every stats field."""
import ctypes
import threading

import numpy as np
import pytest

import route_all_cases as ra
import route_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def compare(got, want, where):
    for k in ra.ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k)
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (where, k, bad[:4], got[k][bad[:4]], want[k][bad[:4]])
    assert got["stats"] == want["stats"], (where, got["stats"], want["stats"])


@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("name", list(rc.SCENARIOS))
def test_route_all_in_scenarios(rp, name, shards):
    n, kw, _, _ = rc.SCENARIOS[name]
    exp, batches = ra.expected(name)
    S = rp.Sim(n, rc.SIM_SEED, **kw, shards=shards)
    for clock in ra.CHECKPOINTS[name]:
        S.run(clock - S.rounds(), churn=True)
        for b, (e, off, h) in batches.items():
            got = S.route_all(e, off, h)
            compare(got, exp[clock][b], (name, shards, clock, b))
            if b == 1:  # a request of one key is rp_sim_route's request
                dests, outcomes, agrees, _ = S.route(e, h)
                live = outcomes != rc.ENTRY_DEAD
                assert np.array_equal(got["group_dest"][live], dests[live]) and (got["group_dest"][~live] == -1).all()
                assert np.array_equal(np.where(live, got["group_outcome"], rc.ENTRY_DEAD), outcomes)
                assert np.array_equal(got["key_agrees"], agrees)
    if name == "shift" and shards == 1:
        # more requests than one pass of the grid holds (65,536 at 8 lanes a request): the K = 8 batch, 330 times over
        e, off, h = batches[8]
        want, t = exp[ra.CHECKPOINTS[name][-1]][8], 330
        got = S.route_all(np.tile(e, t), np.arange(ra.COUNT * t + 1, dtype=np.uint64) * np.uint64(8), np.tile(h, t))
        for k in ra.ARRAYS:
            assert np.array_equal(got[k], np.tile(want[k], t)), k
        assert got["stats"]["keys"] == t * want["stats"]["keys"] and got["stats"]["max_fanout"] == want["stats"]["max_fanout"]
        assert got["stats"]["fanout_hist"] == [t * x for x in want["stats"]["fanout_hist"]]
    S.close()


@pytest.fixture(scope="module")
def failstop(rp):
    n, kw, _, _ = rc.SCENARIOS["failstop"]
    S = rp.Sim(n, rc.SIM_SEED, **kw)
    S.run(29, churn=True)
    yield S
    S.close()


@pytest.mark.parametrize("K", [3, 64, 100])
def test_route_all_uniform_equals_host_generated_requests(failstop, K):
    S, count = failstop, 2_051
    want = S.route_all(*ra.uniform_batch(S.n, count, K))["stats"]
    assert want["requests"] == count and want["keys"] == (count - want["entry_dead"]) * K and want["misrouted_keys"] > 0
    assert S.route_all_uniform(rc.REQ_SEED, count, K) == want


def test_route_all_arguments(rp, failstop):
    from ringpop_amd._lib import RouteAllStats, lib, ptr
    S = failstop
    e, off, h = ra.uniform_batch(S.n, 21, 5)
    dt = (np.uint16, np.uint8, np.int32, np.uint8, np.uint16, np.uint16, np.uint16, np.uint8)
    bufs = [np.full(105 if k < 6 else 21, 77, dtype=t) for k, t in enumerate(dt)]
    st, call = RouteAllStats(), lib().rp_sim_route_all
    outs = tuple(ptr(b) for b in bufs) + (ctypes.byref(st),)
    far, first, down, big = e.copy(), off.copy(), off.copy(), off.copy()
    far[20], first[0], down[3], big[1:] = S.n, 1, 2, off[1:] + np.uint64(252)  # (a first request of 257 keys)
    long_h = np.zeros(105 + 252, dtype=np.uint32)
    for bad in ((None, ptr(e), ptr(off), ptr(h), 21), (S._h, None, ptr(off), ptr(h), 21), (S._h, ptr(e), None, ptr(h), 21),
                (S._h, ptr(e), ptr(off), None, 21), (S._h, ptr(far), ptr(off), ptr(h), 21),
                (S._h, ptr(e), ptr(first), ptr(h), 21), (S._h, ptr(e), ptr(down), ptr(h), 21),
                (S._h, ptr(e), ptr(big), ptr(long_h), 21)):
        assert call(*bad, *outs) == -1  # RP_ERR_INVALID
    for K in (0, 257):
        assert lib().rp_sim_route_all_uniform(S._h, 1, 21, K, ctypes.byref(st)) == -1
    assert all((b == 77).all() for b in bufs)
    assert call(S._h, None, None, None, 0, *outs) == 0 and all((b == 77).all() for b in bufs)
    want = S.route_all(e, off, h)
    assert call(S._h, ptr(e), ptr(off), ptr(h), 21, *([None] * 8), ctypes.byref(st)) == 0 and st.as_dict() == want["stats"]
    assert call(S._h, ptr(e), ptr(off), ptr(h), 21, *outs[:8], None) == 0
    assert all(np.array_equal(b, want[k]) for b, k in zip(bufs, ra.ARRAYS))
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
        for use in (lambda: X.route_all(e[:4] % 64, off[:5], h[:20]), lambda: X.route_all_uniform(1, 16, 5)):
            with pytest.raises(rp.RingpopError) as ei:
                use()
            assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
        X.close()
    loop.close()
