"""Multi-key request traffic on the GPU (rp_traffic_all_*)
against the model restated from the rules over the CPU oracle
(tests/traffic_all_cases.py): after every step every stats field, by_retries,
the open sends with their keys and every request's record."""
import numpy as np
import pytest

import oracle
import route_cases as rc
import traffic_all_cases as ta
import traffic_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def gpu_sim(rp, name, **extra):
    n, kw, _ = ta.SCENARIOS[name]
    return rp.Sim(n, tc.SIM_SEED, **kw, **extra)


def gpu_state(T):
    stats, by = T.stats()
    sends, keys = T.pending()
    return {"stats": stats, "by_retries": by, "sends": [tuple(int(x) for x in s) for s in sends.tolist()],
            "keys": keys.tolist(), "results": T.results(0, stats["requests"])}


def compare(got, want, where):
    assert got["stats"] == want["stats"], (where, got["stats"], want["stats"])
    assert got["by_retries"] == want["by_retries"], (where, got["by_retries"], want["by_retries"])
    assert len(got["sends"]) == len(want["sends"]), (where, len(got["sends"]), len(want["sends"]))
    bad = [i for i, (g, w) in enumerate(zip(got["sends"], want["sends"])) if g != w]
    assert not bad, (where, "sends", bad[:4], [got["sends"][i] for i in bad[:4]], [want["sends"][i] for i in bad[:4]])
    assert got["keys"] == want["keys"], (where, "keys")
    w = np.array(want["results"], dtype=np.int64).reshape(-1, 6)
    g = got["results"]
    gr = np.stack([g[k].astype(np.int64) for k in g.dtype.names], axis=1)
    assert gr.shape == w.shape, (where, gr.shape, w.shape)
    bad = np.flatnonzero((gr != w).any(axis=1))  # (done_clock of a request with an open send: 0 on both sides)
    assert bad.size == 0, (where, "results", bad[:4], gr[bad[:4]], w[bad[:4]])


def drive(rp, name, snaps, shards=1, **cfg):
    n, _, rounds = ta.SCENARIOS[name]
    S = gpu_sim(rp, name, shards=shards)
    T = S.traffic_all(track=True, **cfg)
    for r in range(1, rounds + ta.DRAIN + 1):
        S.round(churn=True)
        T.poll()
        if r <= rounds:
            e, off, h = ta.round_batch(n, r)
            assert T.submit(e, off, h) == (r - 1) * ta.PER_ROUND
            # one instant: the fanout is route_all's
            assert np.array_equal(T.results((r - 1) * ta.PER_ROUND, ta.PER_ROUND)["fanout"], S.route_all(e, off, h)["fanout"])
        compare(gpu_state(T), snaps[r - 1], (name, shards, r))
    assert len(T.pending()[0]) == 0
    T.close()
    S.close()


@pytest.mark.parametrize("name,shards", [(k, 1) for k in sorted(ta.SCENARIOS)] + [("failstop", 4)])
def test_traffic_all_matches_model(rp, name, shards):
    drive(rp, name, ta.expected(name)[1], shards=shards)


@pytest.mark.parametrize("cfg", [{"max_retries": 0}, {"enforce_consistency": False}, {"schedule": (0, 0, 2)}],
                         ids=["no_retries", "no_enforce", "zero_delays"])
def test_traffic_all_configurations(rp, cfg):
    snaps = []
    m = ta.run_model("failstop", per_step=lambda mm, r: snaps.append(ta.snapshot(mm)), **cfg)
    if cfg.get("enforce_consistency") is False:
        assert m.stats["misrouted_keys"] > 0
    if "schedule" in cfg:  # (zero delays are taken in the call that met the error, where nothing has changed)
        assert all(v[1] == v[2] == 0 for v in m.by_retries.values())
        assert m.by_retries["aborted"][3] > 0 and m.by_retries["delivered"][3] > 0
    drive(rp, "failstop", snaps, **cfg)


def test_one_key_requests_equal_the_single_key_tracker(rp):
    name, per = "failstop", 200
    n, _, rounds = ta.SCENARIOS[name]
    a, b = gpu_sim(rp, name), gpu_sim(rp, name)
    Ta, Tb = a.traffic(track=True), b.traffic_all(track=True)
    for r in range(1, rounds + ta.DRAIN + 1):
        a.round(churn=True)
        b.round(churn=True)
        Ta.poll()
        Tb.poll()
        if r <= rounds:
            e, h = tc.stream(n, (r - 1) * per, per)
            Ta.submit(e, h)
            Tb.submit(e, np.arange(per + 1, dtype=np.uint64), h)
    sa, sb = Ta.stats()[0], Tb.stats()[0]
    assert sa["retry_rerouted"] > 0 and sa["failed"] > 0 and sb["aborted"] == 0 and sb["requests"] == sa["submitted"]
    # (a dead entry's request has no send: the single-key tracker counts it under entry_dead)
    assert sa["entry_dead"] == sb["entry_dead"] + sb["requests_entry_dead"] and sa["misrouted"] == sb["misrouted_keys"]
    shared = [k for k in sa if k in sb and k != "entry_dead"]
    assert len(shared) == 12 and [sa[k] for k in shared] == [sb[k] for k in shared]
    ra, rb = Ta.results(0, rounds * per), Tb.results(0, rounds * per)
    for k in ("outcome", "submit_clock", "done_clock"):
        assert np.array_equal(ra[k], rb[k]), k
    a.close()
    b.close()


@pytest.mark.parametrize("K", [1, 8, 70])
def test_generator_and_run_equal_the_calls_one_by_one(rp, K):
    name, per, seed = "failstop_late", 90, 5
    n, _, rounds = ta.SCENARIOS[name]
    sims = [gpu_sim(rp, name) for _ in range(3)]
    Ts = [S.traffic_all(track=True) for S in sims]
    e, h = rc.requests(seed, rounds * per * K, n)
    for r in range(rounds + ta.DRAIN):
        for S, T in zip(sims[:2], Ts[:2]):
            S.round(churn=True)
            T.poll()
        if r < rounds:
            lo, hi = r * per * K, (r + 1) * per * K
            Ts[0].submit(e[lo:hi:K], np.arange(per + 1, dtype=np.uint64) * np.uint64(K), h[lo:hi])
            Ts[1].submit_uniform(seed, r * per, per, K)
    Ts[2].run(20, per, K, seed)
    Ts[2].run(rounds - 20, per, K, seed)  # (the generator index continues)
    mid = len(Ts[2].pending()[0])
    Ts[2].run(ta.DRAIN, 0, K, seed)
    g = [gpu_state(T) for T in Ts]
    assert mid > 0 and g[0]["stats"]["requests"] == rounds * per and g[0]["stats"]["retry_succeeded"] > 0
    for x in g[1:]:
        assert x["stats"] == g[0]["stats"] and x["by_retries"] == g[0]["by_retries"] and x["sends"] == g[0]["sends"] == []
        assert x["results"].tobytes() == g[0]["results"].tobytes()
    for S in sims:
        S.close()


@pytest.mark.parametrize("count,K", [(600, 3), (5, 256)], ids=["three_tiles", "segment_over_a_tile"])
def test_compaction_edges(rp, count, K):
    """The partition scenario inside its window, max_retries 8 and schedule {1}: one batch, then two polls."""
    name, cfg = "partition", {"max_retries": 8, "schedule": (1,)}
    n, kw, _ = ta.SCENARIOS[name]
    S, cpu = gpu_sim(rp, name), oracle.Sim(n, tc.SIM_SEED, **kw)
    T, m = S.traffic_all(track=True, **cfg), ta.Model(cpu, kw.get("partition"), **cfg)
    S.run(30, churn=True)
    for _ in range(30):
        cpu.round(churn=True)
    e, off, h = ta.batch(n, 0, [K] * count)
    T.submit(e, off, h)
    m.submit(30, e, off, h)
    survivors = [len(m.pending)]
    compare(gpu_state(T), ta.snapshot(m), (count, K, "batch"))
    for clock in (31, 32):
        S.round(churn=True)
        cpu.round(churn=True)
        T.poll()
        m.poll(clock)
        survivors.append(len(m.pending))
        compare(gpu_state(T), ta.snapshot(m), (count, K, clock))
    # 600: requests leave between others that stay, over three tiles; 5: every segment of 256 keys moves twice
    assert survivors[0] > 512 and 0 < survivors[2] < survivors[0] if count == 600 else survivors[2] == 5, survivors
    T.close()
    S.close()
    cpu.close()


def test_arguments_and_capacity(rp):
    from ringpop_amd._lib import lib, ptr
    S = gpu_sim(rp, "partition")
    S.run(26, churn=True)
    T = S.traffic_all(track=True, capacity=4, key_capacity=8, max_retries=8, schedule=(1,))
    e, off, h = ta.batch(S.n, 0, [5] * 21)
    far, first, down, big = e.copy(), off.copy(), off.copy(), off.copy()
    far[20], first[0], down[3], big[1:] = S.n, 1, 2, off[1:] + np.uint64(252)  # (a first request of 257 keys)
    long_h = np.zeros(105 + 252, dtype=np.uint32)
    call = lib().rp_traffic_all_submit
    for bad in ((None, ptr(e), ptr(off), ptr(h), 21), (T._h, None, ptr(off), ptr(h), 21), (T._h, ptr(e), None, ptr(h), 21),
                (T._h, ptr(e), ptr(off), None, 21), (T._h, ptr(far), ptr(off), ptr(h), 21),
                (T._h, ptr(e), ptr(first), ptr(h), 21), (T._h, ptr(e), ptr(down), ptr(h), 21),
                (T._h, ptr(e), ptr(big), ptr(long_h), 21)):
        assert call(*bad, None) == -1  # RP_ERR_INVALID
    for K in (0, 257):
        assert lib().rp_traffic_all_submit_uniform(T._h, 1, 0, 21, K) == -1
    assert call(T._h, None, None, None, 0, None) == 0
    T.submit(e[:1], off[:2], h[:5])
    before = gpu_state(T)
    assert before["stats"]["requests"] == 1
    over = (lambda: T.submit(e[:5], off[:6], h[:25]), lambda: T.submit(e[:2], off[:3], h[:10]),  # requests; keys
            lambda: T.submit_uniform(3, 0, 5, 1), lambda: T.submit_uniform(3, 0, 1, 9), lambda: T.run(5, 2, 1, 3))
    for use in over:
        with pytest.raises(rp.RingpopError) as ei:
            use()
        assert ei.value.code == -5  # RP_ERR_CAPACITY
        after = gpu_state(T)
        assert S.rounds() == 26 and after["stats"] == before["stats"] and after["sends"] == before["sends"]
        assert after["keys"] == before["keys"] and after["results"].tobytes() == before["results"].tobytes()
    T.close()
    S.close()
    # a rank of a loop cluster holds its own nodes' views only
    from ringpop_amd.sim import Loop
    loop = Loop(2)
    sims = [rp.Sim(64, rc.SIM_SEED, shards=2, rank=r, loop=loop) for r in range(2)]
    for X in sims:
        with pytest.raises(rp.RingpopError) as ei:
            X.traffic_all()
        assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
    for X in sims:
        X.close()
    loop.close()
