"""Request traffic with proxy retries on the GPU (rp_traffic_*) against the
model restated from DESIGN.md §11 over the CPU oracle (tests/traffic_cases.py):
after every step the cumulative statistics, the clock's history row,
by_retries, the whole pending table and every request's record; in-process
shards, the device generator, run() against the calls made one by one, other
schedules, skipped polls, the ring checksum cache, the capacity error and the
compaction of the pending table at the sizes where it can go wrong."""
import numpy as np
import pytest

import oracle
import route_cases as rc
import traffic_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def gpu_sim(rp, name, **extra):
    n, kw, _ = tc.SCENARIOS[name]
    return rp.Sim(n, tc.SIM_SEED, **kw, **extra)


def result_rows(results):
    """A model's results list as an (ids, 5) array; pending requests: outcome 255."""
    return np.array([r if r else (0, tc.PENDING, 0, 0, 0) for r in results], dtype=np.int64).reshape(-1, 5)


def gpu_state(T, clock):
    """What tc.snapshot holds, read from the tracker."""
    stats, by = T.stats()
    p = T.pending()
    return {"stats": stats, "row": T.history(clock, 1)[0], "by_retries": by,
            "pending": [tuple(int(x) for x in q) for q in p.tolist()],
            "results": T.results(0, stats["submitted"])}


def compare(got, want, where):
    assert got["stats"] == want["stats"], (where, got["stats"], want["stats"])
    assert got["row"] == want["row"], (where, got["row"], want["row"])
    assert got["by_retries"] == want["by_retries"], (where, got["by_retries"], want["by_retries"])
    assert len(got["pending"]) == len(want["pending"]), (where, len(got["pending"]), len(want["pending"]))
    bad = [i for i, (g, w) in enumerate(zip(got["pending"], want["pending"])) if g != w]
    assert not bad, (where, "pending", bad[:4], [got["pending"][i] for i in bad[:4]], [want["pending"][i] for i in bad[:4]])
    w = result_rows(want["results"])
    g = got["results"]
    assert len(g) == len(w), (where, len(g), len(w))
    gr = np.stack([g[k].astype(np.int64) for k in ("dest", "outcome", "retries", "submit_clock", "done_clock")], axis=1)
    done = w[:, 1] != tc.PENDING
    bad = np.flatnonzero((gr[:, 1] != w[:, 1]) | (done[:, None] & (gr != w)).any(axis=1))
    assert bad.size == 0, (where, "results", bad[:4], gr[bad[:4]], w[bad[:4]])


def drive(rp, name, snaps, shards=1, **cfg):
    """The scenario's schedule of tc.run_model on the device, compared with
    the model's snapshots after every step."""
    n, _, rounds = tc.SCENARIOS[name]
    S = gpu_sim(rp, name, shards=shards)
    T = S.traffic(track=True, **cfg)
    for r in range(1, rounds + tc.DRAIN + 1):
        S.round(churn=True)
        T.poll()
        if r <= rounds:
            first = T.submit(*tc.stream(n, (r - 1) * tc.PER_ROUND, tc.PER_ROUND))
            assert first == (r - 1) * tc.PER_ROUND
        compare(gpu_state(T, r), snaps[r - 1], (name, shards, r))
    assert T.pending_count() == 0
    T.close()
    S.close()


@pytest.mark.parametrize("shards", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_traffic_matches_model(rp, name, shards):
    drive(rp, name, tc.expected(name)[1], shards=shards)


@pytest.mark.parametrize("name,cfg", [
    ("failstop_late", {"max_retries": 4, "schedule": (1, 2)}),   # past the end of the schedule
    ("failstop", {"max_retries": 0}),                           # the plain error, no retry counter moves
    ("failstop", {"max_retries": 1, "schedule": (3,)}),
    ("failstop", {"enforce_consistency": False}),
], ids=["past_the_end", "no_retries", "one_retry", "no_enforce"])
def test_traffic_configurations(rp, name, cfg):
    snaps = []
    m = tc.run_model(name, per_step=lambda mm, r: snaps.append(tc.snapshot(mm, r)), **cfg)
    if cfg.get("max_retries") == 4:
        assert m.by_retries["failed"][4] > 0 and all(m.by_retries["delivered"][r] > 0 for r in (1, 2, 3, 4))
    if cfg.get("max_retries") == 0:
        assert m.by_retries["failed"][0] > 0 and m.stats["retry_scheduled"] == 0
    if cfg.get("enforce_consistency") is False:
        assert m.stats["checksums_differ"] > 0 and m.stats["misrouted"] > 0
    drive(rp, name, snaps, **cfg)


class Lockstep:
    """A device simulation with a tracker beside the oracle with the model."""

    def __init__(self, rp, name, capacity=1 << 20, **cfg):
        self.n, kw, _ = tc.SCENARIOS[name]
        self.name = name
        self.S = gpu_sim(rp, name)
        self.T = self.S.traffic(track=True, capacity=capacity, **cfg)
        self.cpu = oracle.Sim(self.n, tc.SIM_SEED, **kw)
        self.m = tc.Model(self.cpu, kw.get("partition"), **cfg)
        self.clock = 0

    def rounds(self, k):
        for _ in range(k):
            self.S.round(churn=True)
            self.cpu.round(churn=True)
        self.clock += k

    def poll(self):
        self.T.poll()
        self.m.poll(self.clock)

    def submit(self, entries, keys):
        self.T.submit(np.asarray(entries, dtype=np.uint32), np.asarray(keys, dtype=np.uint32))
        self.m.submit(self.clock, entries, keys)

    def check(self, what):
        compare(gpu_state(self.T, self.clock), tc.snapshot(self.m, self.clock), (self.name, what, self.clock))

    def close(self):
        self.T.close()
        self.S.close()
        self.cpu.close()


def test_submit_uniform_equals_explicit_submit(rp):
    n = tc.SCENARIOS["failstop"][0]
    a, b = gpu_sim(rp, "failstop"), gpu_sim(rp, "failstop")
    a.run(29, churn=True)
    b.run(29, churn=True)
    Ta, Tb = a.traffic(track=True), b.traffic(track=True)
    e, h = rc.requests(rc.REQ_SEED, 2200, n)
    Ta.submit(e[:1500], h[:1500])
    Tb.submit_uniform(rc.REQ_SEED, 0, 1500)
    Ta.submit(e[1500:], h[1500:])
    Tb.submit_uniform(rc.REQ_SEED, 1500, 700)
    Tb.submit_uniform(rc.REQ_SEED, 2200, 0)
    ga, gb = gpu_state(Ta, 29), gpu_state(Tb, 29)
    assert ga["stats"]["retry_scheduled"] > 0 and len(ga["pending"]) > 0  # (a diverged checkpoint)
    assert ga["stats"] == gb["stats"] and ga["row"] == gb["row"] and ga["by_retries"] == gb["by_retries"]
    assert ga["pending"] == gb["pending"]
    assert ga["results"].tobytes() == gb["results"].tobytes()
    a.close()
    b.close()


def test_run_equals_the_calls_one_by_one(rp):
    name, per, seed = "failstop_late", 300, 5
    rounds = tc.SCENARIOS[name][2]
    a, b = gpu_sim(rp, name), gpu_sim(rp, name)
    Ta, Tb = a.traffic(track=True), b.traffic(track=True)
    for r in range(rounds):
        a.round(churn=True)
        Ta.poll()
        Ta.submit_uniform(seed, r * per, per)
    for _ in range(tc.DRAIN):
        a.round(churn=True)
        Ta.poll()
    Tb.run(20, per, seed)
    Tb.run(rounds - 20, per, seed)  # (the generator index continues)
    mid = Tb.pending_count()
    Tb.run(tc.DRAIN, 0, seed)
    assert mid > 0 and a.rounds() == b.rounds() == rounds + tc.DRAIN
    ga, gb = gpu_state(Ta, rounds), gpu_state(Tb, rounds)
    assert ga["stats"]["submitted"] == rounds * per and ga["stats"]["retry_succeeded"] > 0
    assert ga["stats"] == gb["stats"] and ga["by_retries"] == gb["by_retries"] and ga["pending"] == gb["pending"] == []
    assert Ta.history(0, rounds + tc.DRAIN + 2) == Tb.history(0, rounds + tc.DRAIN + 2)
    assert ga["results"].tobytes() == gb["results"].tobytes()
    assert a.ring_checksums().tolist() == b.ring_checksums().tolist()
    a.close()
    b.close()


def test_polls_skipped_for_seven_rounds(rp):
    """A retry fires at the first poll at or after its due clock, and the
    next delay counts from that poll's clock."""
    L = Lockstep(rp, "partition", max_retries=3, schedule=(2, 3, 4))
    late = 0
    for r in range(1, 49):
        L.rounds(1)
        if r % 8 == 0:
            late += sum(1 for q in L.m.pending if q["due"] < r)
            L.poll()
        if r <= 30:
            L.submit(*tc.stream(L.n, (r - 1) * 100, 100))
        L.check("skipped polls")
    assert late > 0 and L.m.stats["retry_succeeded"] > 0 and L.m.by_retries["failed"][3] > 0
    L.rounds(8)
    L.poll()
    L.check("drained")
    L.close()


def test_ring_change_between_polls_refreshes_the_checksums(rp):
    """Sim.update changes node 0's ring between two calls at one clock: its
    requests now meet differing checksums (the cached ones would deliver)."""
    L = Lockstep(rp, "failstop", max_retries=2, schedule=(1,))
    L.rounds(45)
    assert len({L.cpu.info(v)["ring_checksum"] for v in range(L.n) if not L.cpu.info(v)["dead"]}) == 1
    e, h = tc.stream(L.n, 0, 4000)
    mine = [(a, b) for a, b in zip(e, h) if a == 0][:30]
    assert len(mine) >= 20
    L.poll()
    L.submit([a for a, _ in mine], [b for _, b in mine])
    L.check("converged")
    assert L.m.stats["checksums_differ"] == 0 and L.m.stats["delivered"] > 0
    _, inc = L.S.view(0)
    row = [[7, 3, int(inc[7]), 0, int(inc[0])]]
    assert L.S.update(0, row) == 1 and L.cpu.update(0, row) == 1
    L.m._state_clock = None  # (the model reads the oracle's state once per clock)
    L.submit([a for a, _ in mine], [b for _, b in mine])
    assert L.m.stats["checksums_differ"] > 0 and L.m.pending
    L.check("after the update")
    L.rounds(1)
    L.poll()
    L.check("next clock")
    L.close()


def test_capacity_error_changes_nothing(rp):
    n = tc.SCENARIOS["partition"][0]
    S = gpu_sim(rp, "partition")
    S.run(10, churn=True)
    T = S.traffic(track=True, capacity=300, max_retries=8, schedule=(1,))
    e, h = rc.requests(rc.REQ_SEED, 400, n)
    T.submit(e[:100], h[:100])
    before = gpu_state(T, 10)
    assert 0 < len(before["pending"]) < 100
    for call in (lambda: T.submit(e[:301], h[:301]), lambda: T.submit_uniform(3, 0, 301), lambda: T.run(5, 100, 3)):
        with pytest.raises(rp.RingpopError) as ei:
            call()
        assert ei.value.code == -5  # RP_ERR_CAPACITY
        after = gpu_state(T, 10)
        assert S.rounds() == 10 and after["stats"] == before["stats"] and after["pending"] == before["pending"]
        assert after["results"].tobytes() == before["results"].tobytes()
    room = 300 - len(before["pending"])  # exactly to the capacity
    T.submit(e[100:100 + room], h[100:100 + room])
    assert T.stats()[0]["submitted"] == 100 + room
    with pytest.raises(rp.RingpopError):
        S.traffic(max_retries=9)
    T.close()
    S.close()


def test_compaction_at_its_edge_sizes(rp):
    """The partition scenario inside its window, from round 24 on (the rings
    of the two sides have diverged; retries start to succeed node by node),
    max_retries 8 and schedule {1}: batches whose survivors number 0, 1, 63,
    64, 65, 255, 256 and 257, each with requests that finish between the
    survivors, a poll after each, then one batch of 70,000 and three polls in
    which requests all over the table finish."""
    L = Lockstep(rp, "partition", max_retries=8, schedule=(1,))
    L.rounds(24)
    pool_e, pool_h = tc.stream(L.n, 0, 12000)
    used, between = 0, 0

    def poll():
        nonlocal between
        before = [q["id"] for q in L.m.pending]
        L.rounds(1)
        L.poll()
        left = {q["id"] for q in L.m.pending}
        gone = [i for i in before if i not in left]
        if gone and left and min(left) < max(gone) and max(left) > min(gone):
            between += 1

    for k in (0, 1, 63, 64, 65, 255, 256, 257):
        # classify the next requests of the pool at this clock with a scratch model
        probe = tc.Model(L.cpu, L.m.partition, max_retries=8, schedule=(1,))
        e, h = pool_e[used:used + 1500], pool_h[used:used + 1500]
        probe.submit(L.clock, e, h)
        waits = {q["id"] for q in probe.pending}
        assert len(waits) >= k and len(e) - len(waits) >= 40
        take, nw, nf = [], 0, 0
        for i in range(len(e)):  # the first k survivors, finishers among them (up to 40 more than survivors)
            if i in waits and nw < k:
                take.append(i)
                nw += 1
            elif i not in waits and nf < nw + 40:
                take.append(i)
                nf += 1
        used += 1500
        before = len(L.m.pending)
        L.submit([e[i] for i in take], [h[i] for i in take])
        assert len(L.m.pending) == before + k
        L.check(("batch survivors", k))
        poll()
        L.check(("poll after", k))
    assert between >= 3 and len(L.m.pending) > 256  # (several tiles, requests left between others)
    L.submit(*tc.stream(L.n, 12000, 70000))
    assert len(L.m.pending) > 20000
    L.check("70,000")
    between = 0
    for _ in range(3):
        poll()
        L.check("poll after 70,000")
    assert between == 3 and len(L.m.pending) > 1024
    L.close()


def test_scan_and_chunk_loops_equal_smaller_submits(rp):
    """More tiles than one pass of the scan takes (1,024) and more requests
    than one submit launch (2^20): one call equals two calls of half each."""
    S = gpu_sim(rp, "partition")
    S.run(10, churn=True)
    total = 1100000
    Ta = S.traffic(capacity=total, max_retries=8, schedule=(1,))
    Tb = S.traffic(capacity=total, max_retries=8, schedule=(1,))
    Ta.submit_uniform(9, 0, total)
    Tb.submit_uniform(9, 0, total // 2)
    Tb.submit_uniform(9, total // 2, total // 2)
    pa, pb = Ta.pending(), Tb.pending()
    assert len(pa) > 300000 and Ta.stats()[0]["delivered"] > 300000
    assert Ta.stats() == Tb.stats() and pa.tobytes() == pb.tobytes()
    assert np.all(np.diff(pa["id"].astype(np.int64)) > 0)
    S.round(churn=True)
    Ta.poll()
    Tb.poll()
    qa = Ta.pending()
    assert 0 < len(qa) <= len(pa) and Ta.stats() == Tb.stats() and qa.tobytes() == Tb.pending().tobytes()
    assert np.all(np.diff(qa["id"].astype(np.int64)) > 0) and np.all(qa["retries"] == 1) and np.all(qa["due"] == 12)
    S.close()


def test_traffic_on_loop_ranks_is_unsupported(rp):
    from ringpop_amd.sim import Loop
    loop = Loop(2)
    sims = [rp.Sim(64, rc.SIM_SEED, shards=2, rank=r, loop=loop) for r in range(2)]
    for S in sims:
        with pytest.raises(rp.RingpopError) as ei:
            S.traffic()
        assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
    for S in sims:
        S.close()
    loop.close()
