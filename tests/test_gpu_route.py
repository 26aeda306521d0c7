"""Request routing on the GPU (rp_sim_ring_checksums / rp_sim_route /
rp_sim_route_uniform) against the expectation restated from the CPU oracle
(tests/route_cases.py): every request's destination, outcome and owner
agreement, the statistics and every view's ring checksum, after every round of
a fail-stop, a partition and a colliding-replica-hash scenario; in-process
shards, the device request generator, the checksum cache, the shapes of the
ring checksum string, and the ranks of a loop cluster."""
import threading

import numpy as np
import pytest

import oracle
import route_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def gpu_sim(rp, name, **extra):
    n, kw, _, _ = rc.SCENARIOS[name]
    return rp.Sim(n, rc.SIM_SEED, **kw, **extra)


def run_scenario(rp, name, check_info=False, **extra):
    """The scenario on the device, routed after every round: a list of
    (dests, outcomes, owner_agrees, stats, ring checksums) like rc.expected."""
    n, _, rounds, _ = rc.SCENARIOS[name]
    S = gpu_sim(rp, name, **extra)
    entries, keys = rc.requests(rc.REQ_SEED, rc.REQUESTS, n)
    out = []
    for r in range(1, rounds + 1):
        S.round(churn=True)
        rcs = S.ring_checksums()
        out.append(S.route(entries, keys) + (rcs,))
        if check_info:
            own = [S.info(v)["ring_checksum"] for v in range(n)]
            assert rcs.tolist() == own, (name, r)
    S.close()
    return out


def compare(name, got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want), start=1):
        assert np.array_equal(g[4], w[4]), (name, r, "ring checksums", np.flatnonzero(g[4] != w[4])[:8])
        for k, what in enumerate(("dests", "outcomes", "owner_agrees")):
            bad = np.flatnonzero(g[k] != w[k])
            assert bad.size == 0, (name, r, what, bad[:8], g[k][bad[:8]], w[k][bad[:8]])
        assert g[3] == w[3], (name, r, g[3], w[3])


_one_shard = {}


def one_shard(rp, name):
    """The one-shard run of a scenario (computed once; read-only)."""
    if name not in _one_shard:
        _one_shard[name] = run_scenario(rp, name, check_info=True)
    return _one_shard[name]


@pytest.mark.parametrize("name", ["failstop", "partition", "shift"])
def test_route_matches_oracle(rp, name):
    compare(name, one_shard(rp, name), rc.expected(name))


@pytest.mark.parametrize("shards", [2, 4])
def test_route_on_shards_equals_one_shard(rp, shards):
    got = run_scenario(rp, "failstop", shards=shards)
    compare("failstop", got, rc.expected("failstop"))
    for g, o in zip(got, one_shard(rp, "failstop")):
        for k in (0, 1, 2, 4):
            assert g[k].tobytes() == o[k].tobytes()
        assert g[3] == o[3]


def test_route_uniform_equals_host_generated_requests(rp):
    n = rc.SCENARIOS["failstop"][0]
    S = gpu_sim(rp, "failstop")
    S.run(29, churn=True)
    want = rc.expected("failstop")[28][3]
    assert want["checksums_differ"] > 0 and want["misrouted"] > 0  # (a diverged checkpoint)
    entries, keys = rc.requests(rc.REQ_SEED, rc.REQUESTS, n)
    assert S.route(entries, keys)[3] == want
    assert S.route_uniform(rc.REQ_SEED, rc.REQUESTS) == want
    assert S.route_uniform(rc.REQ_SEED, 0)["requests"] == 0
    S.close()


def test_ring_checksum_cache_tracks_changes(rp):
    n, kw, _, _ = rc.SCENARIOS["failstop"]
    S = gpu_sim(rp, "failstop")
    cpu = oracle.Sim(n, rc.SIM_SEED, **kw)

    def want():
        return [cpu.info(v)["ring_checksum"] for v in range(n)]

    for _ in range(30):
        S.round(churn=True)
        cpu.round(churn=True)
    first = S.ring_checksums().tolist()
    assert first == want()
    assert S.ring_checksums().tolist() == first  # (no call between: the cached values)
    S.round(churn=True)
    cpu.round(churn=True)
    second = S.ring_checksums().tolist()
    assert second == want() and second != first
    # node 0 learns that member 7 is faulty: its ring, and only its, changes
    _, inc = S.view(0)
    row = [[7, 3, int(inc[7]), 0, int(inc[0])]]
    assert S.update(0, row) == 1 and cpu.update(0, row) == 1
    third = S.ring_checksums().tolist()
    assert third == want()
    assert [v for v in range(n) if third[v] != second[v]] == [0]
    S.close()
    cpu.close()


def views_all(n, status=1):
    st = np.full((n, n), status, dtype=np.int32)
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    return st, inc


def check_ring_strings(rp, addresses, views):
    n = len(addresses)
    S = rp.Sim(n, 3, addresses=addresses, views=views)
    got = S.ring_checksums().tolist()
    for v in range(n):
        s = ";".join(addresses[a] for a in range(n) if views[0][v, a] in (1, 2))
        assert got[v] == rp.hash32(s), (v, len(s), s[:80])
        assert got[v] == S.info(v)["ring_checksum"], v
    S.close()
    return [len(";".join(addresses[a] for a in range(n) if views[0][v, a] in (1, 2))) for v in range(n)]


@pytest.mark.parametrize("n,alen,total", [(2, 1, 3), (2, 4, 9), (3, 6, 20), (3, 8, 26)])
def test_ring_checksum_short_strings(rp, n, alen, total):
    """farmhash32's <= 4, 5-12 and 13-24 byte branches and the first length
    past them (one block and the tail)."""
    addresses = [chr(0x61 + i) * alen for i in range(n)]
    assert check_ring_strings(rp, addresses, views_all(n)) == [total] * n


def test_ring_checksum_address_lengths_1_to_32(rp):
    n = 70
    addresses = [chr(0x21 + i) + "x" * (i % 32) for i in range(n)]
    assert sorted(addresses) == addresses and {len(a) for a in addresses} == set(range(1, 33))
    check_ring_strings(rp, addresses, views_all(n))


def test_ring_checksum_sparse_rings(rp):
    """n = 130 (two full chunks and two members): a first chunk that renders
    nothing (the first rendered member gets no separator), a ring of the node
    alone, every second member, and a ring whose last 20 bytes span chunks."""
    n = 130
    addresses = [chr(0x30 + i // 64) + chr(0x30 + i % 64) + "y" * (4 + i % 20) for i in range(n)]
    assert sorted(addresses) == addresses
    st, inc = views_all(n)
    st[129, 0:64] = 3                      # members 0..63 faulty
    st[128, :] = 3
    st[128, 128] = 1                       # itself only
    st[127, 0::2] = 3                      # exactly every second member (the odd ones, itself among them)
    st[126, :] = 3
    st[126, [0, 1, 126]] = 1               # 6 + 7 + 12 bytes and two separators: the tail spans both chunks
    st[125, :] = 3
    st[125, [0, 125]] = 1                  # 6 + 1 + 11 = 18 bytes: a short string from two chunks
    lens = check_ring_strings(rp, addresses, (st, inc))
    assert lens[126] == 27 and lens[125] == 18 and lens[128] == len(addresses[128]) <= 24


def test_route_on_loop_ranks(rp):
    """A rank of a loop cluster holds its own nodes' views only: ring
    checksums of the others are 0 and routing is unsupported."""
    from ringpop_amd.sim import Loop
    G, n, rounds = 2, 64, 6
    loop = Loop(G)
    sims = [rp.Sim(n, rc.SIM_SEED, shards=G, rank=r, loop=loop) for r in range(G)]
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
    ref = rp.Sim(n, rc.SIM_SEED)
    ref.run(rounds, churn=True)
    want = ref.ring_checksums()
    ref.close()
    assert want.all()
    entries, keys = rc.requests(rc.REQ_SEED, 16, n)
    for r, S in enumerate(sims):
        lo, hi = S.shard_range()
        assert (lo, hi) == (r * n // G, (r + 1) * n // G)
        got = S.ring_checksums()
        assert np.array_equal(got[lo:hi], want[lo:hi])
        assert not got[:lo].any() and not got[hi:].any()
        for call in (lambda: S.route(entries, keys), lambda: S.route_uniform(1, 16)):
            with pytest.raises(rp.RingpopError) as ei:
                call()
            assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
    for S in sims:
        S.close()
    loop.close()
