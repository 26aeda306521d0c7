"""Ring checksums one view per lane (k_ring_checksums_pl, forced with
Sim.ring_checksum_lanes(1)) against oracle.farmhash32 of the string built in
Python from the addresses and views, and against the one-view-per-wave path:
string lengths at farmhash32's branches, address lengths 1..32, lanes of one
group that disagree, sizes off every tile boundary, a running cluster on
shards, many groups, and the path selection with its counters."""
import numpy as np
import pytest

import oracle
import route_cases as rc

pytestmark = pytest.mark.gpu
NEVER = 0xFFFFFFFF


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def both_paths(S):
    """(lane path, wave path) checksums of S as it stands, each counted."""
    before = S.ring_checksum_counts()
    S.ring_checksum_lanes(1)
    lane = S.ring_checksums().tolist()
    mid = S.ring_checksum_counts()
    S.ring_checksum_lanes(NEVER)
    wave = S.ring_checksums().tolist()
    after = S.ring_checksum_counts()
    assert (mid["lane_views"] - before["lane_views"], mid["wave_views"] - before["wave_views"]) == (S.n, 0)
    assert (after["lane_views"] - mid["lane_views"], after["wave_views"] - mid["wave_views"]) == (0, S.n)
    return lane, wave


def ring_string(addresses, status_row):
    return ";".join(a for a, s in zip(addresses, status_row) if s in (1, 2))


def check_strings(rp, addresses, st):
    """Loads the views; every view's lane checksum == farmhash32 of its
    string == the wave path's.  Returns the strings' lengths."""
    n = len(addresses)
    assert sorted(addresses) == addresses
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    S = rp.Sim(n, 3, addresses=addresses, views=(st.astype(np.int32), inc))
    lane, wave = both_paths(S)
    S.close()
    strings = [ring_string(addresses, st[v]) for v in range(n)]
    for v, s in enumerate(strings):
        assert lane[v] == oracle.farmhash32(s), (v, len(s), s[:80])
    assert lane == wave
    return [len(s) for s in strings]


def full(n):
    return np.ones((n, n), dtype=np.int32)


@pytest.mark.parametrize("alens,total", [((1, 1), 3), ((4, 4), 9), ((6, 6, 6), 20), ((8, 8, 8), 26),
                                         ((7, 8, 7), 24), ((8, 8, 7), 25), ((14, 14, 14), 44)])
def test_short_and_boundary_strings(rp, alens, total):
    """farmhash32's <= 4, 5-12 and 13-24 byte branches, 24 | 25, and two
    blocks plus the overlapping tail."""
    addresses = [chr(0x61 + i) * k for i, k in enumerate(alens)]
    assert check_strings(rp, addresses, full(len(alens))) == [total] * len(alens)


@pytest.mark.parametrize("n,alen", [(70, None), (200, 32), (94, 1)])
def test_address_lengths(rp, n, alen):
    """Lengths 1..32 in one ring (a partial second tile, rows off 4-byte
    alignment); the largest piece throughout; the smallest throughout."""
    if alen is None:
        addresses = [chr(0x21 + i) + "x" * (i % 32) for i in range(n)]
        assert {len(a) for a in addresses} == set(range(1, 33))
    elif alen == 1:
        addresses = [chr(0x21 + i) for i in range(n)]
    else:
        addresses = [chr(0x21 + i // 90) + chr(0x21 + i % 90) + "z" * (alen - 2) for i in range(n)]
    assert all(len(a) == (alen or len(a)) for a in addresses)
    check_strings(rp, addresses, full(n))


def test_lanes_of_one_group_disagree(rp):
    """n = 130 (a group of 64, one of 64, one of 2 lanes): beside full views,
    a first tile without a member, a view of the node alone, every second
    member, a 27-byte string whose tail spans tiles and an 18-byte one drawn
    from two tiles.  (views= refuses a view without its own node, so a ring
    without any server cannot be loaded.)"""
    n = 130
    addresses = [chr(0x30 + i // 64) + chr(0x30 + i % 64) + "y" * (4 + i % 20) for i in range(n)]
    st = full(n)
    st[129, 0:64] = 3
    st[128, :] = 3
    st[128, 128] = 1
    st[127, 0::2] = 3
    st[126, :] = 3
    st[126, [0, 1, 126]] = 1
    st[125, :] = 3
    st[125, [0, 125]] = 1
    st[3, :] = 3                            # the same shapes inside the first group, beside streaming lanes
    st[3, 3] = 1
    st[5, 0::2] = 3
    st[7, 64:] = 3
    lens = check_strings(rp, addresses, st)
    assert lens[126] == 27 and lens[125] == 18 and lens[128] == len(addresses[128]) <= 24 and lens[3] <= 24


@pytest.mark.parametrize("n", [2, 3, 63, 65, 67, 129])
def test_sizes_off_the_tile(rp, n):
    """(A simulation has at least 2 nodes: n = 2 stands for the smallest.)"""
    addresses = ["%03d.node:%d" % (i, 3000 + i) for i in range(n)]
    check_strings(rp, addresses, full(n))
    st = full(n)
    for v in range(n):                      # members of the view's own parity only
        st[v, (v + 1) % 2::2] = 3
    check_strings(rp, addresses, st)


@pytest.mark.parametrize("shards", [1, 2, 4])
def test_running_cluster(rp, shards):
    n, kw, rounds, _ = rc.SCENARIOS["failstop"]
    S = rp.Sim(n, rc.SIM_SEED, shards=shards, **kw)
    cpu = oracle.Sim(n, rc.SIM_SEED, **kw)
    S.ring_checksum_lanes(1)
    for r in range(1, rounds + 1):
        S.round(churn=True)
        cpu.round(churn=True)
        assert S.ring_checksums().tolist() == [cpu.info(v)["ring_checksum"] for v in range(n)], r
    cpu.close()
    assert S.ring_checksum_counts() == {"wave_views": 0, "lane_views": rounds * n}
    entries, keys = rc.requests(rc.REQ_SEED, rc.REQUESTS, n)
    lane = S.route(entries, keys)
    S.ring_checksum_lanes(NEVER)
    wave = S.route(entries, keys)
    assert S.ring_checksum_counts()["wave_views"] == n
    S.close()
    assert all(np.array_equal(a, b) for a, b in zip(lane[:3], wave[:3])) and lane[3] == wave[3]


def test_many_groups(rp):
    n = 2048
    S = rp.Sim(n, 2024, failures={2: list(range(100, 2048, 100))[:20]})
    S.run(5, churn=True)
    lane, wave = both_paths(S)
    assert lane == wave
    addresses = S.addresses()
    for v in range(0, n, 32):
        assert lane[v] == oracle.farmhash32(ring_string(addresses, S.view(v)[0])), v
    S.close()


def test_selection_and_counters(rp):
    n = 96
    S = rp.Sim(n, rc.SIM_SEED)
    auto = S.ring_checksums().tolist()
    assert S.ring_checksum_counts() == {"wave_views": n, "lane_views": 0}  # (auto: far below any crossover)
    S.ring_checksum_lanes(1)
    assert S.ring_checksums().tolist() == auto
    assert S.ring_checksum_counts() == {"wave_views": n, "lane_views": n}
    assert S.ring_checksums().tolist() == auto
    assert S.ring_checksum_counts() == {"wave_views": n, "lane_views": n}  # (cached)
    S.ring_checksum_lanes(NEVER)
    assert S.ring_checksums().tolist() == auto
    assert S.ring_checksum_counts() == {"wave_views": 2 * n, "lane_views": n}
    S.ring_checksum_lanes(0)
    assert S.ring_checksums().tolist() == auto
    assert S.ring_checksum_counts() == {"wave_views": 3 * n, "lane_views": n}
    S.close()
    S = rp.Sim(n, rc.SIM_SEED, shards=4)
    S.ring_checksum_lanes(1)
    assert S.ring_checksums().tolist() == auto
    assert S.ring_checksum_counts() == {"wave_views": 0, "lane_views": n}
    S.close()
