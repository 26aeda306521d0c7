"""Requests across graceful leaves and rejoins on the
fixture's storm case: handleOrProxy's outcome table restated from the
reference's own ring server ids at a dump round after the leaves and one
after the rejoins, against Sim.route and Sim.ring_checksums; the drain -- a
left node proxies every request that enters it, and stays a destination while
some ring holds it; and the traffic counters' identities across the leave
rounds."""
import numpy as np
import pytest

import lifecycle_cases as lc
import oracle
import route_cases as rc

pytestmark = pytest.mark.gpu

REQUESTS = 4000
AFTER_LEAVES, AFTER_REJOINS = 30, 70


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


@pytest.fixture(scope="module")
def case(golden):
    return golden(lc.FIXTURE)["cases"][lc.STORM]


def expect(dump, addresses, entries, keys):
    """DESIGN §10's table from a reference dump: every node's ring as the
    points of its server ids (no two replica hashes collide at this size: the
    generator asserts it), its ring checksum and whether it fail-stopped."""
    n = len(dump)
    rings = []
    for f in dump:
        ids = np.array(f["ringIds"], dtype=np.int32)
        ph, po = oracle.ring_points_add_only([addresses[i] for i in ids])
        rings.append((ph, ids[po] if len(ids) else po))
    dead = [f["dead"] for f in dump]
    rcs = [f["ringChecksum"] for f in dump]
    m = len(entries)
    dests = np.full(m, -1, dtype=np.int32)
    outcomes = np.zeros(m, dtype=np.uint8)
    agrees = np.zeros(m, dtype=np.uint8)
    first = np.full(m, -1, dtype=np.int32)
    for e in range(n):
        sel = np.flatnonzero(entries == e)
        first[sel] = oracle.ring_lookup_points(rings[e][0], rings[e][1], keys[sel])
    for i, (e, h, d) in enumerate(zip(entries.tolist(), keys.tolist(), first.tolist())):
        if dead[e]:
            outcomes[i] = rc.ENTRY_DEAD
            continue
        if d < 0 or d == e:
            outcomes[i], dests[i] = rc.LOCAL, e
            continue
        dests[i] = d
        if dead[d]:
            outcomes[i] = rc.UNREACHABLE
            continue
        outcomes[i] = rc.CHECKSUMS_DIFFER if rcs[e] != rcs[d] else rc.DELIVERED
        agrees[i] = int(oracle.ring_lookup_points(rings[d][0], rings[d][1], np.array([h], dtype=np.uint32))[0]) == d
    return dests, outcomes, agrees, rcs


def test_route_after_leaves_and_after_rejoins(rp, case):
    cfg = case["config"]
    n = cfg["n"]
    S = rp.Sim(n, cfg["seed"], **lc.sim_kwargs(cfg))
    addresses = [S.address(v) for v in range(n)]
    entries, keys = rc.requests(rc.REQ_SEED, REQUESTS, n)
    left_ever = set()
    for r in range(AFTER_REJOINS + 1):
        S.round(churn=r < cfg["churnRounds"])
        if r not in (AFTER_LEAVES, AFTER_REJOINS):
            continue
        dump = case["dumps"][str(r)]
        dests, outcomes, agrees, rcs = expect(dump, addresses, entries, keys)
        gd, go, ga, st = S.route(entries, keys)
        assert np.array_equal(go, outcomes), (r, np.flatnonzero(go != outcomes)[:8])
        assert np.array_equal(gd, dests), r
        proxied = (outcomes == rc.DELIVERED) | (outcomes == rc.CHECKSUMS_DIFFER)
        assert np.array_equal(ga[proxied], agrees[proxied]), r
        assert S.ring_checksums().tolist() == rcs, r
        for c, k in enumerate(rc.OUTCOMES):
            assert st[k] == int((outcomes == c).sum()), (r, k)
        # the drain: a left node is a valid entry whose ring lacks itself
        left = [v for v, f in enumerate(dump) if not f["gossiping"] and not f["dead"]]
        at_left = np.isin(entries, left)
        if r == AFTER_LEAVES:
            assert sorted(left) == [5, 9, 17, 20, 33] and at_left.sum() > 100
            left_ever.update(left)
        else:
            assert sorted(left) == [9, 33]
            # the rejoined nodes serve their own keys again
            back = np.isin(entries, [5, 17, 20])
            assert (outcomes[back] == rc.LOCAL).any()
        assert not (outcomes[at_left] == rc.LOCAL).any() and not (outcomes[at_left] == rc.ENTRY_DEAD).any()
        assert all(v not in dump[v]["ringIds"] for v in left)
    S.close()


def test_traffic_identities_across_the_leaves(rp, case):
    """rp_traffic_run over rounds 0-39 (the leaves are at rounds 8 and 12), a
    drain, then DESIGN §11's identities on the tracker's counters."""
    cfg = case["config"]
    S = rp.Sim(cfg["n"], cfg["seed"], **lc.sim_kwargs(cfg))
    T = S.traffic(track=True)
    T.run(40, 300, rc.REQ_SEED, churn=True)
    for _ in range(20):
        S.round(churn=False)
        T.poll()
    s, by = T.stats()
    pending = T.pending_count()
    res = T.results(0, s["submitted"])
    outs = T.OUTCOMES
    assert s["submitted"] == 40 * 300
    for k in outs:
        assert s[k] == sum(by[k]), k
    assert s["submitted"] == sum(s[k] for k in outs) + pending
    dead = res["outcome"] == outs.index("entry_dead")
    dead_submit = int((dead & (res["done_clock"] == res["submit_clock"])).sum())
    dead_waiting = s["entry_dead"] - dead_submit
    assert s["retry_scheduled"] == s["retry_attempted"] + dead_waiting + pending
    assert s["proxied"] == s["submitted"] - s["local"] - dead_submit + s["retry_attempted"] - s["rerouted_local"]
    assert s["proxied"] == s["delivered"] + s["retry_scheduled"] + s["failed"]
    assert s["retry_failed"] == s["failed"]
    assert s["send_unreachable"] + s["checksums_differ"] == s["retry_scheduled"] + s["failed"]
    rows = T.history(0, S.rounds() + 1)
    for k in s:
        assert sum(row[k] for row in rows) == s[k], k
    # the leaves showed: rings disagreed while the leave spread
    assert s["checksums_differ"] > 0 and s["retry_succeeded"] > 0
    T.close()
    S.close()
