"""Ownership movement on the GPU (rp_ownership_snapshot_* /
rp_sim_ownership_moved): every stats field, gained[] and lost[]
against the expectation restated from the CPU oracle (tests/movement_cases.py)
on 1, 2 and 4 in-process shards; against a brute force through the existing
per-view lookup kernel where the oracle has no model (graceful leave and
rejoin, sparse views set directly, 1,400 nodes); the cache; the argument
checks; the ranks of a loop cluster; the census beside live snapshots."""
import ctypes
import threading

import numpy as np
import pytest

import movement_cases as mc
import ownership_cases as oc

pytestmark = pytest.mark.gpu

ALL = 1 << 32
FIELDS = ("transition",) + mc.SCALARS


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def check(got, want, where):
    for k in FIELDS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("gained_by", "lost_by"):
        assert got[k].dtype == np.uint64
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (where, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    assert sum(sum(r) for r in got["transition"]) == ALL, where


def same(a, b):
    return all(a[k] == b[k] for k in FIELDS) and np.array_equal(a["gained_by"], b["gained_by"]) and \
        np.array_equal(a["lost_by"], b["lost_by"])


def nothing_moved(got, n):
    quiet = [k for k in mc.SCALARS if k not in ("same_set", "from_clock", "to_clock", "intervals")]
    return (got["same_set"] == ALL and not got["gained_by"].any() and not got["lost_by"].any() and
            all(got[k] == 0 for k in quiet) and len(got["gained_by"]) == n and
            all(got["transition"][a][b] == 0 for a in range(3) for b in range(3) if a != b))


def device_boundaries(S, shift=0):
    return oc.boundaries([S.address(v) for v in range(S.n)], shift)


def brute(S, b, rows_from, rows_to, fc, tc):
    return mc.movement(b, rows_from, rows_to, S.n, fc, tc)


@pytest.mark.parametrize("shards", [1, 2, 4])
@pytest.mark.parametrize("name", list(mc.CLOCKS))
def test_movement_matches_oracle(rp, name, shards):
    n, kw, rounds, _ = oc.SCENARIOS[name]
    b, want, claimed = mc.expected(name)
    clocks, todo = mc.CLOCKS[name], mc.pairs(name)
    S = rp.Sim(n, oc.SIM_SEED, **kw, shards=shards)
    snaps, own = {}, {}
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        if r not in clocks:
            continue
        # (taken while the run proceeds: every earlier one is still live)
        snaps[r] = S.ownership_snapshot()
        own[r] = S.ownership()
        assert snaps[r].clock == r and snaps[r].stats == {k: own[r][k] for k in snaps[r].stats}, (name, r)
        assert np.array_equal(own[r]["claimed"], claimed[r]), (name, r)
        for f, t in todo:
            if max(f, t) != r:
                continue
            got = S.ownership_moved(snaps[f], snaps[t])
            check(got, want[(f, t)], (name, shards, f, t))
            # per node gained - lost is the change of its claimed measure between the two censuses
            d = got["gained_by"].astype(np.int64) - got["lost_by"].astype(np.int64)
            assert np.array_equal(d, own[t]["claimed"].astype(np.int64) - own[f]["claimed"].astype(np.int64))
    # the reversed pair swaps gained and lost and transposes transition
    f, t = mc.REVERSED[name]
    fwd, rev = S.ownership_moved(snaps[t], snaps[f]), S.ownership_moved(snaps[f], snaps[t])
    assert rev["transition"] == [list(r) for r in zip(*fwd["transition"])]
    assert np.array_equal(rev["gained_by"], fwd["lost_by"]) and np.array_equal(rev["lost_by"], fwd["gained_by"])
    assert (rev["gainers"], rev["max_gained"], rev["max_gained_node"]) == (fwd["losers"], fwd["max_lost"],
                                                                          fwd["max_lost_node"])
    # a snapshot compared with itself
    for r in (clocks[0], clocks[-1]):
        assert nothing_moved(S.ownership_moved(snaps[r], snaps[r]), n), (name, r)
    # the last comparison: with the simulation as it is now
    first, last = clocks[0], clocks[-1]
    now = S.ownership_moved(snaps[first])
    check(now, want[(first, last)], (name, shards, "now"))
    assert same(now, S.ownership_moved(snaps[first], snaps[last]))
    for s in snaps.values():
        s.close()
    S.close()


def test_movement_through_leave_and_rejoin(rp):
    """Node 9 leaves at round 5 and rejoins at round 22.  Snapshots before the
    leave, the round after it (the leaver's ring lacks itself: it claims
    nothing and is a claimant with no arcs) and once every view agrees again
    after the rejoin, against the brute force."""
    n, leaver = 64, 9
    S = rp.Sim(n, oc.SIM_SEED, leaves={5: [leaver]}, rejoins={22: [leaver]})
    b = device_boundaries(S)
    S.run(4, churn=True)
    before, rows_before, claimed_before = S.ownership_snapshot(), mc.device_rows(S, b), S.ownership()["claimed"]
    S.run(2, churn=True)
    after, rows_after = S.ownership_snapshot(), mc.device_rows(S, b)
    assert S.info(leaver)["dead"] == 0 and after.stats["claimants"] == n
    got = S.ownership_moved(before, after)
    check(got, brute(S, b, rows_before, rows_after, 4, 6), "leave")
    assert got["lost_by"][leaver] == claimed_before[leaver] > 0 and got["gained_by"][leaver] == 0
    assert got["transition"][1][0] > 0  # (orphaned until the others drop it)
    agreed = None
    for r in range(7, 61):
        S.round(churn=True)
        own = S.ownership()
        if r > 23 and own["claimed"][leaver] > 0 and own["measure"][1] == ALL:
            agreed = r
            break
    assert agreed
    rows_agreed = mc.device_rows(S, b)
    got = S.ownership_moved(after)
    check(got, brute(S, b, rows_after, rows_agreed, 6, agreed), "rejoin")
    assert got["gained_by"][leaver] == own["claimed"][leaver] and got["lost_by"][leaver] == 0
    check(S.ownership_moved(before), brute(S, b, rows_before, rows_agreed, 4, agreed), "leave and rejoin")
    for s in (before, after):
        s.close()
    S.close()


def test_movement_of_sparse_views(rp):
    """Views set directly, 40 nodes: every node's ring holds itself and two
    others (long arcs, one wrapping arc per view), node 39 knows only itself
    (everything).  Against the same cluster after 10 rounds: every view's
    arcs change, the wrapping one too; node 39 leaves in round 0, so its ring
    goes from itself alone to empty -- everything at both instants."""
    n = 40
    st = np.full((n, n), 3, dtype=np.int32)  # faulty: known, not in the ring
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    for v in range(39):
        st[v, [v, (v + 7) % 39, (v + 19) % 39]] = 1
    st[39, 39] = 1
    S = rp.Sim(n, 3, views=(st, inc), leaves={0: [39]})
    b = device_boundaries(S)
    with S.ownership_snapshot() as first:
        rows_first = mc.device_rows(S, b)
        assert first.stats["measure"][0] == first.stats["measure"][1] == 0 and first.stats["max_claims"] > 2
        S.run(10, churn=False)
        rows_later = mc.device_rows(S, b)
        want = brute(S, b, rows_first, rows_later, 0, 10)
        assert want["gainers"] > 0 and want["losers"] > 0
        assert want["gained_by"][39] == want["lost_by"][39] == 0
        # (the wrap, interval 0, changes hands in some view)
        assert any((mc.unpacked(rows_first[v], len(b))[0] != mc.unpacked(rows_later[v], len(b))[0]) for v in range(39))
        got = S.ownership_moved(first)
        check(got, want, "sparse")
        with S.ownership_snapshot() as later:
            check(S.ownership_moved(later, first), brute(S, b, rows_later, rows_first, 10, 0), "sparse, reversed")
    S.close()


def test_movement_at_1400_nodes(rp):
    """140,000 points: 69 scan tiles of 2,048 intervals, two steps of the
    64-tile partial scan; 14 fail-stops, a snapshot before them and one after
    the drain, against the brute force with bit-packed rows."""
    n = 1400
    failed = list(range(50, 1400, 100))
    assert len(failed) == 14
    S = rp.Sim(n, oc.SIM_SEED, failures={3: failed})
    S.run(2, churn=True)
    b = device_boundaries(S)
    assert len(b) > 64 * 2048
    before, rows_before = S.ownership_snapshot(), mc.device_rows(S, b)
    S.run(1, churn=True)
    S.run(40, churn=False)
    rows_after = mc.device_rows(S, b)
    want = brute(S, b, rows_before, rows_after, 2, 43)
    assert want["losers"] == 14 and want["gainers"] > 0 and want["handed_off"] > 0
    check(S.ownership_moved(before), want, "n1400")
    before.close()
    S.close()


def test_movement_cache_tracks_changes(rp):
    n, kw, _, _ = oc.SCENARIOS["failstop"]
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(27, churn=True)
    snap = S.ownership_snapshot()
    S.run(2, churn=True)
    S.enable_timing(True, stages=["other"])
    first = S.ownership_moved(snap)
    launches = S.kernel_times()["other"][1]
    again = S.ownership_moved(snap)
    # (no call between: the comparison's launches, timed as one span, and no census)
    assert S.kernel_times()["other"][1] == launches + 1
    assert same(first, again) and first["gained_by"].sum() > 0
    S.ownership()
    assert S.kernel_times()["other"][1] == launches + 1  # (the census a comparison ran is the cached one)
    S.round(churn=True)
    base = S.kernel_times()["other"][1]
    third = S.ownership_moved(snap)
    assert S.kernel_times()["other"][1] == base + 2  # (a recording census and a comparison)
    assert third["to_clock"] == 30 and third["gained_by"].sum() > first["gained_by"].sum()
    assert third["transition"] != first["transition"]
    # a plain census after the next round records no arcs: the comparison that follows runs a recording one
    S.round(churn=True)
    S.ownership()
    base = S.kernel_times()["other"][1]
    fourth = S.ownership_moved(snap)
    assert S.kernel_times()["other"][1] == base + 2 and fourth["to_clock"] == 31
    with S.ownership_snapshot() as now:
        assert same(fourth, S.ownership_moved(snap, now))
    snap.close()
    S.close()


def test_movement_arguments(rp):
    from ringpop_amd._lib import MovementStats, lib, ptr
    n = 32
    S = rp.Sim(n, oc.SIM_SEED, failures={2: [5]})
    S.run(1, churn=True)
    snap = S.ownership_snapshot()
    S.run(40, churn=True)
    full = S.ownership_moved(snap)
    assert full["lost_by"][5] > 0 and full["handed_off"] > 0
    moved = lib().rp_sim_ownership_moved
    st = MovementStats()
    short = np.full(n - 1, 77, dtype=np.uint64)
    for g, l in ((short, None), (None, short), (short, short)):
        assert moved(S._h, snap._h, None, ctypes.byref(st), ptr(g), ptr(l), n - 1) == -1  # RP_ERR_INVALID
    assert (short == 77).all() and st.same_set == 0 and st.intervals == 0
    assert moved(S._h, snap._h, None, ctypes.byref(st), None, None, 0) == 0  # gained = lost = NULL
    assert st.as_dict() == {k: full[k] for k in FIELDS} and list(st.reserved) == [0] * 8
    lost = np.zeros(n, dtype=np.uint64)
    assert moved(S._h, snap._h, None, ctypes.byref(st), None, ptr(lost), n) == 0
    assert np.array_equal(lost, full["lost_by"])
    assert moved(S._h, None, None, ctypes.byref(st), None, None, 0) == -1
    assert moved(S._h, snap._h, None, None, None, None, 0) == -1
    # a snapshot of another simulation, as either side
    T = rp.Sim(n, oc.SIM_SEED)
    T.run(1, churn=True)
    other = T.ownership_snapshot()
    for f, t in ((other, None), (snap, other), (other, snap)):
        with pytest.raises(rp.RingpopError) as ei:
            S.ownership_moved(f, t)
        assert ei.value.code == -1, (f, t)
    # destroyed in either order
    T.close()
    other.close()
    snap.close()
    snap.close()
    S.close()


def test_snapshot_across_load_addresses(rp):
    """New addresses are new points: a snapshot of the old ones is refused."""
    n = 24
    S = rp.Sim(n, oc.SIM_SEED)
    old = S.ownership_snapshot()
    assert old.clock == 0 and old.stats["measure"][1] == ALL
    S.load_addresses(sorted("10.9.%d.%d:3000" % (i // 7, i) for i in range(n)))
    for f, t in ((old, None), (old, old)):
        with pytest.raises(rp.RingpopError) as ei:
            S.ownership_moved(f, t)
        assert ei.value.code == -6, (f, t)  # RP_ERR_STATE
    new = S.ownership_snapshot()
    with pytest.raises(rp.RingpopError) as ei:
        S.ownership_moved(new, old)
    assert ei.value.code == -6
    S.run(2, churn=True)
    assert nothing_moved(S.ownership_moved(new), n)
    old.close()
    new.close()
    S.close()


def test_movement_on_loop_ranks(rp):
    """A rank of a loop cluster holds its own nodes' views only: unsupported."""
    from ringpop_amd._lib import MovementStats, lib
    from ringpop_amd.sim import Loop
    G, n, rounds = 2, 64, 3
    whole = rp.Sim(n, oc.SIM_SEED)
    snap = whole.ownership_snapshot()
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
    st = MovementStats()
    for S in sims:
        with pytest.raises(rp.RingpopError) as ei:
            S.ownership_snapshot()
        assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
        assert lib().rp_sim_ownership_moved(S._h, snap._h, None, ctypes.byref(st), None, None, 0) == -4
    for S in sims:
        S.close()
    loop.close()
    snap.close()
    whole.close()


def test_census_unchanged_beside_snapshots(rp):
    """Sim.ownership() and ownership_at() with snapshots live and comparisons
    made between them equal the expectation of the census' own cases."""
    name = "partition"
    n, kw, _, _ = oc.SCENARIOS[name]
    b, want = oc.expected(name)
    q = oc.queries(b)
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    snaps = []
    for r in range(1, 37):
        S.round(churn=True)
        if r % 3 == 0:
            if r % 2:
                snaps.append(S.ownership_snapshot())  # (before the census: it reads the recording run's results)
            got = S.ownership()
            if r % 2 == 0:
                snaps.append(S.ownership_snapshot())  # (after it: the census runs again, recording)
            S.ownership_moved(snaps[0])
            again = S.ownership()
            e = want[r]
            for g in (got, again):
                assert all(g[k] == e[k] for k in ("measure", "claimants", "intervals", "max_claims", "max_claims_hash"))
                assert np.array_equal(g["claimed"], e["claimed"]), r
            assert np.array_equal(S.ownership_at(q), oc.claims_at(b, e["claims"], q)), r
            assert snaps[-1].stats["measure"] == e["measure"]
    assert len(snaps) == 12
    for s in snaps:
        s.close()
    S.close()
