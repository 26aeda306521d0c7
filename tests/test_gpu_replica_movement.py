"""Replica-set movement on the GPU (rp_replication_snapshot_* /
rp_sim_replication_moved / rp_sim_replication_moved_at) against
the plain definition: per instant and claimant v, L = ring_lookup(v, b) over
all boundaries b (the per-view kernel, pinned to the oracle), and v holds
interval i at R iff L[0] < 0 or v is in preference(L, R)[i, :R]
(tests/replication_cases.py).  Two instants' rows go through
movement_cases.movement(); the classes against R and the kept_none measures
are restated here.  The per-key query is also checked against two holders
queries, which never touch a snapshot."""
import ctypes
import threading

import numpy as np
import pytest

import movement_cases as mc
import ownership_cases as oc
import replication_cases as rc

pytestmark = pytest.mark.gpu

ALL = 1 << 32
RS = (2, 3, 8)
SHARED = tuple(k for k in mc.SCALARS if k != "handed_off")  # the fields rp_movement_stats has too
FIELDS = ("transition", "kept_none", "kept_none_regained", "replicas") + SHARED


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def held_rows(S, b, rs=RS):
    """{R: {claimant v: its bit-packed held row}} of the simulation as it stands; L is computed once per view."""
    out = {R: {} for R in rs}
    for v in range(S.n):
        if S.info(v)["dead"] == 0:
            L = S.ring_lookup(v, b)
            pref = None if L[0] < 0 else rc.preference(L, max(rs))[0]  # (None: an empty ring, everything)
            for R in rs:
                out[R][v] = np.packbits(np.ones(len(b), dtype=bool) if pref is None else (pref[:, :R] == v).any(axis=1))
    return out


def matrix(rows, n, npts):
    M = np.zeros((n, npts), dtype=bool)
    for v, row in rows.items():
        M[v] = mc.unpacked(row, npts)
    return M


def expect(b, frm, to, n, R, fc, tc):
    """movement() of the two instants' rows, with the issue's classes against R and its kept_none measures."""
    e = mc.movement(b, frm, to, n, fc, tc)
    ln, F, T = oc.lengths(b), matrix(frm, n, len(b)), matrix(to, n, len(b))
    g, l, cf, ct = (T & ~F).sum(axis=0), (F & ~T).sum(axis=0), F.sum(axis=0), T.sum(axis=0)
    a, c = (cf >= R).astype(int) + (cf > R), (ct >= R).astype(int) + (ct > R)
    none = (cf > 0) & (l == cf)
    e.update(transition=[[int(ln[(a == i) & (c == j)].sum()) for j in range(3)] for i in range(3)],
             kept_none=int(ln[none].sum()), kept_none_regained=int(ln[none & (g > 0)].sum()), replicas=R, g=g, l=l, F=F, T=T)
    return e


def check(got, want, where):
    for k in FIELDS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ("gained_by", "lost_by"):
        assert got[k].dtype == np.uint64
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (where, k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    assert sum(sum(r) for r in got["transition"]) == ALL, where


def lists_of(M):
    """Per row of a bool [keys, n]: the set's ids ascending, the rest -1."""
    n = M.shape[1]
    w = np.sort(np.where(M, np.arange(n), n), axis=1)
    w[w == n] = -1
    return w.astype(np.int32)


def check_at(S, frm, to, q, F, T, where, cap=None):
    """moved_at for keys q against bool [keys, n] holder matrices of the two instants."""
    cap = S.n if cap is None else cap
    gain, loss = T & ~F, F & ~T
    gl, ll, ng, nl = S.replication_moved_at(frm, to, q, cap=cap)
    assert gl.dtype == ll.dtype == np.int32 and ng.dtype == nl.dtype == np.uint32 and gl.shape == ll.shape == (len(q), cap)
    for got, cnt, M, what in ((gl, ng, gain, "gainers"), (ll, nl, loss, "losers")):
        bad = np.flatnonzero((got != lists_of(M)[:, :cap]).any(axis=1) | (cnt != M.sum(axis=1)))
        assert bad.size == 0, (where, what, q[bad[:4]], got[bad[:4]], cnt[bad[:4]], M[bad[:4]].sum(axis=1))
    return ng, nl


def at(b, q):
    return np.searchsorted(b, q, side="left") % len(b)


@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_replica_movement_matches_definition(rp, name, shards):
    n, kw, rounds, _ = oc.SCENARIOS[name]
    clocks, todo = mc.CLOCKS[name], mc.pairs(name)
    S = rp.Sim(n, oc.SIM_SEED, **kw, shards=shards)
    b = oc.boundaries([S.address(v) for v in range(n)], kw.get("replica_hash_shift", 0))
    q = oc.queries(b)
    snaps, rows = {}, {}
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        if r in clocks:
            rows[r] = held_rows(S, b)
            for R in RS:  # (taken while the run proceeds, at every R: all stay live)
                snaps[R, r] = s = S.replication_snapshot(R)
                assert (s.clock, s.replicas) == (r, R) and s.stats == {k: v for k, v in S.replication(R).items() if k != "held"}
    first, last = clocks[0], clocks[-1]
    for R in RS:
        want = {(f, t): expect(b, rows[f][R], rows[t][R], n, R, f, t) for f, t in todo + [(first, first), (last, last)]}
        for (f, t), w in want.items():
            check(S.replication_moved(snaps[R, f], snaps[R, t]), w, (name, shards, R, f, t))
        for r in (first, last):  # a snapshot against itself
            assert want[r, r]["same_set"] == ALL and want[r, r]["gained"] == want[r, r]["kept_none"] == 0
        # the reference moves: replicas gained and lost in some pair, and at R = 3 more than one class changes
        assert any(w["gained"] > 0 and w["lost"] > 0 for w in want.values()), (name, R)
        off = {(i, j) for w in want.values() for i in range(3) for j in range(3) if i != j and w["transition"][i][j]}
        print(name, R, "off-diagonal cells:", sorted(off), "kept_none:", {k: w["kept_none"] for k, w in want.items()})
        assert R != 3 or len(off) >= 2, (name, off)
        # (no pair of these scenarios has kept_none > 0 at R >= 3; at R = 2 the fail-stops and the joins do)
        assert (name, R) not in (("failstop", 2), ("join", 2)) or any(w["kept_none"] > 0 for w in want.values())
        # the last pair against the simulation as it is now, and the first -> last pair key by key
        f = clocks[-2]
        check(S.replication_moved(snaps[R, f]), want[f, last], (name, shards, R, "now"))
        w = want[first, last]
        ng, nl = check_at(S, snaps[R, first], None, q, w["F"].T[at(b, q)], w["T"].T[at(b, q)], (name, shards, R))
        assert np.array_equal(ng, w["g"][at(b, q)]) and np.array_equal(nl, w["l"][at(b, q)])
    for s in snaps.values():
        s.close()
    S.close()


@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_one_replica_is_ownership_movement(rp, name):
    n, kw, rounds, _ = oc.SCENARIOS[name]
    clocks = mc.CLOCKS[name]
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    own, rep = {}, {}
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        if r in clocks:
            own[r], rep[r] = S.ownership_snapshot(), S.replication_snapshot(1)
    for f, t in mc.pairs(name):
        a, e = S.replication_moved(rep[f], rep[t]), S.ownership_moved(own[f], own[t])
        assert all(a[k] == e[k] for k in SHARED + ("transition",)), (name, f, t)  # (under / exact / over R = 1 is 0 / 1 / 2+)
        assert np.array_equal(a["gained_by"], e["gained_by"]) and np.array_equal(a["lost_by"], e["lost_by"])
        assert a["kept_none"] >= e["handed_off"] and a["kept_none"] >= a["kept_none_regained"], (name, f, t)
    # fail-stop 1 -> 45: what the four stopped nodes claimed, and nobody else (DESIGN.md §15's 375,943,841)
    assert name != "failstop" or S.replication_moved(rep[1], rep[45])["kept_none"] == 375943841
    for s in list(own.values()) + list(rep.values()):
        s.close()
    S.close()


@pytest.mark.parametrize("R", [2, 3, 4])
def test_replica_movement_of_sparse_views(rp, R):
    """test_gpu_replication's sparse cluster: 40 nodes, rings of three servers
    (long arcs, one wrapping arc per view, the walks that walk_wave ends), node
    39 alone and, a round later, with an empty ring: everything both times.
    From R = 3 on every member of a ring holds everything.  Ten rounds later
    every view has grown."""
    n = 40
    st = np.full((n, n), 3, dtype=np.int32)  # faulty: known, not in the ring
    inc = np.tile(1434401518824 + np.arange(n, dtype=np.int64), (n, 1))
    for v in range(39):
        st[v, [v, (v + 7) % 39, (v + 19) % 39]] = 1
    st[39, 39] = 1
    S = rp.Sim(n, 3, views=(st, inc), leaves={0: [39]})
    b = oc.boundaries([S.address(v) for v in range(n)])
    q = oc.queries(b)
    snaps, rows = {}, {}
    for r in (0, 1, 10):
        if r:
            S.run(r - S.rounds(), churn=False)
        snaps[r], rows[r] = S.replication_snapshot(R), held_rows(S, b, (R,))[R]
        assert mc.unpacked(rows[r][39], len(b)).all()
    assert S.info(39)["ring_servers"] == 0
    for f, t in ((0, 1), (0, 10), (10, 0), (1, 10)):
        w = expect(b, rows[f], rows[t], n, R, f, t)
        check(S.replication_moved(snaps[f], snaps[t]), w, ("sparse", R, f, t))
        assert w["gained_by"][39] == w["lost_by"][39] == 0
        check_at(S, snaps[f], snaps[t], q, w["F"].T[at(b, q)], w["T"].T[at(b, q)], ("sparse", R, f, t))
    assert w["gainers"] + w["losers"] > 0
    check(S.replication_moved(snaps[0]), expect(b, rows[0], rows[10], n, R, 0, 10), ("sparse", R, "now"))
    for s in snaps.values():
        s.close()
    S.close()


@pytest.mark.parametrize("shards", [1, 4])
def test_moved_at_against_two_holders_queries(rp, shards):
    """test_gpu_holders' 200 nodes (ten fail-stops at round 3, a join at round
    25): six whole tiles of 32 nodes and one of 8; on 4 shards of 50 nodes the
    tiles span shards.  60,002 keys: on, below and above every point and both
    ends of the hash space.  The reference is holders_at before and after."""
    n, R = 200, 3
    S = rp.Sim(n, oc.SIM_SEED, failures={3: list(range(7, 200, 19))[:10]}, joins=[(25, 150, [0, 1])], shards=shards)
    S.run(2, churn=True)
    b = oc.boundaries([S.address(v) for v in range(n)])
    q = oc.queries(b)
    assert len(q) % 64 != 0

    def holders():
        ids, _ = S.holders_at(R, q, cap=n)
        M = np.zeros((len(q), n + 1), dtype=bool)
        M[np.arange(len(q))[:, None], ids] = True  # (-1, an unused slot: the spare column)
        return M[:, :n]

    before, F = S.replication_snapshot(R), holders()
    S.run(1, churn=True)
    S.run(24, churn=False)
    T = holders()
    assert (T & ~F).any() and (F & ~T).any() and (T & ~F)[:, 150].any()
    ng, nl = check_at(S, before, None, q, F, T, ("n200", shards))
    with S.replication_snapshot(R) as after:
        for cap in (0, 1):
            assert check_at(S, before, after, q, F, T, ("n200", shards, cap), cap=cap)[0].sum() == ng.sum()
        # null lists: the counts alone, each list alone
        from ringpop_amd._lib import lib, ptr
        call, rows, cg, cl = lib().rp_sim_replication_moved_at, np.full((len(q), 2), 77, dtype=np.int32), np.zeros_like(ng), np.zeros_like(nl)
        assert call(S._h, before._h, after._h, ptr(q), len(q), 2, None, None, ptr(cg), ptr(cl)) == 0
        assert np.array_equal(cg, ng) and np.array_equal(cl, nl)
        assert call(S._h, before._h, after._h, ptr(q), len(q), 2, None, ptr(rows), ptr(cg), ptr(cl)) == 0
        assert np.array_equal(rows, lists_of(F & ~T)[:, :2])
    before.close()
    S.close()


def test_replica_movement_plumbing(rp):
    from ringpop_amd._lib import ReplicaMovementStats, lib, ptr
    from ringpop_amd.sim import Loop
    n, kw, _, _ = oc.SCENARIOS["failstop"]
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(27, churn=True)
    own_snap = S.ownership_snapshot()
    s2, s3 = S.replication_snapshot(2), S.replication_snapshot(3)
    S.run(2, churn=True)
    # the cache, by the timed spans: a comparison is one, a recording census one, a snapshot's copies one
    S.enable_timing(True, stages=["other"])
    spans = lambda: S.kernel_times()["other"][1]
    base, first = spans(), S.replication_moved(s3)
    assert spans() == base + 2 and first["gained"] > 0 and first["to_clock"] == 29
    again = S.replication_moved(s3)
    assert spans() == base + 3 and all(np.array_equal(first[k], again[k]) for k in first)
    S.replication(3)  # (the census a comparison ran is the cached one)
    t3 = S.replication_snapshot(3)
    assert spans() == base + 4
    S.replication_moved(s2)  # another R: a recording census at 2
    assert spans() == base + 6
    S.round(churn=True)
    S.replication(3)  # a plain census records no arcs: the comparison that follows runs a recording one
    base = spans()
    S.replication_moved(s3)
    S.replication_moved_at(s3, None, np.arange(5, dtype=np.uint32))  # (one chunk: one span)
    assert spans() == base + 3
    S.enable_timing(False)
    # arguments
    moved, st, short = lib().rp_sim_replication_moved, ReplicaMovementStats(), np.full(n - 1, 77, dtype=np.uint64)
    assert moved(S._h, s3._h, t3._h, ctypes.byref(st), ptr(short), None, n - 1) == -1 and (short == 77).all()  # cap < n
    assert moved(S._h, s3._h, s2._h, ctypes.byref(st), None, None, 0) == -1  # another R
    assert moved(S._h, None, None, ctypes.byref(st), None, None, 0) == moved(S._h, s3._h, None, None, None, None, 0) == -1
    assert st.intervals == 0 and moved(S._h, s3._h, t3._h, ctypes.byref(st), None, None, 0) == 0
    assert st.as_dict() == {k: again[k] for k in FIELDS} and list(st.reserved) == [0] * 6
    for bad in (0, 9):
        with pytest.raises(rp.RingpopError) as ei:
            S.replication_snapshot(bad)
        assert ei.value.code == -1
    T = rp.Sim(n, oc.SIM_SEED)
    other = T.replication_snapshot(3)
    for f, t in ((other, None), (s3, other), (other, s3)):
        with pytest.raises(rp.RingpopError) as ei:
            S.replication_moved(f, t)
        assert ei.value.code == -1, (f, t)  # RP_ERR_INVALID: a snapshot of another simulation
        with pytest.raises(rp.RingpopError) as ei:
            S.replication_moved_at(f, t, np.zeros(1, dtype=np.uint32))
        assert ei.value.code == -1
    T.close()  # destroyed in either order
    other.close()
    # the censuses and an ownership snapshot beside live replication snapshots return what they returned
    with S.ownership_snapshot() as later:
        back = S.ownership_moved(later, own_snap)
    assert back["to_clock"] == 27 and back["gained"] + back["lost"] > 0
    U = rp.Sim(n, oc.SIM_SEED, **kw)  # (the same run with no snapshot taken)
    U.run(30, churn=True)
    for got, want in ((S.replication(3), U.replication(3)), (S.replication(1), U.replication(1)), (S.ownership(), U.ownership())):
        assert all(np.array_equal(got[k], want[k]) for k in want)
    U.close()
    for s in (s2, s3, t3, own_snap):
        s.close()
    s3.close()
    S.close()
    # new addresses are new points: a snapshot of the old ones is refused before any kernel sees its indices
    V = rp.Sim(24, oc.SIM_SEED)
    old = V.replication_snapshot(3)
    V.load_addresses(sorted("10.9.%d.%d:3000" % (i // 7, i) for i in range(24)))
    new = V.replication_snapshot(3)
    for call in (lambda: V.replication_moved(old), lambda: V.replication_moved(old, old), lambda: V.replication_moved(new, old),
                 lambda: V.replication_moved_at(old, None, np.zeros(1, dtype=np.uint32))):
        with pytest.raises(rp.RingpopError) as ei:
            call()
        assert ei.value.code == -6  # RP_ERR_STATE
    assert V.replication_moved(new)["same_set"] == ALL
    V.close()
    old.close()
    new.close()
    # a rank of a loop cluster holds its own nodes' views only
    whole = rp.Sim(64, oc.SIM_SEED)
    snap = whole.replication_snapshot(3)
    loop = Loop(2)
    sims = [rp.Sim(64, oc.SIM_SEED, shards=2, rank=r, loop=loop) for r in range(2)]
    th = [threading.Thread(target=X.run, args=(3,), kwargs={"churn": True}) for X in sims]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for X in sims:
        with pytest.raises(rp.RingpopError) as ei:
            X.replication_snapshot(3)
        assert ei.value.code == -4  # RP_ERR_UNSUPPORTED
        assert lib().rp_sim_replication_moved(X._h, snap._h, None, ctypes.byref(st), None, None, 0) == -4
        X.close()
    loop.close()
    snap.close()
    whole.close()
