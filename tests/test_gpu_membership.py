"""The membership census on the GPU (rp_sim_membership) against
its definition written out in numpy over Sim.view(v) of every node and
Sim.info(v)["dead"] (both pinned to the oracle by test_gpu_parity.py): the
viewers are the nodes with dead == 0, vs = incarnation << 3 | status, and per
member the status counts, the 64-bit maximum and its multiplicity run over the
viewers' rows.  Everything is compared with exact equality."""
import ctypes
import threading

import numpy as np
import pytest

import ownership_cases as oc

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def reference(S):
    n = S.n
    dead = np.array([S.info(v)["dead"] for v in range(n)])
    vs = np.zeros((n, n), dtype=np.uint64)
    for v in range(n):
        st, inc = S.view(v)
        vs[v] = inc << np.uint64(3) | st.astype(np.uint64)
    V = vs[dead == 0]
    top = V.max(axis=0) if len(V) else np.zeros(n, dtype=np.uint64)
    seen = np.stack([((V & np.uint64(7)) == s).sum(axis=0) for s in range(5)], axis=1).astype(np.uint32)
    at_top = (V == top).sum(axis=0).astype(np.uint32)
    behind = np.where(dead == 0, (vs != top).sum(axis=1), 0).astype(np.uint32)
    lag = len(V) - at_top.astype(np.int64)
    return {"viewers": len(V), "members": n, "agreed": int((lag == 0).sum()), "cells_behind": int(lag.sum()),
            "max_behind_member": int(lag.max()), "max_behind_member_id": int(lag.argmax()),
            "laggards": int((behind > 0).sum()), "max_behind_viewer": int(behind.max()),
            "max_behind_viewer_id": int(behind.argmax()),
            "undetected": int(seen[dead == 1, 1].sum()), "suspected_dead": int(seen[dead == 1, 2].sum()),
            "false_faulty": int(seen[dead == 0, 3].sum()), "false_suspect": int(seen[dead == 0, 2].sum()),
            "unknown": int(seen[dead == 0, 0].sum()),
            "seen": seen, "top_status": (top & np.uint64(7)).astype(np.uint8), "top_incarnation": top >> np.uint64(3),
            "at_top": at_top, "behind": behind, "dead": dead}


def check(S, where):
    want, got = reference(S), S.membership()
    assert got["seen"].shape == (S.n, 5) and got["seen"].dtype == np.uint32 and got["top_status"].dtype == np.uint8, where
    for k in got:
        assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    assert (got["seen"].sum(axis=1) == got["viewers"]).all() and got["cells_behind"] == int(got["behind"].sum()), where
    return got, want


@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_membership_in_scenarios(rp, name, shards):
    """48, 32 and 40 members: a ragged column tile, 64 a whole wave's; fail-stopped
    and not yet joined rows, absent cells (join); on 4 shards four one-slab folds."""
    n, kw, rounds, _ = oc.SCENARIOS[name]
    S = rp.Sim(n, oc.SIM_SEED, **kw, shards=shards)
    non_viewers = absent = 0
    for r in range(rounds + 1):
        if r:
            S.round(churn=True)
        if r in oc.checkpoints(name):
            got, want = check(S, (name, shards, r))
            non_viewers += int((want["dead"] != 0).sum())
            absent += int(got["seen"][:, 0].sum())
    assert name == "partition" or non_viewers > 0
    assert name != "join" or absent > 0
    S.close()


def test_membership_through_leave_and_rejoin(rp):
    """Node 9 leaves at round 5 and rejoins at round 22: status leave in the
    columns, and a node that has left is still a viewer."""
    n, leaver = 64, 9
    S = rp.Sim(n, oc.SIM_SEED, leaves={5: [leaver]}, rejoins={22: [leaver]})
    left = False
    for r in range(1, 31):
        S.round(churn=True)
        if r in (5, 6, 7, 12, 21, 22, 23, 24, 30):
            got, _ = check(S, ("leave", r))
            assert got["viewers"] == n
            left = left or (got["top_status"][leaver] == 4 and got["seen"][leaver, 4] > 0)
    assert left
    S.close()


@pytest.mark.parametrize("shards", [1, 4])
@pytest.mark.parametrize("n", [72, 2112])
def test_membership_of_set_views(rp, n, shards):
    """Every row starts from one draw per member and about a tenth of the cells
    are drawn again, over all five statuses and four incarnations: B, B + 1
    (the low bits alone differ) and both + 2^40 (only bits above 32 of the
    packed value differ), so that many viewers tie at a column's top and every
    row lags on some members; nobody but itself knows member 13.  72 nodes: one shard has
    two slabs of 36 rows.  2,112 nodes: the row pass stages top[] in two LDS
    tiles (2,048 members, then a ragged 64), takes the first in four steps of
    512 cells with eight loads in flight and the second in its 64-cell tail;
    nine column tiles, four slabs of 528 rows (four shards: two of 264 each)."""
    B = 1434401518824
    rng = np.random.default_rng(20)

    def draw(shape, lowest):  # packed cells
        return (B + rng.integers(0, 2, size=shape) + (rng.integers(0, 2, size=shape) << 40)) << 3 | rng.integers(
            lowest, 5, size=shape)

    # (a second draw replaces a cell where it is older; in every tenth column also where it is newer)
    vs, new = np.tile(draw(n, 1), (n, 1)), draw((n, n), 0)
    again = (rng.random((n, n)) < 0.15) & ((new < vs) | (np.arange(n) % 10 == 0))
    vs[again] = new[again]
    st, inc = (vs & 7).astype(np.int32), vs >> 3
    st[:, 13] = 0
    st[np.arange(n), np.arange(n)] = 1
    inc[st == 0] = 0
    S = rp.Sim(n, 3, views=(st, inc), shards=shards)
    got, _ = check(S, ("set views", n, shards))
    assert got["seen"][13].tolist() == [n - 1, 1, 0, 0, 0] and got["at_top"][13] == 1
    assert (got["seen"] > 0).any(axis=0).all() and (got["at_top"] > 1).sum() > n // 2
    assert got["laggards"] == n and 0 < got["behind"].min() and got["behind"].max() < n // 2
    S.close()


@pytest.mark.parametrize("shards", [1, 4])
def test_membership_over_several_tiles_and_slabs(rp, shards):
    """264 nodes.  A column tile is 256 members: tiles of 256 and 8.  The slab
    rule: a shard's rows fall into min(64, n / (512 x shards)) slabs of equal
    height, at least two once it has more than 64 rows -- one shard: two slabs
    of 132 rows; four shards of 66 rows: two slabs of 33 each, eight to fold.
    Ten fail-stops, and a node that joins two rounds before the end, known to
    few views yet: the cluster has not converged."""
    n = 264
    S = rp.Sim(n, oc.SIM_SEED, failures={3: list(range(7, 200, 19))[:10]}, joins=[(25, 150, [0, 1])], shards=shards)
    S.run(3, churn=True)
    S.run(24, churn=False)
    got, _ = check(S, ("n264", shards))
    assert got["agreed"] < n and got["laggards"] > 0 and got["viewers"] == n - 10
    S.close()


def test_membership_arguments_and_isolation(rp):
    from ringpop_amd._lib import MembershipStats, lib, ptr
    n, kw, _, _ = oc.SCENARIOS["failstop"]
    S, T = rp.Sim(n, oc.SIM_SEED, **kw), rp.Sim(n, oc.SIM_SEED, **kw)
    for r in range(12):
        S.round(churn=True)
        T.round(churn=True)
        S.membership()
    assert np.array_equal(S.checksums(), T.checksums()) and S.totals() == T.totals()
    T.close()
    full, call = S.membership(), lib().rp_sim_membership
    top = full["top_incarnation"] << np.uint64(3) | full["top_status"].astype(np.uint64)
    want = [full["seen"], top, full["at_top"], full["behind"]]
    # each array NULL in turn, and the stats: the rest is unchanged
    for skip in range(5):
        st = MembershipStats()
        out = [np.zeros_like(w) for w in want]
        args = [None if i == skip else ptr(o) for i, o in enumerate(out)]
        assert call(S._h, None if skip == 4 else ctypes.byref(st), *args, n) == 0
        assert all(i == skip or np.array_equal(o, w) for i, (o, w) in enumerate(zip(out, want))), skip
        assert skip == 4 or all(full[k] == v for k, v in st.as_dict().items()), skip
    # refused calls write nothing
    st, out = MembershipStats(), [np.full_like(w, 77) for w in want]
    assert call(S._h, ctypes.byref(st), *map(ptr, out), n - 1) == -1  # RP_ERR_INVALID
    assert call(None, ctypes.byref(st), *map(ptr, out), n) == -1
    assert call(S._h, None, None, None, None, None, n) == -1
    assert all((o == 77).all() for o in out) and st.viewers == 0 and st.members == 0
    # the censuses' caches stay: no span is timed for the second ownership() and replication(3)
    S.enable_timing(True, stages=["other"])
    before = S.replication(3), S.ownership()
    spans = S.kernel_times()["other"][1]
    S.membership()
    assert S.kernel_times()["other"][1] == spans + 4  # (column pass, combine, row pass, finish)
    after = S.replication(3), S.ownership()
    assert S.kernel_times()["other"][1] == spans + 4
    for x, y in zip(before, after):
        assert all(np.array_equal(x[k], y[k]) for k in x)
    S.enable_timing(False)
    S.close()
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
        out = [np.full(320, 77, dtype=np.uint32), np.full(64, 77, dtype=np.uint64), np.full(64, 77, dtype=np.uint32),
               np.full(64, 77, dtype=np.uint32)]
        assert call(X._h, ctypes.byref(st), *map(ptr, out), 64) == -4  # RP_ERR_UNSUPPORTED
        assert all((o == 77).all() for o in out) and st.viewers == 0
        X.close()
    loop.close()
