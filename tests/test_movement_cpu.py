"""CPU tests of ownership movement: the API exists at every
layer, and the expectation restated from the oracle (tests/movement_cases.py)
shows, pair by pair, the kinds of movement the GPU comparison relies on, so
that none of it passes vacuously."""
import ctypes
import os
import re

import numpy as np
import pytest

import movement_cases as mc
import ownership_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 1 << 32


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_movement_api_at_every_layer():
    header = re.sub(r"\s+", " ", read("include", "ringpop_hip.h"))
    for decl in ("typedef struct rp_ownership_snapshot rp_ownership_snapshot;",
                 "int rp_ownership_snapshot_create(rp_sim *sim, rp_ownership_snapshot **out);",
                 "int rp_ownership_snapshot_info(const rp_ownership_snapshot *snap, rp_ownership_stats *stats, "
                 "uint64_t *clock);",
                 "int rp_ownership_snapshot_destroy(rp_ownership_snapshot *snap);",
                 "int rp_sim_ownership_moved(rp_sim *sim, const rp_ownership_snapshot *from, "
                 "const rp_ownership_snapshot *to, rp_movement_stats *stats, uint64_t *gained, uint64_t *lost, "
                 "size_t cap);", "} rp_movement_stats;"):
        assert decl in header, decl
    from ringpop_amd import _lib, build, sim
    L = ctypes.CDLL(build.build())
    names = ("rp_ownership_snapshot_create", "rp_ownership_snapshot_info", "rp_ownership_snapshot_destroy",
             "rp_sim_ownership_moved")
    assert all(hasattr(L, s) and s in _lib.SIGNATURES for s in names)
    L.rp_abi_version.restype = ctypes.c_int
    assert L.rp_abi_version() == 2
    assert ctypes.sizeof(_lib.MovementStats) == 256
    assert [f[0] for f in _lib.MovementStats._fields_] == ["transition"] + list(mc.SCALARS) + ["reserved"]
    assert callable(sim.Sim.ownership_snapshot) and callable(sim.Sim.ownership_moved)
    assert all(hasattr(sim.OwnershipSnapshot, a) for a in ("close", "__enter__", "__exit__"))
    js = read("js", "index.js")
    assert "SimCluster.prototype.ownershipSnapshot = " in js and "SimCluster.prototype.ownershipMoved = " in js
    napi = read("js", "ringpop_napi.c")
    assert 'EXPORT("simOwnershipSnapshot"' in napi and 'EXPORT("simOwnershipMoved"' in napi


def test_pairs():
    assert mc.pairs("shift") == [(1, 20), (20, 28), (28, 40), (1, 40), (28, 20)]
    for name, clocks in mc.CLOCKS.items():
        assert clocks == sorted(clocks) and clocks[-1] == oc.SCENARIOS[name][2]
        assert len(mc.pairs(name)) == len(clocks) + 1


@pytest.mark.parametrize("name", list(mc.CLOCKS))
def test_identities(name):
    b, want, claimed = mc.expected(name)
    n = oc.SCENARIOS[name][0]
    assert sorted(want) == sorted(mc.pairs(name)) and sorted(claimed) == mc.CLOCKS[name]
    for (f, t), e in want.items():
        tr = e["transition"]
        assert sum(sum(r) for r in tr) == ALL and e["intervals"] == len(b), (name, f, t)
        assert (e["from_clock"], e["to_clock"]) == (f, t)
        assert e["gained"] == int(e["gained_by"].astype(object).sum()), (name, f, t)
        assert e["lost"] == int(e["lost_by"].astype(object).sum()), (name, f, t)
        # per node gained - lost is the change of its claimed measure
        d = e["gained_by"].astype(np.int64) - e["lost_by"].astype(np.int64)
        assert np.array_equal(d, claimed[t].astype(np.int64) - claimed[f].astype(np.int64)), (name, f, t)
        assert e["handed_off"] <= tr[1][1] and e["handed_off"] <= min(e["gained"], e["lost"]), (name, f, t)
        assert e["same_set"] <= tr[0][0] + tr[1][1] + tr[2][2], (name, f, t)
        assert (e["max_turnover"] == 0) == (e["same_set"] == ALL) == (e["gained"] + e["lost"] == 0), (name, f, t)
        assert e["max_gained"] == int(e["gained_by"].max()) and e["gainers"] <= n and e["losers"] <= n
        if e["gained"]:
            v = e["max_gained_node"]
            assert e["gained_by"][v] == e["max_gained"] and (e["gained_by"][:v] < e["max_gained"]).all()
        else:
            assert e["max_gained_node"] == 0
    # the reversed pair swaps gained and lost and transposes transition
    f, t = mc.REVERSED[name]
    fwd, rev = want[(t, f)], want[(f, t)]
    assert rev["transition"] == [list(r) for r in zip(*fwd["transition"])]
    assert np.array_equal(rev["gained_by"], fwd["lost_by"]) and np.array_equal(rev["lost_by"], fwd["gained_by"])
    assert (rev["same_set"], rev["handed_off"], rev["max_turnover"]) == (fwd["same_set"], fwd["handed_off"],
                                                                        fwd["max_turnover"])
    assert fwd["gained"] + fwd["lost"] > 0


def test_failstop_pairs():
    _, want, _ = mc.expected("failstop")
    e = want[(1, 3)]
    assert (e["lost"], e["losers"], e["gained"]) == (375943841, 4, 0) and e["transition"][1][0] == 375943841
    for p in ((3, 27), (33, 45)):
        assert want[p]["same_set"] == ALL and want[p]["gained"] == want[p]["lost"] == 0, p
    e = want[(27, 30)]
    assert (e["gained"], e["gainers"]) == (279876300, 44) and e["transition"][0][1] == 279876300
    assert e["transition"][0][0] == 96067541
    e = want[(30, 33)]
    assert (e["gained"], e["gainers"]) == (96067541, 26)
    # the case two censuses cannot see: every hash has one claimant at both clocks
    e = want[(1, 45)]
    assert e["transition"][1][1] == ALL
    assert e["handed_off"] == e["gained"] == e["lost"] == 375943841 and (e["gainers"], e["losers"]) == (44, 4)


def test_partition_pairs():
    _, want, _ = mc.expected("partition")
    assert want[(1, 30)]["transition"][1][2] == 1598205498 and want[(1, 30)]["lost"] == 0
    e = want[(39, 42)]
    assert (e["gained"], e["lost"]) == (490794991, 330164554) and e["max_turnover"] >= 3
    e = want[(42, 45)]
    assert (e["gained"], e["gainers"], e["lost"], e["losers"]) == (1964052905, 58, 1588818099, 59)
    assert e["transition"][2][1] == 1173573753
    assert (want[(45, 50)]["lost"], want[(45, 50)]["losers"]) == (3673024427, 64)
    assert want[(1, 50)]["lost"] == 0 and want[(1, 50)]["transition"][1][2] == 735345601


def test_shift_pairs():
    _, want, _ = mc.expected("shift")
    e = want[(20, 28)]
    assert e["transition"][0] == [1048576, 81788928, 31457280] and e["handed_off"] == 33554432
    e = want[(1, 40)]
    assert (e["handed_off"], e["gained"], e["lost"]) == (80740352, 312475648, 396361728)


def test_join_pairs():
    _, want, _ = mc.expected("join")
    e = want[(0, 3)]
    assert e["same_set"] == ALL and e["gained"] == e["lost"] == 0  # (no claimant before joining)
    e = want[(3, 4)]
    assert (e["gained"], e["gainers"], e["lost"], e["losers"], e["handed_off"]) == (214407899, 2, 29803667, 10, 29141662)
    e = want[(0, 14)]
    assert e["handed_off"] == e["gained"] == e["lost"] == 317870900 and (e["gainers"], e["losers"]) == (3, 37)


def test_movement_of_a_hand_made_ring():
    """Three intervals, interval 0 the wrap: node 0 hands interval 1 to node 1,
    node 2 appears and claims everything, node 3 drops the wrap."""
    b = np.array([5, 9, 0xFFFFFFF0], dtype=np.uint32)

    def rows(d):
        return {v: np.packbits(np.array(r, dtype=bool)) for v, r in d.items()}

    frm = rows({0: [0, 1, 0], 1: [0, 0, 1], 3: [1, 0, 0]})
    to = rows({0: [0, 0, 0], 1: [0, 1, 1], 2: [1, 1, 1], 3: [0, 0, 0]})
    e = mc.movement(b, frm, to, 4, 2, 6)
    w, m = 5 + ALL - 0xFFFFFFF0, 0xFFFFFFF0 - 9
    assert e["gained_by"].tolist() == [0, 4, ALL, 0] and e["lost_by"].tolist() == [4, 0, 0, w]
    assert e["transition"] == [[0, 0, 0], [0, w, 4 + m], [0, 0, 0]]
    assert (e["same_set"], e["handed_off"], e["gainers"], e["losers"]) == (0, w, 2, 2)
    assert (e["max_gained"], e["max_gained_node"], e["max_lost"], e["max_lost_node"]) == (ALL, 2, w, 3)
    assert (e["max_turnover"], e["max_turnover_hash"]) == (3, 9)
