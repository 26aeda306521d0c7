"""CPU tests of the ownership census: the API exists at every
layer, and the expectation restated from the oracle (tests/ownership_cases.py)
produces the classes of every scenario that the GPU comparison relies on, so
that none of it passes vacuously."""
import ctypes
import os
import re

import numpy as np
import pytest

import ownership_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 1 << 32


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_ownership_api_at_every_layer():
    header = re.sub(r"\s+", " ", read("include", "ringpop_hip.h"))
    assert "int rp_sim_ownership(rp_sim *sim, rp_ownership_stats *stats, uint64_t *claimed, size_t cap);" in header
    assert "int rp_sim_ownership_at(rp_sim *sim, const uint32_t *key_hashes, size_t n, uint32_t *claims);" in header
    assert "} rp_ownership_stats;" in header
    from ringpop_amd import _lib, build, sim
    L = ctypes.CDLL(build.build())
    assert hasattr(L, "rp_sim_ownership") and hasattr(L, "rp_sim_ownership_at")
    L.rp_abi_version.restype = ctypes.c_int
    assert L.rp_abi_version() == 2
    assert "rp_sim_ownership" in _lib.SIGNATURES and "rp_sim_ownership_at" in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.OwnershipStats) == 128
    assert [f[0] for f in _lib.OwnershipStats._fields_] == ["measure", "claimants", "intervals", "max_claims",
                                                            "max_claims_hash", "reserved"]
    assert callable(sim.Sim.ownership) and callable(sim.Sim.ownership_at)
    js = read("js", "index.js")
    assert "SimCluster.prototype.ownership = " in js and "SimCluster.prototype.ownershipAt = " in js
    napi = read("js", "ringpop_napi.c")
    assert 'EXPORT("simOwnership"' in napi and 'EXPORT("simOwnershipAt"' in napi
    assert "rp_own.hip" in build.SOURCES


def test_checkpoints():
    assert oc.checkpoints("failstop") == sorted(set(range(3, 46, 3)) | set(range(26, 37)))
    assert oc.checkpoints("shift") == sorted(set(range(3, 41, 3)) | set(range(26, 31)))
    assert oc.checkpoints("join") == list(range(15))


@pytest.mark.parametrize("name", list(oc.SCENARIOS))
def test_identities(name):
    b, want = oc.expected(name)
    assert sorted(want) == oc.checkpoints(name)
    assert np.all(b[1:] > b[:-1])
    for r, e in want.items():
        assert sum(e["measure"]) == ALL and e["intervals"] == len(b), (name, r)
        assert e["claimants"] == e["dead"].count(0), (name, r)
        # sum_v claimed[v] = sum_k k x (hashes with exactly k claimants), from the model's exact counts
        assert int(e["claimed"].astype(object).sum()) == sum(k * m for k, m in e["exact"].items()), (name, r)
        if e["max_claims"] <= 6:
            assert int(e["claimed"].astype(object).sum()) == sum(k * m for k, m in enumerate(e["measure"])), (name, r)
        assert e["measure"][min(e["max_claims"], 7)] > 0 and not any(e["measure"][e["max_claims"] + 1:]), (name, r)
        first = int(np.argmax(e["claims"]))
        assert e["max_claims_hash"] == int(b[first]) and (e["claims"][:first] < e["max_claims"]).all(), (name, r)
        for v, d in enumerate(e["dead"]):
            if d:
                assert e["claimed"][v] == 0, (name, r, v)


def test_failstop_classes():
    _, want = oc.expected("failstop")
    orphaned = {r: e["measure"][0] for r, e in want.items()}
    assert all(orphaned[r] == 375943841 for r in orphaned if r <= 27) and orphaned[3] and orphaned[27]
    assert [orphaned[r] for r in range(28, 33)] == [312248380, 207377531, 96067541, 9408337, 0]
    assert all(orphaned[r] == 0 for r in orphaned if r >= 32)
    assert all(e["max_claims"] == 1 and e["claimants"] == 44 for e in want.values())


def test_partition_classes():
    _, want = oc.expected("partition")
    for r, e in want.items():
        if r <= 26:
            assert e["measure"][1] == ALL and e["max_claims"] == 1, r
        else:
            assert e["measure"][2] > 0, r
        assert e["measure"][0] == 0 and e["claimants"] == 64, r
    assert want[39]["measure"][2] == 3877259908
    assert [want[r]["max_claims"] for r in (42, 45, 48)] == [5, 6, 7]
    assert want[48]["measure"][7] > 0  # (the class of 7 or more)


def test_shift_classes():
    b, want = oc.expected("shift")
    assert len(b) < 32 * oc.REPLICAS  # (replicas share points)
    for r, e in want.items():
        assert e["max_claims"] == 5, r
        if r < 29:
            assert all(e["measure"][k] > 0 for k in range(4)), r
        else:
            assert e["measure"][0] == 0 and e["measure"][2] > 0, r


def test_join_classes():
    _, want = oc.expected("join")
    for r in (0, 1, 2, 3):
        assert [want[r]["dead"][v] for v in (7, 33, 12)] == [2, 2, 2] and want[r]["claimants"] == 37, r
        assert want[r]["claimed"][7] == 0 and want[r]["max_claims"] == 1, r
    assert want[4]["claimants"] == 39 and want[7]["claimants"] == 40
    assert want[4]["max_claims"] == 3 and want[4]["claimed"][7] > 0
    assert all(want[r]["max_claims"] > 1 for r in range(4, 10))
    assert all(want[r]["max_claims"] == 1 and want[r]["measure"][1] == ALL for r in range(10, 15))


def test_queries_cover_both_sides_of_every_boundary():
    b = np.array([5, 9, 0xFFFFFFF0], dtype=np.uint32)
    claims = np.array([3, 1, 2], dtype=np.uint32)
    q = oc.queries(b)
    assert set(q.tolist()) == {5, 9, 0xFFFFFFF0, 4, 8, 0xFFFFFFEF, 6, 10, 0xFFFFFFF1, 0, 0xFFFFFFFF}
    got = dict(zip(q.tolist(), oc.claims_at(b, claims, q).tolist()))
    assert got == {5: 3, 4: 3, 0: 3, 0xFFFFFFF1: 3, 0xFFFFFFFF: 3, 6: 1, 8: 1, 9: 1, 10: 2, 0xFFFFFFEF: 2, 0xFFFFFFF0: 2}
    assert oc.lengths(b).tolist() == [5 + ALL - 0xFFFFFFF0, 4, 0xFFFFFFF0 - 9]
