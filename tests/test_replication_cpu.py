"""The replica-set census' reference (tests/replication_cases.py) without a
GPU: at R = 1 it is the ownership census' expectation, and the scenarios show
what the device tests rely on: under-replication while faulty declarations are
pending, divergent preference lists under a partition and with colliding
hashes."""
import numpy as np
import pytest

import ownership_cases as oc
import replication_cases as rc

ALL = 1 << 32


def test_r1_is_the_ownership_census():
    _, own = oc.expected("failstop")
    _, rep = rc.expected("failstop")
    assert sorted(own) == sorted(rep) == oc.checkpoints("failstop")
    for r, want in own.items():
        got = rep[r][1]
        assert got["measure"][:7] + [sum(got["measure"][7:])] == want["measure"], r
        for k in ("claimants", "intervals", "max_claims", "max_claims_hash"):
            assert got[k] == want[k], (r, k)
        assert np.array_equal(got["held"], want["claimed"]) and np.array_equal(got["claims"], want["claims"]), r
    assert rep[28][1]["measure"][:2] == [312248380, 3982718916]


@pytest.mark.parametrize("name,clock,check", [
    ("failstop", 28, lambda e: e["under"] > 0 and e["measure"][1:4] == [36869006, 859989386, 3398108904]),
    ("failstop", 33, lambda e: e["exact"] == ALL and e["min_claims"] == e["max_claims"] == 3),
    ("partition", 39, lambda e: e["over"] > 0 and e["max_claims"] >= 6 and e["measure"][4] == 59696320),
    ("shift", 27, lambda e: e["under"] > 0 and e["over"] > 0 and e["measure"][10] == 1048576),
])
def test_scenarios_at_r3(name, clock, check):
    e = rc.expected(name)[1][clock][3]
    assert sum(e["measure"]) == e["under"] + e["exact"] + e["over"] == ALL
    assert check(e), {k: v for k, v in e.items() if k not in ("held", "claims")}
