"""CPU checks of the request-routing feature (rp_sim_ring_checksums /
rp_sim_route / rp_sim_route_uniform): the boundary exists at every layer, the
request generator is the documented splitmix64, and the GPU tests' scenarios
produce every outcome class they are meant to (so that no GPU comparison
passes vacuously)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("rp_sim_ring_checksums", "rp_sim_route", "rp_sim_route_uniform")


def test_route_api_exists_at_every_layer():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ringpop_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", header))
    assert set(FUNCTIONS) <= declared
    assert "rp_route_stats" in header
    from ringpop_amd import _lib, build
    from ringpop_amd.sim import Sim
    L = ctypes.CDLL(build.build())
    assert all(hasattr(L, f) for f in FUNCTIONS)
    assert set(FUNCTIONS) <= set(_lib.SIGNATURES)
    assert ctypes.sizeof(_lib.RouteStats) == 64
    for m in ("ring_checksums", "route", "route_uniform"):
        assert callable(getattr(Sim, m))
    assert Sim.ROUTE_OUTCOMES == rc.OUTCOMES
    js = open(os.path.join(ROOT, "js", "index.js")).read()
    assert "SimCluster.prototype.ringChecksums" in js and "SimCluster.prototype.route" in js


def test_generator_is_splitmix64():
    # hand-checked: splitmix64's first outputs for the state 0 are the
    # reference values of the published generator (Vigna, splitmix64.c)
    assert rc.splitmix64_finalise(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert rc.splitmix64_finalise(2 * 0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert rc.splitmix64_finalise(3 * 0x9E3779B97F4A7C15) == 0x06C45D188009454F
    assert rc.request(0, 0, 96) == ((0xE220A839 * 96) >> 32, 0x7B1DCDAF)
    assert rc.request(0, 1, 1 << 16) == (0x6E78, 0xA1B965F4)
    for seed, n in ((11, 96), (0xFFFFFFFFFFFFFFFF, 65536), (1 << 63, 2)):
        e, h = rc.requests(seed, 2000, n)
        assert e.dtype == np.uint32 and h.dtype == np.uint32
        for i in (0, 1, 2, 63, 64, 1000, 1999):
            assert (int(e[i]), int(h[i])) == rc.request(seed, i, n), (seed, n, i)
        assert int(e.max()) < n
    # the oracle's key generator is the same stream (decimal strings of r)
    import oracle
    assert [int(s) for s in oracle.lookup_keys(11, [0, 5])] == \
        [rc.splitmix64_finalise(11 + (i + 1) * 0x9E3779B97F4A7C15) for i in (0, 5)]


@pytest.mark.parametrize("name", sorted(rc.SCENARIOS))
def test_scenarios_cover_their_outcome_classes(name):
    """Oracle seed 7, request seed 11, 1,500 requests after every round."""
    want = rc.SCENARIOS[name][3]
    total = dict.fromkeys(rc.COUNTS, 0)
    for _, _, _, stats, _ in rc.expected(name):
        assert stats["requests"] == rc.REQUESTS == sum(stats[k] for k in rc.OUTCOMES)
        for k in rc.COUNTS:
            total[k] += stats[k]
    print(name, total)
    missing = [k for k in want if total[k] == 0]
    assert not missing, (name, total)
    if "entry_dead" not in want:
        assert total["entry_dead"] == 0
