"""Multi-key request traffic without a GPU: the library exports the tracker's
entry points, and the model's default runs (tests/traffic_all_cases.py) contain
every case the GPU parity test is meant to catch."""
import ctypes

import pytest

import traffic_all_cases as ta

NAMES = ("create", "destroy", "submit", "submit_uniform", "poll", "run", "read_stats", "pending", "results")


def test_library_exports_the_tracker():
    from ringpop_amd import _lib, build
    L = ctypes.CDLL(build.build())
    for k in NAMES:
        assert hasattr(L, "rp_traffic_all_" + k) and "rp_traffic_all_" + k in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.TrafficAllStats) == 192 and ctypes.sizeof(_lib.RequestAllResult) == 16
    assert ctypes.sizeof(_lib.SendPending) == 32


@pytest.mark.parametrize("name,cases", [
    ("failstop", ("aborted_2_keys", "aborted_over_64", "multi_rerouted_remote", "mixed_outcomes", "failed_before_done",
                  "over_64_survives_a_poll")),
    ("partition", ("multi_rerouted_local", "aborted_over_64")),
    ("failstop_late", ("entry_dead_at_retry",)),
    ("shift", ("aborted", "mixed_outcomes")),
])
def test_default_runs_contain_the_cases(name, cases):
    m, snaps = ta.expected(name)
    assert not set(cases) - m.seen, set(cases) - m.seen
    assert m.stats["aborted"] > 0 and m.stats["failed"] > 0 and not m.pending
    assert m.stats["requests"] == m.stats["requests_ok"] + m.stats["requests_failed"] == len(snaps[-1]["results"])
    assert sum(m.stats[k] for k in ta.OUTCOMES) == m.stats["sends"] == sum(map(sum, m.by_retries.values()))
