"""CPU checks of request traffic with proxy retries (rp_traffic_*): the
boundary exists at every layer, and the model of DESIGN.md §11 on the CPU
oracle (tests/traffic_cases.py) produces, in every scenario the GPU tests
compare, each class it is meant to -- so that no GPU comparison passes
vacuously -- and keeps the counters' identities."""
import ctypes
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traffic_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("rp_traffic_create", "rp_traffic_destroy", "rp_traffic_submit", "rp_traffic_submit_uniform",
             "rp_traffic_poll", "rp_traffic_run", "rp_traffic_read_stats", "rp_traffic_history", "rp_traffic_pending",
             "rp_traffic_results")
JS_STATS = ("submitted", "local", "delivered", "reroutedLocal", "failed", "entryDead", "requestProxied",
            "sendUnreachable", "checksumsDiffer", "retryScheduled", "retryAttempted", "retryRerouted", "retrySucceeded",
            "retryFailed", "misrouted")


def test_traffic_api_exists_at_every_layer():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ringpop_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", header))
    assert set(FUNCTIONS) <= declared
    for t in ("rp_traffic_config", "rp_traffic_stats", "rp_request_result", "rp_request_pending"):
        assert t in header, t
    from ringpop_amd import _lib, build
    from ringpop_amd.sim import Sim, Traffic
    L = ctypes.CDLL(build.build())
    assert all(hasattr(L, f) for f in FUNCTIONS)
    assert L.rp_abi_version() == 2
    assert set(FUNCTIONS) <= set(_lib.SIGNATURES)
    assert ctypes.sizeof(_lib.TrafficStats) == 128
    assert ctypes.sizeof(_lib.RequestResult) == 16 == Traffic.RESULT_DTYPE.itemsize
    assert ctypes.sizeof(_lib.RequestPending) == 32 == Traffic.PENDING_DTYPE.itemsize
    assert tuple(k for k, _ in _lib.TrafficStats._fields_) == tc.STATS + ("reserved",)
    assert callable(Sim.traffic)
    for m in ("submit", "submit_uniform", "poll", "run", "stats", "history", "pending", "results", "close"):
        assert callable(getattr(Traffic, m)), m
    assert Traffic.OUTCOMES == tc.OUTCOMES and Traffic.PENDING == tc.PENDING
    js = open(os.path.join(ROOT, "js", "index.js")).read()
    assert "SimCluster.prototype.traffic" in js
    napi = open(os.path.join(ROOT, "js", "ringpop_napi.c")).read()
    for k in JS_STATS:
        assert '"%s"' % k in napi, k


def finals(m, outcome, retries=None):
    row = m.by_retries[outcome]
    return sum(row) if retries is None else row[retries]


def check_identities(m, max_retries=3, enforce=True):
    s = m.stats
    pending = len(m.pending)
    assert all(r is not None for i, r in enumerate(m.results) if i not in {q["id"] for q in m.pending})
    assert s["submitted"] == len(m.results)
    for k in tc.OUTCOMES:
        assert s[k] == finals(m, k), k
    assert s["submitted"] == sum(s[k] for k in tc.OUTCOMES) + pending
    # ENTRY_DEAD at submission, and while waiting for a retry.  Under a schedule that starts with 0 the first
    # retry is immediate, so these are the ENTRY_DEAD finals with 0 retries and with more; a first delay > 0
    # lets an entry die with its first retry still to come (0 retries, yet scheduled)
    dead_submit = sum(1 for r in m.results if r and r[1] == tc.ENTRY_DEAD and r[4] == r[3])
    dead_waiting = finals(m, "entry_dead") - dead_submit
    if m.schedule[0] == 0:
        assert dead_submit == finals(m, "entry_dead", 0)
    assert s["retry_scheduled"] == s["retry_attempted"] + dead_waiting + pending
    assert s["proxied"] == s["submitted"] - s["local"] - dead_submit + s["retry_attempted"] - s["rerouted_local"]
    assert s["proxied"] == s["delivered"] + s["retry_scheduled"] + s["failed"]
    assert s["retry_failed"] == (s["failed"] if max_retries > 0 else 0)
    if enforce:
        assert s["send_unreachable"] + s["checksums_differ"] == s["retry_scheduled"] + s["failed"]
    # the per-clock rows sum to the cumulative statistics
    for k in tc.STATS:
        assert sum(row[k] for row in m.history.values()) == s[k], k


@pytest.mark.parametrize("name", sorted(tc.SCENARIOS))
def test_scenarios_cover_their_classes(name):
    """Oracle seed 7, request seed 11, the default schedule {0, 5, 18}."""
    m, snaps = tc.expected(name)
    print(name, m.stats, m.by_retries)
    assert len(snaps) == tc.SCENARIOS[name][2] + tc.DRAIN
    check_identities(m)
    assert not m.pending
    assert max(len(s["pending"]) for s in snaps) > 0
    for r in (0, 2, 3):
        assert finals(m, "delivered", r) > 0, r
    # same clock, same state: the immediate retry meets what the first attempt met
    assert finals(m, "delivered", 1) == 0
    assert finals(m, "failed") > 0 and finals(m, "failed") == finals(m, "failed", 3)
    assert finals(m, "rerouted_local") > 0
    assert m.stats["retry_rerouted"] > m.stats["rerouted_local"]  # (remote reroutes)
    assert m.stats["send_unreachable"] > 0 and m.stats["checksums_differ"] > 0
    assert m.stats["retry_succeeded"] > 0 and m.stats["misrouted"] >= 0
    if name == "partition":
        assert finals(m, "entry_dead") == 0
    else:
        assert finals(m, "entry_dead", 0) > 0
    if name == "failstop_late":
        assert finals(m, "entry_dead", 1) > 0 and finals(m, "entry_dead", 2) > 0
    else:
        assert finals(m, "entry_dead") == finals(m, "entry_dead", 0)


def test_past_the_end_of_the_schedule():
    m = tc.run_model("failstop_late", max_retries=4, schedule=(1, 2))
    print(m.stats, m.by_retries)
    check_identities(m, max_retries=4)
    assert not m.pending
    for r in (1, 2, 3, 4):
        assert finals(m, "delivered", r) > 0, r
    assert finals(m, "failed", 4) > 0 and finals(m, "failed") == finals(m, "failed", 4)


@pytest.mark.parametrize("schedule", [tc.DEFAULT_SCHEDULE, (3,)])
def test_no_retries(schedule):
    m = tc.run_model("failstop", max_retries=0, schedule=schedule)
    print(m.stats, m.by_retries)
    check_identities(m, max_retries=0)
    assert finals(m, "failed", 0) > 0 and finals(m, "failed") == finals(m, "failed", 0)
    assert not m.pending
    for k in tc.STATS:
        if k.startswith("retry_"):
            assert m.stats[k] == 0, k
    assert m.stats["rerouted_local"] == 0


def test_one_retry_after_three_rounds():
    m = tc.run_model("failstop", max_retries=1, schedule=(3,))
    print(m.stats, m.by_retries)
    check_identities(m, max_retries=1)
    assert finals(m, "delivered", 1) > 0 and finals(m, "failed", 1) > 0
    assert not m.pending


def test_without_enforce_consistency():
    m = tc.run_model("failstop", enforce_consistency=False)
    print(m.stats, m.by_retries)
    check_identities(m, enforce=False)
    s = m.stats
    assert s["checksums_differ"] > 0 and s["misrouted"] > 0
    assert s["send_unreachable"] == s["retry_scheduled"] + s["failed"]  # (a differing checksum is no error)
