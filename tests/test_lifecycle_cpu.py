"""CPU checks of graceful leave and rejoin: the boundary exists
at every layer; the committed fixture holds the scenarios it was recorded for,
so that no GPU comparison passes vacuously; and -- where node and the
reference are present -- tools/lifecycle_harness.js without events equals
oracle/harness/sim.js field by field, and the committed fixture is what
tools/gen_lifecycle_fixture.js produces."""
import ctypes
import gzip
import json
import os
import re
import shutil
import subprocess

import pytest

import lifecycle_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
REFERENCE = os.environ.get("RINGPOP_REFERENCE", "/root/reference")  # (the harnesses' own default)
needs_reference = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(REFERENCE, "index.js")),
                                     reason="node or the reference is absent")
NODE_ENV = dict(os.environ, NODE_PATH=os.path.join(ROOT, "oracle", "harness", "shims"))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the boundary
def test_header_declares_the_calls_and_names_the_reference():
    src = read("include", "ringpop_hip.h")
    for sym in ("rp_sim_leave", "rp_sim_rejoin", "rp_sim_node_flags"):
        assert re.search(r"\bint %s\s*\(rp_sim \*sim, uint32_t node, uint32_t" % sym, src), sym
    assert "server/admin-leave-handler.js:30-57" in src and "server/admin-join-handler.js:\n * 36-45" in src
    assert "lib/swim/suspicion.js:87-108" in src


def test_library_exports_the_calls():
    from ringpop_amd import build
    L = ctypes.CDLL(build.build())
    for sym in ("rp_sim_leave", "rp_sim_rejoin", "rp_sim_node_flags"):
        assert hasattr(L, sym), sym


def test_hosts_bind_the_calls():
    from ringpop_amd import _lib
    from ringpop_amd.sim import Sim
    for sym in ("rp_sim_leave", "rp_sim_rejoin", "rp_sim_node_flags"):
        assert sym in _lib.SIGNATURES
    for m in ("leave", "rejoin", "flags"):
        assert callable(getattr(Sim, m))
    napi, index = read("js", "ringpop_napi.c"), read("js", "index.js")
    for name, sym in (("simLeave", "rp_sim_leave"), ("simRejoin", "rp_sim_rejoin"), ("simFlags", "rp_sim_node_flags")):
        assert 'EXPORT("%s"' % name in napi and sym + "(" in napi
    for m in ("leave", "rejoin", "flags"):
        assert "SimCluster.prototype.%s = function %s(" % (m, m) in index


# ---- the committed fixture
@pytest.fixture(scope="module")
def cases(golden):
    return golden(lc.FIXTURE)["cases"]


def converged_rounds(case):
    return [r["round"] for r in case["rounds"] if r["converged"]]


def test_fixture_is_no_larger_than_the_largest_before_it():
    sizes = {f: os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))}
    assert sizes[lc.FIXTURE] <= max(v for f, v in sizes.items() if f != lc.FIXTURE)


def test_fixture_storm_case(cases):
    c = cases[lc.STORM]
    cfg, log = c["config"], c["log"]
    assert cfg["n"] == 64 and cfg["seed"] == 11 and len(c["rounds"]) == 90 and cfg["churnRounds"] == 20 and cfg["churnK"] == 2
    assert cfg["failures"] == {"2": [3, 40]} and cfg["storm"] == {"start": 5, "end": 25, "ppm": 40000}
    assert cfg["leaves"] == {"8": [5, 9, 17, 33], "12": [20]} and cfg["rejoins"] == {"45": [5, 17], "50": [20]}
    assert [e[:2] for e in log["leaves"]] == [[8, 5], [8, 9], [8, 17], [8, 33], [12, 20]]
    assert any(e[2] > 0 for e in log["leaves"])          # a leaver with pending timers
    assert len(log["refusedStarts"]) > 0                  # a suspect update that started no timer
    assert log["pingsToLeft"] > 0 and log["pingReqsToLeft"] > 0
    assert log["fullSyncsToRejoined"] > 0
    conv = converged_rounds(c)
    assert any(r < 45 for r in conv) and any(r > 50 for r in conv)
    # a refused start leaves the member suspect with no timer
    d = c["dumps"]["30"]
    left = [v for v, f in enumerate(d) if not f["gossiping"] and not f["dead"]]
    assert left == [5, 9, 17, 20, 33]
    for v in left:
        assert d[v]["suspicionStopped"] and d[v]["timers"] == [] and d[v]["view"][v][0] == 4 and v not in d[v]["ringIds"]
    assert any(e is not None and e[0] == 2 for v in left for e in d[v]["view"])
    d = c["dumps"]["70"]
    assert [v for v, f in enumerate(d) if not f["gossiping"] and not f["dead"]] == [9, 33]
    assert all(d[v]["view"][v][0] == 1 and v in d[v]["ringIds"] and not d[v]["suspicionStopped"] for v in (5, 17, 20))


def test_fixture_partition_case(cases):
    c = cases[lc.PARTITION]
    cfg = c["config"]
    assert cfg["n"] == 32 and cfg["partition"] == {"start": 2, "end": 40, "split": 16} and len(c["rounds"]) == 120
    assert cfg["leaves"] == {"3": [20]} and cfg["rejoins"] == {"90": [20]} and cfg["churnRounds"] == 0
    assert [e[:2] for e in c["log"]["leaves"]] == [[3, 20]] and c["log"]["rejoins"] == [[90, 20]]


def test_fixture_piggyback_case(cases):
    c = cases[lc.PIGGYBACK]
    assert c["config"]["n"] == 10
    for r, servers, maxpb in (("1", 10, None), ("20", 9, 15), ("45", 10, 30)):
        for f in c["dumps"][r]:
            assert f["ringServers"] == servers and (maxpb is None or f["maxPiggyback"] == maxpb), (r, f["ringServers"])


def test_fixture_sharded_case(cases):
    c = cases[lc.SHARDED]
    cfg = c["config"]
    assert cfg["n"] == 96 and len(cfg["addresses"]) == 96 and cfg["addresses"] == sorted(cfg["addresses"])
    assert cfg["churnRounds"] == len(c["rounds"])  # churn throughout
    rounds = sorted(int(r) for r in cfg["leaves"])
    assert rounds == [rounds[0], rounds[0] + 1, rounds[0] + 2]
    leavers = sorted(v for ids in cfg["leaves"].values() for v in ids)
    assert 24 in leavers and 47 in leavers  # the first and the last node of a 4-shard block
    assert sorted(v for ids in cfg["rejoins"].values() for v in ids) == leavers
    assert len(c["log"]["leaves"]) == 6 and len(c["log"]["rejoins"]) == 6


def test_fixture_join_case(cases):
    c = cases[lc.JOIN]
    cfg = c["config"]
    joins = {e[1]: e for e in cfg["joins"]}
    assert cfg["leaves"] == {"6": [9, 1]}
    assert joins[9][0] < 6                                          # a joiner leaves after its join
    assert any(e[0] == 4 and 1 in e[2] for e in cfg["joins"])       # a seed leaves two rounds after serving a join
    assert len(c["log"]["leaves"]) == 2 and len(c["log"]["rejoins"]) == 2


# ---- against the reference (node)
def run_node(script, arg):
    r = subprocess.run([NODE, os.path.join(ROOT, script), arg], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=NODE_ENV)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@needs_reference
def test_harness_without_events_equals_the_oracle_harness(golden):
    """Drift guard between the two round drivers: sim_small's fail-stop case
    (ping-reqs, suspicion timers, faulty removals) through both."""
    cfg = dict(golden("sim_small.json.gz")["cases"][2]["config"], dumpRounds=[5, 30], plainDumps=True)
    a = json.loads(run_node("oracle/harness/sim.js", json.dumps(cfg)))
    b = json.loads(run_node("tools/lifecycle_harness.js", json.dumps(cfg)))
    assert b.pop("log") == {"leaves": [], "rejoins": [], "refusedStarts": [], "pingsToLeft": 0, "pingReqsToLeft": 0,
                            "fullSyncsToRejoined": 0}
    assert set(b) <= set(a)
    assert a["addresses"] == b["addresses"] and a["convergedAt"] == b["convergedAt"]
    assert len(a["rounds"]) == len(b["rounds"])
    for ra, rb in zip(a["rounds"], b["rounds"]):
        assert ra == rb, ra["round"]
    assert sorted(a["dumps"]) == sorted(b["dumps"]) == ["30", "5"]
    for r in a["dumps"]:
        for v, (fa, fb) in enumerate(zip(a["dumps"][r], b["dumps"][r])):
            assert fa == fb, (r, v)
    for v, (fa, fb) in enumerate(zip(a["final"], b["final"])):
        assert fa == fb, v


@needs_reference
def test_committed_fixture_is_what_the_generator_produces(tmp_path, golden):
    run_node("tools/gen_lifecycle_fixture.js", str(tmp_path))
    with gzip.open(tmp_path / lc.FIXTURE, "rt") as f:
        assert json.load(f) == golden(lc.FIXTURE)
