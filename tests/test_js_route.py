"""The JavaScript host's SimCluster.ringChecksums() / SimCluster.route()
(tests/js/test_route.js) on the 64-node partition scenario after round 30,
against the expectation restated from the CPU oracle (tests/route_cases.py),
which this side passes in as JSON."""
import json
import os
import subprocess

import pytest

import route_cases as rc
from test_js import NODE, ROOT, build_addon

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]

CAMEL = {"requests": "requests", "local": "local", "delivered": "delivered", "checksums_differ": "checksumsDiffer",
         "unreachable": "unreachable", "entry_dead": "entryDead", "misrouted": "misrouted"}


def test_js_route(tmp_path):
    build_addon()
    n, kw, _, _ = rc.SCENARIOS["partition"]
    rounds = 30
    dests, outcomes, agrees, stats, rcs = rc.expected("partition")[rounds - 1]
    assert stats["unreachable"] > 0 and stats["checksums_differ"] > 0  # (inside the window, rings diverged)
    entries, keys = rc.requests(rc.REQ_SEED, rc.REQUESTS, n)
    want = {"n": n, "seed": rc.SIM_SEED, "churnK": -(-n // 100), "partition": kw["partition"], "rounds": rounds,
            "entries": entries.tolist(), "keyHashes": keys.tolist(), "dests": dests.tolist(),
            "outcomes": outcomes.tolist(), "ownerAgrees": agrees.tolist(),
            "stats": {CAMEL[k]: v for k, v in stats.items()}, "ringChecksums": rcs.tolist(),
            "outcomeNames": [CAMEL[k] for k in rc.OUTCOMES]}
    p = tmp_path / "route_expect.json"
    p.write_text(json.dumps(want))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_route.js"), str(p)], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
