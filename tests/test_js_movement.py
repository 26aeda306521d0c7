"""The JavaScript host's SimCluster.ownershipSnapshot() / ownershipMoved()
(tests/js/test_movement.js) on the 64-node partition scenario between clocks
39 and 42, against the Python binding's result on the same scenario, which
equals the expectation restated from the CPU oracle (tests/movement_cases.py);
this side passes it in as JSON."""
import json
import os
import subprocess

import numpy as np
import pytest

import movement_cases as mc
import ownership_cases as oc
from test_js import NODE, ROOT, build_addon

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]

CAMEL = {"transition": "transition", "same_set": "sameSet", "handed_off": "handedOff", "gained": "gained", "lost": "lost",
         "gainers": "gainers", "losers": "losers", "max_gained": "maxGained", "max_gained_node": "maxGainedNode",
         "max_lost": "maxLost", "max_lost_node": "maxLostNode", "max_turnover": "maxTurnover",
         "max_turnover_hash": "maxTurnoverHash", "from_clock": "fromClock", "to_clock": "toClock",
         "intervals": "intervals"}


def test_js_movement(gpu_lib, tmp_path):
    import ringpop_amd as rp
    build_addon()
    n, kw, _, _ = oc.SCENARIOS["partition"]
    frm, to = 39, 42
    _, want, _ = mc.expected("partition")
    e = want[(frm, to)]
    assert e["gained"] > 0 and e["lost"] > 0 and e["max_turnover"] >= 3
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(frm, churn=True)
    with S.ownership_snapshot() as snap:
        S.run(to - frm, churn=True)
        py = S.ownership_moved(snap)
    S.close()
    assert all(py[k] == e[k] for k in CAMEL), {k: (py[k], e[k]) for k in CAMEL if py[k] != e[k]}
    assert np.array_equal(py["gained_by"], e["gained_by"]) and np.array_equal(py["lost_by"], e["lost_by"])
    out = {"n": n, "seed": oc.SIM_SEED, "churnK": -(-n // 100), "partition": kw["partition"], "from": frm, "to": to,
           "stats": {js: py[k] for k, js in CAMEL.items()},
           "gainedBy": [str(int(x)) for x in py["gained_by"]], "lostBy": [str(int(x)) for x in py["lost_by"]]}
    p = tmp_path / "movement_expect.json"
    p.write_text(json.dumps(out))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_movement.js"), str(p)], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
