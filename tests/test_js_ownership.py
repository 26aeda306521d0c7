"""The JavaScript host's SimCluster.ownership() / SimCluster.ownershipAt()
(tests/js/test_ownership.js) on the 64-node partition scenario after round 30,
against the Python binding's result on the same scenario, which equals the
expectation restated from the CPU oracle (tests/ownership_cases.py); this
side passes it in as JSON."""
import json
import os
import subprocess

import numpy as np
import pytest

import ownership_cases as oc
from test_js import NODE, ROOT, build_addon

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_ownership(gpu_lib, tmp_path):
    import ringpop_amd as rp
    build_addon()
    n, kw, _, _ = oc.SCENARIOS["partition"]
    rounds = 30
    b, want = oc.expected("partition")
    e = want[rounds]
    assert e["measure"][2] > 0 and e["measure"][1] > 0  # (inside the window, two owners for part of the keys)
    q = oc.queries(b)
    S = rp.Sim(n, oc.SIM_SEED, **kw)
    S.run(rounds, churn=True)
    py = S.ownership()
    at = S.ownership_at(q)
    S.close()
    assert py["measure"] == e["measure"] and np.array_equal(py["claimed"], e["claimed"])
    assert np.array_equal(at, oc.claims_at(b, e["claims"], q))
    out = {"n": n, "seed": oc.SIM_SEED, "churnK": -(-n // 100), "partition": kw["partition"], "rounds": rounds,
           "measure": py["measure"], "claimants": py["claimants"], "intervals": py["intervals"],
           "maxClaims": py["max_claims"], "maxClaimsHash": py["max_claims_hash"],
           "claimed": [str(int(c)) for c in py["claimed"]], "keyHashes": q.tolist(), "claims": at.tolist()}
    p = tmp_path / "ownership_expect.json"
    p.write_text(json.dumps(out))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_ownership.js"), str(p)], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
