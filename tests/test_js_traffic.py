"""The JavaScript host's SimCluster.traffic() (tests/js/test_traffic.js) on
the 64-node partition scenario for 30 rounds, against the model restated from
the CPU oracle (tests/traffic_cases.py): the statistics, by_retries, the
history rows, the pending counts and table and every outcome, which this side
passes in as JSON."""
import json
import os
import subprocess

import pytest

import oracle
import traffic_cases as tc
from test_js import NODE, ROOT, build_addon

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]

CAMEL = {"submitted": "submitted", "local": "local", "delivered": "delivered", "rerouted_local": "reroutedLocal",
         "failed": "failed", "entry_dead": "entryDead", "proxied": "requestProxied",
         "send_unreachable": "sendUnreachable", "checksums_differ": "checksumsDiffer",
         "retry_scheduled": "retryScheduled", "retry_attempted": "retryAttempted", "retry_rerouted": "retryRerouted",
         "retry_succeeded": "retrySucceeded", "retry_failed": "retryFailed", "misrouted": "misrouted"}


def test_js_traffic(tmp_path):
    build_addon()
    n, kw, _ = tc.SCENARIOS["partition"]
    rounds, per = 30, 100
    cpu = oracle.Sim(n, tc.SIM_SEED, **kw)
    m = tc.Model(cpu, kw["partition"])
    entries, keys = tc.stream(n, 0, rounds * per)
    counts = []
    for r in range(1, rounds + 1):
        cpu.round(churn=True)
        m.poll(r)
        m.submit(r, entries[(r - 1) * per:r * per], keys[(r - 1) * per:r * per])
        counts.append(len(m.pending))
    cpu.close()
    assert m.stats["send_unreachable"] > 0 and m.stats["retry_succeeded"] > 0 and m.pending  # (inside the window)
    want = {"n": n, "seed": tc.SIM_SEED, "churnK": -(-n // 100), "partition": kw["partition"], "rounds": rounds,
            "perRound": per, "reqSeed": tc.REQ_SEED, "entries": entries, "keyHashes": keys,
            "stats": {CAMEL[k]: v for k, v in m.stats.items()},
            "byRetries": {CAMEL[k]: v for k, v in m.by_retries.items()},
            "history": [{CAMEL[k]: v for k, v in m.row(r).items()} for r in range(1, rounds + 1)],
            "pendingCounts": counts,
            "pending": [[q[k] for k in ("id", "entry", "key_hash", "first_dest", "due", "submit_clock", "retries")]
                        for q in m.pending],
            "outcomes": [r[1] if r else tc.PENDING for r in m.results],
            "outcomeNames": [CAMEL[k] for k in tc.OUTCOMES]}
    p = tmp_path / "traffic_expect.json"
    p.write_text(json.dumps(want))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_traffic.js"), str(p)], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
