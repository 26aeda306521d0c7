"""CPU checks of the multi-key expectation (tests/route_all_cases.py): over each
scenario's clocks the batches contain every case the GPU comparison is for, so
that it cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import route_all_cases as ra  # noqa: E402
import route_cases as rc  # noqa: E402


@pytest.mark.parametrize("name", sorted(rc.SCENARIOS))
def test_expectation_covers_what_the_scenario_is_for(name):
    exp, batches = ra.expected(name)
    must = rc.SCENARIOS[name][3]
    groups, misrouted, split, fewer, full, worst = np.zeros(4, dtype=np.int64), 0, 0, 0, 0, np.zeros(5, dtype=np.int64)
    for clock, by_batch in exp.items():
        for b, r in by_batch.items():
            st, K = r["stats"], np.diff(batches[b][1]).astype(np.int64)
            live = r["worst"] != rc.ENTRY_DEAD
            assert st["requests"] == len(K) and st["keys"] == K[live].sum() == sum(st["key_outcome"])
            assert st["groups"] == r["fanout"].sum() == sum(st["group_outcome"])
            assert sum(st["worst_hist"]) == sum(st["fanout_hist"]) == st["requests"] - st["entry_dead"]
            groups += st["group_outcome"]
            misrouted, split = misrouted + st["misrouted_keys"], split + st["split_groups"]
            fewer, full = fewer + int((live & (r["fanout"] < K)).sum()), full + int((live & (K > 0) & (r["fanout"] == K)).sum())
            worst += np.bincount(r["worst"], minlength=5)
    print(name, groups, misrouted, split, fewer, full, worst)
    assert all(groups[rc.OUTCOMES.index(k)] > 0 for k in must if k in rc.OUTCOMES[:4]), groups
    assert (worst[rc.ENTRY_DEAD] > 0) == ("entry_dead" in must)
    assert misrouted > 0 and split > 0 and fewer > 0 and full > 0
    assert worst[0] + worst[1] > 0 and worst[2] + worst[3] > 0
    ragged = exp[min(exp)]["ragged"]
    assert ragged["fanout"][0] == ragged["fanout"][-1] == 0 and ragged["stats"]["empty"] >= 2
    # (with more than 64 nodes: ranks past one chunk's lanes)
    assert ragged["stats"]["max_fanout"] > min(64, rc.SCENARIOS[name][0] // 2)
