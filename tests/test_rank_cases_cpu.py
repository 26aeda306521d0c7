"""tests/rank_cases.py on the CPU: the drawn join and view scenarios of
tests/test_gpu_rank_scenarios.py stay on the paths they are there for (an
edit of a draw that moves a case off them fails here), the oracle runs them,
and the reference's join fixtures meet the same conditions on 2 and 4 ranks."""
import numpy as np
import pytest

import rank_cases as rk


def test_join_scenario_reaches_every_reply_placement():
    n, G = 128, 4
    kw, rounds, churn_rounds = rk.join_scenario(n, G)
    joins = kw["joins"]
    rk.check_join_schedule(joins, n, G)
    assert len(joins) == n - 32 and {a for a, _, _ in joins} == set(range(6))
    assert all(sum(1 for a, _, _ in joins if a == r) == 16 for r in range(6))
    dead = kw["failures"][3][0]
    assert dead not in {j for _, j, _ in joins}  # the fail-stop is among the members from the start
    assert all(dead not in sd and 2 <= len(sd) <= 3 for _, _, sd in joins)
    assert max(a for a, _, _ in joins) < churn_rounds < rounds


@pytest.mark.parametrize("idx,G", [(1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (3, 4)])
def test_join_fixtures_reach_every_reply_placement(golden, idx, G):
    cfg = golden("sim_join.json.gz")["cases"][idx]["config"]
    assert cfg["n"] % G == 0
    rk.check_join_schedule([tuple(e) for e in cfg["joins"]], cfg["n"], G)


def test_join_schedule_conditions_bite():
    n, G = 16, 4
    with pytest.raises(AssertionError, match="crosses"):
        rk.check_join_schedule([(0, 1, [0]), (0, 5, [4])], n, G)
    with pytest.raises(AssertionError, match="stays"):
        rk.check_join_schedule([(0, 1, [4]), (0, 5, [0])], n, G)
    with pytest.raises(AssertionError, match="two ranks"):
        rk.check_join_schedule([(0, 1, [0]), (1, 5, [0])], n, G)
    with pytest.raises(AssertionError, match="earlier round"):
        rk.check_join_schedule([(0, 1, [0, 4]), (0, 5, [4])], n, G)
    rk.check_join_schedule([(0, 1, [0, 4]), (1, 5, [1])], n, G)


def test_views_scenario_spreads_every_status_over_the_ranks():
    n, G = 128, 4
    kw, rounds, churn_rounds, absent = rk.views_scenario(n)
    st, inc = kw["views"]
    rk.check_view_spread(st, n, G)
    assert (np.diag(st) == 1).all()
    others = np.arange(n) != absent
    assert (st[others, absent] == 0).all() and st[absent, absent] == 1 and (st[:, others] != 0).all()
    addrs = kw["addresses"]
    assert len(addrs) == n and addrs == sorted(set(addrs))
    assert min(map(len, addrs)) >= 4 and max(map(len, addrs)) <= 32
    # the two fail-stops sit on different ranks, and neither is the absent member
    dead = kw["failures"][2]
    assert len({v // (n // G) for v in dead}) == 2 and absent not in dead
    with pytest.raises(AssertionError):
        rk.check_view_spread(np.ones((n, n), dtype=np.int32), n, G)


def test_oracle_runs_the_drawn_scenarios():
    """The reference side of the two drawn cases: the joiners all join, the
    fail-stops are the only nodes left out, and the totals are the rounds' sums."""
    n = 128
    kw, rounds, churn_rounds = rk.join_scenario(n, 4)
    t = rk.Trace(n, 51, rounds, churn_rounds, **kw)
    assert sum(f is None for f in t.nodes) == 1  # the fail-stopped member
    assert all(len(f["members"]) == n for f in t.nodes if f is not None)
    assert t.totals()["evaluated"] == sum(o["evaluated"] for o, _ in t.rounds) > 0
    assert sum(c is None for c in t.rounds[0][1]) == n - 32 - 16  # not joined yet after round 0
    kw, rounds, churn_rounds, absent = rk.views_scenario(n)
    t = rk.Trace(n, 31, rounds, churn_rounds, **kw)
    assert sum(f is None for f in t.nodes) == 2
    assert max(o["waves"] for o, _ in t.rounds) > 2  # the fail-stops' ping-req waves
    # (piggyback counts outlast the run: no full sync carries the absent member to the others yet)
    assert {len(f["members"]) for f in t.nodes if f is not None} == {n - 1, n}


def test_notes_keep_the_first_mismatches():
    nt = rk.Notes(3)
    assert nt.check(True, "fine") and not nt.notes
    for i in range(rk.MAX_NOTES + 5):
        nt.check(False, "round", i)
    assert nt.count == rk.MAX_NOTES + 5 and len(nt.notes) == rk.MAX_NOTES and nt.notes[0] == "rank 3: round 0"
