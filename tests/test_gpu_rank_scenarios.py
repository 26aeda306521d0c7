"""The rank path (rp_sim_create_rank's code on loop ranks, one thread each;
DESIGN.md §7) on the scenarios that so far only ran on in-process shards:
joins (rp_sim::join_step's four broadcasts per seed reply, rooted at the
seed's rank), false-suspicion storms (origins and refutes as escapes), loaded
addresses and bootstrap views, shards that are no whole number of 64-row
groups (100, 32, 25 and 8 rows per rank), tiny seen-origin windows, forced
issue-time compaction and prefix packing, and rounds enqueued back to back
(rp_sim_run).  Each rank is compared on the nodes it holds with the CPU
oracle or with the reference's recorded run (tests/rank_cases.py): every
round's counts and checksums, then every own node's view, member order,
dissemination log, ring state, iterator and RNG.  Integer work: bit-exact."""
import pytest

import rank_cases as rk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def _oracle_ranks(rp, n, seed, G, rounds, churn_rounds, device=None, **kw):
    """The scenario on G loop ranks against one oracle run; `device`: keyword
    arguments only the device has (window sizes, compaction thresholds).
    Returns per rank (local_counters(), counters())."""
    trace = rk.Trace(n, seed, rounds, churn_rounds, **kw)
    return rk.run_ranks(rp, G, n, seed, rk.drive_trace(trace), **kw, **(device or {}))


def _case_ranks(rp, case, G):
    cfg = case["config"]
    assert cfg["n"] % G == 0
    rk.run_ranks(rp, G, cfg["n"], cfg["seed"], rk.drive_case(case), **rk.case_kwargs(cfg))


# ------------------------------------------------------------------- joins
# (n = 48, 40 and 128: 2 and 4 ranks divide each)
@pytest.mark.parametrize("idx,G", [(1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (3, 4)])
def test_join_ranks_against_reference(rp, golden, idx, G):
    case = golden("sim_join.json.gz")["cases"][idx]
    cfg = case["config"]
    rk.check_join_schedule([tuple(e) for e in cfg["joins"]], cfg["n"], G)
    _case_ranks(rp, case, G)


def test_join_ranks_against_oracle(rp):
    """128 nodes on 4 ranks of 32 rows: 32 members, 16 joiners per round
    through 3 seeds each, churn and a fail-stop."""
    n, G = 128, 4
    kw, rounds, churn_rounds = rk.join_scenario(n, G)
    rk.check_join_schedule(kw["joins"], n, G)
    _oracle_ranks(rp, n, 51, G, rounds, churn_rounds, **kw)


# ------------------------------------------------------------------ storms
@pytest.mark.parametrize("n,seed,k,G,rounds,storm", [
    (300, 6, 3, 3, 60, {"start": 0, "end": 40, "ppm": 10000}),
    (512, 9, 0, 8, 50, {"start": 0, "end": 30, "ppm": 4000})])
def test_storm_ranks_against_oracle(rp, n, seed, k, G, rounds, storm):
    """test_shard_storm_against_oracle's parameters: suspect origins and the
    victims' refutes cross the ranks as escapes (origin_exchange first)."""
    _oracle_ranks(rp, n, seed, G, rounds, rounds // 2, churn_k=k, failures={0: list(range(1, n, 17))}, storm=storm)


def test_storm_ranks_against_reference(rp, golden):
    _case_ranks(rp, golden("sim_storm.json.gz")["cases"][2], 4)  # (200 nodes: 50 rows per rank)


# ------------------------------------------------------ addresses and views
# (n = 48 and 32: 2 and 4 ranks divide both)
@pytest.mark.parametrize("idx,G", [(1, 2), (2, 2), (1, 4)])
def test_views_ranks_against_reference(rp, golden, idx, G):
    _case_ranks(rp, golden("sim_views.json.gz")["cases"][idx], G)


def test_views_ranks_against_oracle(rp):
    """Every rank loads all n addresses and all n views and keeps its own
    rows: absent members, suspects whose timers are due at round 0, faulty and
    leave members outside the ring, in the rows of every rank."""
    n, G = 128, 4
    kw, rounds, churn_rounds, absent = rk.views_scenario(n)
    rk.check_view_spread(kw["views"][0], n, G)
    addrs = kw["addresses"]
    assert min(map(len, addrs)) >= 4 and max(map(len, addrs)) <= 32 and len({len(a) for a in addrs}) > 8
    trace = rk.Trace(n, 31, rounds, churn_rounds, **kw)
    inner = rk.drive_trace(trace)

    def drive(S, rank, lo, hi, notes):
        vc = S.view_counts()[lo:hi]  # absent / alive / suspect / faulty / leave / ring servers, before round 0
        st = kw["views"][0][lo:hi]
        for status in range(5):
            notes.check(vc[:, status].tolist() == (st == status).sum(axis=1).tolist(), "view counts of status", status)
        notes.check([S.address(v) for v in range(lo, hi)] == addrs[lo:hi], "addresses")
        return inner(S, rank, lo, hi, notes)

    rk.run_ranks(rp, G, n, 31, drive, **kw)


# -------------------------------------------------------- shapes and windows
@pytest.mark.parametrize("n,seed,k,G,rounds,win", [
    (64, 7, 2, 8, 30, 0),         # 8 rows per rank
    (300, 4, 3, 3, 50, 0),        # 100 rows per rank
    (256, 21, 9, 8, 40, 128),     # a seen-origin window of 128 ids
    (500, 5, 40, 5, 25, 32)])     # ... of 32 ids, 40 new origins a round
def test_shapes_ranks_against_oracle(rp, n, seed, k, G, rounds, win):
    """test_shards_against_oracle's parameters: ragged 64-row groups, the
    gseen all-gather sized by nl >> gsz_log and seen_words."""
    _oracle_ranks(rp, n, seed, G, rounds, rounds * 2 // 3, device={"seen_window": win}, churn_k=k)


@pytest.mark.parametrize("n,seed,k,G,rounds,fail,part", [
    (200, 13, 2, 8, 80, {1: list(range(0, 200, 10))}, {"start": 10, "end": 40, "split": 120}),  # 25 rows per rank
    (120, 8, 2, 4, 70, None, {"start": 2, "end": 30, "split": 50})])
def test_fault_shapes_ranks_against_oracle(rp, n, seed, k, G, rounds, fail, part):
    """test_shard_faults_against_oracle's parameters: ping-req waves, settled
    masks (gsettled sized by nl >> fs_log) and full syncs on 25 and 30 rows."""
    _oracle_ranks(rp, n, seed, G, rounds, rounds * 2 // 3, churn_k=k, failures=fail, partition=part)


# ------------------------------------------- forced compaction and packing
def test_compaction_and_packing_ranks_against_oracle(rp):
    """Issue-time compaction and prefix packing forced with tiny thresholds
    (a row of test_sim_prefix_packing_against_oracle) on 4 ranks of 48 rows;
    the oracle has neither."""
    n, G = 192, 4
    out = _oracle_ranks(rp, n, 2, G, 70, 70 * 2 // 3, device={"prefix_min": 1, "compact": (1, 4)}, churn_k=9,
                        failures={10: list(range(0, n, 16))}, storm={"start": 2, "end": 60, "ppm": 10000})
    packs = sum(loc["prefix_packs"] for loc, _ in out)
    compactions = sum(loc["compactions_issue"] for loc, _ in out)
    print("prefix packs", packs, "issue-time compactions", compactions)
    assert packs > n, packs
    assert compactions > 0
    for _, tot in out:  # (every rank's cluster-wide counters are the sum of the ranks' own: k_stats_combine)
        assert tot["prefix_packs"] == packs and tot["compactions_issue"] == compactions, tot


# ------------------------------------------------------------------ run(k)
@pytest.mark.parametrize("fail", [None, {2: [5, 70, 200]}])
def test_run_ranks_against_oracle(rp, fail):
    """12 rounds enqueued back to back on 4 ranks (the planning counts read on
    the host inside; with fail-stops the ping-req counts too), then one sync."""
    n, G, k = 256, 4, 12
    trace = rk.Trace(n, 2024, k, k, churn_k=5, failures=fail)
    rk.run_ranks(rp, G, n, 2024, rk.drive_run(trace, k), churn_k=5, failures=fail)
