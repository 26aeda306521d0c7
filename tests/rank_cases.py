"""Shared by the rank-path scenario tests (tests/test_gpu_rank_scenarios.py;
DESIGN.md §7): G loop ranks (rp_sim_create_rank_loop: rp_sim_create_rank's
code with device-copy collectives) as threads of the test process, each
compared on the nodes it holds with the CPU oracle -- or, for the reference's
fixtures, with the recorded run -- and the host-side conditions that keep a
drawn scenario on the paths it is there for (which ranks a join reply is
rooted at, which ranks' rows hold which view statuses).

The Sims are made in the calling thread (no setup call performs a collective)
and driven from one thread each, every rank making the same calls in the same
order.  A comparison that fails is noted and the rank goes on making its
calls, so that wrong data never keeps a rank from a collective the others
wait in; an error of the library ends the rank, which breaks the loop group
for the others (rp_xport.hip: at most its 120 s rendezvous limit)."""
import threading

import numpy as np

STAT_KEYS = ("evaluated", "applied", "full_syncs", "messages", "waves", "converged")
INFO_KEYS = ("max_pb", "ring_servers", "ring_checksum", "iter_index", "iter_round", "rng")
ROUND_KEYS = (("evaluated", "evaluated"), ("applied", "applied"), ("full_syncs", "fullSyncs"), ("messages", "messages"),
              ("waves", "waves"))
JOIN_TIMEOUT = 150.0  # seconds per rank thread: above the transport's 120 s rendezvous limit
MAX_NOTES = 8         # mismatches kept per rank (the first ones tell; the count is kept too)


class Notes:
    """A rank's failed comparisons."""

    def __init__(self, rank):
        self.rank, self.notes, self.count = rank, [], 0

    def check(self, ok, *what):
        if not ok:
            self.count += 1
            if len(self.notes) < MAX_NOTES:
                self.notes.append("rank %d: %s" % (self.rank, " ".join(str(w) for w in what)))
        return ok


def run_ranks(rp, G, n, seed, drive, **kw):
    """drive(S, rank, lo, hi, notes) on each of the G loop ranks of
    rp.Sim(n, seed, **kw), each from its own thread; its return values in rank
    order.  Raises a rank's error, then AssertionError with the ranks' notes."""
    from ringpop_amd.sim import Loop
    loop = Loop(G)
    sims, threads = [], []
    errs, out = [None] * G, [None] * G
    notes = [Notes(r) for r in range(G)]

    def rank_main(r):
        try:
            lo, hi = sims[r].shard_range()
            assert (lo, hi) == (r * n // G, (r + 1) * n // G), (r, lo, hi)
            out[r] = drive(sims[r], r, lo, hi, notes[r])
            notes[r].check(sims[r].exchange_stats()["bytes_sent"] > 0, "sent nothing over the transport")
        except BaseException as e:  # noqa: BLE001 - reported per rank
            errs[r] = e

    try:
        for r in range(G):
            sims.append(rp.Sim(n, seed, shards=G, rank=r, loop=loop, **kw))
        threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(G)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
    finally:
        stuck = [r for r, t in enumerate(threads) if t.is_alive()]
        if not stuck:  # (a rank still inside the library keeps its Sim and the group)
            for S in sims:
                S.close()
            loop.close()
    assert not stuck, "ranks %s still running after %.0f s" % (stuck, JOIN_TIMEOUT)
    raised = [e for e in errs if e is not None]
    if raised:  # (the rank that failed first, not one whose collective it broke)
        raise next((e for e in raised if "another rank failed" not in str(e)), raised[0])
    bad = [m for nt in notes for m in nt.notes]
    assert not bad, "%d mismatches:\n%s" % (sum(nt.count for nt in notes), "\n".join(bad))
    return out


# ---------------------------------------------------------------- the oracle
class Trace:
    """One oracle run, stepped once and shared by the ranks: per round the
    counts and every node's checksum (None: dead or not joined yet), at the
    end every live node's view, member order, dissemination log and info."""

    def __init__(self, n, seed, rounds, churn_rounds, **kw):
        import oracle
        c = oracle.Sim(n, seed, **kw)
        self.n, self.churn_rounds = n, churn_rounds
        self.rounds = []
        for r in range(rounds):
            o = c.round(churn=r < churn_rounds)
            self.rounds.append(({k: int(o[k]) for k in STAT_KEYS}, c.checksums()))
        self.nodes = []
        for v in range(n):
            info = c.info(v)
            if info["dead"]:  # fail-stopped, or never joined
                self.nodes.append(None)
                continue
            st, inc = c.view(v)
            self.nodes.append({"view": (st.tolist(), inc.tolist()), "members": c.members(v).tolist(),
                               "changes": c.changes(v).tolist(), "info": {k: info[k] for k in INFO_KEYS}})
        c.close()

    def totals(self):
        return {k: sum(o[k] for o, _ in self.rounds) for k in STAT_KEYS}


def check_nodes(S, trace, lo, hi, notes):
    """Every own node that is live in the oracle: view, member order,
    dissemination log (keys in order, counts, sources), ring state, iterator
    and RNG."""
    for v in range(lo, hi):
        f = trace.nodes[v]
        if f is None:
            continue
        st, inc = S.view(v)
        notes.check((st.tolist(), inc.tolist()) == f["view"], "node", v, "view")
        notes.check(S.members(v).tolist() == f["members"], "node", v, "members")
        notes.check(S.changes(v).tolist() == f["changes"], "node", v, "changes")
        info = S.info(v)
        for k in INFO_KEYS:
            notes.check(info[k] == f["info"][k], "node", v, k, info[k], f["info"][k])


def drive_trace(trace):
    """A rank's calls for an oracle scenario: every round's counts and own
    checksums, then every own node."""
    def drive(S, rank, lo, hi, notes):
        for r, (want, cs) in enumerate(trace.rounds):
            o = S.round(churn=r < trace.churn_rounds)
            for k in STAT_KEYS:
                notes.check(o[k] == want[k], "round", r, k, o[k], want[k])
            got = S.checksums()[lo:hi].tolist()
            notes.check([None if w is None else x for x, w in zip(got, cs[lo:hi])] == cs[lo:hi], "round", r, "checksums")
        check_nodes(S, trace, lo, hi, notes)
        return S.local_counters(), S.counters()
    return drive


def drive_run(trace, k):
    """rp_sim_run(k) then a sync: the totals, own checksums and own nodes
    after k rounds enqueued back to back."""
    def drive(S, rank, lo, hi, notes):
        S.run(k, churn=True)
        S.sync()
        got, want = S.totals(), trace.totals()
        for key in STAT_KEYS:
            gk = "converged_rounds" if key == "converged" else key
            notes.check(got[gk] == want[key], "totals", key, got[gk], want[key])
        cs = trace.rounds[-1][1]
        mine = S.checksums()[lo:hi].tolist()
        notes.check([None if w is None else x for x, w in zip(mine, cs[lo:hi])] == cs[lo:hi], "checksums")
        check_nodes(S, trace, lo, hi, notes)
    return drive


# ------------------------------------------------- the reference's fixtures
def views_of(cfg):
    """cfg["views"][i][j] = [status, incarnation] -> (status, inc) arrays, or None"""
    if "views" not in cfg:
        return None
    v = np.array(cfg["views"], dtype=np.int64)
    return v[:, :, 0], v[:, :, 1]


def case_kwargs(cfg):
    """rp.Sim's keyword arguments for a fixture case (test_gpu_parity._gpu_matches_case)."""
    return dict(churn_k=cfg.get("churnK"), failures={int(k): v for k, v in cfg.get("failures", {}).items()},
                partition=cfg.get("partition"), storm=cfg.get("storm"), addresses=cfg.get("addresses"),
                views=views_of(cfg), joins=[tuple(e) for e in cfg.get("joins", [])] or None)


def drive_case(case):
    """test_gpu_parity._gpu_matches_case on the nodes [lo, hi) of a rank:
    every round's counts, own checksums and convergence flag; the final dump
    of every own node where the case has one, else the final checksums."""
    cfg = case["config"]

    def drive(S, rank, lo, hi, notes):
        for r, jr in enumerate(case["rounds"]):
            o = S.round(churn=r < cfg["churnRounds"])
            for k, jk in ROUND_KEYS:
                notes.check(o[k] == jr[jk], "round", r, k, o[k], jr[jk])
            want = jr["checksums"][lo:hi]
            got = S.checksums()[lo:hi].tolist()
            notes.check([None if w is None else x for x, w in zip(got, want)] == want, "round", r, "checksums")
            notes.check(bool(o["converged"]) == jr["converged"], "round", r, "converged")
        for v in range(lo, hi) if "final" in case else ():
            f = case["final"][v]
            st, inc = S.view(v)
            want = [(0, 0) if e is None else tuple(e) for e in f["view"]]
            notes.check(list(zip(st.tolist(), inc.tolist())) == want, "node", v, "view")
            notes.check(S.members(v).tolist() == f["members"], "node", v, "members")
            notes.check(S.changes(v).tolist() == f["changes"], "node", v, "changes")
            info = S.info(v)
            notes.check(info["max_pb"] == f["maxPiggyback"] and info["ring_servers"] == f["ringServers"], "node", v, "ring")
            if f["ringChecksum"] is not None:  # (an empty ring never computed one: a node that never joined)
                notes.check(info["ring_checksum"] == f["ringChecksum"], "node", v, "ring checksum")
            notes.check(info["iter_index"] == f["iterIndex"] and info["iter_round"] == f["iterRound"], "node", v, "iterator")
            notes.check((info["rng"] & (2**64 - 1)) == int(f["rng"]), "node", v, "rng")
        if "final_checksums" in case:
            want = case["final_checksums"][lo:hi]
            got = S.checksums()[lo:hi].tolist()
            notes.check([None if w is None else x for x, w in zip(got, want)] == want, "final checksums")
        if cfg.get("addresses"):
            notes.check([S.address(v) for v in range(lo, hi)] == cfg["addresses"][lo:hi], "addresses")
    return drive


# ---------------------------------------- drawn scenarios and their conditions
def join_scenario(n=128, G=4):
    """n nodes on G ranks: 32 members from the start, the others join 16 per
    round through 3 seeds each (members or earlier joiners), with churn and one
    fail-stop among the members (test_sim_join_against_oracle's shape):
    (Sim keyword arguments, rounds, churn rounds)."""
    r = np.random.default_rng(9)
    ids = r.permutation(n).tolist()
    members, joins, rnd = ids[:32], [], 0
    failed = {3: [members[5]]}
    for q in range(32, n, 16):
        batch = ids[q:q + 16]
        for j in batch:
            joins.append((rnd, j, [int(x) for x in r.choice(members, size=3, replace=False)]))
        members = members + batch
        rnd += 1
    dead = {m for v in failed.values() for m in v}
    joins = [(a, j, [x for x in sd if x not in dead]) for a, j, sd in joins]
    return dict(churn_k=3, joins=joins, failures=failed), 40, 20


def check_join_schedule(joins, n, G):
    """What the join cases are there for, from the schedule alone: a reply
    (one per seed of a joiner, broadcast from the seed's rank: rp_sim::
    join_step) crosses ranks, another stays on its rank, some round's replies
    are rooted at two or more ranks, and a seed is itself an earlier joiner."""
    rank = lambda v: v // (n // G)  # noqa: E731
    joined = {j: a for a, j, _ in joins}
    pairs = [(a, j, s) for a, j, sd in joins for s in sd]
    assert any(rank(s) != rank(j) for _, j, s in pairs), "no reply crosses ranks"
    assert any(rank(s) == rank(j) for _, j, s in pairs), "no reply stays on its rank"
    roots = {}
    for a, _, s in pairs:
        roots.setdefault(a, set()).add(rank(s))
    assert any(len(x) >= 2 for x in roots.values()), "no round has replies rooted at two ranks"
    assert any(s in joined and joined[s] < a for a, _, s in pairs), "no seed joined in an earlier round"
    assert all(s not in joined or joined[s] < a for a, _, s in pairs)  # (what rp_sim_join accepts)


def views_scenario(n=128):
    """Loaded random addresses of 4 to 32 bytes and random bootstrap views
    (test_sim_views_against_oracle's shape): a base column state per member
    (alive, suspect, faulty or leave), 5 % of the cells redrawn over statuses
    1-4, one member absent from every view but its own, and two fail-stops at
    round 2: (Sim keyword arguments, rounds, churn rounds, the absent member)."""
    r = np.random.default_rng(5)
    alphabet = np.frombuffer(b"0123456789abcdefghijklmnopqrstuvwxyz.:-", dtype=np.uint8)
    addrs = set()
    while len(addrs) < n:
        addrs.add(bytes(r.choice(alphabet, size=int(r.integers(4, 33)))).decode())
    addrs = sorted(addrs)
    base_st = r.choice([1, 1, 1, 1, 1, 1, 2, 3, 4], size=n)
    base_inc = 1434401518824 + np.arange(n) + 1000 * r.integers(0, 4, size=n)
    st = np.tile(base_st, (n, 1)).astype(np.int32)
    inc = np.tile(base_inc, (n, 1)).astype(np.int64)
    noise = r.random((n, n)) < 0.05
    st[noise] = r.choice([1, 2, 3, 4], size=int(noise.sum()))
    inc[noise] += 1000 * r.integers(0, 2, size=int(noise.sum()))
    absent = 77
    st[:, absent] = 0
    st[np.arange(n), np.arange(n)] = 1
    return dict(churn_k=3, addresses=addrs, views=(st, inc), failures={2: [7, 100]}), 40, 15, absent


def check_view_spread(st, n, G):
    """Absent, suspect, faulty and leave cells each occur in the rows of at
    least two ranks."""
    nl = n // G
    for status in (0, 2, 3, 4):
        ranks = [g for g in range(G) if (st[g * nl:(g + 1) * nl] == status).any()]
        assert len(ranks) >= 2, (status, ranks)
