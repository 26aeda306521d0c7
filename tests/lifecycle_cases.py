"""Shared by the graceful leave / rejoin tests: the fixture
tests/golden/sim_lifecycle.json.gz recorded from the reference by
tools/gen_lifecycle_fixture.js, and the comparison of a device run with one
of its cases."""
FIXTURE = "sim_lifecycle.json.gz"
STORM, PARTITION, PIGGYBACK, SHARDED, JOIN = range(5)
ROUND_KEYS = (("evaluated", "evaluated"), ("applied", "applied"), ("full_syncs", "fullSyncs"), ("messages", "messages"),
              ("waves", "waves"))


def sim_kwargs(cfg):
    """rp.Sim's keyword arguments for a fixture case's configuration."""
    ints = lambda d: {int(k): v for k, v in (d or {}).items()}  # noqa: E731
    return dict(churn_k=cfg.get("churnK"), failures=ints(cfg.get("failures")), partition=cfg.get("partition"),
                storm=cfg.get("storm"), addresses=cfg.get("addresses"),
                joins=[tuple(e) for e in cfg.get("joins", [])] or None, leaves=ints(cfg.get("leaves")),
                rejoins=ints(cfg.get("rejoins")))


def check_round(o, jr, r):
    for k, jk in ROUND_KEYS:
        assert o[k] == jr[jk], (r, k, o[k], jr[jk])
    assert bool(o["converged"]) == jr["converged"], r


def check_checksums(got, jr, r, lo=0, hi=None):
    want = jr["checksums"][lo:hi]
    assert [None if w is None else int(x) for x, w in zip(got[lo:hi], want)] == want, r


def check_dump(S, dump, r, lo=0, hi=None):
    """Nodes lo .. hi - 1 of the simulation against a full dump of the reference."""
    for v in range(lo, len(dump) if hi is None else hi):
        f = dump[v]
        st, inc = S.view(v)
        want = [(0, 0) if e is None else tuple(e) for e in f["view"]]
        assert list(zip(st.tolist(), inc.tolist())) == want, (r, v)
        assert S.members(v).tolist() == f["members"], (r, v)
        assert S.changes(v).tolist() == f["changes"], (r, v)  # keys in order, counts, sources
        info = S.info(v)
        assert info["max_pb"] == f["maxPiggyback"] and info["ring_servers"] == f["ringServers"], (r, v)
        if f["ringChecksum"] is not None:  # (a node that never joined never computed one)
            assert info["ring_checksum"] == f["ringChecksum"], (r, v)
        assert info["iter_index"] == f["iterIndex"] and info["iter_round"] == f["iterRound"], (r, v)
        assert (info["rng"] & (2**64 - 1)) == int(f["rng"]), (r, v)
        if not f["dead"]:  # (the reference's dump keeps a fail-stopped node's timers; the device drops them)
            assert info["timers"] == len(f["timers"]), (r, v, info["timers"], f["timers"])
        fl = S.flags(v)
        assert fl["gossip_stopped"] == (not f["gossiping"]) and fl["suspicion_stopped"] == f["suspicionStopped"], (r, v)


def run_case(rp, case, lo=0, hi=None, S=None, **kw):
    """Every round of the case and its dumps; returns the simulation."""
    cfg = case["config"]
    if S is None:
        S = rp.Sim(cfg["n"], cfg["seed"], **sim_kwargs(cfg), **kw)
    for r, jr in enumerate(case["rounds"]):
        check_round(S.round(churn=r < cfg["churnRounds"]), jr, r)
        check_checksums(S.checksums().tolist(), jr, r, lo, hi)
        if str(r) in case["dumps"]:
            check_dump(S, case["dumps"][str(r)], r, lo, hi)
    check_dump(S, case["final"], "final", lo, hi)
    return S

