"""GPU parity of graceful leaves and rejoins (rp_sim_leave / rp_sim_rejoin;
DESIGN.md §12) against the reference's own admin handlers
(server/admin-leave-handler.js, server/admin-join-handler.js:36-45), recorded
in tests/golden/sim_lifecycle.json.gz: after every round the counts, every
node's checksum and the convergence flag; at the dump rounds and at the end
every node's view, member order, dissemination log (keys in order, counts,
sources), maxPiggybackCount, ring, iterator, RNG state, pending suspicion
timers and the two flags.  Integer work: bit-exact on 1 to 8 shards and on
loop ranks."""
import threading

import pytest

import lifecycle_cases as lc

pytestmark = pytest.mark.gpu

RP_ERR_INVALID, RP_ERR_STATE = -1, -6


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


@pytest.fixture(scope="module")
def cases(golden):
    return golden(lc.FIXTURE)["cases"]


# (the 10 nodes of the piggyback case split into 1, 2 or 5 shards: 4 does not divide 10)
@pytest.mark.parametrize("idx,shards", [(i, g) for i in range(5) for g in (1, 2, 4) if (i, g) != (lc.PIGGYBACK, 4)] +
                         [(lc.PIGGYBACK, 5), (lc.SHARDED, 8)])
def test_lifecycle_against_reference(rp, cases, idx, shards):
    lc.run_case(rp, cases[idx], shards=shards).close()


@pytest.mark.parametrize("idx", range(5))
@pytest.mark.parametrize("issue_wave,ck_lane_min", [(1, 1), (2, 0xFFFFFFFF)])
def test_lifecycle_kernel_choices_change_nothing(rp, cases, idx, issue_wave, ck_lane_min):
    """The block and the one-wave issue kernels (a run with events takes the
    block ones either way), a lane and a wave per checksummed view."""
    lc.run_case(rp, cases[idx], issue_wave=issue_wave, ck_lane_min=ck_lane_min).close()


def test_lifecycle_loop_ranks(rp, cases):
    """The sharded case on 2 ranks (threads of this process): every rank makes
    the same calls and compares the nodes it holds."""
    from ringpop_amd.sim import Loop
    case = cases[lc.SHARDED]
    cfg = case["config"]
    loop = Loop(2)
    sims = [rp.Sim(cfg["n"], cfg["seed"], shards=2, rank=r, loop=loop, **lc.sim_kwargs(cfg)) for r in range(2)]
    errs = [None, None]

    def rank_main(r):
        try:
            lo, hi = sims[r].shard_range()
            assert (lo, hi) == (r * cfg["n"] // 2, (r + 1) * cfg["n"] // 2)
            lc.run_case(rp, case, lo, hi, S=sims[r])
        except BaseException as e:  # noqa: BLE001 - reported per rank
            errs[r] = e

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for S in sims:
        S.close()
    loop.close()
    for e in errs:
        if e is not None:
            raise e


def test_lifecycle_schedule_is_validated(rp):
    S = rp.Sim(8, 3, churn_k=0)

    def invalid(f, *a):
        with pytest.raises(rp.RingpopError) as e:
            f(*a)
        assert e.value.code == RP_ERR_INVALID, e.value

    invalid(S.rejoin, 2, 4)    # a rejoin first
    invalid(S.leave, 8, 4)     # no such node
    S.leave(2, 4)
    with pytest.raises(rp.RingpopError) as e:  # (the shards it rebuilds would forget the schedule's kernel choices)
        S.load_addresses([f"1.1.1.{i}:1" for i in range(8)])
    assert e.value.code == RP_ERR_STATE
    invalid(S.leave, 2, 6)     # two leaves in a row
    invalid(S.rejoin, 2, 4)    # not a later round
    invalid(S.rejoin, 2, 3)
    S.rejoin(2, 5)
    invalid(S.rejoin, 2, 7)    # two rejoins in a row
    invalid(S.leave, 2, 5)     # not a later round
    S.leave(2, 9)
    for _ in range(3):
        S.round(churn=False)
    invalid(S.leave, 3, 2)     # a past round
    invalid(S.rejoin, 2, 2)
    S.leave(3, 3)              # the current round: allowed, as rp_sim_fail allows it
    assert not S.flags(3)["gossip_stopped"]
    S.round(churn=False)
    assert S.flags(3) == {"gossip_stopped": True, "suspicion_stopped": True}
    S.round(churn=False)
    assert S.flags(2) == {"gossip_stopped": True, "suspicion_stopped": True} and S.view(2)[0][2] == 4
    S.round(churn=False)
    assert S.flags(2) == {"gossip_stopped": False, "suspicion_stopped": False} and S.view(2)[0][2] == 1
    S.close()


def test_rejoin_of_a_node_that_is_not_leave_is_an_error(rp):
    """A left node that refuted a suspicion is alive again: the reference would
    run its join-sender, which is not modelled, so the rejoin raises the
    device's flag and the next read returns RP_ERR_STATE.  The suspicion comes
    over the wire bridge (the local override, lib/membership.js:244-254)."""
    S = rp.Sim(4, 5, churn_k=0)
    S.leave(1, 0)
    S.rejoin(1, 2)
    S.round(churn=False)
    st, inc = S.view(1)
    assert st[1] == 4 and S.flags(1)["gossip_stopped"]
    assert S.update(1, [[1, 2, int(inc[1]), 0, int(S.view(0)[1][0])]]) == 1  # node 0 suspects node 1
    assert S.view(1)[0][1] == 1  # refuted: alive, though its gossip is still stopped
    assert S.flags(1)["gossip_stopped"]
    S.round(churn=False)
    with pytest.raises(rp.RingpopError) as e:
        S.round(churn=False)
    assert e.value.code == RP_ERR_STATE, e.value
    S.close()
