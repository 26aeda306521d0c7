"""The one-wave issue kernels (k_phase1_wave / k_p2_respond_wave: wave_issue,
DESIGN §6.12) against the oracle and against the block kernels they replace
in runs without faults on n % 64 == 0 nodes.  Every case checks the
`wave_issues` counter, so that no comparison can be the block path against
itself."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

ROUND_KEYS = ("evaluated", "applied", "full_syncs", "messages", "waves", "converged")


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def _same_round(a, b, r):
    for key in ROUND_KEYS:
        assert a[key] == b[key], (r, key, a[key], b[key])


def _same_checksums(g, c, r):
    want = c.checksums()
    got = g.checksums().tolist()
    assert [x if w is not None else None for x, w in zip(got, want)] == want, r


def _same_node(g, c, v):
    assert g.changes(v).tolist() == c.changes(v).tolist(), v
    assert np.array_equal(g.view(v)[0], c.view(v)[0]) and np.array_equal(g.view(v)[1], c.view(v)[1]), v
    assert g.members(v).tolist() == c.members(v).tolist(), v


def _against_oracle(rp, n, seed, k, rounds, issue_wave=2, **kw):
    g = rp.Sim(n, seed, churn_k=k, issue_wave=issue_wave, **kw)
    c = oracle.Sim(n, seed, churn_k=k)
    g.max_window = 0.0  # the largest mean window of a round's sender issues (a lower bound of the largest window)
    scanned = pings = 0
    for r in range(rounds):
        a = g.round(churn=r < rounds * 2 // 3)
        b = c.round(churn=r < rounds * 2 // 3)
        _same_round(a, b, r)
        _same_checksums(g, c, r)
        cnt = g.counters()
        g.max_window = max(g.max_window, (cnt["scanned_send_issue"] - scanned) / max(1, cnt["pings"] - pings))
        scanned, pings = cnt["scanned_send_issue"], cnt["pings"]
    for v in range(0, n, max(1, n // 13)):
        _same_node(g, c, v)
    return g, c


@pytest.mark.parametrize("n,seed,k,rounds", [
    # one group per row: with an unaligned head two groups share the row's 64 slots, on disjoint lanes
    (64, 3, 2, 60),
    # the row wraps between groups
    (128, 4, 3, 60),
    (192, 5, 4, 60),
    # windows longer than one unrolled iteration (8 groups, 512 entries): observed, the largest mean
    # window of a round's sender issues is 724 entries with 48 re-assertions a round (365 with 24: not
    # enough), so single issues scan more than that; asserted below
    (1024, 6, 48, 50),
])
def test_wave_issue_against_oracle(rp, n, seed, k, rounds):
    """Case 1: no faults, wave path forced; every round's counters and
    checksums, and sampled nodes' changes, views and member lists at the end."""
    g, _ = _against_oracle(rp, n, seed, k, rounds)
    cnt = g.counters()
    print("wave issues", cnt["wave_issues"], "largest mean sender window of a round", g.max_window, "entries")
    assert cnt["wave_issues"] > 0
    if n == 1024:  # the scan's second batch of groups ran
        assert g.max_window > 512, g.max_window
    # every sender issue took it, and the responses to each receiver's first
    # pings (k_phase2 answers the later ones: the block path)
    assert cnt["pings"] < cnt["wave_issues"] <= 2 * cnt["pings"], (cnt["wave_issues"], cnt["pings"])
    g.close()


@pytest.mark.parametrize("n,seed,k,rounds", [(256, 5, 6, 60), (512, 7, 12, 60)])
@pytest.mark.parametrize("pmin", [1, 8])
def test_wave_issue_packing_and_compaction(rp, n, seed, k, rounds, pmin):
    """Case 2: prefix packing and compaction inside the wave path
    (wave_pack_prefix, wave_compact) forced with tiny thresholds; key order,
    counts and sources must stay the oracle's, which has neither."""
    g, _ = _against_oracle(rp, n, seed, k, rounds, prefix_min=pmin, compact=(1, 16))
    cnt = g.counters()
    print("prefix packs", cnt["prefix_packs"], "compactions", cnt["compactions_issue"], "same-view issues",
          cnt["same_view_issues"], "wave issues", cnt["wave_issues"])
    assert cnt["wave_issues"] > 0
    assert cnt["prefix_packs"] > n, cnt["prefix_packs"]
    assert cnt["compactions_issue"] > 0
    assert cnt["same_view_issues"] > 0
    g.close()


def _wave_equals_block(rp, n, seed, k, rounds, shards):
    """The same run on the wave kernels (switch 2) and the block kernels
    (switch 1): counters and checksums after every round, every node at the end."""
    w = rp.Sim(n, seed, churn_k=k, shards=shards, issue_wave=2)
    b = rp.Sim(n, seed, churn_k=k, shards=shards, issue_wave=1)
    for r in range(rounds):
        x, y = w.round(churn=r < rounds * 2 // 3), b.round(churn=r < rounds * 2 // 3)
        assert x == y, (r, x, y)
        assert np.array_equal(w.checksums(), b.checksums()), r
    for v in range(n):
        assert np.array_equal(w.changes(v), b.changes(v)), v
        assert np.array_equal(w.view(v)[0], b.view(v)[0]) and np.array_equal(w.view(v)[1], b.view(v)[1]), v
        assert np.array_equal(w.members(v), b.members(v)), v
    cw, cb = w.counters(), b.counters()
    assert cw["wave_issues"] > 0 and cb["wave_issues"] == 0, (cw["wave_issues"], cb["wave_issues"])
    # (not written_recv_issue: k_phase2 merges into a receiver's seen bitset while
    # other receivers' responses read it, so how many provable no-ops a
    # response leaves out varies from run to run on either path)
    for key in ("scanned_send_issue", "emitted_send_issue", "written_send_issue", "scanned_recv_issue",
                "emitted_recv_issue", "prefix_packs", "compactions_issue", "same_view_issues"):
        assert cw[key] == cb[key], (key, cw[key], cb[key])
    return w, b


@pytest.mark.parametrize("n,seed,k,shards", [(2048, 11, 20, 1), (256, 12, 5, 4)])
def test_wave_issue_equals_block_issue(rp, n, seed, k, shards):
    """Case 3: one shard at n = 2048 (windows of several unrolled iterations),
    and four shards at n = 256 (the ESC instantiation: written entries without
    a makeAlive origin are counted as wire escapes)."""
    w, b = _wave_equals_block(rp, n, seed, k, 40, shards)
    w.close()
    b.close()


def test_wave_issue_receiver_filter(rp):
    """Case 4: a cluster created without faults whose logs come to hold
    changes with a source and a source incarnation (injected through
    Sim.update, the wire bridge: `dangerous` is set), so issueAsReceiver's
    sender filter (lib/dissemination.js:91-98) can match in the wave kernel.
    Wave path == block path == oracle over the rounds that follow."""
    n, seed, k, rounds = 128, 21, 3, 24
    c = oracle.Sim(n, seed, churn_k=k)

    def inject(r, *sims):
        if r not in (3, 4, 9):
            return
        # suspect claims about a few members, each said to come from a live
        # node s at its current incarnation, planted at several holders: when s
        # pings a holder, the holder's response filters them
        rng = np.random.default_rng(100 + r)
        inc = c.view(0)[1]
        for s in rng.choice(n, size=6, replace=False):
            x = int((s + 1 + rng.integers(0, n - 1)) % n)
            row = np.array([[x, 2, int(inc[x]), int(s), int(c.view(int(s))[1][int(s)])]], dtype=np.int64)
            for h in rng.choice(n, size=24, replace=False):
                if int(h) in (x, int(s)):
                    continue
                got = [sim.update(int(h), row) for sim in sims]
                assert got == [got[0]] * len(got), (r, int(h), got)

    w = rp.Sim(n, seed, churn_k=k, issue_wave=2)
    b = rp.Sim(n, seed, churn_k=k, issue_wave=1)
    for r in range(rounds):
        inject(r, w, b, c)
        x, y, z = w.round(churn=r < 16), b.round(churn=r < 16), c.round(churn=r < 16)
        assert x == y, (r, x, y)
        _same_round(x, z, r)
        assert np.array_equal(w.checksums(), b.checksums()), r
        _same_checksums(w, c, r)
    for v in range(n):
        assert np.array_equal(w.changes(v), b.changes(v)), v
        _same_node(w, c, v)
    cw, cb = w.counters(), b.counters()
    assert cw["wave_issues"] > 0 and cb["wave_issues"] == 0
    w.close()
    b.close()


def test_wave_issue_ineligible_shape_takes_block_kernels(rp):
    """Case 5: n = 300 (rows that are no whole number of 64-entry groups) with
    the switch on the wave kernels still runs the block kernels -- the one
    case where the counter must stay 0 -- and matches the oracle."""
    g, _ = _against_oracle(rp, 300, 9, 4, 40)
    assert g.counters()["wave_issues"] == 0
    g.close()
