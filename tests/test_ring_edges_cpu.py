"""tests/ring_cases.py on the CPU: RingModel against the C oracle's ring
(oracle/sim_oracle.c orc_ring_*) after every call of the small scenarios and
against the reference's own HashRing (tests/golden/ring_collisions.json,
ring_edges.json); the floors that keep every scenario on the edge it is there
for; and the constants of the sources the shapes are built around."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
import ring_cases as rc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ringpop_amd", "csrc")


def _blob(names):
    bs = [s.encode() for s in names]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in bs]) if bs else []
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8), off


class OracleRing:
    def __init__(self, replicas):
        self.L = oracle.lib()
        self.r = self.L.orc_ring_new(replicas)

    def add_remove(self, add, ah, rm, rh):
        ab, ao = _blob(add)
        rb, ro = _blob(rm)
        ah = np.ascontiguousarray(ah, dtype=np.uint32).reshape(-1)
        rh = np.ascontiguousarray(rh, dtype=np.uint32).reshape(-1)
        return bool(self.L.orc_ring_add_remove(self.r, oracle._ptr(ab), oracle._ptr(ao), len(add),
                                               oracle._ptr(ah) if len(add) else None, oracle._ptr(rb),
                                               oracle._ptr(ro), len(rm), oracle._ptr(rh) if len(rm) else None))

    def name(self, i):
        if i < 0:
            return None
        buf = ctypes.create_string_buffer(64)
        self.L.orc_ring_server_name(self.r, int(i), buf, 64)
        return buf.value.decode()

    def points(self):
        n = self.L.orc_ring_points(self.r, None, None)
        H = np.zeros(max(n, 1), dtype=np.uint32)
        O = np.zeros(max(n, 1), dtype=np.int32)
        self.L.orc_ring_points(self.r, oracle._ptr(H), oracle._ptr(O))
        return H[:n], O[:n]

    def lookup(self, hashes):
        h = np.ascontiguousarray(hashes, dtype=np.uint32)
        out = np.zeros(len(h), dtype=np.int32)
        self.L.orc_ring_lookup_hashes(self.r, oracle._ptr(h), len(h), oracle._ptr(out))
        return out

    def lookup_n(self, h, n):
        out = np.full(max(n, 1), -1, dtype=np.int32)
        k = self.L.orc_ring_lookup_n(self.r, int(h), int(n), oracle._ptr(out))
        return out[:k].tolist()

    def count(self):
        return self.L.orc_ring_server_count(self.r)

    def close(self):
        self.L.orc_ring_free(self.r)


def _ns(count):
    return list(rc.LOOKUP_N) + ([count, count + 3] if count <= rc.N_ALL_MAX else [])


@pytest.mark.parametrize("name", rc.SMALL)
def test_model_matches_oracle(name):
    """after every call: changed, the points with their owners' names, the
    server count, lookup on the scenario's probes and lookupN on its placed
    values (n in 1, 2, 3; on rings of at most 300 servers also count and
    count + 3, which leaves those two out while delta_edges holds 2,000 to
    18,000 one-point servers: an n of that size is a walk of the whole ring
    per probe.  delta_edges compares lookupN on every third probe.)"""
    sc = rc.scenario(name)
    orc = OracleRing(sc.R)
    probes = rc.probes(sc)
    nprobes = probes[::3] if name == "delta_edges" else probes  # (47 calls, one oracle call per probe and n)
    try:
        for step, (c, m, changed) in enumerate(sc.replay()):
            assert orc.add_remove(c.add, c.add_h, c.rm, c.rm_h) == changed, step
            oh, oo = orc.points()
            assert np.array_equal(m.h, oh), step
            names = {int(i): orc.name(i) for i in np.unique(oo)}
            assert m.owner_names(m.own).tolist() == [names[int(i)] for i in oo], step
            assert m.count == orc.count(), step
            got = orc.lookup(probes)
            names[-1] = None
            assert m.owner_names(m.lookup(probes)).tolist() == [names[int(i)] for i in got], step
            for n in _ns(m.count):
                # (the oracle walks O(points * n) per probe: beyond n = 100 every 8th probe)
                for x in (nprobes[::8] if n > 100 else nprobes):
                    a, b = m.lookup_n(x, n), orc.lookup_n(x, n)
                    assert [m.names[i] for i in a] == [names[i] for i in b], (step, n, int(x))
    finally:
        orc.close()


@pytest.mark.parametrize("fixture", ["ring_collisions.json", "ring_edges.json"])
def test_model_and_oracle_match_reference_fixture(golden, fixture):
    """the reference's HashRing through its hashFunc seam: forced collisions,
    and points at 0 and 4294967295 with a present server that owns nothing.
    lookupN for n >= 1 (n = 0: the reference's do-while returns one owner
    unless the key lies past the largest point; this project returns none,
    INTEGRATION.md section 1 -- recorded in the fixture, not compared)"""
    g = golden(fixture)
    R = g["replica_points"]
    if fixture == "ring_edges.json":
        rows = lambda s: np.array(g["table"][s], dtype=np.uint32)
        probes = np.array(g["probes"], dtype=np.uint32)
    else:
        rows = lambda s: np.array([g["table"][f"{s}{i}"] for i in range(R)], dtype=np.uint32)
        probes = np.array([int(p[4:]) for p in g["probes"]], dtype=np.uint32)
    m, orc = rc.RingModel(R), OracleRing(R)
    try:
        for step in g["steps"]:
            add, rm = step["add"], step["remove"]
            ah = np.stack([rows(s) for s in add]) if add else np.zeros((0, R), np.uint32)
            rh = np.stack([rows(s) for s in rm]) if rm else np.zeros((0, R), np.uint32)
            assert m.add_remove(add, ah, rm, rh) == step["changed"]
            assert orc.add_remove(add, ah, rm, rh) == step["changed"]
            assert [[int(a), b] for a, b in zip(m.h, m.owner_names(m.own))] == step["points"]
            oh, oo = orc.points()
            assert [[int(a), orc.name(b)] for a, b in zip(oh, oo)] == step["points"]
            assert m.count == orc.count() == len(step["servers"])
            assert m.owner_names(m.lookup(probes)).tolist() == step["lookups"]
            assert [orc.name(i) for i in orc.lookup(probes)] == step["lookups"]
            if fixture == "ring_edges.json":
                for n in g["ns"]:
                    if n == 0:
                        continue
                    want = step["lookupN"][str(n)]
                    assert [[m.names[i] for i in m.lookup_n(x, n)] for x in probes] == want, n
                    assert [[orc.name(i) for i in orc.lookup_n(x, n)] for x in probes] == want, n
            else:
                want = step["lookupN"]
                assert [[m.names[i] for i in m.lookup_n(x, 3)] for x in probes[:40]] == want
    finally:
        orc.close()


def test_ring_edges_fixture_has_its_edges(golden):
    g = golden("ring_edges.json")
    first = g["steps"][0]
    hashes = [p[0] for p in first["points"]]
    assert 0 in hashes and 4294967295 in hashes
    assert "D" in first["servers"] and all(o != "D" for _, o in first["points"])  # present, owns nothing
    assert g["steps"][-1]["points"] == [] and g["steps"][-1]["lookups"][0] is None
    # the n = 0 divergence is on record: one owner, or none past the largest point
    second = g["steps"][1]
    assert second["lookupN"]["0"][0] == ["C"] and second["lookupN"]["0"][-1] == []


# What each scenario is there for, as conditions on its inputs (from the
# seeded inputs' own counts, with room below them): an edit that moves a case
# off its edge fails here.
PLACED_FLOOR = {"exact": 50, "one_above": 50, "one_below": 50, "last_key_11": 20, "first_key_11": 20,
                "last_key_16": 20, "first_key_16": 20}


@pytest.mark.parametrize("name", rc.PLACED)
def test_placed_scenarios_keep_their_edges(name):
    cov = rc.cover(rc.scenario(name).model)
    for k, floor in PLACED_FLOOR.items():
        assert cov[k] >= floor, (name, k, cov)


def test_scenarios_reach_their_paths():
    cov = {n: rc.cover(rc.scenario(n).model) for n in rc.SMALL + rc.LARGE}
    # placed_small / no_extremes: incremental calls whose delta is staged, a ring under the scatter threshold
    for n in ("placed_small", "no_extremes"):
        words = []
        for _, m, _ in rc.scenario(n).replay():
            assert 0 < m.touched <= rc.INCR_MAX
            words.append(2 * m.delta[0] + m.delta[1])
        # (the last call's draws repeat earlier hashes: a few hundred inserts through k_ring_merge_small)
        assert sum(w > rc.DELTA_WORDS for w in words) >= 3 and min(words) > 0
        assert cov[n]["points"] < rc.SCATTER_MIN and cov[n]["present_owning_nothing"] >= 1
    assert cov["placed_small"]["wraps"] == 0  # (0xFFFFFFFF is a point)
    assert cov["no_extremes"]["wraps"] >= 5 and cov["no_extremes"]["at_or_below_min"] >= 5
    # a directory bucket past the last point
    assert int(rc.scenario("no_extremes").model.h.max()) >> rc.S_DIR < (1 << 21) - 1
    # placed_bulk: one bulk add with about half the hashes colliding, one bulk remove erasing others' points
    calls = list(rc.scenario("placed_bulk").calls)
    touched, deltas = [], []
    for _, m, _ in rc.scenario("placed_bulk").replay():
        touched.append(m.touched)
        deltas.append(m.delta)
    assert touched[0] == 9600 > rc.INCR_MAX and 3500 <= deltas[0][0] <= 6000
    gone = np.unique(calls[1].rm_h)
    first = rc.RingModel(32)
    first.add_remove(calls[0].add, calls[0].add_h, [], [])
    victims = first.owner_names(first.own[np.isin(first.h, gone)])
    assert sum(v not in set(calls[1].rm) for v in victims) >= 100
    # scatter / dense_group / many_servers: k_index_build; dense_group once below the threshold too
    assert cov["scatter"]["points"] >= rc.SCATTER_MIN and cov["scatter"]["max_group"] < 0x8000
    dense = [(len(m.h), rc.cover(m)["max_group"]) for _, m, _ in rc.scenario("dense_group").replay()]
    assert dense[0][0] < rc.SCATTER_MIN <= dense[1][0] and dense[0][1] >= 0x8000 and dense[1][1] >= 0x8000
    # many_names: owner ids on both sides of 0x8000 on a small ring; many_servers: on a large one
    assert cov["many_names"]["points"] < rc.SCATTER_MIN
    assert cov["many_names"]["own_lt_0x8000"] >= 100 and cov["many_names"]["own_ge_0x8000"] >= 100
    assert cov["many_names"]["max_group"] < 0x8000  # (only the owner ids keep it out of the 16-bit directory)
    assert cov["many_servers"]["points"] >= rc.SCATTER_MIN
    assert cov["many_servers"]["own_lt_0x8000"] >= 100 and cov["many_servers"]["own_ge_0x8000"] >= 100


def test_many_names_is_misread_by_a_bit15_rule():
    """What many_names is there for, restated: the 16-bit directory of its
    final ring (k_dir_both's entries: a direct owner, or 0x8000 | offset from
    the group's first point) read the way k_lookup_keys reads it.  With the
    overflow test keyed on bit 15 of the entry, as it once was, the directory
    is not flagged and keys of K get another owner, some from a start index
    past the points; keyed on the branch taken it is flagged."""
    m = rc.scenario("many_names").model
    h, own, n = m.h.astype(np.int64), m.own.astype(np.int64), len(m.h)
    b = np.arange(1 << 21, dtype=np.int64)
    lo = np.searchsorted(h, b << rc.S_DIR)
    base = lo[(b >> 6) << 6]
    hv = h[np.minimum(lo, n - 1)]
    direct = (lo == n) | (hv >= (b << rc.S_DIR) + (1 << rc.S_DIR) - 1)
    e = np.where(lo == n, own[0], np.where(direct, own[np.minimum(lo, n - 1)], 0x8000 | (lo - base)))
    assert np.where(direct, e >= 0x8000, lo - base >= 0x8000).any()              # by the branch: flagged
    assert not np.where((e & 0x8000) != 0, lo - base >= 0x8000, e >= 0x8000).any()  # by bit 15: not flagged
    kh = rc.key_hashes().astype(np.int64)
    e16 = e[kh >> rc.S_DIR]
    start = base[(kh >> rc.S_GROUP) << 6] + (e16 & 0x7FFF)
    wrong = past = 0
    for x, ent, p, want in zip(kh, e16, start, m.lookup(rc.key_hashes())):
        if not ent & 0x8000:
            wrong += ent != want
        elif p > n:
            past += 1
        else:
            while p < n and h[p] < x:
                p += 1
            wrong += own[p % n] != want
    assert wrong + past >= 20 and past >= 1, (wrong, past)  # (39 and 10 with the seeded inputs)


def test_delta_edges_hits_every_switch():
    sc = rc.scenario("delta_edges")
    words, touched, empty, taken, single = set(), set(), False, False, set()
    for c, m, changed in sc.replay():
        words.add(2 * m.delta[0] + m.delta[1])
        touched.add(m.touched)
        empty |= len(m.h) == 0 and bool(c.rm)
        taken |= changed and m.delta == (0, 0) and bool(c.add)
        if m.touched == 1:
            single.add((int(c.add_h[0, 0]) if c.add else int(c.rm_h[0, 0]), bool(c.add)))
    W, T = rc.DELTA_WORDS, rc.INCR_MAX
    assert {W - 1, W, W + 1} <= words and {T, T + 1} <= touched and empty and taken
    for x in (0, rc.M32, 1 << 16, (1 << 16) - 1, 0x8000 << 16, (0x8000 << 16) - 1, 0xFFFF << 16, (0xFFFF << 16) - 1):
        assert (x, True) in single and (x, False) in single, hex(x)


@pytest.mark.parametrize("S,run", rc.SORT_RUNS)
def test_sort_runs_shape(S, run):
    sc = rc.scenario("sort_runs", S, run)
    assert S > rc.INCR_MAX  # (one replica per server: the call is bulk)
    m = sc.model
    assert len(m.h) == -(-S // (run or S)) and m.count == 2 * S
    assert np.array_equal(np.sort(m.own), np.arange(0, S, run or S))


def _constant(text, name):
    m = re.search(r"(?:#define|constexpr\s+\w+)\s+%s\s*=?\s*([^;\n]+)" % name, text)
    assert m, name
    return m.group(1).split("//")[0].strip()


def test_constants():
    """the numbers the scenarios are built around; after a retune move the
    cases in tests/ring_cases.py to the new switches, then the values here"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("rp_ring.h", "rp_capi.hip", "rp_sort.h", "rp_block.h")}
    hint = "retuned: move the cases of tests/ring_cases.py to the new value, then CONSTANTS"
    C = rc.CONSTANTS
    assert int(_constant(src["rp_capi.hip"], "RP_RING_INCR_MAX_POINTS")) == C["RP_RING_INCR_MAX_POINTS"], hint
    assert int(_constant(src["rp_ring.h"], "RING_DELTA_WORDS")) == C["RING_DELTA_WORDS"], hint
    assert int(_constant(src["rp_ring.h"], "RP_DIR_BITS")) == C["RP_DIR_BITS"], hint
    assert int(_constant(src["rp_ring.h"], "RP_D16_BITS")) == C["RP_D16_BITS"], hint
    assert int(_constant(src["rp_ring.h"], "D16_GROUP_LOG")) == C["D16_GROUP_LOG"], hint
    assert _constant(src["rp_ring.h"], "INDEX_SCATTER_MIN") == "DIR_SIZE / 4", hint
    assert _constant(src["rp_ring.h"], "DIR_SIZE") == "1u << DIR_BITS", hint
    assert C["INDEX_SCATTER_MIN"] == (1 << C["RP_DIR_BITS"]) // 4
    assert _constant(src["rp_sort.h"], "PS_TILE") == "BLOCK * PS_IPT", hint
    assert int(_constant(src["rp_block.h"], "BLOCK")) * int(_constant(src["rp_sort.h"], "PS_IPT")) == C["PS_TILE"], hint
    assert int(_constant(src["rp_ring.h"], "HASH_LONG_MIN")) == C["HASH_LONG_MIN"], hint
