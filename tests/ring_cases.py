"""The drop-in ring at its edges: a NumPy model of the reference's HashRing and
scenarios whose points are placed relative to a fixed key set, shared by
tests/test_ring_edges_cpu.py (model against the C oracle and the reference
fixture, and the floors that keep every scenario on its edge) and
tests/test_gpu_ring_edges.py (the device against the model).  No GPU import.

lib/ring.js + lib/rbtree.js as oracle/sim_oracle.c states them: the ring is a
sorted array of distinct u32 hashes with owners; addRemoveServers adds (in
order, skipping present names), then removes (skipping absent ones); an insert
keeps the first inserter of a hash (lib/rbtree.js:112-117), a remove erases by
hash whoever owns it (:152); lookup is the inclusive lower bound wrapping to
the minimum (lib/ring.js:138-147); lookupN walks one circle collecting
distinct owners (:150-182).

Every scenario is a list of add/remove calls with explicit replica hashes
(the hashFunc seam, lib/ring.js:29), so the points sit where the kernels
branch: on a key, one above and one below it, on the first and last key of a
directory bucket (2^11 hash values) and of a bucket-index bucket (2^16), at 0
and 0xFFFFFFFF, 40,000 deep in one coarse group, and under owner ids on both
sides of 0x8000.  The shapes rest on constants of the sources (CONSTANTS
below); test_ring_edges_cpu.py fails when one of them moves."""
import functools
from collections import namedtuple

import numpy as np

import oracle

U32 = np.uint32
M32 = 0xFFFFFFFF
# the constants the shapes below are built around (checked against the sources
# by test_ring_edges_cpu.py::test_constants)
CONSTANTS = {
    "RP_RING_INCR_MAX_POINTS": 8192,  # touched replica points: at most this many -> incremental
    "RING_DELTA_WORDS": 768,          # 2 * nins + ndel: at most this many -> k_ring_merge_small
    "RP_DIR_BITS": 21,
    "RP_D16_BITS": 21,
    "D16_GROUP_LOG": 6,
    "INDEX_SCATTER_MIN": (1 << 21) // 4,  # DIR_SIZE / 4: at least this many points -> k_index_build
    "PS_TILE": 4096,
    "HASH_LONG_MIN": 1024,
}
INCR_MAX = CONSTANTS["RP_RING_INCR_MAX_POINTS"]
DELTA_WORDS = CONSTANTS["RING_DELTA_WORDS"]
SCATTER_MIN = CONSTANTS["INDEX_SCATTER_MIN"]
S_DIR = 32 - CONSTANTS["RP_DIR_BITS"]          # 11 = DIR_SHIFT = D16_SHIFT
S_GROUP = S_DIR + CONSTANTS["D16_GROUP_LOG"]   # 17: hash values per coarse group of the 16-bit directory
LOOKUP_N = (1, 2, 3)                            # plus count and count + 3 on rings of at most N_ALL_MAX servers
N_ALL_MAX = 300


class RingModel:
    def __init__(self, replicas):
        self.R = replicas
        self.h = np.zeros(0, dtype=U32)
        self.own = np.zeros(0, dtype=np.int32)
        self.names = []   # interned in first-seen order, never reused (rp_ring::intern)
        self.index = {}
        self.present = []
        self.count = 0
        self.touched = 0  # replica points the last call touched (the incremental / bulk switch)
        self.delta = (0, 0)  # points the last call inserted, erased (the merge kernels' switch)

    def _intern(self, name):
        i = self.index.get(name)
        if i is None:
            i = self.index[name] = len(self.names)
            self.names.append(name)
            self.present.append(False)
        return i

    def add_remove(self, add, add_hashes, rm, rm_hashes):
        R = self.R
        before = self.h
        ids, rows = [], []
        for k, name in enumerate(add):
            i = self._intern(name)
            if self.present[i]:  # hasServer (lib/ring.js:72); a repeat within the call too
                continue
            self.present[i] = True
            ids.append(i)
            rows.append(np.asarray(add_hashes[k], dtype=U32).reshape(R))
        if ids:
            allh = np.concatenate([self.h] + rows)
            allo = np.concatenate([self.own, np.repeat(np.array(ids, dtype=np.int32), R)])
            self.h, first = np.unique(allh, return_index=True)  # (first occurrence: the old points come first)
            self.own = allo[first]
        gone = []
        for k, name in enumerate(rm):
            i = self.index.get(name)
            if i is None or not self.present[i]:  # lib/ring.js:81
                continue
            self.present[i] = False
            gone.append(np.asarray(rm_hashes[k], dtype=U32).reshape(R))
        if gone:
            keep = ~np.isin(self.h, np.concatenate(gone))
            self.h, self.own = self.h[keep], self.own[keep]
        self.count += len(ids) - len(gone)
        self.touched = (len(ids) + len(gone)) * R
        self.delta = (int((~np.isin(self.h, before)).sum()), int((~np.isin(before, self.h)).sum()))
        return bool(ids or gone)

    def lookup(self, hashes):
        hashes = np.asarray(hashes, dtype=U32)
        if len(self.h) == 0:
            return np.full(len(hashes), -1, dtype=np.int32)
        p = np.searchsorted(self.h, hashes, side="left")
        p[p == len(self.h)] = 0
        return self.own[p]

    def lookup_n(self, h, n):
        """Owner ids, at most min(n, present servers): a present server may
        own no point, so the walk can end short of that."""
        n = min(n, self.count)
        npts = len(self.h)
        if n <= 0 or npts == 0:
            return []
        start = int(np.searchsorted(self.h, U32(h), side="left"))
        w = min(npts, 4 * n + 16)
        while True:
            o = self.own[(start + np.arange(w)) % npts]
            _, first = np.unique(o, return_index=True)
            if len(first) >= n or w == npts:
                return o[np.sort(first)[:n]].tolist()
            w = min(npts, 4 * w)

    def lookup_n_padded(self, hashes, n):
        """(owners[len(hashes), n] padded with -1, counts) as rp_ring_lookup_n_hashes returns them"""
        out = np.full((len(hashes), max(n, 1)), -1, dtype=np.int32)
        counts = np.zeros(len(hashes), dtype=np.int32)
        for k, x in enumerate(hashes):
            o = self.lookup_n(x, n)
            out[k, :len(o)] = o
            counts[k] = len(o)
        return out[:, :n], counts

    def owner_names(self, ids):
        table = np.array(self.names + [None], dtype=object)  # (-1 -> None: an empty ring)
        return table[np.asarray(ids, dtype=np.int64)]


# ------------------------------------------------------------------ the keys
@functools.lru_cache(None)
def keys():
    """K: 520 decimal u64 strings (config 3's shape), b"", every length from 1
    to 64 (arbitrary bytes, high ones included) and eight strings of 100-300
    bytes."""
    rng = np.random.default_rng(20)
    ks = [s.encode() for s in oracle.lookup_keys(5, np.arange(520))]
    ks.append(b"")
    ks += [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in range(1, 65)]
    ks += [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (100, 127, 128, 129, 200, 255, 256, 300)]
    return tuple(ks)


@functools.lru_cache(None)
def key_hashes():
    kh = oracle.farmhash32_batch(list(keys()))
    kh.setflags(write=False)
    return kh


def placement_pool(seed, lo=None, hi=None):
    """For every key a seeded subset of: the key's hash, one above, one below,
    the first and last key of its directory bucket and of its bucket-index
    bucket; and 0, 1, 0xFFFFFFFE, 0xFFFFFFFF.  Sorted, distinct; lo / hi:
    only the values strictly between them."""
    rng = np.random.default_rng(seed)
    kh = key_hashes().astype(np.uint64)
    d, b = np.uint64((1 << S_DIR) - 1), np.uint64(0xFFFF)
    m = np.uint64(M32)
    cand = np.stack([kh, (kh + np.uint64(1)) & m, (kh + m) & m, kh & (m ^ d), kh | d, kh & (m ^ b), kh | b], axis=1)
    use = rng.random(cand.shape) < 0.45
    vals = np.unique(np.concatenate([cand[use], np.array([0, 1, M32 - 1, M32], dtype=np.uint64)]))
    if lo is not None:
        vals = vals[(vals > np.uint64(lo)) & (vals < np.uint64(hi))]
    return vals.astype(U32)


def _filler(rng, count, avoid):
    """count distinct seeded u32 outside `avoid`, shuffled"""
    x = np.unique(rng.integers(0, 2**32, size=count + count // 8 + 4096, dtype=np.uint64).astype(U32))
    x = x[~np.isin(x, avoid)]
    assert len(x) >= count
    return rng.permutation(x)[:count]


def _draw(rng, values, count):
    """every value once, shuffled; beyond that, draws with replacement"""
    v = rng.permutation(values)
    if count <= len(v):
        return v[:count]
    return np.concatenate([v, rng.choice(values, size=count - len(v))])


# ------------------------------------------------------------- the scenarios
# check: compare the device after this call (the small scenarios: every call)
Call = namedtuple("Call", "add add_h rm rm_h check")


class Scenario:
    """calls with their replica hashes; a name keeps its hashes for life (the
    reference recomputes hashFunc(name + i) on every add and remove)"""

    def __init__(self, name, replicas, large=False):
        self.name, self.R, self.large = name, replicas, large
        self.table = {}
        self.calls = []
        self.pool = np.zeros(0, dtype=U32)  # the placed values: lookup probes
        self.model = RingModel(replicas)  # the ring after the calls so far

    def define(self, names, hashes):
        hashes = np.asarray(hashes).astype(U32).reshape(len(names), self.R)
        for n, row in zip(names, hashes):
            assert n not in self.table
            self.table[n] = row

    def call(self, add=(), rm=(), check=True):
        add, rm = list(add), list(rm)
        ah = np.stack([self.table[n] for n in add]) if add else np.zeros((0, self.R), dtype=U32)
        rh = np.stack([self.table[n] for n in rm]) if rm else np.zeros((0, self.R), dtype=U32)
        self.calls.append(Call(add, ah, rm, rh, check))
        return self.model.add_remove(add, ah, rm, rh)

    def replay(self):
        """(call, model after it, changed) for every call, on a fresh model"""
        m = RingModel(self.R)
        for c in self.calls:
            changed = m.add_remove(c.add, c.add_h, c.rm, c.rm_h)
            yield c, m, changed


def _placed(name, pool, seed):
    """64 servers x 32 replicas in 4 calls of 16 servers (512 touched points
    and a delta over RING_DELTA_WORDS each: incremental, staged)"""
    sc = Scenario(name, 32)
    sc.pool = pool
    rng = np.random.default_rng(seed)
    names = [f"s{i}" for i in range(64)]
    sc.define(names, _draw(rng, pool, 64 * 32))
    for c in range(4):
        sc.call(add=names[16 * c:16 * c + 16])
    return sc


def _placed_small():
    return _placed("placed_small", placement_pool(1), 101)


def _no_extremes():
    """no point at or beyond the 8th smallest / 8th largest key hash: keys on
    both sides of every point, and directory buckets past the last point"""
    kh = np.sort(key_hashes())
    return _placed("no_extremes", placement_pool(2, lo=int(kh[7]), hi=int(kh[-8])), 102)


def _placed_bulk():
    """300 x 32 in one call (9,600 > 8,192 touched points: bulk) drawn with
    replacement from 6,000 values so that about half collide; then 100 servers
    removed by one call, erasing points other servers own"""
    sc = Scenario("placed_bulk", 32)
    rng = np.random.default_rng(103)
    pool = sc.pool = placement_pool(3)
    values = np.concatenate([pool, _filler(rng, 6000 - len(pool), pool)])
    names = [f"s{i}" for i in range(300)]
    sc.define(names, rng.choice(values, size=300 * 32))
    sc.call(add=names)
    sc.call(rm=[names[i] for i in rng.choice(300, size=100, replace=False)])
    return sc


def _scatter_hashes(rng, avoid):
    """655,360 distinct hashes outside `avoid`, shuffled: the pool and filler"""
    pool = placement_pool(4)
    pool = pool[~np.isin(pool, avoid)]
    h = np.concatenate([pool, _filler(rng, 8192 * 80 - len(pool), np.concatenate([pool, avoid]))])
    return pool, rng.permutation(h)


def _scatter():
    """8,192 x 80 distinct hashes: k_index_build"""
    sc = Scenario("scatter", 80, large=True)
    sc.pool, h = _scatter_hashes(np.random.default_rng(104), np.zeros(0, dtype=U32))
    names = [f"w{i}" for i in range(8192)]
    sc.define(names, h)
    sc.call(add=names)
    return sc


def _dense_group():
    """400 x 100 on 40,000 consecutive hashes in one coarse group of the
    16-bit directory (escape offsets >= 0x8000: not representable, lookups
    through the 32-bit directory), built by k_dir_both; then scatter's hashes
    on top as 6,553 more servers (k_index_build)"""
    assert S_GROUP == 17
    sc = Scenario("dense_group", 100, large=True)
    rng = np.random.default_rng(105)
    start = int(key_hashes()[3]) & ~0x1FFFF
    assert start + 40000 <= 2**32
    dense = (start + np.arange(40000, dtype=np.uint64)).astype(U32)
    names = [f"d{i}" for i in range(400)]
    sc.define(names, rng.permutation(dense))
    sc.call(add=names)
    pool, h = _scatter_hashes(rng, dense)
    sc.pool = np.concatenate([pool, dense[::97]])
    more = [f"w{i}" for i in range(len(h) // 100)]
    sc.define(more, h[:len(more) * 100])
    sc.call(add=more)
    return sc


def _many_names():
    """33,000 names x 2 in one call, then all but ids 32,400-32,999 removed:
    ~1,200 points whose owner ids lie on both sides of 0x8000 (k_dir_both)"""
    sc = Scenario("many_names", 2, large=True)
    rng = np.random.default_rng(106)
    names = [f"n{i}" for i in range(33000)]
    pool = sc.pool = placement_pool(5)
    h = _filler(rng, 33000 * 2, pool).reshape(33000, 2)
    ends = np.array([0, 1, M32 - 1, M32], dtype=U32)
    inner = rng.permutation(pool[~np.isin(pool, ends)])[:1196]
    h[32400:33000] = rng.permutation(np.concatenate([ends, inner])).reshape(600, 2)
    sc.define(names, h)
    sc.call(add=names, check=False)
    sc.call(rm=names[:32400])
    return sc


def _many_servers():
    """40,000 x 16: owner ids on both sides of 0x8000 through k_index_build"""
    sc = Scenario("many_servers", 16, large=True)
    rng = np.random.default_rng(107)
    names = [f"m{i}" for i in range(40000)]
    pool = sc.pool = placement_pool(6)
    sc.define(names, rng.permutation(np.concatenate([pool, _filler(rng, 40000 * 16 - len(pool), pool)])))
    sc.call(add=names)
    return sc


def _delta_edges():
    """One replica per server on placed_small's hashes: calls at the switches
    between k_ring_merge_small and k_ring_merge (767, 768, 769 delta words)
    and between incremental and bulk (8,192 and 8,193 servers), single adds
    and removes at bucket-index boundaries (the in-place bucket shift), an add
    whose hashes are all taken, and a remove that empties the ring."""
    sc = Scenario("delta_edges", 1)
    rng = np.random.default_rng(108)
    m = sc.model
    src = _placed_small()
    sc.pool = src.pool
    base_h = np.concatenate([c.add_h.reshape(-1) for c in src.calls])
    base = [f"p{i}" for i in range(len(base_h))]
    sc.define(base, base_h)
    for c in range(4):
        sc.call(add=base[512 * c:512 * c + 512])
    fresh = iter(_filler(rng, 40000, base_h).tolist())
    serial = iter(range(10**6))

    def new(hashes):
        names = [f"f{next(serial)}" for _ in hashes]
        sc.define(names, np.array(hashes, dtype=U32))
        return names

    def owners_of_distinct_points(k):
        """k present servers, each the owner of its point"""
        return [m.names[i] for i in m.own[rng.permutation(len(m.own))[:k]]]

    # 2 * 300 + ndel delta words on either side of RING_DELTA_WORDS
    for ndel in (DELTA_WORDS - 601, DELTA_WORDS - 600, DELTA_WORDS - 599):
        sc.call(add=new([next(fresh) for _ in range(300)]), rm=owners_of_distinct_points(ndel))
        assert m.delta == (300, ndel), m.delta
    # INCR_MAX and INCR_MAX + 1 servers, added and removed
    big0 = new([next(fresh) for _ in range(INCR_MAX)])
    big1 = new([next(fresh) for _ in range(INCR_MAX + 1)])
    sc.call(add=big0)
    sc.call(add=big1)
    sc.call(rm=big0[:INCR_MAX - 7] + big1[:7])
    sc.call(rm=big0[INCR_MAX - 7:] + big1[7:])
    assert m.touched == INCR_MAX + 1
    # single servers on the edges of bucket-index buckets and of the hash space
    kb = int(key_hashes()[0]) >> 16
    for x in [0, M32] + [v for b in (1, 0x8000, 0xFFFF, kb) for v in ((b << 16) - 1, b << 16)]:
        at = np.searchsorted(m.h, U32(x))
        if at < len(m.h) and m.h[at] == x:  # (a pool value: its owner leaves first)
            sc.call(rm=[m.names[m.own[at]]])
        one = new([x])
        sc.call(add=one)
        sc.call(rm=one)
        sc.call(add=one)
    # every hash taken: the server is present and owns nothing
    sc.call(add=new(m.h[[0, len(m.h) // 2, len(m.h) - 1]].tolist()))
    assert m.delta == (0, 0)
    # empty the ring, then add again
    sc.call(rm=[n for n, p in zip(m.names, m.present) if p])
    assert len(m.h) == 0 and m.count == 0
    sc.call(add=new([next(fresh) for _ in range(5)]))
    sc.call(add=base[:40], rm=base[40:50])
    return sc


SORT_RUNS = [(S, run) for S in (INCR_MAX + 1, 12289) for run in (1, 63, 65, 1025, 4097, None)]


def _sort_runs(S, run):
    """One replica per server, S servers in one bulk call, server i at hash
    (i // run) * 2654435761: runs of equal keys across the radix sort's
    64-item rows, 1,024-item wave spans and 4,096-item tiles (run None: one
    run of S), several digits in every pass; the first inserter of a hash
    survives.  Then a bulk call of new servers that all find their hash taken."""
    run = run or S
    sc = Scenario(f"sort_runs_{S}_{run}", 1, large=True)
    names = [f"r{i}" for i in range(S)]
    h = ((np.arange(S, dtype=np.uint64) // np.uint64(run)) * np.uint64(2654435761)) & np.uint64(M32)
    sc.define(names, h)
    sc.call(add=names)
    assert np.array_equal(np.sort(sc.model.own), np.arange(0, S, run))  # the lowest index of every run
    late = [f"t{i}" for i in range(S)]
    sc.define(late, h[::-1])
    sc.call(add=late)
    assert sc.model.delta == (0, 0) and sc.model.count == 2 * S
    return sc


_BUILDERS = {
    "placed_small": _placed_small, "placed_bulk": _placed_bulk, "no_extremes": _no_extremes, "scatter": _scatter,
    "dense_group": _dense_group, "many_names": _many_names, "many_servers": _many_servers,
    "delta_edges": _delta_edges,
}
SMALL = ("placed_small", "placed_bulk", "no_extremes", "delta_edges")  # checked after every call, and by the oracle
LARGE = ("scatter", "dense_group", "many_names", "many_servers")
PLACED = ("placed_small", "placed_bulk", "no_extremes", "scatter", "many_names", "many_servers")


@functools.lru_cache(None)
def scenario(name, *args):
    return _sort_runs(*args) if name == "sort_runs" else _BUILDERS[name]()


def probes(sc):
    """the hashes of every lookup-by-hash check: the scenario's placed values,
    K's hashes, both ends of the hash space and 200 random u32"""
    rng = np.random.default_rng(9)
    return np.concatenate([sc.pool, key_hashes(), np.array([0, 1, M32 - 1, M32], dtype=U32),
                           rng.integers(0, 2**32, size=200, dtype=np.uint64).astype(U32)])


# cover() of every scenario's final ring, in the order of its keys (delta_edges
# ends on a 45-point ring after it emptied itself; its edges are its calls):
#   scenario      points exact above below wraps <=min first11 last11 first16 last16 max_group own<0x8000 own>=0x8000 idle
#   placed_small    1861   252   271   257     0     0     528    551     261    290         7       1861           0    5
#   placed_bulk     2406   117   106   105     0     0     206    227     101    120         5       2406           0    0
#   no_extremes     1838   256   272   286     8     8     501    523     258    267         8       1838           0    6
#   delta_edges       45     2     4     8     0     6      11     14       4     10         2         45           0    0
#   scatter       655360   260   248   266     0     0     855    845     301    277        42     655360           0    0
#   dense_group   695300   261   248   267     0     0     880    826     298    278     40011     695300           0    0
#   many_names      1200   168   177   153     0     0     326    374     155    187         7        736         464    0
#   many_servers  640000   280   249   272     0     0     824    833     271    277        42     524288      115712    0
# (wraps are 0 wherever 0xFFFFFFFF is a point; no_extremes is the scenario without it)
def cover(model):
    """where the final ring's points lie relative to K and the directories"""
    h = model.h.astype(np.int64)
    kh = key_hashes().astype(np.int64)
    out = {
        "points": int(len(h)),
        "exact": int(np.isin(kh, h).sum()),
        "one_above": int(np.isin(kh - 1, h).sum()),   # keys one above a point
        "one_below": int(np.isin(kh + 1, h).sum()),   # keys one below a point
        "wraps": int((kh > h.max()).sum()) if len(h) else 0,
        "at_or_below_min": int((kh <= h.min()).sum()) if len(h) else 0,
    }
    for s in (S_DIR, 16):
        mask = (1 << s) - 1
        out[f"first_key_{s}"] = int(((h & mask) == 0).sum())
        out[f"last_key_{s}"] = int(((h & mask) == mask).sum())
    out["max_group"] = int(np.bincount(h >> S_GROUP).max()) if len(h) else 0
    out["own_lt_0x8000"] = int((model.own < 0x8000).sum())
    out["own_ge_0x8000"] = int((model.own >= 0x8000).sum())
    present = np.flatnonzero(np.array(model.present, dtype=bool))
    out["present_owning_nothing"] = int((~np.isin(present, model.own)).sum())
    return out
