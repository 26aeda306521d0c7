"""The drop-in ring (rp_ring.hip, rp_sort.h, rp_capi.hip rp_ring) against
tests/ring_cases.py: scenarios whose points are placed on the keys' hashes,
one above and one below them, on the first and last key of the directory and
bucket-index buckets, at 0 and 0xFFFFFFFF, 40,000 deep in one coarse group of
the 16-bit directory and under owner ids on both sides of 0x8000; driven
through rp_ring_add_remove with explicit replica hashes and compared, all
exact, with RingModel (itself checked against the C oracle and the reference
fixtures by test_ring_edges_cpu.py).  After a call: the points with their
owners' names and the server count; lookups by hash; k_lookup_keys on the
whole key set, in slices of 255 / 256 / 257 keys from an odd byte offset and
with a block of 3,000-byte keys (the unstaged branch); scalar lookups
(k_lookup_small); both groupings; lookupN for every probe in one call; and on
the default library which of the incremental and bulk paths the call took.

Tests named *_large build rings of more than 100,000 points (the child run of
test_gpu_alt_build.py may deselect them by name)."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import ring_cases as rc

pytestmark = pytest.mark.gpu

RP_RING_PROF_MERGE = 2  # include/ringpop_hip.h
DEFAULT_LIB = not os.environ.get("RINGPOP_HIP_LIB")  # (another build may put every call on the bulk path)


@pytest.fixture(scope="module")
def rp(gpu_lib):
    import ringpop_amd
    return ringpop_amd


def _encode(strings):
    from ringpop_amd.farmhash import _encode as enc
    return enc(strings)


@pytest.fixture(scope="module")
def keyset():
    """K and K with three 3,000-byte keys after it, encoded once"""
    K = list(rc.keys())
    rng = np.random.default_rng(77)
    longk = [rng.integers(0, 256, size=3000, dtype=np.uint8).tobytes() for _ in range(3)]
    return {"K": _encode(K), "n": len(K), "long": _encode(K + longk), "long_h": oracle.farmhash32_batch(longk),
            "bytes": K}


class Dev:
    """one device ring, driven through the C ABI"""

    def __init__(self, rp, replicas):
        from ringpop_amd._lib import check, lib, ptr
        self.check, self.L, self.ptr = check, lib(), ptr
        self.ring = rp.HashRing(replica_points=replicas)
        self.h = self.ring._h
        self._names = []

    def close(self):
        self.ring.close()

    def add_remove(self, c):
        ab, ao = _encode(c.add)
        rb, ro = _encode(c.rm)
        ah = np.ascontiguousarray(c.add_h, dtype=np.uint32).reshape(-1)
        rh = np.ascontiguousarray(c.rm_h, dtype=np.uint32).reshape(-1)
        changed = ctypes.c_int(-1)
        self.check(self.L.rp_ring_add_remove(self.h, self.ptr(ab), self.ptr(ao), len(c.add),
                                             self.ptr(ah) if len(c.add) else None, self.ptr(rb), self.ptr(ro),
                                             len(c.rm), self.ptr(rh) if len(c.rm) else None, ctypes.byref(changed)))
        return bool(changed.value)

    def merge_us(self):
        us = (ctypes.c_double * 7)()
        self.check(self.L.rp_ring_profile(self.h, us, 7))
        return us[RP_RING_PROF_MERGE]

    def names(self, ids):
        """owner ids -> server names (None for -1)"""
        ids = np.asarray(ids, dtype=np.int64)
        top = int(ids.max()) if ids.size else -1
        while len(self._names) <= top:
            self._names.append(self.ring.server_name(len(self._names)))
        return np.array(self._names + [None], dtype=object)[ids]

    def lookup_keys(self, blob, off, n):
        out = np.full(n, -7, dtype=np.int32)
        self.check(self.L.rp_ring_lookup_batch(self.h, self.ptr(blob), self.ptr(off), n, self.ptr(out)))
        return out

    def lookup_n(self, hashes, n):
        hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
        out = np.full((len(hashes), max(n, 1)), -7, dtype=np.int32)
        cnt = np.full(len(hashes), -7, dtype=np.int32)
        self.check(self.L.rp_ring_lookup_n_hashes(self.h, self.ptr(hashes), len(hashes), int(n), self.ptr(out),
                                                  self.ptr(cnt)))
        return out[:, :n] if n else out[:, :0], cnt

    def group(self, keys=None, hashes=None):
        n = len(hashes) if hashes is not None else keys[2]
        dests = np.zeros(max(n, 1), dtype=np.int32)
        goff = np.zeros(n + 1, dtype=np.uint32)
        kidx = np.zeros(max(n, 1), dtype=np.uint32)
        ng = ctypes.c_size_t(0)
        if hashes is not None:
            hashes = np.ascontiguousarray(hashes, dtype=np.uint32)
            self.check(self.L.rp_ring_group_hashes(self.h, self.ptr(hashes), n, self.ptr(dests), self.ptr(goff),
                                                   self.ptr(kidx), ctypes.byref(ng)))
        else:
            self.check(self.L.rp_ring_group_keys(self.h, self.ptr(keys[0]), self.ptr(keys[1]), n, self.ptr(dests),
                                                 self.ptr(goff), self.ptr(kidx), ctypes.byref(ng)))
        g = ng.value
        return dests[:g], goff[:g + 1], kidx[:n]


def _same_names(dev, got_ids, m, want_ids, what):
    got, want = dev.names(got_ids), m.owner_names(want_ids)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad.size), [(int(i), got[i], want[i]) for i in bad[:5]])


def _scalar_picks(m, kh):
    """40 keys: exact hits, keys past the largest point (the wrap), keys at or
    below the smallest, and an even spread of the rest"""
    if len(m.h) == 0:
        return list(range(0, len(kh), 15))[:40]
    pick = list(np.flatnonzero(np.isin(kh, m.h))[:10]) + list(np.flatnonzero(kh > m.h.max())[:4]) + \
        list(np.flatnonzero(kh <= m.h.min())[:4])
    pick += [i for i in range(0, len(kh), 13) if i not in pick]
    return [int(i) for i in pick[:40]]


def _check(dev, m, sc, keyset, probes, nprobes, ns):
    kh = rc.key_hashes()
    # the points and the server count
    h, o = dev.ring.points()
    assert np.array_equal(h, m.h), ("points", len(h), len(m.h))
    _same_names(dev, o, m, m.own, "point owners")
    assert dev.ring.getServerCount() == m.count
    # lookups by hash (k_lookup_hashes, the 32-bit directory)
    _same_names(dev, dev.ring.lookup_hashes(probes), m, m.lookup(probes), "lookup_hashes")
    # k_lookup_keys: all of K in one call (the 16-bit directory, or the 32-bit one where that cannot hold the ring)
    blob, off = keyset["K"]
    nK = keyset["n"]
    want = m.lookup(kh)
    _same_names(dev, dev.lookup_keys(blob, off, nK), m, want, "lookup_batch K")
    # ... slices from an odd byte offset: one key short of a block, one block, one key more
    s = next(i for i in range(1, nK) if int(off[i]) & 1)
    for n in (255, 256, 257):
        assert s + n <= nK
        got = dev.lookup_keys(blob, np.ascontiguousarray(off[s:s + n + 1]), n)
        _same_names(dev, got, m, want[s:s + n], f"lookup_batch K[{s}:{s}+{n}]")
    # ... and with three 3,000-byte keys in the last block: more bytes than its stage holds
    lblob, loff = keyset["long"]
    lwant = np.concatenate([want, m.lookup(keyset["long_h"])])
    _same_names(dev, dev.lookup_keys(lblob, loff, nK + 3), m, lwant, "lookup_batch K + long keys")
    # scalar lookups: ring.lookup(key) is rp_ring_lookup_batch with one key, which takes k_lookup_small when the
    # ring has points and the key fits the kernel arguments (3,072 bytes: every key of K; an empty ring answers
    # through k_lookup_keys)
    assert max(len(k) for k in keyset["bytes"]) <= 3072
    for i in _scalar_picks(m, kh):
        got = dev.lookup_keys(blob, np.ascontiguousarray(off[i:i + 2]), 1)
        _same_names(dev, got, m, want[i:i + 1], f"scalar lookup of key {i}")
    # handleOrProxyAll's grouping, by key and by hash
    wd, wg, wk = oracle.group_by_owner_np(want)
    for what, (d, g, k) in (("group_keys", dev.group(keys=(blob, off, nK))), ("group_hashes", dev.group(hashes=kh))):
        _same_names(dev, d, m, wd, what)
        assert np.array_equal(g, wg) and np.array_equal(k, wk), what
    # lookupN, every probe in one call (k_lookup_n, the only reader of the bucket index)
    full, fcnt = m.lookup_n_padded(nprobes, max(ns))
    for n in ns:
        nn = min(n, m.count)
        wantn = np.full((len(nprobes), n), -1, dtype=np.int32)
        wantn[:, :nn] = full[:, :nn]
        got, cnt = dev.lookup_n(nprobes, n)
        assert np.array_equal(cnt, np.minimum(fcnt, nn)), ("lookupN counts", n)
        assert np.array_equal(got < 0, wantn < 0), ("lookupN padding", n)
        _same_names(dev, got.reshape(-1), m, wantn.reshape(-1), f"lookupN n={n}")


def _ns(m, large):
    return list(rc.LOOKUP_N) + ([m.count, m.count + 3] if m.count <= rc.N_ALL_MAX and not large else [])


def _run(rp, sc, keyset, first=0, last=None):
    """every call of the scenario in order; calls first..last-1 are checked
    (those the scenario marks), earlier ones only applied"""
    probes = rc.probes(sc)
    nprobes = probes[:: max(1, len(probes) // 200)] if sc.large else probes
    dev = Dev(rp, sc.R)
    try:
        for step, (c, m, changed) in enumerate(sc.replay()):
            if last is not None and step >= last:
                break
            assert dev.add_remove(c) == changed, step
            if step < first:
                continue
            if DEFAULT_LIB:
                incremental = 0 < m.touched <= rc.INCR_MAX
                assert (dev.merge_us() > 0) == incremental, (step, m.touched, dev.merge_us())
            if c.check:
                try:
                    _check(dev, m, sc, keyset, probes, nprobes, _ns(m, sc.large))
                except AssertionError as e:
                    raise AssertionError(f"{sc.name} after call {step}: {e}") from e
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["placed_small", "placed_bulk", "no_extremes"])
def test_placed(rp, keyset, name):
    _run(rp, rc.scenario(name), keyset)


# delta_edges in three stretches of its 47 calls (each applies the calls before it unchecked)
@pytest.mark.parametrize("first,last", [(0, 11), (11, 29), (29, None)])
def test_delta_edges(rp, keyset, first, last):
    _run(rp, rc.scenario("delta_edges"), keyset, first, last)


def test_many_names(rp, keyset):
    """owner ids on both sides of 0x8000 on a ~1,200-point ring: k_dir_both
    must flag the 16-bit directory as unable to hold them"""
    _run(rp, rc.scenario("many_names"), keyset)


@pytest.mark.parametrize("S,run", rc.SORT_RUNS)
def test_sort_runs(rp, keyset, S, run):
    _run(rp, rc.scenario("sort_runs", S, run), keyset)


@pytest.mark.parametrize("name", ["scatter", "dense_group", "many_servers"])
def test_index_build_large(rp, keyset, name):
    _run(rp, rc.scenario(name), keyset)


def test_reference_fixture(rp, golden):
    """tests/golden/ring_edges.json, the reference's own HashRing: points at 0
    and 4294967295, shared hashes, a present server that owns nothing, an
    emptied ring.  lookupN for n >= 1 (n = 0: INTEGRATION.md section 1)."""
    g = golden("ring_edges.json")
    R = g["replica_points"]
    probes = np.array(g["probes"], dtype=np.uint32)
    Call = rc.Call
    dev = Dev(rp, R)
    try:
        for step in g["steps"]:
            add, rm = step["add"], step["remove"]
            ah = np.array([g["table"][s] for s in add], dtype=np.uint32).reshape(len(add), R)
            rh = np.array([g["table"][s] for s in rm], dtype=np.uint32).reshape(len(rm), R)
            assert dev.add_remove(Call(add, ah, rm, rh, True)) == step["changed"]
            h, o = dev.ring.points()
            assert [[int(a), b] for a, b in zip(h, dev.names(o))] == step["points"]
            assert dev.ring.getServerCount() == step["server_count"]
            assert dev.names(dev.ring.lookup_hashes(probes)).tolist() == step["lookups"]
            for n in g["ns"]:
                if n == 0:
                    continue
                got, cnt = dev.lookup_n(probes, n)
                rows = [dev.names(got[k, :cnt[k]]).tolist() for k in range(len(probes))]
                assert rows == step["lookupN"][str(n)], n
                assert all((got[k, cnt[k]:] == -1).all() for k in range(len(probes))), n
    finally:
        dev.close()
