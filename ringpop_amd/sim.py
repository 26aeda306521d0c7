"""Device-resident simulation of N ringpop instances (rp_sim_* C ABI)."""
import ctypes

import numpy as np

from ._lib import (MovementStats, OwnershipStats, RequestPending, RequestResult, RoundStats, RouteStats, SimConfig, TrafficConfig, TrafficStats, check,
                   lib, ptr)

KERNEL_CATEGORIES = ("churn", "issue", "merge_ping", "merge_resp", "checksum", "other")
STATUS_NAMES = {0: None, 1: "alive", 2: "suspect", 3: "faulty", 4: "leave"}


class Loop:
    """rp_loop: the ranks of a `nranks`-rank cluster as threads of this process
    on one GPU (rp_sim_create_rank_loop; the rank code of an RCCL cluster with
    device-copy collectives).  Each rank's Sim is driven from its own thread."""

    def __init__(self, nranks):
        self._h = ctypes.c_void_p()
        self.nranks = nranks
        check(lib().rp_loop_create(nranks, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().rp_loop_destroy(self._h)
            self._h = ctypes.c_void_p()


class Traffic:
    """rp_traffic: requests with the request proxy's retries across rounds
    (Sim.traffic).  The tracker's clock is its Sim's round
    count; close it before the Sim (Sim.close does)."""

    OUTCOMES = ("local", "delivered", "rerouted_local", "failed", "entry_dead")
    PENDING = 255
    RESULT_DTYPE = np.dtype([("dest", "<i4"), ("outcome", "u1"), ("retries", "u1"), ("reserved", "<u2"),
                             ("submit_clock", "<u4"), ("done_clock", "<u4")])
    PENDING_DTYPE = np.dtype([("id", "<u8"), ("entry", "<u4"), ("key_hash", "<u4"), ("first_dest", "<i4"),
                              ("due", "<u4"), ("submit_clock", "<u4"), ("retries", "<u4")])

    def __init__(self, sim, max_retries=3, schedule=(0, 5, 18), enforce_consistency=True, track=False,
                 capacity=1 << 20, timing=False):
        schedule = [int(x) for x in schedule]
        if not 1 <= len(schedule) <= 8:
            raise ValueError("traffic: a schedule of 1 to 8 delays")
        if max_retries < 0:
            raise ValueError("traffic: max_retries >= 0")
        cfg = TrafficConfig(max_retries=int(max_retries), nschedule=len(schedule),
                            enforce_consistency=1 if enforce_consistency else 0, track=1 if track else 0,
                            timing=1 if timing else 0, capacity=int(capacity))
        for i, x in enumerate(schedule):
            cfg.schedule[i] = x
        self._sim = sim
        self._h = ctypes.c_void_p()
        check(lib().rp_traffic_create(sim._h, ctypes.byref(cfg), ctypes.byref(self._h)))
        sim._traffic.append(self)

    def close(self):
        if self._h:
            lib().rp_traffic_destroy(self._h)
            self._h = ctypes.c_void_p()
            if self in self._sim._traffic:
                self._sim._traffic.remove(self)

    def submit(self, entries, key_hashes):
        """First attempts of request i = (entries[i], key_hashes[i]) now; the id of request 0."""
        e = np.ascontiguousarray(entries, dtype=np.uint32)
        h = np.ascontiguousarray(key_hashes, dtype=np.uint32)
        if e.ndim != 1 or e.shape != h.shape:
            raise ValueError("submit: two arrays of one length")
        first = ctypes.c_uint64(0)
        check(lib().rp_traffic_submit(self._h, ptr(e), ptr(h), len(e), ctypes.byref(first)))
        return int(first.value)

    def submit_uniform(self, seed, first, count):
        """Requests first .. first + count - 1 of route_uniform's generator, drawn on the device."""
        check(lib().rp_traffic_submit_uniform(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(count)))

    def poll(self):
        """Every pending request that is due retries."""
        check(lib().rp_traffic_poll(self._h))

    def run(self, k, per_round, seed, churn=True):
        """k times: a round, a poll, a submit_uniform of per_round requests (rp_traffic_run)."""
        check(lib().rp_traffic_run(self._h, int(k), 1 if churn else 0, int(per_round), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def stats(self):
        """(cumulative statistics, by_retries: {outcome: [finals with 0..8 retries]})."""
        st = TrafficStats()
        by = np.zeros(45, dtype=np.uint64)
        check(lib().rp_traffic_read_stats(self._h, ctypes.byref(st), ptr(by)))
        return st.as_dict(), {k: by[9 * i:9 * i + 9].astype(np.int64).tolist() for i, k in enumerate(self.OUTCOMES)}

    def history(self, first_clock, count):
        """One statistics dict per clock first_clock .. first_clock + count - 1."""
        rows = (TrafficStats * max(int(count), 1))()
        check(lib().rp_traffic_history(self._h, int(first_clock), int(count), rows))
        return [rows[i].as_dict() for i in range(int(count))]

    def pending_count(self):
        cnt = ctypes.c_uint64(0)
        check(lib().rp_traffic_pending(self._h, None, 0, ctypes.byref(cnt)))
        return int(cnt.value)

    def pending(self):
        """The pending table in submission order (a PENDING_DTYPE array)."""
        assert self.PENDING_DTYPE.itemsize == ctypes.sizeof(RequestPending)
        out = np.zeros(self.pending_count(), dtype=self.PENDING_DTYPE)
        cnt = ctypes.c_uint64(0)
        check(lib().rp_traffic_pending(self._h, ptr(out), len(out), ctypes.byref(cnt)))
        return out[:int(cnt.value)]

    def results(self, first_id, n):
        """The records of requests first_id .. first_id + n - 1 (track=True; a RESULT_DTYPE array)."""
        assert self.RESULT_DTYPE.itemsize == ctypes.sizeof(RequestResult)
        out = np.zeros(int(n), dtype=self.RESULT_DTYPE)
        check(lib().rp_traffic_results(self._h, int(first_id), len(out), ptr(out)))
        return out

    def times(self):
        """timing=True: device ms and calls of the polls and submits, and the peak pending count."""
        ms = (ctypes.c_double * 2)()
        calls = (ctypes.c_uint64 * 2)()
        peak = ctypes.c_uint64(0)
        check(lib().rp_traffic_times(self._h, ms, calls, ctypes.byref(peak)))
        return {"poll_ms": ms[0], "polls": int(calls[0]), "submit_ms": ms[1], "submits": int(calls[1]),
                "peak_pending": int(peak.value)}


class OwnershipSnapshot:
    """rp_ownership_snapshot: every node's claim set at one clock
    (Sim.ownership_snapshot).  `clock` is the round count it
    was taken at, `stats` the census' stats dict then.  It owns its device
    buffers: close it (or use it as a context manager) when done; it may
    outlive its Sim."""

    def __init__(self, sim):
        self._h = ctypes.c_void_p()
        check(lib().rp_ownership_snapshot_create(sim._h, ctypes.byref(self._h)))
        st, clock = OwnershipStats(), ctypes.c_uint64(0)
        check(lib().rp_ownership_snapshot_info(self._h, ctypes.byref(st), ctypes.byref(clock)))
        self.stats = st.as_dict()
        self.clock = int(clock.value)

    def close(self):
        if self._h:
            lib().rp_ownership_snapshot_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sim:
    def __init__(self, n, seed, churn_k=None, arena_entries=0, snapshot_slots=0, origin_slots=0, failures=None,
                 partition=None, seen_window=0, replica_hash_shift=0, shards=1, rank=None, unique_id=None,
                 storm=None, addresses=None, views=None, joins=None, compact=None, loop=None, prefix_min=0, ck_lane_min=0,
                 issue_wave=0, leaves=None, rejoins=None):
        """shards > 1: the nodes are split into `shards` shards.  With rank=None
        all shards run in this process (rp_sim_create_shards); with a rank, this
        process holds that shard of a one-process-per-GPU cluster whose RCCL
        communicator is named by `unique_id` (rp_sim_create_rank), or -- with
        loop=Loop(shards) -- that rank of a cluster of threads of this process
        (rp_sim_create_rank_loop).
        addresses: the cluster's n address strings in sort order
        (rp_sim_load_addresses); views: (status, incarnation) arrays of shape
        (n, n) for the bootstrap (rp_sim_set_views; status 0 = absent);
        joins: [(round, joiner, [seeds...]), ...] (rp_sim_join);
        leaves, rejoins: {round: [ids]} graceful leaves and rejoins (rp_sim_leave,
        rp_sim_rejoin; per node they alternate, starting with a leave);
        compact: (mul, add) log-compaction thresholds (testing; None = auto);
        prefix_min: the window shrink that triggers the issue's head packing
        beyond the entries it moves (testing; 0 = auto, 512);
        ck_lane_min: checksum lists this long are hashed one view per lane
        (0 = auto; 1 = always, 0xFFFFFFFF = never);
        issue_wave: the issue kernels of runs without faults on n % 64 == 0
        nodes (0 = the build's default; 1 = one block per node; 2 = one wave
        per node); counters()["wave_issues"] counts the latter's issues."""
        self.n = n
        self.churn_k = -(-n // 100) if churn_k is None else churn_k
        cfg = SimConfig(n=n, churn_k=self.churn_k, seed=seed, arena_entries=arena_entries,
                        snapshot_slots=snapshot_slots, origin_slots=origin_slots,
                        seen_window=seen_window, replica_hash_shift=replica_hash_shift,
                        compact_mul=compact[0] if compact else 0, compact_add=compact[1] if compact else 0,
                        prefix_min=prefix_min, ck_lane_min=ck_lane_min, issue_wave=issue_wave)
        self._h = ctypes.c_void_p()
        self._traffic = []  # open trackers: closed before the simulation
        self.shards = shards
        if rank is not None and loop is not None:
            check(lib().rp_sim_create_rank_loop(ctypes.byref(cfg), loop._h, rank, ctypes.byref(self._h)))
        elif rank is not None:
            uid = ctypes.create_string_buffer(bytes(unique_id), 128)
            check(lib().rp_sim_create_rank(ctypes.byref(cfg), shards, rank, uid, ctypes.byref(self._h)))
        elif shards > 1:
            check(lib().rp_sim_create_shards(ctypes.byref(cfg), shards, ctypes.byref(self._h)))
        else:
            check(lib().rp_sim_create(ctypes.byref(cfg), ctypes.byref(self._h)))
        for rnd, ids in (failures or {}).items():
            for v in ids:
                check(lib().rp_sim_fail(self._h, int(v), int(rnd)))
        if partition:
            check(lib().rp_sim_partition(self._h, partition["start"], partition["end"], partition["split"]))
        if storm:  # {"start", "end", "ppm"}: false suspicions (rp_sim_storm)
            check(lib().rp_sim_storm(self._h, storm["start"], storm["end"], storm["ppm"]))
        if addresses is not None:
            self.load_addresses(addresses)
        if joins:
            self.join(joins)
        if views is not None:
            self.set_views(views[0], views[1])
        # (per node in round order, as the schedule's rules ask; a round's leaves first)
        events = [(int(r), 0, int(v)) for r, ids in (leaves or {}).items() for v in ids]
        events += [(int(r), 1, int(v)) for r, ids in (rejoins or {}).items() for v in ids]
        for rnd, kind, v in sorted(events):
            (self.rejoin if kind else self.leave)(v, rnd)

    def leave(self, node, round):
        """rp_sim_leave: `node` leaves gracefully at the start of `round` (>= the
        current one): makeLeave(self), gossip.stop(), suspicion.stopAll()."""
        check(lib().rp_sim_leave(self._h, int(node), int(round)))

    def rejoin(self, node, round):
        """rp_sim_rejoin: a node that left rejoins at the start of `round`:
        makeAlive(self, now), gossip.start(), suspicion.reenable()."""
        check(lib().rp_sim_rejoin(self._h, int(node), int(round)))

    def flags(self, v):
        """rp_sim_node_flags: {"gossip_stopped", "suspicion_stopped"} of node v."""
        f = ctypes.c_uint32(0)
        check(lib().rp_sim_node_flags(self._h, int(v), ctypes.byref(f)))
        return {"gossip_stopped": bool(f.value & 1), "suspicion_stopped": bool(f.value & 2)}

    def join(self, joins):
        """rp_sim_join: [(round, joiner, [seed, ...]), ...] in processing order."""
        k = len(joins)
        sp = max([len(j[2]) for j in joins] + [1])
        ids = np.array([j[1] for j in joins], dtype=np.uint32)
        rounds = np.array([j[0] for j in joins], dtype=np.uint32)
        seeds = np.full((k, sp), -1, dtype=np.int32)
        for i, j in enumerate(joins):
            seeds[i, :len(j[2])] = j[2]
        check(lib().rp_sim_join(self._h, ptr(ids), ptr(rounds), ptr(seeds), k, sp))

    def load_addresses(self, addresses):
        """rp_sim_load_addresses: node i is addresses[i] (sorted, distinct)."""
        bs = [a.encode() if isinstance(a, str) else bytes(a) for a in addresses]
        off = np.zeros(len(bs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b) for b in bs])
        blob = np.frombuffer(b"".join(bs) or b"\0", dtype=np.uint8)
        check(lib().rp_sim_load_addresses(self._h, ptr(blob), ptr(off), len(bs)))

    def set_views(self, status, incarnation, node_lo=0):
        """rp_sim_set_views for nodes node_lo .. node_lo + len(status): rows of
        member statuses (1..4) and incarnations, shape (count, n)."""
        st = np.ascontiguousarray(status, dtype=np.int32)
        inc = np.ascontiguousarray(incarnation, dtype=np.int64)
        if st.ndim != 2 or st.shape != inc.shape or st.shape[1] != self.n:
            raise ValueError("views: two (count, n) arrays")
        check(lib().rp_sim_set_views(self._h, int(node_lo), st.shape[0], ptr(st), ptr(inc)))

    @staticmethod
    def unique_id():
        """A fresh RCCL communicator id (128 bytes) for rp_sim_create_rank."""
        buf = ctypes.create_string_buffer(128)
        check(lib().rp_comm_unique_id(buf, 128))
        return buf.raw

    def shard_range(self):
        lo, hi = ctypes.c_uint32(0), ctypes.c_uint32(0)
        check(lib().rp_sim_shard_range(self._h, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def exchange_stats(self):
        ms, b, r = ctypes.c_double(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(lib().rp_sim_exchange_stats(self._h, ctypes.byref(ms), ctypes.byref(b), ctypes.byref(r)))
        out = {"ms": ms.value, "bytes_sent": b.value, "rounds": r.value}
        if hasattr(lib(), "rp_sim_exchange_shard_bytes"):  # (an older A/B variant may lack it)
            arr, cnt = (ctypes.c_uint64 * 64)(), ctypes.c_int(0)
            check(lib().rp_sim_exchange_shard_bytes(self._h, arr, 64, ctypes.byref(cnt)))
            out["shard_bytes"] = [int(arr[i]) for i in range(min(cnt.value, 64))]
        return out

    def close(self):
        if self._h:
            for t in list(self._traffic):
                t.close()
            lib().rp_sim_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def round(self, churn=True):
        st = RoundStats()
        check(lib().rp_sim_round(self._h, 1 if churn else 0, ctypes.byref(st)))
        return st.as_dict()

    def run(self, k, churn=True):
        check(lib().rp_sim_run(self._h, int(k), 1 if churn else 0))

    def sync(self):
        check(lib().rp_sim_sync(self._h))

    def totals(self):
        st = RoundStats()
        check(lib().rp_sim_totals(self._h, ctypes.byref(st)))
        d = st.as_dict()
        d["converged_rounds"] = d.pop("converged")
        return d

    COUNTERS = ("evaluated", "applied", "full_syncs", "messages", "waves", "pings", "eval_ping_merge",
                "applied_ping_merge", "eval_resp_merge", "applied_resp_merge", "scanned_send_issue",
                "emitted_send_issue", "scanned_recv_issue", "emitted_recv_issue", "written_send_issue",
                "written_recv_issue", "touched", "touched_ping_merge", "checksum_views", "compactions_issue",
                "compactions_apply", "prefix_packs", "same_view_issues", "diag0", "diag1", "diag2", "diag3", "diag4", "diag5",
                "wave_issues")

    def counters(self):
        """Cumulative counters: the round statistics, per-kernel unit counts and
        diagnostics (rp_sim_counters); the last entry is converged_rounds."""
        out = np.zeros(64, dtype=np.uint64)
        n = ctypes.c_int(0)
        check(lib().rp_sim_counters(self._h, ptr(out), 64, ctypes.byref(n)))
        d = {k: int(out[i]) for i, k in enumerate(self.COUNTERS[: n.value - 1])}
        d["converged_rounds"] = int(out[n.value - 1])
        return d

    def local_counters(self):
        """counters() of this process's shards only (equal to counters() for one
        shard or all shards in process)."""
        out = np.zeros(64, dtype=np.uint64)
        n = ctypes.c_int(0)
        check(lib().rp_sim_local_counters(self._h, ptr(out), 64, ctypes.byref(n)))
        return {k: int(out[i]) for i, k in enumerate(self.COUNTERS[: n.value - 1])}

    def rounds(self):
        r = ctypes.c_uint32(0)
        check(lib().rp_sim_rounds(self._h, ctypes.byref(r)))
        return r.value

    def checksums(self):
        out = np.zeros(self.n, dtype=np.uint32)
        check(lib().rp_sim_read_checksums(self._h, ptr(out), len(out)))
        return out

    def view_counts(self):
        """Per node: members absent / alive / suspect / faulty / leave and its
        ring server count ([n, 6]; nodes held by other processes are 0)."""
        out = np.zeros((self.n, 6), dtype=np.uint32)
        check(lib().rp_sim_view_counts(self._h, ptr(out), out.size))
        return out

    def view(self, v):
        st = np.zeros(self.n, dtype=np.uint8)
        inc = np.zeros(self.n, dtype=np.uint64)
        check(lib().rp_sim_read_view(self._h, v, ptr(st), ptr(inc), self.n))
        return st, inc

    def members(self, v):
        out = np.zeros(self.n, dtype=np.uint32)
        cnt = ctypes.c_uint32(0)
        check(lib().rp_sim_read_members(self._h, v, ptr(out), len(out), ctypes.byref(cnt)))
        return out[: cnt.value].astype(np.int32)

    def changes(self, v):
        cnt = ctypes.c_uint32(0)
        check(lib().rp_sim_read_changes(self._h, v, None, 0, ctypes.byref(cnt)))
        rows = np.zeros((max(cnt.value, 1), 6), dtype=np.int64)
        check(lib().rp_sim_read_changes(self._h, v, ptr(rows), rows.shape[0], ctypes.byref(cnt)))
        return rows[: cnt.value]

    def info(self, v):
        out = np.zeros(8, dtype=np.int64)
        check(lib().rp_sim_node_info(self._h, v, ptr(out)))
        keys = ("max_pb", "ring_servers", "ring_checksum", "iter_index", "iter_round", "dead", "rng", "timers")
        return dict(zip(keys, out.tolist()))

    def ring_lookup(self, v, hashes):
        h = np.ascontiguousarray(hashes, dtype=np.uint32)
        out = np.zeros(len(h), dtype=np.int32)
        check(lib().rp_sim_ring_lookup(self._h, v, ptr(h), len(h), ptr(out)))
        return out

    # ---- request routing between rounds (rp_sim_ring_checksums / rp_sim_route)
    ROUTE_OUTCOMES = ("local", "delivered", "checksums_differ", "unreachable", "entry_dead")

    def ring_checksums(self):
        """HashRing.checksum of every node's ring (lib/ring.js:96-105); nodes
        held by other processes are 0."""
        out = np.zeros(self.n, dtype=np.uint32)
        check(lib().rp_sim_ring_checksums(self._h, ptr(out), len(out)))
        return out

    def route(self, entries, key_hashes):
        """handleOrProxy for request i entering at node entries[i] with key hash
        key_hashes[i], with the next round's clock: (dests, outcomes (indices
        into ROUTE_OUTCOMES), owner_agrees, stats dict)."""
        e = np.ascontiguousarray(entries, dtype=np.uint32)
        h = np.ascontiguousarray(key_hashes, dtype=np.uint32)
        if e.ndim != 1 or e.shape != h.shape:
            raise ValueError("route: two arrays of one length")
        dests = np.zeros(len(e), dtype=np.int32)
        outcomes = np.zeros(len(e), dtype=np.uint8)
        agrees = np.zeros(len(e), dtype=np.uint8)
        st = RouteStats()
        check(lib().rp_sim_route(self._h, ptr(e), ptr(h), len(e), ptr(dests), ptr(outcomes), ptr(agrees),
                                 ctypes.byref(st)))
        return dests, outcomes, agrees, st.as_dict()

    def route_uniform(self, seed, count):
        """The stats of route() for `count` requests drawn on the device from
        splitmix64(seed) (rp_sim_route_uniform)."""
        st = RouteStats()
        check(lib().rp_sim_route_uniform(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(count), ctypes.byref(st)))
        return st.as_dict()

    # ---- ownership census between rounds (rp_sim_ownership)
    def ownership(self):
        """How many live nodes claim each key, over the whole 2^32 hash space:
        a dict of `measure` (hashes with exactly 0..6 claimants, [7]: 7 or
        more), `claimants`, `intervals`, `max_claims`, `max_claims_hash` and
        `claimed` (per node the hashes it claims, uint64)."""
        st = OwnershipStats()
        claimed = np.zeros(self.n, dtype=np.uint64)
        check(lib().rp_sim_ownership(self._h, ctypes.byref(st), ptr(claimed), len(claimed)))
        d = st.as_dict()
        d["claimed"] = claimed
        return d

    def ownership_at(self, hashes):
        """The number of live nodes that claim each key hash (rp_sim_ownership_at)."""
        h = np.ascontiguousarray(hashes, dtype=np.uint32)
        if h.ndim != 1:
            raise ValueError("ownership_at: one array of key hashes")
        out = np.zeros(len(h), dtype=np.uint32)
        check(lib().rp_sim_ownership_at(self._h, ptr(h), len(h), ptr(out)))
        return out

    # ---- ownership movement between two instants (rp_sim_ownership_moved)
    def ownership_snapshot(self):
        """Every node's claim set now, to compare later (an OwnershipSnapshot)."""
        return OwnershipSnapshot(self)

    def ownership_moved(self, frm, to=None):
        """Which keys changed hands between snapshot `frm` and snapshot `to`
        (None: the simulation as it is now): a dict of rp_movement_stats'
        fields (`transition` as 3 x 3 lists) plus `gained_by` and `lost_by`
        (the JS host's gainedBy / lostBy): per node the hashes it claims at
        `to` and not at `frm`, and the reverse, as uint64 arrays whose sums
        are the stats' `gained` and `lost`."""
        st = MovementStats()
        gained = np.zeros(self.n, dtype=np.uint64)
        lost = np.zeros(self.n, dtype=np.uint64)
        check(lib().rp_sim_ownership_moved(self._h, frm._h, to._h if to is not None else None, ctypes.byref(st),
                                           ptr(gained), ptr(lost), self.n))
        d = st.as_dict()
        d["gained_by"] = gained
        d["lost_by"] = lost
        return d

    def traffic(self, **cfg):
        """A request tracker on this simulation (rp_traffic_create): max_retries=3,
        schedule=(0, 5, 18) rounds, enforce_consistency=True, track=False,
        capacity=2**20, timing=False."""
        return Traffic(self, **cfg)

    def address(self, v):
        buf = ctypes.create_string_buffer(64)
        check(lib().rp_sim_address(self._h, v, buf, 64))
        return buf.value.decode()

    # ---- wire bridge: the node-level ping path between rounds (wire.py codes
    # the JSON); changes are int64 rows (address, status, incarnation,
    # source, source incarnation), -1 / 0 = undefined
    def _rows(self, rows):
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 5))
        return r, len(r)

    def ping_body(self, v):
        """PingSender.send (lib/swim/ping-sender.js:70-76): (changes, checksum, incarnation)."""
        out = np.zeros((self.n, 5), dtype=np.int64)
        cnt, cs, inc = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        check(lib().rp_sim_ping_body(self._h, v, ptr(out), self.n, ctypes.byref(cnt), ctypes.byref(cs),
                                     ctypes.byref(inc)))
        return out[: cnt.value], cs.value, inc.value

    def handle_ping(self, v, source, source_inc, checksum, rows):
        """handlePing (server/ping-handler.js:22-40): (response changes, applied, full_sync)."""
        r, k = self._rows(rows)
        out = np.zeros((self.n, 5), dtype=np.int64)
        cnt, ap, fs = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0)
        check(lib().rp_sim_handle_ping(self._h, v, int(source), int(source_inc), int(checksum) & 0xFFFFFFFF,
                                       ptr(r), k, ptr(out), self.n, ctypes.byref(cnt), ctypes.byref(ap),
                                       ctypes.byref(fs)))
        return out[: cnt.value], ap.value, bool(fs.value)

    def update(self, v, rows):
        """Membership.update at node v (PingSender.onPing, lib/swim/ping-sender.js:36-39): applied count."""
        r, k = self._rows(rows)
        ap = ctypes.c_uint32(0)
        check(lib().rp_sim_update(self._h, v, ptr(r), k, ctypes.byref(ap)))
        return ap.value

    def checksum(self, v):
        """membership.checksum of node v."""
        return int(self.checksums()[v])

    def addresses(self):
        if getattr(self, "_addrs", None) is None:
            self._addrs = [self.address(v) for v in range(self.n)]
        return self._addrs

    def enable_timing(self, on=True, stages=None):
        """Per-stage device time from now on (kernel_times).  stages: the
        KERNEL_CATEGORIES names (and "exchange") to time; None = all.  Each
        timed stage puts two events per launch on the simulation stream."""
        if stages is None:
            check(lib().rp_sim_enable_timing(self._h, 1 if on else 0))
            return
        names = list(KERNEL_CATEGORIES) + ["exchange"]
        mask = 0
        for st in stages:
            mask |= 1 << names.index(st)
        check(lib().rp_sim_enable_timing_stages(self._h, mask if on else 0))

    def kernel_times(self):
        ms = np.zeros(6, dtype=np.float64)
        cnt = np.zeros(6, dtype=np.uint64)
        check(lib().rp_sim_kernel_times(self._h, ptr(ms), ptr(cnt)))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(KERNEL_CATEGORIES)}

    def side_ms(self):
        """Device ms of the side stream's checksum chains and fullSync decisions
        (beside the ping and response merges; one shard), since enable_timing."""
        ms = np.zeros(1, dtype=np.float64)
        check(lib().rp_sim_side_ms(self._h, ptr(ms)))
        return float(ms[0])
