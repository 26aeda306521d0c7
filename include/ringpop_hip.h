/*
 * ringpop_hip.h — C ABI of the MI355X-native ringpop membership-convergence
 * path (libringpop_hip.so, gfx950).
 *
 * Drop-in boundary: these entry points are what the reference's JavaScript
 * would bind through a thin N-API addon.  Each block
 * names the reference interface it replaces (paths relative to the
 * reference repository).  Plain pointers and sizes only; every function
 * returns RP_OK (0) or a negative RP_ERR_* code, with a message available from
 * rp_last_error().  Host buffers are copied; *_device variants take device
 * pointers and a hipStream_t (passed as void *).
 */
#ifndef RINGPOP_HIP_H
#define RINGPOP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_OK 0
#define RP_ERR_INVALID (-1)     /* bad argument */
#define RP_ERR_HIP (-2)         /* HIP runtime error (no GPU, launch failure, ...) */
#define RP_ERR_NOMEM (-3)       /* device allocation failed */
#define RP_ERR_UNSUPPORTED (-4) /* configuration outside what the device path models */
#define RP_ERR_CAPACITY (-5)    /* a device arena overflowed; recreate with more capacity */
#define RP_ERR_STATE (-6)       /* a kernel raised an error flag */

const char *rp_last_error(void);
int rp_abi_version(void);
/* select the HIP device used by objects created afterwards (default 0) */
int rp_set_device(int device);

/* ---- device utilities --------------------------------------------------------
 * Buffers, streams and events of the HIP runtime this library links, for
 * callers of the *_device entry points that have no runtime handle of their
 * own (bench.py, tests).  memcpy kind: 1 host->device, 2 device->host,
 * 3 device->device. */
int rp_device_malloc(size_t bytes, void **out);
int rp_device_free(void *ptr);
int rp_device_memcpy(void *dst, const void *src, size_t bytes, int kind);
int rp_device_synchronize(void);
/* free / total bytes of the current device (hipMemGetInfo): the footprint report of bench.py */
int rp_device_memory(size_t *free_bytes, size_t *total_bytes);
int rp_stream_create(void **out);
int rp_stream_destroy(void *stream);
int rp_stream_synchronize(void *stream);
int rp_event_create(void **out);
int rp_event_record(void *event, void *stream);
int rp_event_elapsed_ms(void *start, void *end, float *ms);
int rp_event_destroy(void *event);
/* this box's memory ceilings for the round kernels' access kinds (bench.py's
 * box_ceiling; measurement infrastructure, no reference counterpart): over a
 * fresh device allocation of `bytes` (>= 1 GiB, past the Infinity Cache),
 * out[0..4] = accesses per second of random 16-byte reads, random 16-byte
 * read + 8-byte write-backs, random 4-byte reads, 16-byte-per-lane streaming
 * reads and 4-byte-per-lane streaming reads (nout >= 5) */
int rp_calibrate(size_t bytes, double *out, int nout);
/* the current device's PCI bus id ("0000:xx:yy.z"), to find its sysfs clocks */
int rp_device_pci_bus_id(char *buf, int len);

/* ---- farmhash.hash32 -------------------------------------------------------
 * Replaces npm `farmhash` ^0.2.0 `hash32(string)` (package.json:30), called at
 * lib/membership.js:57 and as HashRing's default hashFunc at lib/ring.js:29.
 * Strings are given as one byte buffer plus n+1 offsets (string i is
 * bytes[offsets[i] .. offsets[i+1])). Computed on the device. */
int rp_hash32(const uint8_t *bytes, size_t len, uint32_t *out);
int rp_hash32_batch(const uint8_t *bytes, const uint64_t *offsets, size_t n, uint32_t *out);
int rp_hash32_batch_device(const uint8_t *d_bytes, const uint64_t *d_offsets, size_t n, uint32_t *d_out,
                           void *stream);

/* ---- HashRing ----------------------------------------------------------------
 * Replaces lib/ring.js:25-184 (HashRing) and its lib/rbtree.js index.
 * Servers are identified by the index of their first appearance
 * (rp_ring_server_name maps back).  add/remove follow addRemoveServers
 * (lib/ring.js:60-94): adds in order (insert-if-absent per replica point),
 * then removes (erase by hash).  add_hashes / rm_hashes, when non-NULL, give
 * the replica hashes [n * replica_points] instead of farmhash32(name + i):
 * the reference's `hashFunc` option (lib/ring.js:29). */
typedef struct rp_ring rp_ring;
int rp_ring_create(int replica_points, rp_ring **out);
int rp_ring_destroy(rp_ring *ring);
int rp_ring_add_remove(rp_ring *ring, const uint8_t *add_bytes, const uint64_t *add_offsets, size_t nadd,
                       const uint32_t *add_hashes, const uint8_t *rm_bytes, const uint64_t *rm_offsets,
                       size_t nrm, const uint32_t *rm_hashes, int *changed);
/* device time of the last rp_ring_add_remove that changed the ring: replica
 * hashing, the stable radix sort of the points, first-inserter dedupe and
 * compaction, the lookup directories (HIP events around the device work;
 * names cross PCIe inside it) */
int rp_ring_build_ms(rp_ring *ring, double *device_ms);
/* host microseconds of the last rp_ring_add_remove by phase and of the last
 * computed rp_ring_checksum (measurement): us[i] for
 * i < n, indexed by RP_RING_PROF_*; phases a bulk call skips are 0 */
#define RP_RING_PROF_SELECT 0   /* name interning, present / duplicate checks */
#define RP_RING_PROF_HASH 1     /* replica hashes (incremental path: on the host) */
#define RP_RING_PROF_MERGE 2    /* host mirror delta, staging copy, k_ring_merge launch */
#define RP_RING_PROF_INDEX 3    /* lookup-index rebuild launches and events */
#define RP_RING_PROF_TOTAL 4    /* the whole call */
#define RP_RING_PROF_CK_BUILD 5 /* checksum: the sorted, ';'-joined server string */
#define RP_RING_PROF_CK_HASH 6  /* checksum: copy, hash kernel, synchronisation */
#define RP_RING_PROF_N 7
int rp_ring_profile(rp_ring *ring, double *us, int n);
int rp_ring_server_count(rp_ring *ring, int *out);                                  /* :107-109 */
int rp_ring_has_server(rp_ring *ring, const uint8_t *name, size_t len, int *out);   /* :111-113 */
int rp_ring_checksum(rp_ring *ring, uint32_t *out);                                 /* :96-105 */
int rp_ring_server_name(rp_ring *ring, int index, char *buf, size_t cap, size_t *len);
/* lookup (lib/ring.js:138-147): owner server index per key, -1 on an empty ring */
int rp_ring_lookup_batch(rp_ring *ring, const uint8_t *bytes, const uint64_t *offsets, size_t n,
                         int32_t *owners);
int rp_ring_lookup_batch_device(rp_ring *ring, const uint8_t *d_bytes, const uint64_t *d_offsets, size_t n,
                                int32_t *d_owners, void *stream);
/* lookup for precomputed key hashes (custom hashFunc) */
int rp_ring_lookup_hashes(rp_ring *ring, const uint32_t *key_hashes, size_t n, int32_t *owners);
/* lookupN (lib/ring.js:150-182): up to n distinct owners per key hash; out is
 * [nkeys * n], unused slots -1; counts[k] = owners found */
int rp_ring_lookup_n_hashes(rp_ring *ring, const uint32_t *key_hashes, size_t nkeys, int n, int32_t *out,
                            int32_t *counts);
/* handleOrProxyAll's grouping (index.js:636-645: _.groupBy(keys, this.lookup),
 * then Object.keys): groups in first-appearance order of their owner, keys of
 * a group in input order.  dests[g] = owner server index (-1: empty ring, the
 * reference's "null" group); the keys of group g are
 * key_index[group_off[g] .. group_off[g + 1]).  Arrays: dests and key_index
 * [n], group_off [n + 1]; *ngroups receives the group count (n < 2^31 - 1). */
int rp_ring_group_keys(rp_ring *ring, const uint8_t *bytes, const uint64_t *offsets, size_t n, int32_t *dests,
                       uint32_t *group_off, uint32_t *key_index, size_t *ngroups);
/* the same for precomputed key hashes (custom hashFunc) */
int rp_ring_group_hashes(rp_ring *ring, const uint32_t *key_hashes, size_t n, int32_t *dests, uint32_t *group_off,
                         uint32_t *key_index, size_t *ngroups);
/* device arrays: owners from rp_ring_lookup_batch_device; synchronises `stream` */
int rp_ring_group_device(rp_ring *ring, const int32_t *d_owners, size_t n, int32_t *d_dests, uint32_t *d_group_off,
                         uint32_t *d_key_index, size_t *ngroups, void *stream);
/* sorted distinct points (rbtree in-order walk) */
int rp_ring_points(rp_ring *ring, uint32_t *hashes, int32_t *owners, size_t cap, size_t *count);
/* device-generated synthetic keys: decimal strings of splitmix64(seed + i*golden)
 * (benchmark config 3); returns device pointers owned by the ring object */
int rp_ring_make_keys_device(rp_ring *ring, uint64_t seed, size_t n, const uint8_t **d_bytes,
                             const uint64_t **d_offsets, uint64_t *total_bytes);

/* ---- Simulation of N ringpop instances ---------------------------------------
 * Each simulated node runs the reference's Membership (lib/membership.js),
 * Dissemination (lib/dissemination.js), HashRing and MembershipIterator
 * state; a round is one protocol period for every live node
 * (index.js:458-515) under the synchronous semantics of DESIGN.md §3. */
typedef struct rp_sim rp_sim;
typedef struct {
    uint32_t n;               /* simulated nodes (<= 65536) */
    uint32_t churn_k;         /* alive re-assertions per churning round */
    uint64_t seed;
    uint64_t arena_entries;   /* message arena capacity (16-byte changes); 0 = auto */
    uint32_t snapshot_slots;  /* full-sync snapshots per round; 0 = auto */
    uint32_t origin_slots;    /* update-origin table capacity (0 = auto = 2^23 - 1, the maximum): n + 1 fixed slots, a ring of
                                 makeAlive origins (a power of two) and per-shard rings of local
                                 suspect/faulty origins in the top quarter; slots are reused once
                                 every reference to their previous origin has expired */
    uint32_t seen_window;     /* ids per node in the seen-origin bitset (power of two in [32, 32768]); 0 = auto */
    uint32_t replica_hash_shift; /* testing: clear this many low bits of every replica hash (forces
                                    rbtree collisions; 0 = the reference's hashes, < 32) */
    uint32_t compact_mul;     /* an issue squeezes the tombstones out of a dissemination log whose span */
    uint32_t compact_add;     /* exceeds compact_mul x its live keys + compact_add (0, 0 = auto: 4, 8192);
                                 a layout choice with no observable effect (tests force it with tiny values) */
    uint32_t prefix_min;      /* after an issue, the live entries of the window's first groups move forward to the
                                 end of that prefix when that shrinks the window by >= (entries moved) + prefix_min
                                 (0 = auto: 512; never below 1); a layout choice with no observable effect */
    uint32_t ck_lane_min;     /* a list of at least this many distinct views to checksum is hashed one view per
                                 lane (k_checksums_lanes), shorter ones one view per wave (0 = auto: 12288;
                                 1 = always per lane, 0xFFFFFFFF = never); same checksums either way */
    uint32_t issue_wave;      /* the issue kernels of runs without faults on n % 64 == 0 nodes: 1 = one 256-thread
                                 block per node, 2 = one wave per node in one pass, 0 = the build's default (2);
                                 every other run takes the block kernels; same results either way */
} rp_sim_config;

typedef struct {
    uint64_t evaluated;   /* changes passed to Membership.update() */
    uint64_t applied;     /* changes applied */
    uint64_t full_syncs;  /* Dissemination.fullSync() responses */
    uint64_t messages;    /* requests + responses */
    uint64_t waves;
    uint64_t pings;
    uint64_t converged;   /* all live views identical after the round */
} rp_round_stats;

int rp_sim_create(const rp_sim_config *cfg, rp_sim **out);
int rp_sim_destroy(rp_sim *sim);

/* ---- Sharded simulations -------------------------------------
 * The N nodes are split into G shards of N/G consecutive ids (G divides N,
 * G <= 64).  Each round the shards exchange ping metadata, checksum
 * snapshots, ping bodies and responses, and with fail-stops or partitions
 * the ping-req waves (ping-req bodies, relay pings, their responses; the
 * suspect/faulty update origins travel with them).  Results equal the
 * single-shard run's bit for bit.
 *   rp_sim_create_shards: all G shards in this process on the current device
 *     (exchanges are device copies); results equal rp_sim_create's.
 *   rp_sim_create_rank: this process holds shard `rank` of `nranks`, one
 *     process per GPU; exchanges are RCCL all-gathers and send/recv groups
 *     over the communicator named by `unique_id` (from rp_comm_unique_id on
 *     one rank, 128 bytes, distributed by the caller).  Per-node reads
 *     (read_view, read_changes, ...) only reach this process's nodes;
 *     rp_sim_read_checksums leaves other nodes' entries 0. */
int rp_sim_create_shards(const rp_sim_config *cfg, int nshards, rp_sim **out);
int rp_comm_unique_id(uint8_t *unique_id, size_t cap);
int rp_sim_create_rank(const rp_sim_config *cfg, int nranks, int rank, const uint8_t *unique_id, rp_sim **out);
/* The RCCL transport the rank path uses (in-place all-gather, u32 sum
 * all-reduce, a grouped send/recv with every rank, broadcast), run on small
 * buffers of `words` u32 with predictable contents over the communicator
 * named by `unique_id`; *failures = words that differ from the expectation.
 * Every rank calls it; nranks = 1 exercises every call on one GPU (sends to
 * itself).  Replaces nothing in the reference: a check of the transport that
 * carries lib/swim/ping-sender.js:81-99's traffic between GPUs. */
int rp_comm_selftest(int nranks, int rank, const uint8_t *unique_id, uint32_t words, uint32_t *failures);
/* The rank path without RCCL, for one GPU: the ranks of an nranks-rank
 * cluster as host threads of this process on the current device (each rank
 * its own rp_sim, its calls made from its own thread, every rank making the
 * same calls in the same order).  The collectives are device copies after a
 * rendezvous of the rank threads; everything else is rp_sim_create_rank's
 * code.  A rank that fails or stalls for 120 s fails the others'
 * collectives.  Destroy the loop after its ranks. */
typedef struct rp_loop rp_loop;
int rp_loop_create(int nranks, rp_loop **out);
int rp_loop_destroy(rp_loop *loop);
int rp_sim_create_rank_loop(const rp_sim_config *cfg, rp_loop *loop, int rank, rp_sim **out);
/* nodes [lo, hi) held by this process */
int rp_sim_shard_range(rp_sim *sim, uint32_t *lo, uint32_t *hi);
/* rp_sim_counters restricted to the work of this process's shards (the
 * per-kernel unit counts behind its own kernel times); converged rounds 0 */
int rp_sim_local_counters(rp_sim *sim, uint64_t *out, int cap, int *n);
/* since rp_sim_enable_timing: device time of the exchange steps (planning and
 * packing kernels, copies / RCCL collectives, host waits for their counts;
 * ms, timing enabled only), bytes this process sent, rounds exchanged */
int rp_sim_exchange_stats(rp_sim *sim, double *ms, uint64_t *bytes_sent, uint64_t *rounds);
/* since rp_sim_enable_timing: bytes each of this process's shards sent to
 * other shards (all-gathers, all-to-alls, all-reduces; in-process shards
 * count the device copies a shard's data is the source of), out[i] for its
 * i-th local shard; *count = the local shards */
int rp_sim_exchange_shard_bytes(rp_sim *sim, uint64_t *out, int cap, int *count);
/* Arbitrary clusters; both before the first round, and in a
 * multi-process cluster every rank makes the same calls.
 * rp_sim_load_addresses: the cluster's n address strings (bytes[off[i] ..
 * off[i+1]), 1..32 printable ASCII bytes, distinct, in ascending sort order:
 * node i is the i-th address, so a view indexed by id is in the order
 * generateChecksumString sorts members, lib/membership.js:62-93).  Replaces
 * the 10.x.x.x:300x scheme; every view is re-bootstrapped as rp_sim_create does,
 * so it must come FIRST: after rp_sim_set_views, rp_sim_join, rp_sim_leave or
 * rp_sim_rejoin it fails with RP_ERR_STATE.  Call order: create,
 * load_addresses, set_views / join / leave / rejoin, rounds.
 * rp_sim_set_views: re-bootstrap nodes [node_lo, node_lo + count) from
 * views -- status[r * n + a] (0 absent, 1 alive, 2 suspect, 3 faulty, 4 leave) and
 * incarnation[r * n + a] of member a in node node_lo + r's view, its own
 * entry alive -- as the reference's bootstrap does with that join result:
 * makeAlive(self, inc), set() (lib/membership.js:162-206) whose listener adds
 * the alive members to the ring and starts a suspicion timer per suspect
 * (lib/membership-set-listener.js:24-48; due at round 0), shuffle(),
 * clearChanges().  Replaces the full-alive views of rp_sim_create (index.js:
 * 233-267 with a full-membership join result). */
int rp_sim_load_addresses(rp_sim *sim, const uint8_t *bytes, const uint64_t *offsets, uint32_t n);
/* Join path, before the first round: node joiners[i]
 * stays outside the cluster (no view, not pinging, absent from every view)
 * until the start of round rounds[i] (after the due suspicion timers, before
 * churn), when it joins through seeds[i * seeds_per ..] (-1 = none; each
 * seed a member from the start or joined in an earlier round) as the
 * reference bootstraps: makeAlive(self, now) (index.js:235), each seed's
 * handleJoin -- makeAlive(joiner) then its checksum and fullSync()
 * (server/join-handler.js:76-98) --, mergeJoinResponses (lib/swim/
 * join-response-merge.js:40-56), update() + set() (lib/membership.js:162-206)
 * and shuffle().  The other nodes are re-bootstrapped with views of each
 * other (everyone alive at 1434401518824 + id); the merges then splice
 * members they learn of at getJoinPosition (lib/membership.js:99-101,
 * 285-298).  Once per simulation. */
int rp_sim_join(rp_sim *sim, const uint32_t *joiners, const uint32_t *rounds, const int32_t *seeds, uint32_t count,
                uint32_t seeds_per);
int rp_sim_set_views(rp_sim *sim, uint32_t node_lo, uint32_t count, const int32_t *status,
                     const int64_t *incarnation);
/* fail-stop `node` at the start of `round` (it stops pinging and answering;
 * requests to it come back as transport errors one wave later) */
int rp_sim_fail(rp_sim *sim, uint32_t node, uint32_t round);
/* Graceful leave and rejoin: scheduled events of round
 * `round` >= the current one, run after the round's joins and before its
 * churn.  Per node the events alternate leave, rejoin, leave, ... in strictly
 * increasing rounds, added in that order; anything else is RP_ERR_INVALID.
 * An event of a node that has fail-stopped or not joined yet is skipped.
 * Both calls mark the ring checksums stale; in a multi-process cluster every
 * rank makes the same calls.
 * rp_sim_leave replaces server/admin-leave-handler.js:30-57:
 * membership.makeLeave(self, own incarnation) (lib/membership.js:150-152,
 * 324-352; the update listener takes the node out of its own ring and
 * records the change, lib/membership-update-listener.js:42-47), gossip.stop()
 * -- the node pings nobody; it still answers pings and ping-reqs, applies
 * updates and refutes suspicions of itself -- and suspicion.stopAll()
 * (lib/swim/suspicion.js:87-108: pending timers cancelled, and no suspect
 * update starts one until the rejoin, :46-51).  Churn, storms and
 * rp_round_stats.converged range over nodes that are live and gossiping.
 * rp_sim_rejoin replaces the rejoin branch of server/admin-join-handler.js:
 * 36-45: makeAlive(self, now), gossip.start() (one membership.shuffle(),
 * lib/swim/gossip.js:85) and suspicion.reenable() (lib/swim/suspicion.js:
 * 30-43).  The node's own status must be leave then: a left node that refuted
 * a suspicion is alive, the reference would run its join-sender, which is not
 * modelled -- the next call that reads the simulation returns RP_ERR_STATE. */
int rp_sim_leave(rp_sim *sim, uint32_t node, uint32_t round);
int rp_sim_rejoin(rp_sim *sim, uint32_t node, uint32_t round);
/* bit 0: the node's gossip is stopped (Gossip.isStopped, lib/swim/gossip.js);
 * bit 1: its suspicion is stopped (Suspicion.isStoppedAll, lib/swim/
 * suspicion.js:26).  Marks the ring checksums stale. */
int rp_sim_node_flags(rp_sim *sim, uint32_t node, uint32_t *flags);
/* requests between ids on different sides of `split` fail during rounds
 * [start, end) (partition injection; split = 0 disables) */
int rp_sim_partition(rp_sim *sim, uint32_t start, uint32_t end, uint32_t split);
/* false-suspicion storm (config 5): in rounds [start, end),
 * after churn, ceil(live * ppm / 10^6) seeded live victims are each suspected
 * by a seeded live accuser through Membership.makeSuspect(victim, the
 * accuser's incarnation of it) (lib/membership.js:154-156); victims refute
 * through the local override (:244-254).  ppm = 0 disables. */
int rp_sim_storm(rp_sim *sim, uint32_t start, uint32_t end, uint32_t ppm);
/* run one round and return its statistics (synchronous) */
int rp_sim_round(rp_sim *sim, int churn_active, rp_round_stats *stats);
/* enqueue k rounds on the simulation's stream (asynchronous); totals accumulate */
int rp_sim_run(rp_sim *sim, int k_rounds, int churn_active);
int rp_sim_sync(rp_sim *sim);
int rp_sim_totals(rp_sim *sim, rp_round_stats *totals);
int rp_sim_rounds(rp_sim *sim, uint32_t *rounds);
/* cumulative device counters: evaluated, applied, full_syncs, messages, waves,
 * pings, then per kernel: ping-merge evaluated/applied, response-merge
 * evaluated/applied, sender-issue scanned/emitted, receiver-issue
 * scanned/emitted and written, touched (all merges / ping merge), views
 * checksummed by k_checksums, six diagnostic counters, then converged
 * rounds (ringpop_amd/sim.py Sim.COUNTERS); returns the count in *n */
int rp_sim_counters(rp_sim *sim, uint64_t *out, int cap, int *n);
/* simulated node count */
int rp_sim_size(rp_sim *sim, uint32_t *n);
/* Membership.checksum of every node (farmhash32 of the checksum string);
 * out holds cap >= n entries */
int rp_sim_read_checksums(rp_sim *sim, uint32_t *out, size_t cap);
/* status (0 absent,1 alive,2 suspect,3 faulty,4 leave) and incarnation per address */
/* ---- Wire-format bridge (node-level ping path, between rounds) -------------
 * The reference's ping wire surface for one simulated node, so that a host
 * codec can speak the JSON bodies of lib/swim/ping-sender.js:70-76 and
 * server/ping-handler.js:36-39 (ringpop_amd/wire.py, js/index.js).  A change
 * is 5 int64: address and source are member ids (rp_sim_address; source -1 =
 * undefined), status 1 alive 2 suspect 3 faulty 4 leave, source_incarnation 0
 * = undefined.  Each call runs on the node's shard with the next round's
 * clock; changes from the wire get update origins of their own (the receiver
 * filter compares origins by value), so round results stay the reference's.
 *   rp_sim_ping_body    PingSender.send (ping-sender.js:70-76): issueAsSender
 *                       (advances piggyback counts), membership.checksum,
 *                       getIncarnationNumber()
 *   rp_sim_handle_ping  handlePing (server/ping-handler.js:22-40):
 *                       Membership.update(changes), then issueAsReceiver(source,
 *                       source_incarnation, checksum); *full_sync = 1 when the
 *                       response is Dissemination.fullSync() (:102-117)
 *   rp_sim_update       PingSender.onPing's Membership.update (ping-sender.js:36-39)
 * Output buffers must hold cap >= n changes (a fullSync is n of them; the
 * call is refused before any state changes otherwise); *count is the list
 * length. */
typedef struct {
    int64_t address;
    int64_t status;
    int64_t incarnation;
    int64_t source;
    int64_t source_incarnation;
} rp_change;
int rp_sim_ping_body(rp_sim *sim, uint32_t node, rp_change *out, uint32_t cap, uint32_t *count, uint32_t *checksum,
                     uint64_t *incarnation);
int rp_sim_handle_ping(rp_sim *sim, uint32_t node, int64_t source, uint64_t source_incarnation, uint32_t checksum,
                       const rp_change *changes, uint32_t n, rp_change *out, uint32_t cap, uint32_t *count,
                       uint32_t *applied, int *full_sync);
int rp_sim_update(rp_sim *sim, uint32_t node, const rp_change *changes, uint32_t n, uint32_t *applied);

/* per node, 6 counts: members absent / alive / suspect / faulty / leave in its
 * view and its ring's server count (nodes of other processes: 0); out holds
 * cap >= 6 n entries */
int rp_sim_view_counts(rp_sim *sim, uint32_t *out, size_t cap);
/* status / inc hold cap >= n entries (either may be NULL) */
int rp_sim_read_view(rp_sim *sim, uint32_t node, uint8_t *status, uint64_t *inc, size_t cap);
/* Membership.members order; out holds cap >= n entries */
int rp_sim_read_members(rp_sim *sim, uint32_t node, uint32_t *out, size_t cap, uint32_t *count);
/* Dissemination.changes in key order: rows of 6 int64 {address, piggybackCount
 * (-1 undefined), source (-1), sourceIncarnationNumber (0 undefined), status,
 * incarnationNumber} */
int rp_sim_read_changes(rp_sim *sim, uint32_t node, int64_t *rows, uint32_t cap, uint32_t *count);
/* {maxPiggybackCount, ring server count, ring checksum, iterator index,
 *  iterator round, dead, rng state, pending suspicion timers} */
int rp_sim_node_info(rp_sim *sim, uint32_t node, int64_t *info8);
/* ring.lookup in one node's view, for precomputed key hashes */
int rp_sim_ring_lookup(rp_sim *sim, uint32_t node, const uint32_t *key_hashes, size_t n, int32_t *owners);
int rp_sim_address(rp_sim *sim, uint32_t node, char *buf, size_t cap);

/* ---- Request routing across the cluster (between rounds) ---------------------
 * rp_sim_ring_checksums: HashRing.checksum of every node's ring (lib/ring.js:
 * 96-105): farmhash32 of its servers' addresses, sorted and joined by ';'
 * (node ids are in address sort order).  out holds cap >= n entries; a
 * fail-stopped node reports its frozen ring, nodes of other processes' shards
 * report 0.  Computed on the device, one wave per view, and cached until a
 * call that can change a ring (round / run, update, handle_ping, set_views,
 * join, load_addresses).
 *
 * rp_sim_route: what RingPop.handleOrProxy (index.js:607-634; lookup :409-423)
 * and the request proxy see for a batch of requests, request i entering the cluster
 * at node entries[i] with farmhash32(key) = key_hashes[i].  Like the wire
 * bridge it runs with the clock of the next round: after k rounds the
 * partition window is tested with round k.  The first rule that applies:
 *   4 ENTRY_DEAD        the entry node is fail-stopped; dest -1
 *   0 LOCAL             dest = HashRing.lookup(key) in the entry's ring
 *                       (lib/ring.js:138-147) is the entry itself, or its ring
 *                       is empty (lookup falls back to whoami); dest = entry
 *   3 UNREACHABLE       dest is fail-stopped or the partition separates the
 *                       two: a transport error, the reference would enter
 *                       scheduleRetry (lib/request-proxy/send.js:105-127)
 *   2 CHECKSUMS_DIFFER  the two nodes' ring checksums differ
 *                       (lib/request-proxy/index.js:172-187)
 *   1 DELIVERED         otherwise
 * owner_agrees[i] = 1 for outcomes 1 and 2 when the lookup of the key in the
 * destination's ring is the destination itself, else 0 (such a request counts
 * in `misrouted`; for the other outcomes it is 0).  dests, outcomes and
 * owner_agrees may each be NULL; stats->requests is the sum of the five
 * outcome counts.  A route is one instant: requests that retry across rounds
 * (send.js:267-294) are rp_traffic_*'s, below.
 *
 * rp_sim_route_uniform: the same for `count` requests generated on the
 * device, only the statistics returned.  Request i (0-based) is
 *   r = splitmix64_finalise(seed + (i + 1) * 0x9E3779B97F4A7C15)   (mod 2^64)
 *   entry = ((r >> 32) * n) >> 32,   key_hash = (uint32_t)r
 * with the finaliser z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 * z *= 0x94D049BB133111EB; z ^= z >> 31.
 *
 * Both need every node's view on this process's device: on one rank of a
 * multi-process or loop cluster they return RP_ERR_UNSUPPORTED. */
typedef struct {
    uint64_t requests, local, delivered, checksums_differ, unreachable, entry_dead, misrouted, reserved;
} rp_route_stats;
int rp_sim_ring_checksums(rp_sim *sim, uint32_t *out, size_t cap);
int rp_sim_route(rp_sim *sim, const uint32_t *entries, const uint32_t *key_hashes, size_t n, int32_t *dests,
                 uint8_t *outcomes, uint8_t *owner_agrees, rp_route_stats *stats);
int rp_sim_route_uniform(rp_sim *sim, uint64_t seed, uint64_t count, rp_route_stats *stats);

/* ---- Ownership census (between rounds) ---------------------------------------
 * For the whole 2^32 hash space, how many live nodes believe they own a key
 * (DESIGN.md §13).  Node v is a claimant iff it is neither fail-stopped nor
 * still outside the cluster (rp_sim_node_info's dead == 0; a node that left
 * gracefully is one, and its ring, which lacks itself, claims nothing).  v
 * claims hash h iff HashRing.lookup(h) in v's own view is v (index.js:409-423,
 * handleOrProxy's dest === whoami() test, :607-634), or v's ring is empty
 * (lookup falls back to whoami: rp_sim_route's LOCAL rule).
 *
 * The sorted distinct replica hashes pt_hash[0 .. intervals) of all n servers
 * cut the hash space into `intervals` intervals: interval i >= 1 is
 * (pt_hash[i-1], pt_hash[i]], interval 0 is the wrap -- the hashes above the
 * last point and up to the first.  Every view's lookup is constant on an
 * interval; claims(i) is the number of claimants that claim it.
 *
 * rp_sim_ownership: measure[k] is the number of hashes with exactly k
 * claimants (k < 7; measure[7]: 7 or more; the eight sum to 2^32);
 * max_claims the largest claims(i) and max_claims_hash the pt_hash[i] of the
 * first interval (lowest i) that reaches it.  claimed (NULL, or cap >= n
 * entries) gets per node the number of hashes it claims: 0 for a node that is
 * no claimant, 2^32 for an empty ring or a ring of the node alone.
 *
 * rp_sim_ownership_at: claims[j] = claims(i) of the interval key_hashes[j]
 * falls in (the first point >= the hash, else interval 0).
 *
 * Both are exact, computed on the device in time proportional to the ring's
 * points, and cached like the ring checksums: a second call without a call
 * that can change a ring in between only copies.  Like a route they need every
 * node's view on this process's device: RP_ERR_UNSUPPORTED on one rank of a
 * multi-process or loop cluster; in-process shards give the one-shard results.
 * A claimed buffer with cap < n is RP_ERR_INVALID before any state changes. */
typedef struct {
    uint64_t measure[8];
    uint64_t claimants, intervals, max_claims, max_claims_hash;
    uint64_t reserved[4];
} rp_ownership_stats;
int rp_sim_ownership(rp_sim *sim, rp_ownership_stats *stats, uint64_t *claimed, size_t cap);
int rp_sim_ownership_at(rp_sim *sim, const uint32_t *key_hashes, size_t n, uint32_t *claims);

/* ---- Ownership movement between two instants ---------------------------------
 * Which keys changed hands.  A snapshot fixes, at the clock it
 * is taken (rounds run so far), the claim set C(v) of every node v: the
 * intervals v claims under the census' definition -- none for a node that is
 * no claimant, every interval for an empty ring or a ring of v alone.  It owns
 * its device buffers (per node up to 100 arcs, and the census' claims(i):
 * about 79 MB at 65,536 nodes); any number may be live, and a snapshot and its
 * simulation may be destroyed in either order.
 * rp_ownership_snapshot_info: the census' stats at the snapshot and its clock
 * (each may be NULL).
 *
 * rp_sim_ownership_moved compares `from` with `to`, or with the simulation as
 * it is now when `to` is NULL (through the census' cache: without a call that
 * can change a ring in between, the current arcs are recorded once).  Node v
 * gains C_to(v) \ C_from(v) and loses C_from(v) \ C_to(v); gained[v] and
 * lost[v] (each NULL, or cap >= n entries) are the numbers of hashes in them,
 * 0 to 2^32.  Per interval i, g(i) nodes gain it and l(i) lose it, and
 * claims_to(i) = claims_from(i) + g(i) - l(i).  In the stats
 *   transition[a][b]  hashes with min(claims_from, 2) = a and
 *                     min(claims_to, 2) = b (the nine sum to 2^32);
 *   same_set          hashes with g = l = 0;
 *   handed_off        hashes with claims_from = claims_to = 1 and g = l = 1:
 *                     one owner before, another after;
 *   gained, lost      the sums of gained[v] and lost[v]; gainers, losers the
 *                     numbers of nodes where they are not 0;
 *   max_gained(_node), max_lost(_node)  the largest, and the lowest node id
 *                     that reaches it (node 0 when nothing moved);
 *   max_turnover(_hash)  the largest g(i) + l(i) and the pt_hash[i] of the
 *                     lowest such interval (hash 0 when nothing moved);
 *   from_clock, to_clock, intervals  the two clocks and the interval count.
 * Exact, on the device, in time proportional to the ring's points.  Errors:
 * RP_ERR_UNSUPPORTED on one rank of a multi-process or loop cluster (as for
 * the census); RP_ERR_INVALID for a snapshot of another simulation or
 * cap < n; RP_ERR_STATE for a snapshot taken before rp_sim_load_addresses
 * changed the points. */
typedef struct rp_ownership_snapshot rp_ownership_snapshot;
typedef struct {
    uint64_t transition[3][3];
    uint64_t same_set, handed_off, gained, lost, gainers, losers;
    uint64_t max_gained, max_gained_node, max_lost, max_lost_node, max_turnover, max_turnover_hash;
    uint64_t from_clock, to_clock, intervals;
    uint64_t reserved[8];
} rp_movement_stats;
int rp_ownership_snapshot_create(rp_sim *sim, rp_ownership_snapshot **out);
int rp_ownership_snapshot_info(const rp_ownership_snapshot *snap, rp_ownership_stats *stats, uint64_t *clock);
int rp_ownership_snapshot_destroy(rp_ownership_snapshot *snap);
int rp_sim_ownership_moved(rp_sim *sim, const rp_ownership_snapshot *from, const rp_ownership_snapshot *to,
                           rp_movement_stats *stats, uint64_t *gained, uint64_t *lost, size_t cap);

/* ---- Request traffic with proxy retries across rounds ------------------------
 * Replaces the RequestProxySend state machine (lib/request-proxy/send.js) for
 * batches of single-key requests that live across rounds: a tracker keeps a
 * request table on its simulation's device and advances it between rounds
 * (DESIGN.md §11).  Its clock is the number of rounds run so far, as for
 * rp_sim_route: a partition window and a fail-stop scheduled for round k are
 * tested the same way.  A request is (entry e, key hash h) and gets a 64-bit
 * id in submission order.  "lookup" is HashRing.lookup(h) in e's view at the
 * current clock (an empty ring gives e).  Line numbers are send.js's unless
 * marked.
 *   1 first attempt, at submission (index.js:607-634): e fail-stopped: final
 *     ENTRY_DEAD.  d0 = lookup; d0 == e: final LOCAL.  Otherwise proxied++ and
 *     send(e -> d0).
 *   2 send(e -> d): d fail-stopped or the partition between them:
 *     send_unreachable++, an error.  Else, when the two nodes' ring checksums
 *     differ: checksums_differ++, an error with enforce_consistency
 *     (lib/request-proxy/index.js:172-187), a success without.  A success is
 *     final DELIVERED with dest d; retry_succeeded++ after at least one retry
 *     (:158-167); misrouted++ when the lookup of h in d's own view is not d
 *     (rp_sim_route's owner_agrees rule).
 *   3 on an error (:286-293): retries >= max_retries: final FAILED (dest: the
 *     last destination tried), retry_failed++ unless max_retries is 0 (:261,
 *     :296-304 raise the plain error).  Otherwise retry_scheduled++ and due =
 *     clock + schedule[min(retries, nschedule - 1)] (an index past the end
 *     takes the last entry, as numOrDefault does, :216-217).
 *   4 retry, at the first poll whose clock is >= due (:105-127): e
 *     fail-stopped: final ENTRY_DEAD, nothing else counted.  Otherwise
 *     retries++, retry_attempted++, nd = lookup, compared with the ORIGINAL d0
 *     (channelOpts.host is never updated, :121; a reroute passes other
 *     options to send only, :200-205).  nd == d0: proxied++, send(e -> d0).
 *     Otherwise retry_rerouted++; nd == e: final REROUTED_LOCAL (handleRequest
 *     with e's own checksum; not through handleSuccess, :188-196); else
 *     proxied++, send(e -> nd).
 *   5 a delay of 0 is taken at the same clock in the same call: a call loops a
 *     request until it is final or due later (at most max_retries + 1
 *     attempts).  Requests never change membership state, so their order
 *     changes no result.
 * Multi-key requests (handleOrProxyAll, abortOnKeyDivergence :90-113) are out
 * of scope.  On one rank of a multi-process or loop cluster rp_traffic_create
 * returns RP_ERR_UNSUPPORTED.  Destroy a tracker before its simulation. */
typedef struct rp_traffic rp_traffic;
typedef struct {
    int32_t max_retries;         /* 0..8; < 0 = the default, 3 */
    uint32_t nschedule;          /* delays in schedule[], <= 8; 0 = the default {0, 5, 18}: RETRY_SCHEDULE
                                    [0, 1, 3.5] s (:49) in 200 ms periods, rounded up */
    uint32_t schedule[8];        /* rounds */
    int32_t enforce_consistency; /* < 0 = the default, 1 (lib/request-proxy/index.js:49) */
    uint32_t track;              /* keep a final record per request (rp_traffic_results) */
    uint32_t timing;             /* HIP events around every poll and submit (rp_traffic_times) */
    uint32_t reserved;
    uint64_t capacity;           /* most records the pending table may hold (<= 2^30); 0 = 2^20 */
} rp_traffic_config;
typedef struct {
    uint64_t submitted, local, delivered, rerouted_local, failed, entry_dead, proxied, send_unreachable,
        checksums_differ, retry_scheduled, retry_attempted, retry_rerouted, retry_succeeded, retry_failed,
        misrouted, reserved;
} rp_traffic_stats;
#define RP_REQUEST_LOCAL 0
#define RP_REQUEST_DELIVERED 1
#define RP_REQUEST_REROUTED_LOCAL 2
#define RP_REQUEST_FAILED 3
#define RP_REQUEST_ENTRY_DEAD 4
#define RP_REQUEST_PENDING 255
typedef struct {
    int32_t dest;          /* LOCAL, REROUTED_LOCAL: the entry; DELIVERED: where; FAILED: the last destination
                              tried; ENTRY_DEAD: -1; pending: the first destination */
    uint8_t outcome;       /* RP_REQUEST_* */
    uint8_t retries;
    uint16_t reserved;
    uint32_t submit_clock;
    uint32_t done_clock;   /* pending: 0 */
} rp_request_result;
typedef struct {
    uint64_t id;
    uint32_t entry, key_hash;
    int32_t first_dest;    /* d0 */
    uint32_t due;          /* the clock its next retry is due at */
    uint32_t submit_clock;
    uint32_t retries;
} rp_request_pending;
int rp_traffic_create(rp_sim *sim, const rp_traffic_config *cfg, rp_traffic **out); /* cfg NULL: the defaults */
int rp_traffic_destroy(rp_traffic *traffic);
/* n requests make their first attempts now; *first_id (may be NULL) = the id of request 0 */
int rp_traffic_submit(rp_traffic *traffic, const uint32_t *entries, const uint32_t *key_hashes, size_t n,
                      uint64_t *first_id);
/* the same for requests first .. first + count - 1 of rp_sim_route_uniform's generator with `seed`, drawn on the
 * device; nothing is allocated per request */
int rp_traffic_submit_uniform(rp_traffic *traffic, uint64_t seed, uint64_t first, uint64_t count);
/* every pending request that is due retries */
int rp_traffic_poll(rp_traffic *traffic);
/* k times: one round (rp_sim_round), a poll, a submit_uniform of per_round requests whose generator index continues
 * from the requests earlier rp_traffic_run calls on this tracker drew (0 at first); equal to those calls made one
 * by one, with no readback per round beyond rp_sim_round's error check */
int rp_traffic_run(rp_traffic *traffic, int k_rounds, int churn_active, uint64_t per_round, uint64_t seed);
/* cumulative statistics and by_retries[outcome * 9 + r]: final requests per outcome (5) and retry count r = 0..8
 * (either may be NULL) */
int rp_traffic_read_stats(rp_traffic *traffic, rp_traffic_stats *cumulative, uint64_t *by_retries);
/* rows[i] = what happened in calls made at clock first_clock + i (zero where none was) */
int rp_traffic_history(rp_traffic *traffic, uint32_t first_clock, uint32_t count, rp_traffic_stats *rows);
/* the pending table in submission order; *count = its length; out may be NULL, else cap >= that length */
int rp_traffic_pending(rp_traffic *traffic, rp_request_pending *out, size_t cap, uint64_t *count);
/* the records of requests first_id .. first_id + n - 1 (track only) */
int rp_traffic_results(rp_traffic *traffic, uint64_t first_id, size_t n, rp_request_result *out);
/* timing only: device ms and calls of {polls, submits} since creation; the largest pending count so far (measurement,
 * no reference counterpart; any may be NULL) */
int rp_traffic_times(rp_traffic *traffic, double *ms2, uint64_t *calls2, uint64_t *peak_pending);
/* Capacity: the pending table grows on demand up to `capacity` and never drops a request: submit presizes it for
 * pending + n, run for pending + per_round x min(k_rounds, the retry delays' sum + 1) -- a request stays pending for
 * at most the sum of the delays of its max_retries retries -- and a call that would need more fails with
 * RP_ERR_CAPACITY before any state changes. */

/* per-kernel device time (HIP events on the simulation stream), ms, summed
 * since enable; names: churn, issue(phase1), merge_ping(phase2),
 * merge_resp(phase3), checksum, other */
int rp_sim_enable_timing(rp_sim *sim, int enable);
/* the same for some stages only: bit i of mask times stage i (the order of
 * rp_sim_kernel_times, then 6 = the exchange steps); every timed stage adds
 * two events per launch to the simulation stream, which the timed rounds pay
 * for (bench.py times only the ping merge inside its timed region) */
int rp_sim_enable_timing_stages(rp_sim *sim, uint32_t mask);
int rp_sim_kernel_times(rp_sim *sim, double *ms6, uint64_t *launches6);
/* device time (ms, summed since enable) of the work one shard runs on its
 * side stream beside the round kernels: the round's sender checksum chains
 * (beside the ping merge) and the fullSync decisions (beside the response
 * merge); the "checksum" category above counts only the checksum work left
 * on the simulation stream */
int rp_sim_side_ms(rp_sim *sim, double *ms);

/* ---- One ringpop instance: Membership + Dissemination ------------------------
 * Replaces lib/membership.js:31-354 (Membership) and lib/dissemination.js:
 * 27-184 (Dissemination) for one ringpop process; js/index.js and
 * ringpop_amd/node.py wrap it with the reference's classes, methods and
 * events.  Address strings are interned to dense ids in first-seen order
 * (rp_node_intern; the local address is id 0).  Math.random, read by
 * getJoinPosition (lib/membership.js:99-101), shuffle and sample, is the
 * instance's splitmix64 stream, settable for replay.
 * A change is 48 bytes; incarnations are integers < 2^53.  */
typedef struct {
    int64_t address;            /* address id; -1: undefined (update() only) */
    int64_t incarnation;        /* -1: undefined */
    int64_t source;             /* address id; -1: undefined */
    int64_t source_incarnation; /* -1: undefined */
    int32_t status;             /* 1 alive, 2 suspect, 3 faulty, 4 leave */
    int32_t piggyback;          /* piggybackCount in rp_dissemination_changes (-1: undefined) */
    int64_t reserved;
} rp_member_change;
typedef struct rp_node rp_node;
int rp_node_create(const uint8_t *self_address, size_t len, uint64_t rng_state, rp_node **out);
int rp_node_destroy(rp_node *node);
/* ids[i] = id of address i (interning unknown ones) */
int rp_node_intern(rp_node *node, const uint8_t *bytes, const uint64_t *offsets, size_t n, uint32_t *ids);
int rp_node_address(rp_node *node, uint32_t id, char *buf, size_t cap, size_t *len);
/* read (get) and/or replace (set) the Math.random state */
int rp_node_rng(rp_node *node, uint64_t *get, const uint64_t *set);
/* Membership.update(changes) once ringpop is ready (lib/membership.js:208-313):
 * rules (lib/membership-update-rules.js:25-59), unknown members taken
 * wholesale and spliced at getJoinPosition(), the local suspect/faulty
 * override rewritten in place to {alive, now} (_.extend, :246-251).
 * applied[i] = 1 for every change on the returned list; when any applied the
 * checksum is recomputed (:266-268) and returned. */
int rp_membership_update(rp_node *node, rp_member_change *changes, uint32_t n, uint64_t now, uint8_t *applied,
                         uint32_t *napplied, uint32_t *checksum);
/* Membership.set() (:162-206) over the flattened stashed changesets:
 * mergeMembershipChangesets (lib/membership-changeset-merge.js:22-51), then
 * each update pushed at the end of members; winners[k] = index into `stash`
 * of the k-th update (the set listener's list). */
int rp_membership_set(rp_node *node, const rp_member_change *stash, uint32_t n, uint32_t *winners,
                      uint32_t *nwinners, uint32_t *checksum);
int rp_membership_checksum(rp_node *node, uint32_t *checksum);                       /* computeChecksum :41-64 */
int rp_membership_checksum_string(rp_node *node, char *buf, size_t cap, size_t *len); /* :70-93 */
/* members in order: ids / status / incarnation (any may be NULL) */
int rp_membership_members(rp_node *node, uint32_t *ids, uint8_t *status, uint64_t *inc, size_t cap,
                          uint32_t *count);
int rp_membership_shuffle(rp_node *node);                                         /* :315-317 */
/* replace the member order with a permutation of it (ids, count = the member
 * count): getStats() sorts `members` in place with localeCompare
 * (lib/membership.js:122-129), which the JS host computes and writes back */
int rp_membership_set_order(rp_node *node, const uint32_t *ids, uint32_t count);
int rp_membership_random(rp_node *node, uint32_t k, double *out);                 /* k Math.random() draws */
/* set a member's status / incarnation directly (what tests do to Member objects) */
int rp_membership_force(rp_node *node, uint32_t id, int status, uint64_t incarnation);
/* Dissemination.recordChange for a batch, in order (:125-127) */
int rp_dissemination_record(rp_node *node, const rp_member_change *changes, uint32_t n);
/* issueAsSender (:78-84): the list; cap must cover every recorded change */
int rp_dissemination_issue(rp_node *node, int32_t max_piggyback, rp_member_change *out, size_t cap, uint32_t *count);
/* issueAsReceiver (:86-119) with its fullSync fallback (*full_sync = 1);
 * sender -1 / sender_incarnation -1 = undefined, has_checksum 0 = undefined */
int rp_dissemination_issue_as_receiver(rp_node *node, int64_t sender, int64_t sender_incarnation,
                                       uint32_t sender_checksum, int has_checksum, int32_t max_piggyback,
                                       rp_member_change *out, size_t cap, uint32_t *count, int *full_sync);
int rp_dissemination_full_sync(rp_node *node, rp_member_change *out, size_t cap, uint32_t *count); /* :61-76 */
int rp_dissemination_clear(rp_node *node);                                                        /* :57-59 */
/* Dissemination.changes in key order, with piggybackCount */
int rp_dissemination_changes(rp_node *node, rp_member_change *out, size_t cap, uint32_t *count);

#ifdef __cplusplus
}
#endif
#endif
