// ringpop_amd — request traffic with proxy retries across rounds (rp_traffic_*;
// DESIGN.md §11): what the host side (rp_sim.hip) and the kernels that advance
// the device-resident request table (rp_traffic.hip) share, and the ring walk
// and bucket search that k_route (rp_sim.hip) and k_traffic_step both use.
// The traffic kernels are a translation unit of their own, so that the code
// object of the round kernels does not change with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rp_sim.h"

namespace rp {

// ---- shared with k_route
// What a route reads of one shard's rings.  In-process shards keep their
// nodes' rows in buffers of their own on one device: node v's are at row
// v % nl of shard v / nl.
struct RouteShard {
    const uint8_t* in_ring;     // nl x n
    const int32_t* coll_owner;  // nl x ncoll
    const int32_t* ring_count;  // n (global ids; the shard's own nodes)
    const uint32_t* ring_csum;  // n (the same)
};

struct RouteRing {
    const uint8_t* in_ring;
    const int32_t* coll_owner;
    // the owner of point p in this view, -1: none (k_view_lookup's rule)
    __device__ inline int32_t owner(int32_t coll, int32_t server) const {
        if (coll >= 0) return coll_owner[coll];
        return in_ring[server] ? server : -1;
    }
};
// HashRing.lookup from point p on (lib/ring.js:138-147), -1: an empty ring
__device__ inline int32_t route_walk(const RouteRing& r, const int32_t* pt_server, const int32_t* pt_coll,
                                     uint32_t npts, uint32_t p) {
    for (uint32_t k = 0; k < npts; k++) {
        const int32_t o = r.owner(pt_coll[p], pt_server[p]);
        if (o >= 0) return o;
        if (++p == npts) p = 0;
    }
    return -1;
}
// The point a key hash starts its walk at in every view: one binary search
// inside the key's directory bucket (the first point >= h, else point 0).
__device__ inline uint32_t route_point(const uint32_t* pt_hash, uint32_t npts, const uint32_t* dir, uint32_t dir_shift,
                                       uint32_t h) {
    const uint32_t b = (uint32_t)((uint64_t)h >> dir_shift);
    uint32_t lo = dir[b], hi = dir[b + 1];
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (pt_hash[m] < h) lo = m + 1; else hi = m; }
    return lo == npts ? 0 : lo;
}
// node v's ring: row v % nl of its shard's buffers
__device__ inline RouteRing route_ring_of(const SimDev& S, const RouteShard& t, uint32_t v) {
    const size_t r = v % S.nl;
    return RouteRing{t.in_ring + r * S.n, t.coll_owner + r * S.ncoll};
}

// ---- the request table

// rp_traffic_stats, then by_retries[outcome][0..8]
enum : uint32_t {
    TS_SUBMITTED = 0, TS_LOCAL = 1, TS_DELIVERED = 2, TS_REROUTED_LOCAL = 3, TS_FAILED = 4, TS_ENTRY_DEAD = 5,
    TS_PROXIED = 6, TS_SEND_UNREACHABLE = 7, TS_CHECKSUMS_DIFFER = 8, TS_RETRY_SCHEDULED = 9, TS_RETRY_ATTEMPTED = 10,
    TS_RETRY_REROUTED = 11, TS_RETRY_SUCCEEDED = 12, TS_RETRY_FAILED = 13, TS_MISROUTED = 14, TS_RESERVED = 15,
    TS_NSTATS = 16, TS_NREG = 15, TS_RETRY_SLOTS = 9, TS_NOUTCOMES = 5, TS_NSLOTS = TS_NSTATS + TS_NOUTCOMES * TS_RETRY_SLOTS
};
enum : uint32_t { TO_LOCAL = 0, TO_DELIVERED = 1, TO_REROUTED_LOCAL = 2, TO_FAILED = 3, TO_ENTRY_DEAD = 4, TO_PENDING = 255 };
// control words of a tracker (device): the pending count, the count the last
// compaction started from, where the last batch's survivors were appended,
// an overflow flag (a survivor that found no room: the host presizes the
// table, so it stays 0) and the largest pending count seen
enum : uint32_t { TC_COUNT = 0, TC_PREV = 1, TC_BASE = 2, TC_OVERFLOW = 3, TC_PEAK = 4, TC_NWORDS = 8 };
constexpr uint32_t TRAFFIC_TILE = 256;
constexpr uint32_t TRAFFIC_SCAN = 1024;
constexpr uint32_t TRAFFIC_MAX_SCHEDULE = 8;

// A pending record is two 16-byte words (rp_request_pending):
//   {id lo, id hi, entry, key_hash} {first_dest, due, submit_clock, retries}
// A final record is one (rp_request_result):
//   {dest, outcome | retries << 8, submit_clock, done_clock}
struct TrafficArgs {
    const RouteShard* tab;
    const uint32_t* pt_hash;
    const int32_t* pt_server;
    const int32_t* pt_coll;
    const uint32_t* dir;
    uint32_t npts, dir_shift;
    uint32_t max_retries, nschedule, enforce;
    uint32_t schedule[TRAFFIC_MAX_SCHEDULE];
    unsigned long long* cum;  // TS_NSLOTS cumulative counters
    unsigned long long* row;  // TS_NSTATS: the clock's history row
    uint4* results;           // by id, or null (not tracking)
    uint64_t results_cap;
    uint32_t* ctl;            // TC_*
    uint32_t* tile_count;     // survivors per tile of 256 records
    uint32_t* tile_off;       // their exclusive prefix sums
    uint32_t tiles_cap;
};

enum : int { TRAFFIC_PENDING = 0, TRAFFIC_BATCH = 1, TRAFFIC_UNIFORM = 2 };

// launches on `st` (rp_traffic.hip); mode: TRAFFIC_*
void traffic_step(int mode, unsigned grid, hipStream_t st, const SimDev& S, const TrafficArgs& A, uint4* recs, uint32_t cap,
                  const uint32_t* entries, const uint32_t* keys, uint64_t seed, uint64_t first_index, uint64_t first_id,
                  uint32_t count);
void traffic_scan(bool append, hipStream_t st, const TrafficArgs& A, uint32_t count, uint32_t cap_src, uint32_t cap_table);
void traffic_scatter(bool append, unsigned grid, hipStream_t st, const TrafficArgs& A, const uint4* src, uint4* dst,
                     uint32_t count, uint32_t cap_src, uint32_t cap_dst);

}  // namespace rp
