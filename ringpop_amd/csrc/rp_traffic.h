// ringpop_amd — what the kernels that walk a view's ring between rounds share:
// k_route (rp_route.hip), the request tracker's k_traffic_step
// (rp_traffic.hip; §11) and the ownership census (rp_own.hip; §13).  The
// per-shard pointer table, the ring walk and the bucket search.  Each of those
// features is a translation unit of its own, kernels and host side together,
// so that the code object of the round kernels (rp_sim.hip) does not change
// with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rp_sim.h"

namespace rp {

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

}  // namespace rp
