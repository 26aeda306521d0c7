// ringpop_amd — what multi-key requests at one instant (rp_routeall.hip;
// DESIGN.md §21) share with multi-key requests across rounds
// (rp_trafficall.hip; §23): the generator's draw, the lookups in a view and the
// in-wave group-by.  Each feature stays a translation unit of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rp_own.h"
#include "rp_traffic.h"

namespace rp {

constexpr uint32_t RA_MAX_K = 256;  // keys of a request, at the most

// the lanes of a request: the smallest W >= the batch's largest request, 64 beyond
inline uint32_t ra_lanes_for(uint32_t max_k) { return max_k <= 8 ? 8 : max_k <= 16 ? 16 : max_k <= 32 ? 32 : 64; }

// one wave's LDS traffic stays in order
__device__ inline void ra_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline uint64_t ra_draw(uint64_t seed, uint64_t at) {
    uint64_t s = seed + at * 0x9E3779B97F4A7C15ULL;
    return splitmix_next(s);
}

// HashRing.lookup from point p in node v's view, -1: an empty ring
__device__ inline int32_t ra_lookup(const OwnArgs& A, uint32_t v, int32_t ring_count, uint32_t p) {
    if (ring_count <= 0) return -1;
    const RouteShard& t = A.tab[v / A.nl];
    const size_t r = v % A.nl;
    return route_walk(RouteRing{t.in_ring + r * A.n, t.coll_owner + r * A.ncoll}, A.pt_server, A.pt_coll, A.npts, p);
}

// key h's point and its owner in e's view (an empty ring: e itself)
__device__ inline int32_t ra_entry_dest(const OwnArgs& A, uint32_t e, int32_t rce, uint32_t h, uint32_t& p0) {
    p0 = route_point(A.pt_hash, A.npts, A.dir, A.dir_shift, h);
    const int32_t d = ra_lookup(A, e, rce, p0);
    return d < 0 ? (int32_t)e : d;
}

// does d, in its own view, own the key whose walk starts at p0
__device__ inline bool ra_agrees(const OwnArgs& A, int32_t d, uint32_t p0) {
    return ra_lookup(A, (uint32_t)d, A.tab[(uint32_t)d / A.nl].ring_count[d], p0) == d;
}

// The group-by of every W-lane segment of the wave at once.  `has`: the lane
// holds a key, with owner d.  While any lane is unassigned, a segment's leader
// is its lowest unassigned lane (one ballot, sliced); its owner comes round by
// shuffle, and the ballot of "my owner is my leader's" is the new group's
// member mask.  Lowest lane first is first appearance: the ranks are
// _.groupBy's order.  Returns the segment's groups; rank: the lane's group;
// lane j of the segment receives group j's owner and member mask (gd, gm; a
// lane past the groups -1 and 0).  The loop runs max-groups-in-wave times.
template <uint32_t W>
__device__ inline uint32_t ra_group_by(bool has, int32_t d, uint32_t j, uint32_t sshift, uint32_t& rank, int32_t& gd,
                                       uint64_t& gm) {
    constexpr uint64_t SEG = ~0ull >> (64 - W);
    bool un = has;
    uint32_t ng = 0;
    rank = 0;
    gd = -1;
    gm = 0;
    for (;;) {
        const uint64_t u = __ballot(un);
        if (u == 0) break;
        const uint64_t us = (u >> sshift) & SEG;
        const bool lead = us != 0;
        const uint32_t L = lead ? (uint32_t)__ffsll((unsigned long long)us) - 1 : 0;
        const int32_t ld = __shfl(d, (int)(sshift + L));
        const bool mine = un && d == ld;  // (un: the segment has a leader)
        const uint64_t ms = (__ballot(mine) >> sshift) & SEG;
        if (mine) {
            rank = ng;
            un = false;
        }
        if (lead && j == ng) {  // (ng < the segment's keys <= W: the lane exists)
            gd = ld;
            gm = ms;
        }
        ng += lead ? 1u : 0u;
    }
    return ng;
}

}  // namespace rp
