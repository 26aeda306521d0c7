// ringpop_amd — ownership census (rp_sim_ownership / rp_sim_ownership_at;
// DESIGN.md §13): for every interval between two ring points, how many live
// nodes claim it in their own view.  What the host side (rp_sim.hip) and the
// census kernels (rp_own.hip) share.  The kernels are a translation unit of
// their own, like the traffic kernels, so that the code object of the round
// kernels does not change with them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rp_traffic.h"

namespace rp {

// the census' device results: rp_ownership_stats' measure[8], the claimant
// count, and the largest claim count packed with its first interval
// (claims << 32 | ~index, so that an atomic max keeps the lowest index)
enum : uint32_t { OWN_MEASURE = 0, OWN_CLAIMANTS = 8, OWN_MAX = 9, OWN_NOUT = 10 };
constexpr uint32_t OWN_REPLICAS = (uint32_t)REPLICAS;
constexpr uint32_t OWN_BLOCK = 256;     // threads of a scan block ...
constexpr uint32_t OWN_ITEMS = 8;       // ... and consecutive intervals of each
constexpr uint32_t OWN_TILE = OWN_BLOCK * OWN_ITEMS;
constexpr uint32_t OWN_WALK_STEPS = 4;  // backward steps a lane takes alone before the wave searches for it

struct OwnArgs {
    const RouteShard* tab;            // node v's rows: row v % nl of shard v / nl
    const uint8_t* const* dead;       // per shard: n bytes by global id (valid for the shard's own nodes)
    const uint32_t* pt_hash;
    const int32_t* pt_server;
    const int32_t* pt_coll;
    const uint32_t* dir;
    const uint32_t* srv_pt;           // n x OWN_REPLICAS point indices, each row ascending
    uint32_t n, nl, ncoll, npts, dir_shift, ntiles;
    int32_t* diff;                    // npts + 1
    uint32_t* claims;                 // npts
    int32_t* tile_sum;                // ntiles: each tile's sum of diff, then its exclusive prefix
    unsigned long long* claimed;      // n
    unsigned long long* out;          // OWN_NOUT
};

// launches on `st` (rp_own.hip)
void own_point_index(hipStream_t st, const OwnArgs& A, const uint32_t* rep_hash, uint32_t* srv_pt);
void own_census(hipStream_t st, const OwnArgs& A);
void own_at(hipStream_t st, const OwnArgs& A, const uint32_t* keys, uint32_t nk, uint32_t* claims_out);

}  // namespace rp
