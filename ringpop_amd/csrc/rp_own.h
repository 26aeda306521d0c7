// ringpop_amd — what the ownership census (rp_own.hip) shares
// with the replica-set census (rp_repl.hip; §16): the kernels' argument block,
// the scan tiles' geometry, the wave helpers, and the launch of the two scan
// kernels, which the replica census reuses unchanged.  Each feature stays a
// translation unit of its own, so that neither changes the other's code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rp_cluster.h"

namespace rp {

constexpr uint32_t OWN_REPLICAS = (uint32_t)REPLICAS;
constexpr uint32_t OWN_BLOCK = 256;     // threads of a scan block ...
constexpr uint32_t OWN_ITEMS = 8;       // ... and consecutive intervals of each
constexpr uint32_t OWN_TILE = OWN_BLOCK * OWN_ITEMS;

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

__device__ inline unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

__device__ inline int32_t wave_scan_incl(int32_t x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    return x;
}

// claims(i) is the inclusive prefix sum of diff, in tiles of OWN_TILE: launches
// k_own_tile_sums (each tile's sum of A.diff into A.tile_sum) and
// k_own_tile_scan (the sums' exclusive prefix, in place) on st (rp_own.hip)
void own_scan_tiles(const OwnArgs& A, hipStream_t st);

// ---- what ownership movement (rp_own.hip; §15) shares with replica-set
// movement (rp_rmove.hip; §19), which runs the same merge on the arcs the
// replica census records

constexpr uint32_t OWN_ARC_ALL = 0x80000000u;  // a recorded arc count: the node claims every interval

// the comparison's device results: rp_movement_stats' transition[3][3] and
// measures, the per-node sums and counts, and three packed maxima
enum : uint32_t {
    MV_TRANS = 0, MV_SAME = 9, MV_HANDED = 10, MV_GAINED = 11, MV_LOST = 12, MV_GAINERS = 13, MV_LOSERS = 14,
    MV_MAXG = 15, MV_MAXL = 16, MV_MAXT = 17, MV_NOUT = 18
};
constexpr uint32_t MV_SEGS = OWN_REPLICAS + 1;  // a side's arcs as index segments: the wrapping arc is two
constexpr uint32_t MV_WAVES = OWN_BLOCK / 64;
constexpr uint32_t MV_NODE_MASK = 0x7FFFFFFFu;

struct MoveArgs {
    // side 0: from, side 1: to -- recorded arcs (k_own_arcs<true>, k_rep_arcs<true>) and claims
    const uint32_t* arc_n[2];
    const uint2* arcs[2];
    const uint32_t* claims[2];
    const uint32_t* pt_hash;
    uint32_t n, npts, ntiles;
    int32_t* diff;               // 2 x (npts + 1): the gains' difference array, then the losses'
    int32_t* tile_sum;           // 2 x ntiles
    unsigned long long* gained;  // n
    unsigned long long* lost;    // n
    unsigned long long* out;     // MV_NOUT (replica-set movement: RMV_NOUT)
};

// The comparison up to g(i) and l(i) as difference arrays with their tiles'
// exclusive prefixes: launches k_move_arcs (A.gained, A.lost, A.out[MV_GAINED
// .. MV_MAXL]), k_move_tile_sums and k_move_tile_scan on st (rp_own.hip).
// A.diff and A.out are zero before.  The finish pass is the caller's.
void move_scan(const MoveArgs& A, hipStream_t st);

// the id that names a simulation in its snapshots of either kind, given on first use
uint64_t snapshot_sim_id(rp_sim* c);

}  // namespace rp
