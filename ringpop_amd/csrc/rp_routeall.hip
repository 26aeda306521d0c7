// ringpop_amd — multi-key requests (rp_sim_route_all / rp_sim_route_all_uniform;
// DESIGN.md §21): RingPop.handleOrProxyAll (index.js:636-694) across the
// simulated cluster at one instant, between rounds.  A request enters at node e
// with 0 .. 256 keys; e groups them by HashRing.lookup in its own view
// (_.groupBy: groups in order of first appearance), handles its own group and
// sends every other group to its owner, and every send is judged as
// rp_sim_route judges its one.  k_route_all puts a request's keys on lanes, W
// lanes a request, and does the group-by in the wave with ballots: no sort, no
// per-request memory.  Requests of more than 64 keys go through the wave in
// chunks of 64 with the request's groups in an LDS table.  The kernel is
// launched by no round; every store is a vector store or an integer atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "rp_routeall.h"

namespace rp {

constexpr uint32_t RA_BLOCK = 256;            // four waves
constexpr uint32_t RA_WAVES = RA_BLOCK / 64;
constexpr uint32_t RA_SLOTS = 2 * RA_MAX_K;   // the chunked path's table: half full at the most
constexpr uint32_t RA_EMPTY = 255;            // the outcome of a group slot past the request's groups
constexpr uint32_t RA_NO_GROUP = 0xFFFF;      // the group of a dead entry's key

// rp_route_all_stats as words: RA_NSUM sums, then the maximum
enum : uint32_t { RA_REQUESTS = 0, RA_ENTRY_DEAD, RA_NOKEYS, RA_KEYS, RA_GROUPS, RA_GROUP_OC = 5, RA_KEY_OC = 9,
                  RA_MISROUTED = 13, RA_SPLIT = 14, RA_WORST = 15, RA_FANOUT = 19, RA_NSUM = 29, RA_MAX_FANOUT = 29,
                  RA_NCOUNT = 30 };
enum : uint32_t { RA_OC_LOCAL = 0, RA_OC_DELIVERED = 1, RA_OC_DIFFER = 2, RA_OC_UNREACHABLE = 3, RA_OC_ENTRY_DEAD = 4 };

// the batch (CSR) and its result arrays; any result pointer may be null
struct RouteAllArgs {
    const uint32_t* entries;       // n
    const uint64_t* offsets;       // n + 1
    const uint32_t* keys;          // T = offsets[n]
    uint16_t* key_group;           // T
    uint8_t* key_agrees;           // T
    int32_t* group_dest;           // T: request i's group j at offsets[i] + j
    uint8_t* group_outcome;        // T
    uint16_t* group_keys;          // T
    uint16_t* group_agree;         // T
    uint16_t* fanout;              // n
    uint8_t* worst;                // n
    uint64_t seed;                 // UNIFORM: rp_sim_route_uniform's generator ...
    uint32_t uniform_k;            // ... and the keys of every request
};

// A request of more than 64 keys: its groups, in one wave's LDS.  An open-
// addressing table dest -> rank, and the groups' records by rank.
struct RaTable {
    int32_t dest[RA_SLOTS];    // -1: free
    uint16_t rank[RA_SLOTS];
    int32_t gdest[RA_MAX_K];
    uint16_t gkeys[RA_MAX_K];
    uint16_t gagree[RA_MAX_K];
    uint8_t goc[RA_MAX_K];
};

// the first rule of rp_sim_route's table that applies to a send from e to d
__device__ inline uint32_t ra_outcome(const SimDev& S, const OwnArgs& A, uint32_t e, uint32_t cse, uint32_t d) {
    if (d == e) return RA_OC_LOCAL;
    if (unreachable(S, e, d)) return RA_OC_UNREACHABLE;
    return A.tab[d / A.nl].ring_csum[d] != cse ? RA_OC_DIFFER : RA_OC_DELIVERED;
}

// the largest outcome among the segment's group lanes (0 where it has none)
template <uint32_t W>
__device__ inline uint32_t ra_worst(uint32_t goc, uint32_t sshift) {
    constexpr uint64_t SEG = ~0ull >> (64 - W);
    const bool s3 = ((__ballot(goc == RA_OC_UNREACHABLE) >> sshift) & SEG) != 0;
    const bool s2 = ((__ballot(goc == RA_OC_DIFFER) >> sshift) & SEG) != 0;
    const bool s1 = ((__ballot(goc == RA_OC_DELIVERED) >> sshift) & SEG) != 0;
    return s3 ? 3u : (s2 ? 2u : (s1 ? 1u : 0u));
}

// a lane's counters for its request (leader lanes) ...
__device__ inline void ra_count_request(uint32_t* cnt, uint32_t& maxf, bool leader, bool live, uint32_t K, uint32_t ng,
                                        uint32_t worst) {
    cnt[RA_REQUESTS] += leader ? 1u : 0u;
    cnt[RA_ENTRY_DEAD] += leader && !live ? 1u : 0u;
    cnt[RA_NOKEYS] += leader && live && K == 0 ? 1u : 0u;
    const uint32_t fb = ng ? 32u - (uint32_t)__clz((int)ng) : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) cnt[RA_WORST + k] += leader && live && worst == k ? 1u : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 10; k++) cnt[RA_FANOUT + k] += leader && live && fb == k ? 1u : 0u;
    maxf = leader && ng > maxf ? ng : maxf;
}
// ... its key (koc: its group's outcome) ...
__device__ inline void ra_count_key(uint32_t* cnt, bool has, uint32_t koc, bool ag) {
    cnt[RA_KEYS] += has ? 1u : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) cnt[RA_KEY_OC + k] += has && koc == k ? 1u : 0u;
    cnt[RA_MISROUTED] += has && (koc == RA_OC_DELIVERED || koc == RA_OC_DIFFER) && !ag ? 1u : 0u;
}
// ... and its group
__device__ inline void ra_count_group(uint32_t* cnt, bool isg, uint32_t goc, uint32_t gk, uint32_t ga) {
    cnt[RA_GROUPS] += isg ? 1u : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) cnt[RA_GROUP_OC + k] += isg && goc == k ? 1u : 0u;
    cnt[RA_SPLIT] += isg && (goc == RA_OC_DELIVERED || goc == RA_OC_DIFFER) && ga > 0 && ga < gk ? 1u : 0u;
}

__device__ inline void ra_store_key(const RouteAllArgs& B, uint64_t at, uint32_t group, bool ag) {
    if (B.key_group) B.key_group[at] = (uint16_t)group;
    if (B.key_agrees) B.key_agrees[at] = ag ? 1 : 0;
}
__device__ inline void ra_store_group(const RouteAllArgs& B, uint64_t at, bool isg, int32_t gd, uint32_t goc, uint32_t gk,
                                      uint32_t ga) {
    if (B.group_dest) B.group_dest[at] = isg ? gd : -1;
    if (B.group_outcome) B.group_outcome[at] = (uint8_t)(isg ? goc : RA_EMPTY);
    if (B.group_keys) B.group_keys[at] = (uint16_t)(isg ? gk : 0u);
    if (B.group_agree) B.group_agree[at] = (uint16_t)(isg ? ga : 0u);
}

// What a segment's lanes know of their request (the leader loaded it).
struct RaRequest {
    uint64_t i, off;  // the request, its first key
    uint32_t e, K, cse;
    int32_t rce;      // e's ring_count
    bool active, live;
};

// A request of at most W keys on the W lanes of a segment: lane j holds key j,
// then group j.
//  1 every key lane: route_point and the walk in e's row (the segment shares
//    the row);
//  2 ra_group_by;
//  3 group lanes: dead[d], the cut and d's ring checksum, one group per lane,
//    all loads in flight together; the outcome goes back to the members by
//    shuffle;
//  4 key lanes of a group with outcome 1 or 2: the walk in d's row from the
//    same point; group_agree is the popcount of the agreeing lanes under the
//    member mask;
//  5 lane j stores key j's and group j's slots at off + j: consecutive lanes,
//    consecutive addresses.
template <uint32_t W, bool UNIFORM>
__device__ inline void ra_segment(const SimDev& S, const OwnArgs& A, const RouteAllArgs& B, const RaRequest& q, uint32_t j,
                                  uint32_t sshift, uint32_t* cnt, uint32_t& maxf) {
    constexpr uint64_t SEG = ~0ull >> (64 - W);
    const bool slot = q.active && j < q.K, has = slot && q.live;
    uint32_t h = 0, p0 = 0;
    if (UNIFORM) h = (uint32_t)ra_draw(B.seed, q.off + j);
    else if (has) h = B.keys[q.off + j];
    int32_t d = (int32_t)q.e;
    if (has) d = ra_entry_dest(A, q.e, q.rce, h, p0);
    uint32_t rank;
    int32_t gd;
    uint64_t gm;
    const uint32_t ng = ra_group_by<W>(has, d, j, sshift, rank, gd, gm);
    const bool isg = j < ng;
    const uint32_t goc = isg ? ra_outcome(S, A, q.e, q.cse, (uint32_t)gd) : RA_EMPTY;
    const uint32_t koc = (uint32_t)__shfl((int)goc, (int)(sshift + (has ? rank : 0u)));
    const bool ag = has && (koc == RA_OC_DELIVERED || koc == RA_OC_DIFFER) && ra_agrees(A, d, p0);
    const uint64_t am = (__ballot(ag) >> sshift) & SEG;
    const uint32_t gk = (uint32_t)__popcll(gm), ga = (uint32_t)__popcll(am & gm);
    const uint32_t worst = q.live ? ra_worst<W>(goc, sshift) : RA_OC_ENTRY_DEAD;
    if (slot) {
        ra_store_key(B, q.off + j, has ? rank : RA_NO_GROUP, ag);
        ra_store_group(B, q.off + j, isg, gd, goc, gk, ga);
    }
    const bool leader = q.active && j == 0;
    if (leader && B.fanout) B.fanout[q.i] = (uint16_t)ng;
    if (leader && B.worst) B.worst[q.i] = (uint8_t)worst;
    ra_count_key(cnt, has, koc, ag);
    ra_count_group(cnt, isg, goc, gk, ga);
    ra_count_request(cnt, maxf, leader, q.live, q.K, ng, worst);
}

// A request of 65 .. 256 keys on a whole wave, 64 keys a chunk, in order.  A
// chunk is grouped as a segment is; its groups, one per lane, then probe the
// table: a destination an earlier chunk met keeps its rank, new ones take the
// next ranks in lane order (first appearance).  A group's outcome is evaluated
// once, when it is created; its key and agree counts accumulate in the table.
// After the last chunk the lanes write the groups out by rank.
template <bool UNIFORM>
__device__ inline void ra_chunked(const SimDev& S, const OwnArgs& A, const RouteAllArgs& B, const RaRequest& q, RaTable& T,
                                  uint32_t lane, uint32_t* cnt, uint32_t& maxf) {
    for (uint32_t s = lane; s < RA_SLOTS; s += 64) T.dest[s] = -1;
    ra_fence();
    uint32_t ng = 0;
    for (uint32_t c0 = 0; c0 < q.K; c0 += 64) {
        const uint32_t k = c0 + lane;
        const bool slot = k < q.K, has = slot && q.live;
        uint32_t h = 0, p0 = 0;
        if (UNIFORM) h = (uint32_t)ra_draw(B.seed, q.off + k);
        else if (has) h = B.keys[q.off + k];
        int32_t d = (int32_t)q.e;
        if (has) d = ra_entry_dest(A, q.e, q.rce, h, p0);
        uint32_t lr;
        int32_t gd;
        uint64_t gm;
        const uint32_t nc = ra_group_by<64>(has, d, lane, 0, lr, gd, gm);
        const bool isg = lane < nc;
        uint32_t at = 0;
        bool fresh = false;
        if (isg) {
            // (the chunk's groups have distinct owners; at most RA_MAX_K of the RA_SLOTS are ever taken)
            at = ((uint32_t)gd * 0x9E3779B1u) >> 23;
            for (;;) {
                const int32_t old = atomicCAS(&T.dest[at], -1, gd);
                fresh = old == -1;
                if (fresh || old == gd) break;
                at = (at + 1) & (RA_SLOTS - 1);
            }
        }
        const uint64_t fm = __ballot(fresh);
        uint32_t r = 0, goc = RA_EMPTY;
        if (fresh) {
            r = ng + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));  // (r < the keys seen so far <= RA_MAX_K)
            goc = ra_outcome(S, A, q.e, q.cse, (uint32_t)gd);
            T.rank[at] = (uint16_t)r;
            T.gdest[r] = gd;
            T.goc[r] = (uint8_t)goc;
        } else if (isg) {
            r = T.rank[at];
            goc = T.goc[r];
        }
        ng += (uint32_t)__popcll(fm);
        const uint32_t koc = (uint32_t)__shfl((int)goc, (int)(has ? lr : 0u));
        const uint32_t kr = (uint32_t)__shfl((int)r, (int)(has ? lr : 0u));
        const bool ag = has && (koc == RA_OC_DELIVERED || koc == RA_OC_DIFFER) && ra_agrees(A, d, p0);
        const uint64_t am = __ballot(ag);
        if (isg) {
            const uint32_t gk = (uint32_t)__popcll(gm), ga = (uint32_t)__popcll(am & gm);
            T.gkeys[r] = (uint16_t)((fresh ? 0u : T.gkeys[r]) + gk);
            T.gagree[r] = (uint16_t)((fresh ? 0u : T.gagree[r]) + ga);
        }
        ra_fence();
        if (slot) ra_store_key(B, q.off + k, has ? kr : RA_NO_GROUP, ag);
        ra_count_key(cnt, has, koc, ag);
    }
    uint32_t wmax = 0;
    for (uint32_t r = lane; r < q.K; r += 64) {
        const bool isg = r < ng;
        const int32_t gd = isg ? T.gdest[r] : -1;
        const uint32_t goc = isg ? T.goc[r] : RA_EMPTY, gk = isg ? T.gkeys[r] : 0u, ga = isg ? T.gagree[r] : 0u;
        ra_store_group(B, q.off + r, isg, gd, goc, gk, ga);
        ra_count_group(cnt, isg, goc, gk, ga);
        wmax = isg && goc > wmax ? goc : wmax;
    }
    ra_fence();  // (the next request clears the table)
    const uint32_t worst = q.live ? ra_worst<64>(wmax ? wmax : RA_EMPTY, 0) : RA_OC_ENTRY_DEAD;
    const bool leader = lane == 0;
    if (leader && B.fanout) B.fanout[q.i] = (uint16_t)ng;
    if (leader && B.worst) B.worst[q.i] = (uint8_t)worst;
    ra_count_request(cnt, maxf, leader, q.live, q.K, ng, worst);
}

// Requests [first, first + count) of the batch (UNIFORM: request i has
// B.uniform_k keys, the draws i * K .. i * K + K - 1 of rp_sim_route_uniform's
// generator; its entry is the first draw's).  W lanes a request, 64 / W
// requests a wave, 256 / W a block and pass (grid-stride).  A segment's leader
// loads the request, dead[e], e's ring_count and ring checksum; they come round
// by shuffle.  W < 64: every request has at most W keys (the host has the
// offsets).  W == 64: a request of more than 64 keys takes the chunked path.
// Counters live in registers, are summed per block in LDS and flushed with one
// atomic per counter and block (k_route's scheme).
template <uint32_t W, bool UNIFORM>
__global__ void __launch_bounds__(RA_BLOCK) k_route_all(SimDev S, OwnArgs A, RouteAllArgs B, uint64_t first, uint64_t count,
                                                        unsigned long long* stats) {
    constexpr uint32_t PER_BLOCK = RA_BLOCK / W;
    __shared__ unsigned long long bc[RA_NCOUNT];
    if (threadIdx.x < RA_NCOUNT) bc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, j = lane & (W - 1), sshift = lane & ~(W - 1);
    uint32_t cnt[RA_NSUM], maxf = 0;
#pragma unroll
    for (uint32_t k = 0; k < RA_NSUM; k++) cnt[k] = 0;
    // (the bound is the block's: every wave goes round together)
    for (uint64_t b0 = (uint64_t)blockIdx.x * PER_BLOCK; b0 < count; b0 += (uint64_t)gridDim.x * PER_BLOCK) {
        const uint64_t at = b0 + threadIdx.x / W;
        RaRequest q;
        q.active = at < count;
        q.i = first + at;
        uint32_t e = 0, K = 0, cse = 0, dead = 1;
        int32_t rce = 0;
        uint64_t off = 0;
        if (q.active && j == 0) {
            if (UNIFORM) {
                K = B.uniform_k;
                off = q.i * K;
                e = (uint32_t)(((ra_draw(B.seed, off) >> 32) * S.n) >> 32);
            } else {
                e = B.entries[q.i];
                off = B.offsets[q.i];
                K = (uint32_t)(B.offsets[q.i + 1] - off);
            }
            dead = S.dead[e];
            const RouteShard& te = A.tab[e / A.nl];
            rce = te.ring_count[e];
            cse = te.ring_csum[e];
        }
        q.e = (uint32_t)__shfl((int)e, 0, (int)W);
        q.K = (uint32_t)__shfl((int)K, 0, (int)W);
        q.cse = (uint32_t)__shfl((int)cse, 0, (int)W);
        q.rce = __shfl(rce, 0, (int)W);
        q.live = q.active && __shfl((int)dead, 0, (int)W) == 0;
        q.off = (uint64_t)__shfl((unsigned long long)off, 0, (int)W);
        if constexpr (W == 64) {
            __shared__ RaTable tabs[RA_WAVES];
            if (q.K > 64)  // (the wave's one request)
                ra_chunked<UNIFORM>(S, A, B, q, tabs[threadIdx.x >> 6], lane, cnt, maxf);
            else
                ra_segment<W, UNIFORM>(S, A, B, q, j, sshift, cnt, maxf);
        } else {
            ra_segment<W, UNIFORM>(S, A, B, q, j, sshift, cnt, maxf);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < RA_NSUM; k++)
        if (cnt[k]) atomicAdd(&bc[k], (unsigned long long)cnt[k]);
    if (maxf) atomicMax(&bc[RA_MAX_FANOUT], (unsigned long long)maxf);
    __syncthreads();
    if (threadIdx.x < RA_NSUM && bc[threadIdx.x]) atomicAdd(&stats[threadIdx.x], bc[threadIdx.x]);
    if (threadIdx.x == RA_MAX_FANOUT && bc[threadIdx.x]) atomicMax(&stats[threadIdx.x], bc[threadIdx.x]);
}

}  // namespace rp

// =====================================================================
// Host side (on the first shard's stream, like rp_sim_route).
// =====================================================================
using rp::DevBuf;
using rp::Error;
using rp::Shard;

namespace {

constexpr uint64_t RA_LAUNCH_KEYS = 1ull << 31;  // keys of a launch, at the most: a lane's counters are 32-bit
constexpr unsigned RA_BLOCKS = 2048;             // blocks of a launch, at the most (k_route_n's grid)

template <uint32_t W, bool UNIFORM>
void launch_w(Shard& s0, const rp::SimDev& S, const rp::OwnArgs& A, const rp::RouteAllArgs& B, uint64_t first, uint64_t m,
              unsigned long long* dst) {
    s0.timed(5, [&] {
        hipLaunchKernelGGL((rp::k_route_all<W, UNIFORM>), dim3(std::min(rp::grid_for(m, rp::RA_BLOCK / W), RA_BLOCKS)),
                           dim3(rp::RA_BLOCK), 0, s0.st, S, A, B, first, m, dst);
    });
    RP_HIP(hipGetLastError());
}

// Requests [0, n) in launches of at most 2^31 keys; host_offsets: the CSR
// offsets (null: UNIFORM, B.uniform_k keys a request).  B's arrays are the
// whole batch's, on the device.
template <bool UNIFORM>
void route_all_launch(rp_sim* c, const rp::RouteAllArgs& B, const uint64_t* host_offsets, uint64_t n, uint32_t max_k,
                      rp_route_all_stats* stats) {
    static_assert(sizeof(rp_route_all_stats) == 256, "rp_route_all_stats is 32 x u64");
    static_assert(offsetof(rp_route_all_stats, group_outcome) == 8 * rp::RA_GROUP_OC &&
                      offsetof(rp_route_all_stats, key_outcome) == 8 * rp::RA_KEY_OC &&
                      offsetof(rp_route_all_stats, misrouted_keys) == 8 * rp::RA_MISROUTED &&
                      offsetof(rp_route_all_stats, worst_hist) == 8 * rp::RA_WORST &&
                      offsetof(rp_route_all_stats, fanout_hist) == 8 * rp::RA_FANOUT &&
                      offsetof(rp_route_all_stats, max_fanout) == 8 * rp::RA_MAX_FANOUT &&
                      offsetof(rp_route_all_stats, reserved) == 8 * rp::RA_NCOUNT,
                  "the device counters are the struct's first fields, in order");
    Shard& s0 = *c->sh.front();
    rp::SimDev S = s0.d;
    S.round = c->round;  // the clock of the next round, as rp_sim_route
    S.part_start = c->part[0]; S.part_end = c->part[1]; S.part_split = c->part[2];
    const rp::OwnArgs A = c->own_args();  // (the routing tables and the points: no census buffer is read)
    DevBuf<unsigned long long> dst(rp::RA_NCOUNT);
    RP_HIP(hipMemsetAsync(dst.p, 0, dst.bytes(), s0.st));
    const uint32_t W = rp::ra_lanes_for(max_k);
    for (uint64_t first = 0; first < n;) {
        uint64_t m;
        if (UNIFORM) {
            m = std::min<uint64_t>(n - first, RA_LAUNCH_KEYS / B.uniform_k);
        } else {  // the requests whose keys end within 2^31 of this launch's first key (at least one: K <= 256)
            const uint64_t* end = std::upper_bound(host_offsets + first + 1, host_offsets + n + 1,
                                                   host_offsets[first] + RA_LAUNCH_KEYS);
            m = (uint64_t)(end - (host_offsets + first + 1));
        }
        switch (W) {
            case 8: launch_w<8, UNIFORM>(s0, S, A, B, first, m, dst.p); break;
            case 16: launch_w<16, UNIFORM>(s0, S, A, B, first, m, dst.p); break;
            case 32: launch_w<32, UNIFORM>(s0, S, A, B, first, m, dst.p); break;
            default: launch_w<64, UNIFORM>(s0, S, A, B, first, m, dst.p); break;
        }
        first += m;
    }
    unsigned long long h[rp::RA_NCOUNT];
    RP_HIP(hipMemcpyAsync(h, dst.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
    RP_HIP(hipStreamSynchronize(s0.st));
    if (stats) memcpy(stats, h, sizeof h);  // (the reserved words stay 0)
}

template <class T>
void fetch(T* host, const DevBuf<T>& dev, size_t count, hipStream_t st) {
    if (host && count) RP_HIP(hipMemcpyAsync(host, dev.p, count * sizeof(T), hipMemcpyDeviceToHost, st));
}

}  // namespace

extern "C" {

int rp_sim_route_all(rp_sim* c, const uint32_t* entries, const uint64_t* offsets, const uint32_t* key_hashes, size_t n,
                     uint16_t* key_group, uint8_t* key_agrees, int32_t* group_dest, uint8_t* group_outcome,
                     uint16_t* group_keys, uint16_t* group_agree, uint16_t* fanout, uint8_t* worst,
                     rp_route_all_stats* stats) {
    return rp::guarded([&] {
        if (!c || (n && (!entries || !offsets))) throw Error(RP_ERR_INVALID, "null pointer");
        uint32_t max_k = 0;
        if (n && offsets[0] != 0) throw Error(RP_ERR_INVALID, "offsets[0] must be 0");
        for (size_t i = 0; i < n; i++) {
            const std::string at = "request " + std::to_string(i);
            if (entries[i] >= c->n) throw Error(RP_ERR_INVALID, at + ": entry node out of range");
            if (offsets[i + 1] < offsets[i]) throw Error(RP_ERR_INVALID, at + ": offsets decrease");
            if (offsets[i + 1] - offsets[i] > rp::RA_MAX_K) throw Error(RP_ERR_INVALID, at + ": more than 256 keys");
            max_k = std::max(max_k, (uint32_t)(offsets[i + 1] - offsets[i]));
        }
        const size_t T = n ? (size_t)offsets[n] : 0;
        if (T && !key_hashes) throw Error(RP_ERR_INVALID, "null pointer");
        c->route_prepare(true);
        if (stats) memset(stats, 0, sizeof *stats);
        if (n == 0) return;
        Shard& s0 = *c->sh.front();
        DevBuf<uint32_t> de(n), dh(T);
        DevBuf<uint64_t> doff(n + 1);
        DevBuf<uint16_t> dkg(key_group ? T : 0), dgk(group_keys ? T : 0), dga(group_agree ? T : 0), dfan(fanout ? n : 0);
        DevBuf<uint8_t> dka(key_agrees ? T : 0), dgo(group_outcome ? T : 0), dworst(worst ? n : 0);
        DevBuf<int32_t> dgd(group_dest ? T : 0);
        RP_HIP(hipMemcpyAsync(de.p, entries, n * 4, hipMemcpyHostToDevice, s0.st));
        RP_HIP(hipMemcpyAsync(doff.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s0.st));
        if (T) RP_HIP(hipMemcpyAsync(dh.p, key_hashes, T * 4, hipMemcpyHostToDevice, s0.st));
        const rp::RouteAllArgs B{de.p, doff.p, dh.p, dkg.p, dka.p, dgd.p, dgo.p, dgk.p, dga.p, dfan.p, dworst.p, 0, 0};
        route_all_launch<false>(c, B, offsets, n, max_k, stats);  // (the stream is drained)
        fetch(key_group, dkg, T, s0.st);
        fetch(key_agrees, dka, T, s0.st);
        fetch(group_dest, dgd, T, s0.st);
        fetch(group_outcome, dgo, T, s0.st);
        fetch(group_keys, dgk, T, s0.st);
        fetch(group_agree, dga, T, s0.st);
        fetch(fanout, dfan, n, s0.st);
        fetch(worst, dworst, n, s0.st);
        RP_HIP(hipStreamSynchronize(s0.st));
    });
}

int rp_sim_route_all_uniform(rp_sim* c, uint64_t seed, uint64_t count, uint32_t keys_per_request,
                             rp_route_all_stats* stats) {
    return rp::guarded([&] {
        if (!c) throw Error(RP_ERR_INVALID, "null pointer");
        if (keys_per_request < 1 || keys_per_request > rp::RA_MAX_K)
            throw Error(RP_ERR_INVALID, "keys_per_request must be 1..256");
        c->route_prepare(true);
        if (stats) memset(stats, 0, sizeof *stats);
        if (count == 0) return;
        rp::RouteAllArgs B{};
        B.seed = seed;
        B.uniform_k = keys_per_request;
        route_all_launch<true>(c, B, nullptr, count, keys_per_request, stats);
    });
}

}  // extern "C"
