// ringpop_amd — replicated requests (rp_sim_route_n / rp_sim_route_n_uniform;
// DESIGN.md §18): a request for key h enters at node e, e sends it to the
// owners of RingPop.lookupN(h, R) in its own view, and every send is judged as
// rp_sim_route judges its one (LOCAL, UNREACHABLE, CHECKSUMS_DIFFER,
// DELIVERED) and by §17's holder rule in the destination's own view.  One
// instant, between rounds, like rp_sim_route; the kernel is launched by no
// round.  A request's R + 1 walks (the entry's, then one per destination) all
// run over the same global points from the key's point on: k_route_n gives a
// request eight lanes, fetches a window of sixteen points once, decides the
// entry's preference list across the lanes with one ballot and then runs the
// destinations' walks side by side, one per lane.  Every store is a vector
// store or an integer atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "rp_repl.h"

namespace rp {

constexpr uint32_t RN_BLOCK = 256;                    // four waves ...
constexpr uint32_t RN_GROUP = 8;                      // ... of eight requests, eight lanes each (lane j: slot j)
constexpr uint32_t RN_PER_BLOCK = RN_BLOCK / RN_GROUP;
constexpr uint32_t RN_WINDOW = 2 * RN_GROUP;          // points a group fetches: two per lane
constexpr uint32_t RN_SPAN = REP_MAX_R + REP_SOLO_EXTRA;  // points a destination's lane examines alone, at the most
constexpr uint32_t RN_EMPTY = 255;                    // the outcome of a slot past the list's end
constexpr uint32_t RN_COLL = 0x80000000u;             // a window word: a collision point's group, else its server
static_assert(REP_MAX_R == RN_GROUP, "a lane per slot");
static_assert(RN_SPAN <= RN_WINDOW, "a destination's own steps stay inside the window");

// rp_route_n_stats as words: the device counters are the struct's first RN_NCOUNT fields
enum : uint32_t { RN_REQUESTS = 0, RN_ENTRY_DEAD, RN_SLOTS, RN_LOCAL, RN_DELIVERED, RN_DIFFER, RN_UNREACHABLE, RN_MISPLACED,
                  RN_SHORT, RN_ACKS = 9, RN_STRICT = 18, RN_NCOUNT = 27 };
enum : uint32_t { RN_OC_LOCAL = 0, RN_OC_DELIVERED = 1, RN_OC_DIFFER = 2, RN_OC_UNREACHABLE = 3, RN_OC_ENTRY_DEAD = 4 };

__device__ inline int32_t rn_owner(const RouteRing& ring, uint32_t w) {
    return (w & RN_COLL) ? ring.owner((int32_t)(w & ~RN_COLL), 0) : ring.owner(-1, (int32_t)w);
}

// One point of a destination's walk (k_hold_mask's rule): its view owns the
// point (it holds the key), the point's owner is the R-th distinct other one
// (it does not), or the walk goes on.
__device__ inline void rn_take(OwnerSet<REP_MAX_R - 1>& u, int32_t o, int32_t self, uint32_t R, bool& done, bool& held) {
    if (done || o < 0 || (o != self && u.has(o))) return;
    if (walk_take(u, o, self, R)) {
        done = true;
        held = o == self;
    }
}

// a lane's byte of a ballot's slice for its group of eight
__device__ inline uint32_t rn_slice(bool p, uint32_t gshift) {
    return (uint32_t)(__ballot(p) >> gshift) & 0xFFu;
}

// Requests [0, count) of a launch: request i is (entries[i], keys[i]) or,
// UNIFORM, rp_sim_route_uniform's draw at index first + i.  A block takes 32
// requests a pass (grid-stride), lanes 8g .. 8g + 7 of a wave one of them.
//
//  1 the window: lane j reads points p0 + j and p0 + 8 + j (pt_coll,
//    pt_server; p0 the key's point) and their owners in the entry's view --
//    two independent loads a lane where a lane alone would chain R + 3.
//  2 the entry's list: a window point is a first appearance iff it is present
//    and no earlier window point has its owner (fifteen 8-wide shuffles of the
//    owners); the group's two bytes of the ballots are the first-appearance
//    mask, slot j's destination the owner at its j-th set bit, cut at
//    min(R, the ring's servers).  A list still short after sixteen points of
//    a longer ring is a sparse view: the wave finishes it with walk_wave from
//    the window's end for the group's leader, the kept owners in OwnerSet<8>.
//    An empty list (an empty ring, or servers that own no point) is [e].
//  3 the destinations: lane j < c judges d = L[j].  LOCAL and UNREACHABLE need
//    no walk.  Otherwise the lane walks d's view from p0 with stop owner d and
//    target R: the window's first R + 3 points come round the group by
//    shuffle, the first R owner loads, both ring checksums, d's ring_count and
//    in_ring[d] are issued together, the REP_SOLO_EXTRA further owners only
//    while some lane of the wave is undecided, and walk_wave ends what is left.
//  4 lane j stores slot j of the three rows (consecutive lanes, consecutive
//    addresses); acks and strict are popcounts of the group's ballot byte.
// Counters are kept per lane in registers by selects, summed per block in LDS
// and flushed with one atomic per counter and block (k_route's scheme).
template <bool UNIFORM>
__global__ void __launch_bounds__(RN_BLOCK) k_route_n(SimDev S, OwnArgs A, uint32_t R, const uint32_t* __restrict__ entries,
                                                      const uint32_t* __restrict__ keys, uint64_t seed, uint64_t first,
                                                      uint64_t count, int32_t* __restrict__ dests,
                                                      uint8_t* __restrict__ outcomes, uint8_t* __restrict__ holds,
                                                      uint8_t* __restrict__ acks, unsigned long long* stats) {
    __shared__ unsigned long long bc[RN_NCOUNT];
    if (threadIdx.x < RN_NCOUNT) bc[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, j = lane & (RN_GROUP - 1), gshift = lane & ~(RN_GROUP - 1);
    const uint32_t npts = A.npts;
    const uint32_t W = npts < RN_WINDOW ? npts : RN_WINDOW;
    const uint32_t span = R + REP_SOLO_EXTRA < npts ? R + REP_SOLO_EXTRA : npts;
    const uint32_t lead = R < span ? R : span;
    uint32_t cnt[RN_NCOUNT];
#pragma unroll
    for (uint32_t k = 0; k < RN_NCOUNT; k++) cnt[k] = 0;
    // (the bound is the block's: every wave goes round together)
    for (uint64_t b0 = (uint64_t)blockIdx.x * RN_PER_BLOCK; b0 < count; b0 += (uint64_t)gridDim.x * RN_PER_BLOCK) {
        const uint64_t i = b0 + threadIdx.x / RN_GROUP;
        const bool active = i < count;
        uint32_t e = 0, h = 0;
        if (UNIFORM) {
            uint64_t s = seed + (first + i) * 0x9E3779B97F4A7C15ULL;
            const uint64_t r = splitmix_next(s);
            e = (uint32_t)(((r >> 32) * S.n) >> 32);
            h = (uint32_t)r;
        } else if (active) {
            e = entries[i];
            h = keys[i];
        }
        const bool live = active && S.dead[e] == 0;
        const RouteShard& te = A.tab[e / A.nl];
        const size_t er = e % A.nl;
        const RouteRing ring_e{te.in_ring + er * A.n, te.coll_owner + er * A.ncoll};
        const int32_t rce = live ? te.ring_count[e] : 0;
        const uint32_t target = rce <= 0 ? 0u : ((uint32_t)rce < R ? (uint32_t)rce : R);

        // 1: the window, and its owners in the entry's view
        const uint32_t p0 = route_point(A.pt_hash, npts, A.dir, A.dir_shift, h);
        uint32_t pk[2];
        int32_t oe[2];
#pragma unroll
        for (uint32_t s = 0; s < 2; s++) {
            const uint32_t k = j + s * RN_GROUP;
            pk[s] = 0;
            oe[s] = -1;
            if (k < W) {
                const uint32_t idx = walk_move<false>(p0, k, npts);  // (k < W <= npts)
                const int32_t pc = A.pt_coll[idx], ps = A.pt_server[idx];
                pk[s] = pc >= 0 ? RN_COLL | (uint32_t)pc : (uint32_t)ps;
                if (target) oe[s] = ring_e.owner(pc, ps);
            }
        }

        // 2: first appearances, in window order (positions j and 8 + j)
        bool f0 = oe[0] >= 0, f1 = oe[1] >= 0;
#pragma unroll
        for (uint32_t t = 0; t < RN_GROUP; t++) {
            const int32_t x = __shfl(oe[0], (int)t, (int)RN_GROUP), y = __shfl(oe[1], (int)t, (int)RN_GROUP);
            f0 = f0 && !(t < j && x == oe[0]);
            f1 = f1 && x != oe[1] && !(t < j && y == oe[1]);
        }
        const uint32_t m = rn_slice(f0, gshift) | rn_slice(f1, gshift) << RN_GROUP;
        uint32_t c = (uint32_t)__popc(m);
        c = c < target ? c : target;
        uint32_t mm = m;  // (its j lowest bits cleared: the j-th set bit is the lowest left)
#pragma unroll
        for (uint32_t t = 0; t + 1 < RN_GROUP; t++) mm = t < j ? mm & (mm - 1) : mm;
        const uint32_t kj = mm ? (uint32_t)__ffs(mm) - 1 : 0;
        const int32_t a0 = __shfl(oe[0], (int)(kj & (RN_GROUP - 1)), (int)RN_GROUP);
        const int32_t a1 = __shfl(oe[1], (int)(kj & (RN_GROUP - 1)), (int)RN_GROUP);
        int32_t d = j < c ? (kj < RN_GROUP ? a0 : a1) : -1;

        // sparse views: the wave walks on for one group's leader at a time
        const bool sparse = c < target && W < npts;  // (the group's; W == 16 here)
        unsigned long long pe = __ballot(sparse && j == 0);
        if (pe != 0) {
            OwnerSet<REP_MAX_R> ue;
#pragma unroll
            for (uint32_t t = 0; t < REP_MAX_R; t++) {
                const int32_t x = __shfl(d, (int)t, (int)RN_GROUP);
                ue.s[t] = t < c ? x : -2;
            }
            ue.cnt = c;
            while (pe != 0) {
                const int L = __ffsll(pe) - 1;
                pe &= pe - 1;
                const uint32_t el = (uint32_t)__builtin_amdgcn_readlane((int)e, L);
                const RouteShard& tl = A.tab[el / A.nl];
                const size_t lr = el % A.nl;
                const RouteRing served{tl.in_ring + lr * A.n, tl.coll_owner + lr * A.ncoll};
                const uint32_t from = walk_move<false>((uint32_t)__builtin_amdgcn_readlane((int)p0, L), RN_WINDOW, npts);
                uint32_t q = REP_NONE;
                walk_wave<REP_MAX_R, false>(served, A, ue, from, RN_WINDOW, lane == (uint32_t)L, q, -1,
                                            (uint32_t)__builtin_amdgcn_readlane((int)target, L), lane);
            }
            const uint32_t cs = (uint32_t)__shfl((int)ue.cnt, 0, (int)RN_GROUP);
#pragma unroll
            for (uint32_t t = 0; t < REP_MAX_R; t++) {
                const int32_t x = __shfl(ue.s[t], 0, (int)RN_GROUP);
                if (sparse && t == j) d = t < cs ? x : -1;
            }
            if (sparse) c = cs;
        }
        if (live && c == 0) {  // an empty ring, or a ring whose servers own no point: lookupN gives [whoami]
            c = 1;
            if (j == 0) d = (int32_t)e;
        }

        // 3: slot j's destination
        const bool slot = live && j < c;
        const uint32_t dd = slot ? (uint32_t)d : e;  // (a node id in every lane)
        const bool local = slot && dd == e;
        const bool unr = slot && !local && unreachable(S, e, dd);
        const bool walk = slot && !local && !unr;
        const RouteShard& td = A.tab[dd / A.nl];
        const size_t dr = dd % A.nl;
        const RouteRing ring_d{td.in_ring + dr * A.n, td.coll_owner + dr * A.ncoll};
        uint32_t wk[RN_SPAN];
#pragma unroll
        for (uint32_t k = 0; k < RN_SPAN; k++)
            wk[k] = (uint32_t)__shfl((int)pk[k / RN_GROUP], (int)(k % RN_GROUP), (int)RN_GROUP);
        uint32_t cse = 0, csd = 0;
        int32_t rcd = 0;
        uint32_t self_in = 0;
        int32_t o[REP_MAX_R];
        if (walk) {
            cse = te.ring_csum[e];
            csd = td.ring_csum[dd];
            rcd = td.ring_count[dd];
            self_in = ring_d.in_ring[dd];
        }
#pragma unroll
        for (uint32_t k = 0; k < REP_MAX_R; k++) {
            o[k] = -1;
            if (k < lead && walk) o[k] = rn_owner(ring_d, wk[k]);
        }
        // an empty ring or a ring of d alone holds every key without a walk
        bool held = walk && (rcd <= 0 || (rcd == 1 && self_in));
        bool done = !walk || held;
        OwnerSet<REP_MAX_R - 1> u;  // (the R-th other owner ends the walk: it is never stored)
        u.clear();
#pragma unroll
        for (uint32_t k = 0; k < REP_MAX_R; k++)
            if (k < lead) rn_take(u, o[k], (int32_t)dd, R, done, held);
#pragma unroll
        for (uint32_t k = 1; k < RN_SPAN; k++) {
            if (k >= lead && k < span && __ballot(!done) != 0) {
                if (!done) rn_take(u, rn_owner(ring_d, wk[k]), (int32_t)dd, R, done, held);
            }
        }
        if (span == npts) done = true;  // once round
        unsigned long long pend = __ballot(!done);
        while (pend != 0) {
            const int L = __ffsll(pend) - 1;
            pend &= pend - 1;
            const uint32_t vl = (uint32_t)__builtin_amdgcn_readlane((int)dd, L);
            const RouteShard& tl = A.tab[vl / A.nl];
            const size_t lr = vl % A.nl;
            const RouteRing served{tl.in_ring + lr * A.n, tl.coll_owner + lr * A.ncoll};
            const uint32_t from = walk_move<false>((uint32_t)__builtin_amdgcn_readlane((int)p0, L), span, npts);
            uint32_t q = REP_NONE;
            walk_wave<REP_MAX_R - 1, false>(served, A, u, from, span, lane == (uint32_t)L, q, (int32_t)vl, R, lane);
            // (it ended at a point of vl's before the R-th other owner was kept, or it did not)
            if (lane == (uint32_t)L) held = q != REP_NONE && u.cnt < R;
        }

        // 4: the slot's row entries, the request's acks, the counters
        uint32_t oc = RN_EMPTY, hl = 0;
        if (local) {
            oc = RN_OC_LOCAL;
            hl = 1;
        } else if (unr) {
            oc = RN_OC_UNREACHABLE;
        } else if (walk) {
            oc = cse != csd ? RN_OC_DIFFER : RN_OC_DELIVERED;
            hl = held ? 1u : 0u;
        }
        const bool leader = active && j == 0;
        if (leader && !live) oc = RN_OC_ENTRY_DEAD;
        if (active && j < R) {
            const uint64_t at = i * R + j;
            if (dests) dests[at] = slot ? d : -1;
            if (outcomes) outcomes[at] = (uint8_t)oc;
            if (holds) holds[at] = (uint8_t)hl;
        }
        const bool ok = oc <= RN_OC_DIFFER && hl != 0;
        const uint32_t na = (uint32_t)__popc(rn_slice(ok, gshift));
        const uint32_t ns = (uint32_t)__popc(rn_slice(ok && oc != RN_OC_DIFFER, gshift));
        if (leader && acks) acks[i] = (uint8_t)na;
        cnt[RN_REQUESTS] += leader ? 1u : 0u;
        cnt[RN_ENTRY_DEAD] += leader && !live ? 1u : 0u;
        cnt[RN_SLOTS] += slot ? 1u : 0u;
        cnt[RN_LOCAL] += oc == RN_OC_LOCAL ? 1u : 0u;
        cnt[RN_DELIVERED] += oc == RN_OC_DELIVERED ? 1u : 0u;
        cnt[RN_DIFFER] += oc == RN_OC_DIFFER ? 1u : 0u;
        cnt[RN_UNREACHABLE] += oc == RN_OC_UNREACHABLE ? 1u : 0u;
        cnt[RN_MISPLACED] += walk && hl == 0 ? 1u : 0u;
        cnt[RN_SHORT] += leader && live && c < R ? 1u : 0u;
#pragma unroll
        for (uint32_t k = 0; k <= REP_MAX_R; k++) {  // (registers: no indexed access)
            cnt[RN_ACKS + k] += leader && live && na == k ? 1u : 0u;
            cnt[RN_STRICT + k] += leader && live && ns == k ? 1u : 0u;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < RN_NCOUNT; k++)
        if (cnt[k]) atomicAdd(&bc[k], (unsigned long long)cnt[k]);
    __syncthreads();
    if (threadIdx.x < RN_NCOUNT && bc[threadIdx.x]) atomicAdd(&stats[threadIdx.x], bc[threadIdx.x]);
}

}  // namespace rp

// =====================================================================
// Host side (on the first shard's stream, like rp_sim_route).
// =====================================================================
using rp::DevBuf;
using rp::Error;
using rp::Shard;

namespace {

constexpr uint64_t RN_LAUNCH = 1ull << 31;  // requests of a launch, at the most: a lane's counters are 32-bit
constexpr unsigned RN_BLOCKS = 2048;        // blocks of a launch, at the most: 65,536 requests a pass of the grid

// the device rows are for the whole batch: request `first + i` of a launch writes at (first + i) * R
template <bool UNIFORM>
void route_n_launch(rp_sim* c, uint32_t R, const uint32_t* entries, const uint32_t* keys, uint64_t seed, uint64_t count,
                    int32_t* dests, uint8_t* outcomes, uint8_t* holds, uint8_t* acks, rp_route_n_stats* stats) {
    static_assert(sizeof(rp_route_n_stats) == 256, "rp_route_n_stats is 32 x u64");
    static_assert(offsetof(rp_route_n_stats, acks_hist) == 8 * rp::RN_ACKS &&
                      offsetof(rp_route_n_stats, strict_hist) == 8 * rp::RN_STRICT &&
                      offsetof(rp_route_n_stats, reserved) == 8 * rp::RN_NCOUNT,
                  "the device counters are the struct's first fields, in order");
    Shard& s0 = *c->sh.front();
    rp::SimDev S = s0.d;
    S.round = c->round;  // the clock of the next round, as rp_sim_route
    S.part_start = c->part[0]; S.part_end = c->part[1]; S.part_split = c->part[2];
    const rp::OwnArgs A = c->own_args();  // (the routing tables and the points: no census buffer is read)
    DevBuf<unsigned long long> dst(rp::RN_NCOUNT);
    RP_HIP(hipMemsetAsync(dst.p, 0, dst.bytes(), s0.st));
    for (uint64_t first = 0; first < count; first += RN_LAUNCH) {
        const uint64_t m = std::min<uint64_t>(count - first, RN_LAUNCH);
        s0.timed(5, [&] {
            hipLaunchKernelGGL(rp::k_route_n<UNIFORM>, dim3(std::min(rp::grid_for(m, rp::RN_PER_BLOCK), RN_BLOCKS)),
                               dim3(rp::RN_BLOCK), 0, s0.st, S, A, R, UNIFORM ? nullptr : entries + first,
                               UNIFORM ? nullptr : keys + first, seed, first, m, dests ? dests + first * R : nullptr,
                               outcomes ? outcomes + first * R : nullptr, holds ? holds + first * R : nullptr,
                               acks ? acks + first : nullptr, dst.p);
        });
        RP_HIP(hipGetLastError());
    }
    unsigned long long h[rp::RN_NCOUNT];
    RP_HIP(hipMemcpyAsync(h, dst.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
    RP_HIP(hipStreamSynchronize(s0.st));
    if (stats) memcpy(stats, h, sizeof h);  // (the reserved words stay 0)
}

void check_replicas(uint32_t replicas) {
    if (replicas < 1 || replicas > rp::REP_MAX_R) throw Error(RP_ERR_INVALID, "replicas must be 1..8");
}

}  // namespace

extern "C" {

int rp_sim_route_n(rp_sim* c, uint32_t replicas, const uint32_t* entries, const uint32_t* key_hashes, size_t nk,
                   int32_t* dests, uint8_t* outcomes, uint8_t* holds, uint8_t* acks, rp_route_n_stats* stats) {
    return rp::guarded([&] {
        if (!c || (nk && (!entries || !key_hashes))) throw Error(RP_ERR_INVALID, "null pointer");
        check_replicas(replicas);
        for (size_t i = 0; i < nk; i++)
            if (entries[i] >= c->n) throw Error(RP_ERR_INVALID, "request " + std::to_string(i) + ": entry node out of range");
        c->route_prepare(true);
        if (stats) memset(stats, 0, sizeof *stats);
        if (nk == 0) return;
        Shard& s0 = *c->sh.front();
        const size_t R = replicas;
        DevBuf<uint32_t> de(nk), dh(nk);
        DevBuf<int32_t> dd(dests ? nk * R : 0);
        DevBuf<uint8_t> dout(outcomes ? nk * R : 0), dhl(holds ? nk * R : 0), dack(acks ? nk : 0);
        RP_HIP(hipMemcpyAsync(de.p, entries, nk * 4, hipMemcpyHostToDevice, s0.st));
        RP_HIP(hipMemcpyAsync(dh.p, key_hashes, nk * 4, hipMemcpyHostToDevice, s0.st));
        route_n_launch<false>(c, replicas, de.p, dh.p, 0, nk, dd.p, dout.p, dhl.p, dack.p, stats);  // (the stream is drained)
        if (dests) RP_HIP(hipMemcpyAsync(dests, dd.p, nk * R * 4, hipMemcpyDeviceToHost, s0.st));
        if (outcomes) RP_HIP(hipMemcpyAsync(outcomes, dout.p, nk * R, hipMemcpyDeviceToHost, s0.st));
        if (holds) RP_HIP(hipMemcpyAsync(holds, dhl.p, nk * R, hipMemcpyDeviceToHost, s0.st));
        if (acks) RP_HIP(hipMemcpyAsync(acks, dack.p, nk, hipMemcpyDeviceToHost, s0.st));
        RP_HIP(hipStreamSynchronize(s0.st));
    });
}

int rp_sim_route_n_uniform(rp_sim* c, uint32_t replicas, uint64_t seed, uint64_t count, rp_route_n_stats* stats) {
    return rp::guarded([&] {
        if (!c) throw Error(RP_ERR_INVALID, "null pointer");
        check_replicas(replicas);
        c->route_prepare(true);
        if (stats) memset(stats, 0, sizeof *stats);
        if (count)
            route_n_launch<true>(c, replicas, nullptr, nullptr, seed, count, nullptr, nullptr, nullptr, nullptr, stats);
    });
}

}  // extern "C"
