// ringpop_amd — replica-set census (rp_sim_replication / rp_sim_replication_at)
// and HashRing.lookupN in one node's view (rp_sim_ring_lookup_n); DESIGN.md
// §16.  For every interval between two ring points, how many live nodes
// believe they hold one of its R replicas in their own view.  The kernels, the
// host side that launches them and the three entry points.  The difference
// array and the tile scan are the ownership census' (rp_own.h); the walk that
// collects distinct owners is shared with the holders query (rp_repl.h); the
// arc kernel, the finish pass and the per-view lookupN are this file's.  None
// of the kernels is launched by a round.  Every store is a vector store or an
// integer atomic, and the phases are separate kernels: no block waits for
// another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rp_repl.h"

namespace rp {

// the census' device results: rp_replication_stats' measure[16], the claimant
// count, the largest count packed with its first interval (claims << 32 |
// ~index: an atomic max keeps the lowest index), the smallest (claims << 32 |
// index: an atomic min does), and the arc kernel's work: per view one add of
// (arcs << 40 | walk steps) to one of REP_WORK_SLOTS words a cache line apart,
// so that the views' adds do not queue at one address
enum : uint32_t { REP_MEASURE = 0, REP_CLAIMANTS = 16, REP_MAX = 17, REP_MIN = 18, REP_WORK = 32 };
constexpr uint32_t REP_WORK_SLOTS = 64, REP_WORK_STRIDE = 16;
constexpr uint32_t REP_NOUT = REP_WORK + REP_WORK_SLOTS * REP_WORK_STRIDE;

// One wave per view v, one lane per distinct own point p that the view gives
// to v, in two passes of 64 + 36 lanes (k_own_arcs' layout).  In its own view
// v is on the R-list of exactly the intervals from which a forward walk meets
// p before it meets R distinct other servers, and no other point of v first:
// the lane walks back from p and ends at (a) a point v owns -- the previous
// own point p', whose lane covers the rest --, (b) the point q where the R-th
// distinct other owner appears, or (c) p itself after a whole turn (the view's
// only own point: everything).  The arc is the intervals q + 1 .. p, added to
// the difference array as the ownership census does; the arcs of a view are
// disjoint, at most 100.  A dead node, an empty ring and a ring of v alone
// are answered without a walk.  A lane examines R + REP_SOLO_EXTRA points
// alone, then walk_wave takes over: the work of a wave is bounded by
// 100 (R + 3) + (npts + 100 x 63) / 64 + 100 R steps whatever the view.
//
// REC (a snapshot, or a comparison with the simulation as it is: DESIGN.md
// §19) also writes the arcs as (q, p) to the node's row of `arcs`, in
// ascending p, once both walks of a pass have ended and the wave is converged
// -- a pass' arcs ranked by a ballot, the second pass after the first -- and
// their number to arc_n[v]: 0 for a node that is no claimant, OWN_ARC_ALL for
// one that holds everything (an empty ring, a ring of v alone, a whole turn).
// The plain census launches k_rep_arcs<false> (arc_n = arcs = nullptr), whose
// instructions are those of the kernel before it became a template.
template <bool REC>
__global__ void __launch_bounds__(OWN_BLOCK) k_rep_arcs(OwnArgs A, uint32_t R, uint32_t* arc_n, uint2* arcs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t v = blockIdx.x * (OWN_BLOCK / 64) + (threadIdx.x >> 6);
    if (v >= A.n) return;  // (the whole wave)
    const uint32_t g = v / A.nl;
    if (A.dead[g][v] != 0) {  // fail-stopped, or not joined yet: no claimant
        if (lane == 0) {
            A.claimed[v] = 0;
            if (REC) arc_n[v] = 0;
        }
        return;
    }
    const RouteShard& t = A.tab[g];
    const size_t lr = v % A.nl;
    const RouteRing ring{t.in_ring + lr * A.n, t.coll_owner + lr * A.ncoll};
    const int32_t rc = t.ring_count[v];
    const uint32_t npts = A.npts;
    if (lane == 0) atomicAdd(&A.out[REP_CLAIMANTS], 1ull);
    // an empty ring (RingPop.lookupN returns [whoami]) or a ring of v alone: everything
    if (rc <= 0 || (rc == 1 && ring.in_ring[v])) {
        if (lane == 0) {
            atomicAdd(&A.diff[0], 1);
            A.claimed[v] = 1ull << 32;
            if (REC) arc_n[v] = OWN_ARC_ALL;
        }
        return;
    }
    const uint32_t* row = A.srv_pt + (size_t)v * OWN_REPLICAS;
    unsigned long long total = 0;
    uint32_t solo = 0, coop = 0, narc = 0;
    uint32_t kept = 0;  // REC: arcs stored so far, or OWN_ARC_ALL
    for (uint32_t r0 = 0; r0 < OWN_REPLICAS; r0 += 64) {
        const uint32_t rr = r0 + lane;
        bool search = false;
        uint32_t p = 0;
        if (rr < OWN_REPLICAS) {
            p = row[rr];
            const bool dup = rr > 0 && row[rr - 1] == p;
            search = !dup && ring.owner(A.pt_coll[p], A.pt_server[p]) == (int32_t)v;
        }
        OwnerSet<REP_MAX_R - 1> u;  // (the R-th other owner ends the walk: it is never stored)
        u.clear();
        uint32_t pos = walk_move<true>(p, 1 % npts, npts), dist = 0, q = p;
        bool done = !search;
        walk_solo<REP_MAX_R - 1, true>(ring, A, u, pos, dist, done, q, (int32_t)v, R, R + REP_SOLO_EXTRA);
        solo += dist;
        coop += walk_wave<REP_MAX_R - 1, true>(ring, A, u, pos, dist, !done, q, (int32_t)v, R, lane);
        if (search) {
            narc++;
            if (q == p || q == REP_NONE) {  // the view's only own point (the walk ends at p at the latest)
                atomicAdd(&A.diff[0], 1);
                total += 1ull << 32;
            } else {
                atomicAdd(&A.diff[q + 1], 1);
                atomicSub(&A.diff[p + 1], 1);
                if (q > p) atomicAdd(&A.diff[0], 1);  // the arc wraps
                total += (uint32_t)(A.pt_hash[p] - A.pt_hash[q]);
            }
        }
        if (REC) {
            // (p ascends with the lane: the rank among the pass' searching lanes is the arc's place)
            const bool whole = search && (q == p || q == REP_NONE);
            const unsigned long long arc = __ballot(search && !whole);
            if (__ballot(whole)) kept = OWN_ARC_ALL;
            if (search && !whole)
                arcs[(size_t)v * OWN_REPLICAS + (kept & ~OWN_ARC_ALL) + __popcll(arc & ((1ull << lane) - 1))] = make_uint2(q, p);
            kept += (uint32_t)__popcll(arc);
        }
    }
    total = wave_sum_u64(total);
    const unsigned long long steps = wave_sum_u64(solo);
    const unsigned long long narcs = wave_sum_u64(narc);
    if (lane == 0) {
        A.claimed[v] = total;
        if (REC) arc_n[v] = (kept & OWN_ARC_ALL) ? OWN_ARC_ALL : kept;
        atomicAdd(&A.out[REP_WORK + (v % REP_WORK_SLOTS) * REP_WORK_STRIDE], narcs << 40 | (steps + coop));
    }
}

// claims_R(i) stored; measure[min(claims, 15)] += length(i) by selects, the
// largest and the smallest claims with their first interval; per thread in
// registers, per block in LDS, one atomic per counter and block
// (k_own_finish's scheme with sixteen classes and the minimum)
__global__ void __launch_bounds__(OWN_BLOCK) k_rep_finish(OwnArgs A) {
    __shared__ int32_t ws[OWN_BLOCK / 64];
    __shared__ unsigned long long bm[16];
    __shared__ unsigned long long bmax, bmin;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16) bm[threadIdx.x] = 0;
    if (threadIdx.x == 16) bmax = 0;
    if (threadIdx.x == 17) bmin = ~0ull;
    const uint32_t first = blockIdx.x * OWN_TILE + threadIdx.x * OWN_ITEMS;
    int32_t c[OWN_ITEMS];
    int32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++) {
        if (first + j < A.npts) s += A.diff[first + j];
        c[j] = s;
    }
    const int32_t incl = wave_scan_incl(s, lane);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int32_t base = A.tile_sum[blockIdx.x] + incl - s;
    for (uint32_t w = 0; w < wave; w++) base += ws[w];
    unsigned long long m[16], best = 0, least = ~0ull;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) m[k] = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++) {
        const uint32_t i = first + j;
        if (i < A.npts) {
            const uint32_t cl = (uint32_t)(base + c[j]);
            A.claims[i] = cl;
            // interval i is (pt_hash[i - 1], pt_hash[i]]; interval 0 wraps
            const unsigned long long len = i ? (unsigned long long)(A.pt_hash[i] - A.pt_hash[i - 1])
                                             : (unsigned long long)A.pt_hash[0] + (1ull << 32) - A.pt_hash[A.npts - 1];
            const uint32_t cls = cl < 15u ? cl : 15u;
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) m[k] += cls == k ? len : 0ull;
            const unsigned long long hi = (unsigned long long)cl << 32;
            best = (hi | (uint32_t)~i) > best ? (hi | (uint32_t)~i) : best;
            least = (hi | i) < least ? (hi | i) : least;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        if (m[k]) atomicAdd(&bm[k], m[k]);
    if (best) atomicMax(&bmax, best);
    if (least != ~0ull) atomicMin(&bmin, least);
    __syncthreads();
    if (threadIdx.x < 16 && bm[threadIdx.x]) atomicAdd(&A.out[REP_MEASURE + threadIdx.x], bm[threadIdx.x]);
    if (threadIdx.x == 16 && bmax) atomicMax(&A.out[REP_MAX], bmax);
    if (threadIdx.x == 17 && bmin != ~0ull) atomicMin(&A.out[REP_MIN], bmin);
}

// claims_R of the interval a key hash falls in: the first point >= h, else interval 0
__global__ void __launch_bounds__(256) k_rep_at(OwnArgs A, const uint32_t* keys, uint32_t nk, uint32_t* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x)
        out[i] = A.claims[route_point(A.pt_hash, A.npts, A.dir, A.dir_shift, keys[i])];
}

// HashRing.lookupN(key, n) in view v (lib/ring.js:150-182): one lane per key.
// The walk starts at the key's point and goes forward until min(n, servers of
// the ring) owners are kept or it has been once round (a server whose every
// point collides and is another's owns none).  A lane examines target + 3
// points alone -- a dense view ends there --, then walk_wave serves the lanes
// of a sparse view 64 points a step.  The sixteen owners live in registers;
// the row is written with its unused slots -1.
__global__ void __launch_bounds__(256) k_rep_lookup_n(OwnArgs A, uint32_t v, const uint32_t* keys, uint32_t nk, uint32_t n,
                                                      int32_t* out, int32_t* counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const RouteShard& t = A.tab[v / A.nl];
    const size_t lr = v % A.nl;
    const RouteRing ring{t.in_ring + lr * A.n, t.coll_owner + lr * A.ncoll};
    const int32_t rc = t.ring_count[v];
    const uint32_t target = rc <= 0 ? 0u : ((uint32_t)rc < n ? (uint32_t)rc : n);
    // (the bound is the block's: every wave goes round together)
    for (uint64_t b0 = (uint64_t)blockIdx.x * blockDim.x; b0 < nk; b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = b0 + threadIdx.x;
        const bool active = i < nk;
        OwnerSet<REP_MAX_N> u;
        u.clear();
        uint32_t pos = 0, dist = 0, q = REP_NONE;
        bool done = !active || target == 0;
        if (!done) pos = route_point(A.pt_hash, A.npts, A.dir, A.dir_shift, keys[i]);
        walk_solo<REP_MAX_N, false>(ring, A, u, pos, dist, done, q, -1, target, target + REP_SOLO_EXTRA);
        walk_wave<REP_MAX_N, false>(ring, A, u, pos, dist, !done, q, -1, target, lane);
        if (active) {
            counts[i] = (int32_t)u.cnt;
#pragma unroll
            for (uint32_t j = 0; j < REP_MAX_N; j++)
                if (j < n) out[i * n + j] = j < u.cnt ? u.s[j] : -1;
        }
    }
}

static unsigned rep_blocks(uint64_t items, unsigned per_block, unsigned cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace rp

// =====================================================================
// Host side (on the first shard's stream, like the ownership census).
// =====================================================================
using rp::DevBuf;
using rp::Error;
using rp::Shard;

// the census' argument block with the replica census' own result buffers
static rp::OwnArgs rep_args(rp_sim* c) {
    rp::OwnArgs A = c->own_args();
    A.diff = c->rep_diff.p; A.claims = c->rep_claims.p; A.tile_sum = c->rep_tile.p;
    A.claimed = c->rep_held.p; A.out = c->rep_out.p;
    return A;
}

// The replica census for R, unless it is the cached one and no call that can
// change a ring ran since (timed as "other", like a route).
// record: the arcs are wanted too (§19) -- a cached census that did not
// record them runs again, with the recording kernel.
void rp_sim::rep_refresh(uint32_t R, bool record) {
    own_prepare();
    Shard& s0 = *sh.front();
    const uint32_t npts = s0.npts;
    if (!rep_stale && rep_r == R && rep_claims.n == npts && rep_held.n == n && (!record || rep_arcs_valid)) return;
    rep_r = 0;  // (nothing is cached until this run is complete)
    rep_arcs_valid = false;
    if (record) {
        if (rep_arc_n.n != n) rep_arc_n.alloc(n);
        if (rep_arcs.n != (size_t)n * rp::OWN_REPLICAS) rep_arcs.alloc((size_t)n * rp::OWN_REPLICAS);
    }
    if (rep_diff.n != (size_t)npts + 1) rep_diff.alloc((size_t)npts + 1);
    if (rep_claims.n != npts) rep_claims.alloc(npts);
    if (rep_held.n != n) rep_held.alloc(n);
    if (!rep_out.p) rep_out.alloc(rp::REP_NOUT);
    const uint32_t ntiles = (npts + rp::OWN_TILE - 1) / rp::OWN_TILE;
    if (rep_tile.n != ntiles) rep_tile.alloc(ntiles);
    const rp::OwnArgs A = rep_args(this);
    s0.timed(5, [&] {
        RP_HIP(hipMemsetAsync(rep_diff.p, 0, rep_diff.bytes(), s0.st));
        RP_HIP(hipMemsetAsync(rep_out.p, 0, rep_out.bytes(), s0.st));
        RP_HIP(hipMemsetAsync(rep_out.p + rp::REP_MIN, 0xFF, sizeof(unsigned long long), s0.st));
        const unsigned per = rp::OWN_BLOCK / 64;  // views (waves) per block
        if (record)
            hipLaunchKernelGGL(rp::k_rep_arcs<true>, dim3((n + per - 1) / per), dim3(rp::OWN_BLOCK), 0, s0.st, A, R,
                               rep_arc_n.p, rep_arcs.p);
        else
            hipLaunchKernelGGL(rp::k_rep_arcs<false>, dim3((n + per - 1) / per), dim3(rp::OWN_BLOCK), 0, s0.st, A, R,
                               (uint32_t*)nullptr, (uint2*)nullptr);
        rp::own_scan_tiles(A, s0.st);
        hipLaunchKernelGGL(rp::k_rep_finish, dim3(ntiles), dim3(rp::OWN_BLOCK), 0, s0.st, A);
    });
    RP_HIP(hipGetLastError());
    unsigned long long h[rp::REP_NOUT];
    RP_HIP(hipMemcpyAsync(h, rep_out.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
    RP_HIP(hipStreamSynchronize(s0.st));
    rp_replication_stats st{};
    for (uint32_t k = 0; k < 16; k++) {
        const uint64_t m = h[rp::REP_MEASURE + k];
        st.measure[k] = m;
        // (R <= 8: the class of 15 or more is over-replicated)
        if (k < R) st.under += m; else if (k == R) st.exact += m; else st.over += m;
    }
    st.replicas = R;
    st.claimants = h[rp::REP_CLAIMANTS];
    st.intervals = npts;
    st.max_claims = h[rp::REP_MAX] >> 32;
    st.min_claims = h[rp::REP_MIN] >> 32;
    const uint32_t at[2] = {~(uint32_t)h[rp::REP_MAX], (uint32_t)h[rp::REP_MIN]};
    uint32_t hash[2] = {0, 0};
    for (int k = 0; k < 2; k++)
        if (at[k] < npts) RP_HIP(hipMemcpy(&hash[k], s0.pt_hash.p + at[k], 4, hipMemcpyDeviceToHost));
    st.max_claims_hash = hash[0];
    st.min_claims_hash = hash[1];
    for (uint32_t k = 0; k < rp::REP_WORK_SLOTS; k++) {
        const uint64_t w = h[rp::REP_WORK + k * rp::REP_WORK_STRIDE];
        st.walk_steps += w & ((1ull << 40) - 1);
        st.arcs += w >> 40;
    }
    rep_stats = st;
    rep_r = R;
    rep_stale = false;
    rep_arcs_valid = record;
}

extern "C" {

int rp_sim_replication(rp_sim* c, uint32_t replicas, rp_replication_stats* stats, uint64_t* held, size_t cap) {
    return rp::guarded([&] {
        static_assert(sizeof(rp_replication_stats) == 256, "rp_replication_stats is 32 x u64");
        if (!c || !stats) throw Error(RP_ERR_INVALID, "null pointer");
        if (replicas < 1 || replicas > rp::REP_MAX_R) throw Error(RP_ERR_INVALID, "replicas must be 1..8");
        if (held && cap < c->n) throw Error(RP_ERR_INVALID, "held buffer holds fewer than n entries");
        c->rep_refresh(replicas);
        *stats = c->rep_stats;
        if (held) RP_HIP(hipMemcpy(held, c->rep_held.p, (size_t)c->n * 8, hipMemcpyDeviceToHost));
    });
}

int rp_sim_replication_at(rp_sim* c, uint32_t replicas, const uint32_t* key_hashes, size_t nk, uint32_t* claims) {
    return rp::guarded([&] {
        if (!c || (nk && (!key_hashes || !claims))) throw Error(RP_ERR_INVALID, "null pointer");
        if (replicas < 1 || replicas > rp::REP_MAX_R) throw Error(RP_ERR_INVALID, "replicas must be 1..8");
        c->rep_refresh(replicas);
        if (nk == 0) return;
        Shard& s0 = *c->sh.front();
        const rp::OwnArgs A = rep_args(c);
        // (launches of at most 2^30 keys: a thread's index is 32-bit)
        const size_t chunk = std::min<size_t>(nk, (size_t)1 << 30);
        DevBuf<uint32_t> dh(chunk), dc(chunk);
        for (size_t first = 0; first < nk; first += chunk) {
            const size_t m = std::min(nk - first, chunk);
            RP_HIP(hipMemcpyAsync(dh.p, key_hashes + first, m * 4, hipMemcpyHostToDevice, s0.st));
            s0.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_rep_at, dim3(rp::rep_blocks(m, 256, 16384)), dim3(256), 0, s0.st, A,
                                   (const uint32_t*)dh.p, (uint32_t)m, dc.p);
            });
            RP_HIP(hipGetLastError());
            RP_HIP(hipMemcpyAsync(claims + first, dc.p, m * 4, hipMemcpyDeviceToHost, s0.st));
            RP_HIP(hipStreamSynchronize(s0.st));
        }
    });
}

int rp_sim_ring_lookup_n(rp_sim* c, uint32_t node, const uint32_t* key_hashes, size_t nk, int n, int32_t* out,
                         int32_t* counts) {
    return rp::guarded([&] {
        if (!c || node >= c->n) throw Error(RP_ERR_INVALID, "bad node");
        if (n < 0 || n > (int)rp::REP_MAX_N) throw Error(RP_ERR_INVALID, "n must be 0..16");
        if (nk && (!key_hashes || !counts || (n && !out))) throw Error(RP_ERR_INVALID, "null pointer");
        c->route_prepare(false);
        if (nk == 0) return;
        Shard& s0 = *c->sh.front();
        const rp::OwnArgs A = c->own_args();  // (the routing tables and the points: the census' buffers are not read)
        // (launches of at most 2^26 keys: a row index times 16 stays far below 2^32 words)
        const size_t chunk = std::min<size_t>(nk, (size_t)1 << 26);
        DevBuf<uint32_t> dh(chunk);
        DevBuf<int32_t> dout(chunk * (size_t)n), dcnt(chunk);
        for (size_t first = 0; first < nk; first += chunk) {
            const size_t m = std::min(nk - first, chunk);
            RP_HIP(hipMemcpyAsync(dh.p, key_hashes + first, m * 4, hipMemcpyHostToDevice, s0.st));
            s0.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_rep_lookup_n, dim3(rp::rep_blocks(m, 256, 16384)), dim3(256), 0, s0.st, A, node,
                                   (const uint32_t*)dh.p, (uint32_t)m, (uint32_t)n, dout.p, dcnt.p);
            });
            RP_HIP(hipGetLastError());
            if (n) RP_HIP(hipMemcpyAsync(out + first * (size_t)n, dout.p, m * (size_t)n * 4, hipMemcpyDeviceToHost, s0.st));
            RP_HIP(hipMemcpyAsync(counts + first, dcnt.p, m * 4, hipMemcpyDeviceToHost, s0.st));
            RP_HIP(hipStreamSynchronize(s0.st));
        }
    });
}

}  // extern "C"
