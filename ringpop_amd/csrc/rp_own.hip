// ringpop_amd — ownership census (rp_sim_ownership / rp_sim_ownership_at;
// DESIGN.md §13): for every interval between two ring points, how many live
// nodes claim it in their own view.  The kernels, the host side that launches
// them and the two entry points; and ownership movement between two instants
// (rp_ownership_snapshot_* / rp_sim_ownership_moved; §15), which compares the
// arcs the census' first kernel can record.  None of the kernels is launched by a round.
// Every store is a vector store or an integer atomic, and the phases are
// separate kernels: no block waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <string>

#include "rp_cluster.h"

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
constexpr uint32_t OWN_ARC_ALL = 0x80000000u;  // a recorded arc count: the node claims every interval

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

// replica hash -> index of its point (every replica hash is a point: the
// search is exact).  The host sorted each server's hashes, so a row's indices
// ascend and the replicas that share a point are adjacent.
__global__ void __launch_bounds__(256) k_own_point_index(OwnArgs A, const uint32_t* rep_hash, uint32_t* srv_pt) {
    const uint64_t total = (uint64_t)A.n * OWN_REPLICAS;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
        srv_pt[i] = route_point(A.pt_hash, A.npts, A.dir, A.dir_shift, rep_hash[i]);
}

__device__ inline unsigned long long wave_sum_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}

// One wave per view v.  v claims the arcs that end at its own points in its
// own view: a lane takes one distinct own point p, keeps it if the view gives
// it to v (a colliding point may be another server's), and walks back to the
// nearest point q some server of the view owns; the arc is the intervals
// q + 1 .. p (cyclically), added to the difference array.  The walk ends at p
// itself at the latest (p is owned).  A lane walks OWN_WALK_STEPS points
// alone -- a converged view finds q in one -- then the wave serves the lanes
// still searching one after the other, 64 preceding points per step, so that
// a view with few servers costs npts / 64 steps per arc and not npts.
//
// REC (a snapshot, or a comparison with the simulation as it is: DESIGN.md
// §15) also writes the kept arcs as (q, p) to the node's row of `arcs`, in
// ascending p -- a pass' arcs ranked by a ballot, the second pass after the
// first -- and their number to arc_n[v]: 0 for a node that is no claimant,
// OWN_ARC_ALL for one that claims everything.  The plain census launches
// k_own_arcs<false> (arc_n = arcs = nullptr), whose instructions are those of
// the kernel before it became a template.
template <bool REC>
__global__ void __launch_bounds__(OWN_BLOCK) k_own_arcs(OwnArgs A, uint32_t* arc_n, uint2* arcs) {
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
    if (lane == 0) atomicAdd(&A.out[OWN_CLAIMANTS], 1ull);
    // an empty ring (lookup falls back to whoami) or a ring of v alone: everything
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
    uint32_t kept = 0;  // REC: arcs stored so far, or OWN_ARC_ALL
    for (uint32_t r0 = 0; r0 < OWN_REPLICAS; r0 += 64) {
        const uint32_t rr = r0 + lane;
        bool search = false, found = false;
        uint32_t p = 0, q = 0;
        if (rr < OWN_REPLICAS) {
            p = row[rr];
            const bool dup = rr > 0 && row[rr - 1] == p;
            search = !dup && ring.owner(A.pt_coll[p], A.pt_server[p]) == (int32_t)v;
            q = p;
        }
        if (search) {
            for (uint32_t k = 0; k < OWN_WALK_STEPS && !found; k++) {
                q = q ? q - 1 : npts - 1;
                found = ring.owner(A.pt_coll[q], A.pt_server[q]) >= 0;
            }
        }
        unsigned long long pend;
        while ((pend = __ballot(search && !found)) != 0) {
            const int L = __ffsll(pend) - 1;
            const uint32_t base = __shfl(q, L, 64);
            // the point (lane + 1) before base; lanes past a whole turn repeat nearer points, further away
            const uint32_t d = (lane + 1) % npts;
            const uint32_t idx = base >= d ? base - d : base + npts - d;
            const unsigned long long hits = __ballot(ring.owner(A.pt_coll[idx], A.pt_server[idx]) >= 0);
            if (hits) {
                const uint32_t nq = __shfl(idx, __ffsll(hits) - 1, 64);
                if (lane == (uint32_t)L) { q = nq; found = true; }
            } else if (lane == (uint32_t)L) {
                const uint32_t d64 = 64u % npts;
                q = base >= d64 ? base - d64 : base + npts - d64;
            }
        }
        if (search) {
            if (q == p) {  // the view's only present point
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
            const unsigned long long arc = __ballot(search && q != p);
            if (__ballot(search && q == p)) kept = OWN_ARC_ALL;
            if (search && q != p)
                arcs[(size_t)v * OWN_REPLICAS + (kept & ~OWN_ARC_ALL) + __popcll(arc & ((1ull << lane) - 1))] = make_uint2(q, p);
            kept += (uint32_t)__popcll(arc);
        }
    }
    total = wave_sum_u64(total);
    if (lane == 0) {
        A.claimed[v] = total;
        if (REC) arc_n[v] = (kept & OWN_ARC_ALL) ? OWN_ARC_ALL : kept;
    }
}

// ---- claims(i): the inclusive prefix sum of diff, in tiles of OWN_TILE

__device__ inline int32_t wave_scan_incl(int32_t x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    return x;
}

// each tile's sum of diff
__global__ void __launch_bounds__(OWN_BLOCK) k_own_tile_sums(OwnArgs A) {
    __shared__ int32_t ws[OWN_BLOCK / 64];
    const uint32_t first = blockIdx.x * OWN_TILE + threadIdx.x * OWN_ITEMS;
    int32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++)
        if (first + j < A.npts) s += A.diff[first + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t b = 0;
        for (uint32_t w = 0; w < OWN_BLOCK / 64; w++) b += ws[w];
        A.tile_sum[blockIdx.x] = b;
    }
}

// the tile sums' exclusive prefix sums, in place: one wave, 64 tiles a step
__global__ void __launch_bounds__(64) k_own_tile_scan(OwnArgs A) {
    const uint32_t lane = threadIdx.x;
    int32_t carry = 0;
    for (uint32_t b0 = 0; b0 < A.ntiles; b0 += 64) {
        const uint32_t b = b0 + lane;
        const int32_t x = b < A.ntiles ? A.tile_sum[b] : 0;
        const int32_t incl = wave_scan_incl(x, lane);
        if (b < A.ntiles) A.tile_sum[b] = carry + incl - x;
        carry += __shfl(incl, 63, 64);
    }
}

// claims(i) stored; measure[min(claims, 7)] += length(i) and the largest
// claims with its first interval, per thread in registers, per block in LDS,
// one atomic per counter and block
__global__ void __launch_bounds__(OWN_BLOCK) k_own_finish(OwnArgs A) {
    __shared__ int32_t ws[OWN_BLOCK / 64];
    __shared__ unsigned long long bm[8];
    __shared__ unsigned long long bmax;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 8) bm[threadIdx.x] = 0;
    if (threadIdx.x == 8) bmax = 0;
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
    unsigned long long m[8], best = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) m[k] = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++) {
        const uint32_t i = first + j;
        if (i < A.npts) {
            const uint32_t cl = (uint32_t)(base + c[j]);
            A.claims[i] = cl;
            // interval i is (pt_hash[i - 1], pt_hash[i]]; interval 0 wraps
            const unsigned long long len = i ? (unsigned long long)(A.pt_hash[i] - A.pt_hash[i - 1])
                                             : (unsigned long long)A.pt_hash[0] + (1ull << 32) - A.pt_hash[A.npts - 1];
            const uint32_t cls = cl < 7u ? cl : 7u;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) m[k] += cls == k ? len : 0ull;
            const unsigned long long pk = (unsigned long long)cl << 32 | (uint32_t)~i;
            best = pk > best ? pk : best;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; k++)
        if (m[k]) atomicAdd(&bm[k], m[k]);
    if (best) atomicMax(&bmax, best);
    __syncthreads();
    if (threadIdx.x < 8 && bm[threadIdx.x]) atomicAdd(&A.out[OWN_MEASURE + threadIdx.x], bm[threadIdx.x]);
    if (threadIdx.x == 8 && bmax) atomicMax(&A.out[OWN_MAX], bmax);
}

// claims of the interval a key hash falls in: the first point >= h, else interval 0
__global__ void __launch_bounds__(256) k_own_at(OwnArgs A, const uint32_t* keys, uint32_t nk, uint32_t* out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x)
        out[i] = A.claims[route_point(A.pt_hash, A.npts, A.dir, A.dir_shift, keys[i])];
}

// ---- ownership movement between two instants (rp_sim_ownership_moved)

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
    // side 0: from, side 1: to -- recorded arcs (k_own_arcs<true>) and claims
    const uint32_t* arc_n[2];
    const uint2* arcs[2];
    const uint32_t* claims[2];
    const uint32_t* pt_hash;
    uint32_t n, npts, ntiles;
    int32_t* diff;               // 2 x (npts + 1): the gains' difference array, then the losses'
    int32_t* tile_sum;           // 2 x ntiles
    unsigned long long* gained;  // n
    unsigned long long* lost;    // n
    unsigned long long* out;     // MV_NOUT
};

// a node's measure (0 .. 2^32) with its id, so that an atomic max keeps the
// lowest id among equals; the measure needs 33 bits, which leaves 31 for the id
__device__ inline unsigned long long move_pack(unsigned long long measure, uint32_t v) {
    return measure << 31 | (MV_NODE_MASK - v);
}

// where x lies among a side's sorted disjoint segments [lo, hi): is it
// covered, is it one of their endpoints, and the side's next endpoint after it
struct SegAt {
    bool covered, endpoint;
    uint32_t next;
};
__device__ inline SegAt seg_at(const uint32_t* lo, const uint32_t* hi, uint32_t nseg, uint32_t npts, uint32_t x) {
    uint32_t a = 0, b = nseg;  // the number of segments with lo <= x
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (lo[m] <= x) a = m + 1; else b = m;
    }
    SegAt r{false, false, a < nseg ? lo[a] : npts};
    if (a) {
        const uint32_t l = lo[a - 1], h = hi[a - 1];
        r.covered = x < h;
        // (an earlier segment that ends at x makes this one start there)
        r.endpoint = l == x || h == x;
        if (r.covered) r.next = h;
    }
    return r;
}

// One wave per node v: what v claims at `to` and not at `from` (gains) and
// the reverse (losses).  Both sides' arcs become sorted disjoint segments of
// interval indices in LDS -- arc (q, p) is [q + 1, p + 1), the wrapping one
// (only the first can wrap: the others end at the previous own point at the
// latest) is [0, p + 1) and [q + 1, npts) -- at most MV_SEGS a side.  Between
// two consecutive endpoints of either side both coverages are constant: a
// lane takes an endpoint x, drops it unless it is the first of its value in
// the order from-starts, from-ends, to-starts, to-ends, and finds by binary
// search both coverages at x and the next endpoint.  A piece covered by one
// side only is +1 / -1 at its two ends in the gains' or the losses'
// difference array, and its hash length goes to the lane's total.  Work is
// bounded by the arc counts: at most 4 x MV_SEGS endpoints, two searches each.
__global__ void __launch_bounds__(OWN_BLOCK) k_move_arcs(MoveArgs A) {
    __shared__ uint32_t seg_lo[MV_WAVES][2][MV_SEGS], seg_hi[MV_WAVES][2][MV_SEGS];
    __shared__ unsigned long long bsum[4], bmax[2];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t v = blockIdx.x * MV_WAVES + wave;
    const uint32_t npts = A.npts;
    if (threadIdx.x < 4) bsum[threadIdx.x] = 0;
    if (threadIdx.x < 2) bmax[threadIdx.x] = 0;
    uint32_t nseg[2] = {0, 0};
    if (v < A.n) {
#pragma unroll
        for (uint32_t s = 0; s < 2; s++) {
            uint32_t c = A.arc_n[s][v];
            if (!(c & OWN_ARC_ALL) && c > OWN_REPLICAS) c = OWN_REPLICAS;  // (never: the rows hold no more)
            uint32_t* lo = seg_lo[wave][s];
            uint32_t* hi = seg_hi[wave][s];
            if (c & OWN_ARC_ALL) {
                if (lane == 0) { lo[0] = 0; hi[0] = npts; }
                nseg[s] = 1;
            } else if (c) {  // (c <= OWN_REPLICAS: k_own_arcs<true> keeps one arc per own point at most)
                const uint2* row = A.arcs[s] + (size_t)v * OWN_REPLICAS;
                const uint2 a0 = row[0];
                const bool wraps = a0.x > a0.y;
                for (uint32_t k = lane; k < c; k += 64) {
                    const uint2 a = row[k];
                    lo[k] = k == 0 && wraps ? 0u : a.x + 1;
                    hi[k] = a.y + 1;
                }
                // the wrapping arc's upper part lies after every other arc (q >= the last own point)
                const bool tail = wraps && a0.x + 1 < npts;
                if (tail && lane == 0) { lo[c] = a0.x + 1; hi[c] = npts; }
                nseg[s] = c + (tail ? 1u : 0u);
            }
        }
    }
    __syncthreads();
    unsigned long long gain = 0, loss = 0;
    const uint32_t nf = nseg[0], nt = nseg[1];
    const uint32_t* flo = seg_lo[wave][0];
    const uint32_t* fhi = seg_hi[wave][0];
    const uint32_t* tlo = seg_lo[wave][1];
    const uint32_t* thi = seg_hi[wave][1];
    for (uint32_t e = lane; e < 2 * (nf + nt); e += 64) {
        uint32_t x;
        bool first;  // no earlier list of the order holds x
        bool of_to = false;
        if (e < nf) {
            x = flo[e];
            first = true;
        } else if (e < 2 * nf) {
            const uint32_t j = e - nf;
            x = fhi[j];
            first = !(j + 1 < nf && flo[j + 1] == x);
        } else if (e < 2 * nf + nt) {
            x = tlo[e - 2 * nf];
            first = true;
            of_to = true;
        } else {
            const uint32_t j = e - 2 * nf - nt;
            x = thi[j];
            first = !(j + 1 < nt && tlo[j + 1] == x);
            of_to = true;
        }
        if (!first || x >= npts) continue;  // (a segment that ends at npts: nothing follows)
        const SegAt f = seg_at(flo, fhi, nf, npts, x);
        if (of_to && f.endpoint) continue;
        const SegAt t = seg_at(tlo, thi, nt, npts, x);
        if (f.covered == t.covered) continue;
        const uint32_t next = f.next < t.next ? f.next : t.next;  // x < next <= npts
        // intervals x .. next - 1; interval 0 runs from the last point round to the first
        const unsigned long long len = x ? (unsigned long long)(A.pt_hash[next - 1] - A.pt_hash[x - 1])
                                         : (unsigned long long)A.pt_hash[next - 1] + (1ull << 32) - A.pt_hash[npts - 1];
        int32_t* d = A.diff + (t.covered ? 0 : (size_t)npts + 1);
        atomicAdd(&d[x], 1);
        atomicSub(&d[next], 1);
        if (t.covered) gain += len; else loss += len;
    }
    gain = wave_sum_u64(gain);
    loss = wave_sum_u64(loss);
    if (lane == 0 && v < A.n) {
        A.gained[v] = gain;
        A.lost[v] = loss;
        if (gain) {
            atomicAdd(&bsum[0], gain);
            atomicAdd(&bsum[2], 1ull);
            atomicMax(&bmax[0], move_pack(gain, v));
        }
        if (loss) {
            atomicAdd(&bsum[1], loss);
            atomicAdd(&bsum[3], 1ull);
            atomicMax(&bmax[1], move_pack(loss, v));
        }
    }
    __syncthreads();
    // (bsum's order is out's: MV_GAINED, MV_LOST, MV_GAINERS, MV_LOSERS)
    if (threadIdx.x < 4 && bsum[threadIdx.x]) atomicAdd(&A.out[MV_GAINED + threadIdx.x], bsum[threadIdx.x]);
    if (threadIdx.x >= 4 && threadIdx.x < 6 && bmax[threadIdx.x - 4])
        atomicMax(&A.out[MV_MAXG + threadIdx.x - 4], bmax[threadIdx.x - 4]);
}

// g(i) and l(i): the inclusive prefix sums of the two difference arrays, by
// the census' tile scheme.  blockIdx.y is the array.
__global__ void __launch_bounds__(OWN_BLOCK) k_move_tile_sums(MoveArgs A) {
    __shared__ int32_t ws[OWN_BLOCK / 64];
    const int32_t* diff = A.diff + (size_t)blockIdx.y * ((size_t)A.npts + 1);
    const uint32_t first = blockIdx.x * OWN_TILE + threadIdx.x * OWN_ITEMS;
    int32_t s = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++)
        if (first + j < A.npts) s += diff[first + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t b = 0;
        for (uint32_t w = 0; w < OWN_BLOCK / 64; w++) b += ws[w];
        A.tile_sum[(size_t)blockIdx.y * A.ntiles + blockIdx.x] = b;
    }
}

// each array's tile sums to their exclusive prefix sums, in place: one wave an array
__global__ void __launch_bounds__(64) k_move_tile_scan(MoveArgs A) {
    const uint32_t lane = threadIdx.x;
    int32_t* ts = A.tile_sum + (size_t)blockIdx.x * A.ntiles;
    int32_t carry = 0;
    for (uint32_t b0 = 0; b0 < A.ntiles; b0 += 64) {
        const uint32_t b = b0 + lane;
        const int32_t x = b < A.ntiles ? ts[b] : 0;
        const int32_t incl = wave_scan_incl(x, lane);
        if (b < A.ntiles) ts[b] = carry + incl - x;
        carry += __shfl(incl, 63, 64);
    }
}

// Per interval g, l and the two censuses' claims give its cell of
// transition[3][3], same_set and handed_off (length added by selects, in
// registers) and its turnover g + l, packed with ~i so that a max keeps the
// lowest interval; per block in LDS, one atomic per counter and block.
__global__ void __launch_bounds__(OWN_BLOCK) k_move_finish(MoveArgs A) {
    __shared__ int32_t ws[2][OWN_BLOCK / 64];
    __shared__ unsigned long long bm[MV_HANDED + 1];
    __shared__ unsigned long long bmax;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x <= MV_HANDED) bm[threadIdx.x] = 0;
    if (threadIdx.x == MV_HANDED + 1) bmax = 0;
    const uint32_t first = blockIdx.x * OWN_TILE + threadIdx.x * OWN_ITEMS;
    const int32_t* dg = A.diff;
    const int32_t* dl = A.diff + (size_t)A.npts + 1;
    int32_t cg[OWN_ITEMS], cl[OWN_ITEMS];
    int32_t sg = 0, sl = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++) {
        if (first + j < A.npts) { sg += dg[first + j]; sl += dl[first + j]; }
        cg[j] = sg;
        cl[j] = sl;
    }
    const int32_t ig = wave_scan_incl(sg, lane), il = wave_scan_incl(sl, lane);
    if (lane == 63) { ws[0][wave] = ig; ws[1][wave] = il; }
    __syncthreads();
    int32_t bg = A.tile_sum[blockIdx.x] + ig - sg, bl = A.tile_sum[(size_t)A.ntiles + blockIdx.x] + il - sl;
    for (uint32_t w = 0; w < wave; w++) { bg += ws[0][w]; bl += ws[1][w]; }
    unsigned long long m[MV_HANDED + 1], best = 0;
#pragma unroll
    for (uint32_t k = 0; k <= MV_HANDED; k++) m[k] = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++) {
        const uint32_t i = first + j;
        if (i < A.npts) {
            const uint32_t g = (uint32_t)(bg + cg[j]), l = (uint32_t)(bl + cl[j]);
            const uint32_t cf = A.claims[0][i], ct = A.claims[1][i];
            const unsigned long long len = i ? (unsigned long long)(A.pt_hash[i] - A.pt_hash[i - 1])
                                             : (unsigned long long)A.pt_hash[0] + (1ull << 32) - A.pt_hash[A.npts - 1];
            const uint32_t cell = (cf < 2u ? cf : 2u) * 3u + (ct < 2u ? ct : 2u);
#pragma unroll
            for (uint32_t k = 0; k < 9; k++) m[MV_TRANS + k] += cell == k ? len : 0ull;
            m[MV_SAME] += (g | l) == 0 ? len : 0ull;
            m[MV_HANDED] += (cf == 1 && ct == 1 && g == 1 && l == 1) ? len : 0ull;
            const unsigned long long pk = (unsigned long long)(g + l) << 32 | (uint32_t)~i;
            best = g + l != 0 && pk > best ? pk : best;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k <= MV_HANDED; k++)
        if (m[k]) atomicAdd(&bm[k], m[k]);
    if (best) atomicMax(&bmax, best);
    __syncthreads();
    if (threadIdx.x <= MV_HANDED && bm[threadIdx.x]) atomicAdd(&A.out[threadIdx.x], bm[threadIdx.x]);
    if (threadIdx.x == MV_HANDED + 1 && bmax) atomicMax(&A.out[MV_MAXT], bmax);
}

static unsigned blocks_for(uint64_t items, unsigned per_block, unsigned cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace rp

// =====================================================================
// Host side (on the first shard's stream, like a route).
// =====================================================================
using rp::DevBuf;
using rp::Error;
using rp::Shard;

// (after route_prepare(false): the pointer table and the directory exist)
rp::OwnArgs rp_sim::own_args() {
    Shard& s0 = *sh.front();
    rp::OwnArgs A{};
    A.tab = route_tab.p;
    A.dead = own_dead.p;
    A.pt_hash = s0.pt_hash.p; A.pt_server = s0.pt_server.p; A.pt_coll = s0.pt_coll.p;
    A.dir = route_dir.p;
    A.srv_pt = own_srv_pt.p;
    A.n = n; A.nl = s0.nl; A.ncoll = s0.ncoll; A.npts = s0.npts; A.dir_shift = route_dir_shift;
    A.ntiles = (s0.npts + rp::OWN_TILE - 1) / rp::OWN_TILE;
    A.diff = own_diff.p; A.claims = own_claims.p; A.tile_sum = own_tile.p;
    A.claimed = own_claimed.p; A.out = own_out.p;
    return A;
}

// What the census and a comparison need beside the routing tables: the
// shards' dead arrays and the server -> point index.
void rp_sim::own_prepare() {
    route_prepare(false);
    Shard& s0 = *sh.front();
    if (!own_dead.p) {
        std::vector<const uint8_t*> h;
        for (auto& s : sh) h.push_back(s->dead.p);
        own_dead.alloc(h.size());
        RP_HIP(hipMemcpy(own_dead.p, h.data(), h.size() * sizeof h[0], hipMemcpyHostToDevice));
    }
    if (!own_srv_pt.p) {
        // every server's replica hashes as the constructor made them, each
        // row sorted: the device search turns them into point indices
        std::string blob;
        std::vector<uint64_t> off{0};
        for (const std::string& a : s0.addrs) { blob += a; off.push_back(blob.size()); }
        std::vector<uint32_t> rep;
        rp::device_replica_hashes(blob, off, rp::REPLICAS, rep, s0.st);
        if (cfg.replica_hash_shift)
            for (auto& h : rep) h = (h >> cfg.replica_hash_shift) << cfg.replica_hash_shift;
        for (size_t sv = 0; sv < n; sv++) std::sort(rep.begin() + sv * rp::REPLICAS, rep.begin() + (sv + 1) * rp::REPLICAS);
        DevBuf<uint32_t> dh(rep.size()), idx(rep.size());
        RP_HIP(hipMemcpyAsync(dh.p, rep.data(), rep.size() * 4, hipMemcpyHostToDevice, s0.st));
        hipLaunchKernelGGL(rp::k_own_point_index, dim3(rp::blocks_for(rep.size(), 256, 16384)), dim3(256), 0, s0.st,
                           own_args(), (const uint32_t*)dh.p, idx.p);
        RP_HIP(hipGetLastError());
        RP_HIP(hipStreamSynchronize(s0.st));
        // (kept only once it is complete; the census is stale already: the
        // index is dropped only where the rings changed, rp_sim_load_addresses)
        own_srv_pt = std::move(idx);
        own_gen++;  // (other points than any snapshot taken so far may index)
    }
}

// The census, unless no call that can change a ring ran since the last one
// (timed as "other", like a route).  Runs on the first shard's stream.
// record: the arcs are wanted too (§15) -- a cached census that did not
// record them runs again, with the recording kernel.
void rp_sim::own_refresh(bool record) {
    own_prepare();
    Shard& s0 = *sh.front();
    const uint32_t npts = s0.npts;
    if (!own_stale && own_claims.n == npts && own_claimed.n == n && (!record || own_arcs_valid)) return;
    own_arcs_valid = false;
    if (record) {
        if (own_arc_n.n != n) own_arc_n.alloc(n);
        if (own_arcs.n != (size_t)n * rp::OWN_REPLICAS) own_arcs.alloc((size_t)n * rp::OWN_REPLICAS);
    }
    if (own_diff.n != (size_t)npts + 1) own_diff.alloc((size_t)npts + 1);
    if (own_claims.n != npts) own_claims.alloc(npts);
    if (own_claimed.n != n) own_claimed.alloc(n);
    if (!own_out.p) own_out.alloc(rp::OWN_NOUT);
    const uint32_t ntiles = (npts + rp::OWN_TILE - 1) / rp::OWN_TILE;
    if (own_tile.n != ntiles) own_tile.alloc(ntiles);
    const rp::OwnArgs A = own_args();
    s0.timed(5, [&] {
        RP_HIP(hipMemsetAsync(own_diff.p, 0, own_diff.bytes(), s0.st));
        RP_HIP(hipMemsetAsync(own_out.p, 0, own_out.bytes(), s0.st));
        // (diff and out are zero; A.ntiles = ceil(npts / OWN_TILE))
        const unsigned per = rp::OWN_BLOCK / 64;  // views (waves) per block
        if (record)
            hipLaunchKernelGGL(rp::k_own_arcs<true>, dim3((n + per - 1) / per), dim3(rp::OWN_BLOCK), 0, s0.st, A,
                               own_arc_n.p, own_arcs.p);
        else
            hipLaunchKernelGGL(rp::k_own_arcs<false>, dim3((n + per - 1) / per), dim3(rp::OWN_BLOCK), 0, s0.st, A,
                               (uint32_t*)nullptr, (uint2*)nullptr);
        hipLaunchKernelGGL(rp::k_own_tile_sums, dim3(ntiles), dim3(rp::OWN_BLOCK), 0, s0.st, A);
        hipLaunchKernelGGL(rp::k_own_tile_scan, dim3(1), dim3(64), 0, s0.st, A);
        hipLaunchKernelGGL(rp::k_own_finish, dim3(ntiles), dim3(rp::OWN_BLOCK), 0, s0.st, A);
    });
    RP_HIP(hipGetLastError());
    unsigned long long h[rp::OWN_NOUT];
    RP_HIP(hipMemcpyAsync(h, own_out.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
    RP_HIP(hipStreamSynchronize(s0.st));
    rp_ownership_stats st{};
    for (int k = 0; k < 8; k++) st.measure[k] = h[rp::OWN_MEASURE + k];
    st.claimants = h[rp::OWN_CLAIMANTS];
    st.intervals = npts;
    st.max_claims = h[rp::OWN_MAX] >> 32;
    const uint32_t first = ~(uint32_t)h[rp::OWN_MAX];
    uint32_t hash = 0;
    if (first < npts) RP_HIP(hipMemcpy(&hash, s0.pt_hash.p + first, 4, hipMemcpyDeviceToHost));
    st.max_claims_hash = hash;
    own_stats = st;
    own_stale = false;
    own_arcs_valid = record;
}

extern "C" {

int rp_sim_ownership(rp_sim* c, rp_ownership_stats* stats, uint64_t* claimed, size_t cap) {
    return rp::guarded([&] {
        if (!c || !stats) throw Error(RP_ERR_INVALID, "null pointer");
        if (claimed && cap < c->n) throw Error(RP_ERR_INVALID, "claimed buffer holds fewer than n entries");
        c->own_refresh();
        static_assert(sizeof(rp_ownership_stats) == 128, "rp_ownership_stats is 16 x u64");
        *stats = c->own_stats;
        if (claimed) RP_HIP(hipMemcpy(claimed, c->own_claimed.p, (size_t)c->n * 8, hipMemcpyDeviceToHost));
    });
}

int rp_sim_ownership_at(rp_sim* c, const uint32_t* key_hashes, size_t nk, uint32_t* claims) {
    return rp::guarded([&] {
        if (!c || (nk && (!key_hashes || !claims))) throw Error(RP_ERR_INVALID, "null pointer");
        c->own_refresh();
        if (nk == 0) return;
        Shard& s0 = *c->sh.front();
        const rp::OwnArgs A = c->own_args();
        // (launches of at most 2^30 keys: a thread's index is 32-bit)
        const size_t chunk = std::min<size_t>(nk, (size_t)1 << 30);
        DevBuf<uint32_t> dh(chunk), dc(chunk);
        for (size_t first = 0; first < nk; first += chunk) {
            const size_t m = std::min(nk - first, chunk);
            RP_HIP(hipMemcpyAsync(dh.p, key_hashes + first, m * 4, hipMemcpyHostToDevice, s0.st));
            s0.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_own_at, dim3(rp::blocks_for(m, 256, 16384)), dim3(256), 0, s0.st, A,
                                   (const uint32_t*)dh.p, (uint32_t)m, dc.p);
            });
            RP_HIP(hipGetLastError());
            RP_HIP(hipMemcpyAsync(claims + first, dc.p, m * 4, hipMemcpyDeviceToHost, s0.st));
            RP_HIP(hipStreamSynchronize(s0.st));
        }
    });
}

}  // extern "C"

// ---- ownership movement

// Every node's recorded arcs and the census' claims at one clock, in device
// buffers of its own: it outlives its simulation, which it names by id.
struct rp_ownership_snapshot {
    uint64_t sim_id = 0, gen = 0, clock = 0;
    int dev = 0;
    uint32_t n = 0, npts = 0;
    DevBuf<uint32_t> arc_n, claims;
    DevBuf<uint2> arcs;
    rp_ownership_stats stats{};
};

namespace {

std::atomic<uint64_t> g_snapshot_sims{0};

void check_snapshot(const rp_sim* c, const rp_ownership_snapshot* s, const char* which) {
    if (s->sim_id != c->own_id) throw Error(RP_ERR_INVALID, std::string(which) + ": a snapshot of another simulation");
    if (s->gen != c->own_gen || s->n != c->n || s->npts != c->sh.front()->npts)
        throw Error(RP_ERR_STATE, std::string(which) + ": the snapshot was taken before rp_sim_load_addresses changed the points");
}

}  // namespace

extern "C" {

int rp_ownership_snapshot_create(rp_sim* c, rp_ownership_snapshot** out) {
    return rp::guarded([&] {
        if (!c || !out) throw Error(RP_ERR_INVALID, "null pointer");
        *out = nullptr;
        c->own_refresh(true);
        if (!c->own_id) c->own_id = ++g_snapshot_sims;
        Shard& s0 = *c->sh.front();
        std::unique_ptr<rp_ownership_snapshot> s(new rp_ownership_snapshot());
        s->sim_id = c->own_id; s->gen = c->own_gen; s->clock = c->round;
        s->dev = c->dev; s->n = c->n; s->npts = s0.npts;
        s->stats = c->own_stats;
        s->arc_n.alloc(c->own_arc_n.n);
        s->arcs.alloc(c->own_arcs.n);
        s->claims.alloc(c->own_claims.n);
        s0.timed(5, [&] {
            RP_HIP(hipMemcpyAsync(s->arc_n.p, c->own_arc_n.p, s->arc_n.bytes(), hipMemcpyDeviceToDevice, s0.st));
            RP_HIP(hipMemcpyAsync(s->arcs.p, c->own_arcs.p, s->arcs.bytes(), hipMemcpyDeviceToDevice, s0.st));
            RP_HIP(hipMemcpyAsync(s->claims.p, c->own_claims.p, s->claims.bytes(), hipMemcpyDeviceToDevice, s0.st));
        });
        RP_HIP(hipStreamSynchronize(s0.st));
        *out = s.release();
    });
}

int rp_ownership_snapshot_info(const rp_ownership_snapshot* s, rp_ownership_stats* stats, uint64_t* clock) {
    return rp::guarded([&] {
        if (!s) throw Error(RP_ERR_INVALID, "null pointer");
        if (stats) *stats = s->stats;
        if (clock) *clock = s->clock;
    });
}

int rp_ownership_snapshot_destroy(rp_ownership_snapshot* s) {
    return rp::guarded([&] {
        if (!s) return;
        (void)hipSetDevice(s->dev);
        delete s;
    });
}

int rp_sim_ownership_moved(rp_sim* c, const rp_ownership_snapshot* from, const rp_ownership_snapshot* to,
                           rp_movement_stats* stats, uint64_t* gained, uint64_t* lost, size_t cap) {
    return rp::guarded([&] {
        static_assert(sizeof(rp_movement_stats) == 256, "rp_movement_stats is 32 x u64");
        if (!c || !stats) throw Error(RP_ERR_INVALID, "null pointer");
        // (a rank holds its own nodes' views only: unsupported, whatever else is passed)
        c->own_prepare();
        if (!from) throw Error(RP_ERR_INVALID, "null pointer");
        if ((gained || lost) && cap < c->n) throw Error(RP_ERR_INVALID, "gained / lost buffer holds fewer than n entries");
        // (own_prepare rebuilt the point index if the points changed: a stale
        // snapshot's generation differs, and no kernel sees its indices)
        check_snapshot(c, from, "from");
        if (to) check_snapshot(c, to, "to");
        else c->own_refresh(true);
        Shard& s0 = *c->sh.front();
        const uint32_t n = c->n, npts = s0.npts;
        const uint32_t ntiles = (npts + rp::OWN_TILE - 1) / rp::OWN_TILE;
        if (c->mv_diff.n != 2 * ((size_t)npts + 1)) c->mv_diff.alloc(2 * ((size_t)npts + 1));
        if (c->mv_tile.n != 2 * (size_t)ntiles) c->mv_tile.alloc(2 * (size_t)ntiles);
        if (c->mv_gained.n != n) c->mv_gained.alloc(n);
        if (c->mv_lost.n != n) c->mv_lost.alloc(n);
        if (!c->mv_out.p) c->mv_out.alloc(rp::MV_NOUT);
        rp::MoveArgs A{};
        A.arc_n[0] = from->arc_n.p; A.arcs[0] = from->arcs.p; A.claims[0] = from->claims.p;
        A.arc_n[1] = to ? to->arc_n.p : c->own_arc_n.p;
        A.arcs[1] = to ? to->arcs.p : c->own_arcs.p;
        A.claims[1] = to ? to->claims.p : c->own_claims.p;
        A.pt_hash = s0.pt_hash.p;
        A.n = n; A.npts = npts; A.ntiles = ntiles;
        A.diff = c->mv_diff.p; A.tile_sum = c->mv_tile.p;
        A.gained = c->mv_gained.p; A.lost = c->mv_lost.p; A.out = c->mv_out.p;
        s0.timed(5, [&] {
            RP_HIP(hipMemsetAsync(c->mv_diff.p, 0, c->mv_diff.bytes(), s0.st));
            RP_HIP(hipMemsetAsync(c->mv_out.p, 0, c->mv_out.bytes(), s0.st));
            hipLaunchKernelGGL(rp::k_move_arcs, dim3((n + rp::MV_WAVES - 1) / rp::MV_WAVES), dim3(rp::OWN_BLOCK), 0, s0.st, A);
            hipLaunchKernelGGL(rp::k_move_tile_sums, dim3(ntiles, 2), dim3(rp::OWN_BLOCK), 0, s0.st, A);
            hipLaunchKernelGGL(rp::k_move_tile_scan, dim3(2), dim3(64), 0, s0.st, A);
            hipLaunchKernelGGL(rp::k_move_finish, dim3(ntiles), dim3(rp::OWN_BLOCK), 0, s0.st, A);
        });
        RP_HIP(hipGetLastError());
        unsigned long long h[rp::MV_NOUT];
        RP_HIP(hipMemcpyAsync(h, c->mv_out.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
        if (gained) RP_HIP(hipMemcpyAsync(gained, c->mv_gained.p, (size_t)n * 8, hipMemcpyDeviceToHost, s0.st));
        if (lost) RP_HIP(hipMemcpyAsync(lost, c->mv_lost.p, (size_t)n * 8, hipMemcpyDeviceToHost, s0.st));
        RP_HIP(hipStreamSynchronize(s0.st));
        rp_movement_stats st{};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) st.transition[a][b] = h[rp::MV_TRANS + 3 * a + b];
        st.same_set = h[rp::MV_SAME]; st.handed_off = h[rp::MV_HANDED];
        st.gained = h[rp::MV_GAINED]; st.lost = h[rp::MV_LOST];
        st.gainers = h[rp::MV_GAINERS]; st.losers = h[rp::MV_LOSERS];
        // (a packed maximum is 0 when nothing moved: node 0, hash 0)
        st.max_gained = h[rp::MV_MAXG] >> 31;
        st.max_gained_node = h[rp::MV_MAXG] ? rp::MV_NODE_MASK - (h[rp::MV_MAXG] & rp::MV_NODE_MASK) : 0;
        st.max_lost = h[rp::MV_MAXL] >> 31;
        st.max_lost_node = h[rp::MV_MAXL] ? rp::MV_NODE_MASK - (h[rp::MV_MAXL] & rp::MV_NODE_MASK) : 0;
        st.max_turnover = h[rp::MV_MAXT] >> 32;
        uint32_t hash = 0;
        if (h[rp::MV_MAXT]) {
            const uint32_t first = ~(uint32_t)h[rp::MV_MAXT];
            if (first < npts) RP_HIP(hipMemcpy(&hash, s0.pt_hash.p + first, 4, hipMemcpyDeviceToHost));
        }
        st.max_turnover_hash = hash;
        st.from_clock = from->clock;
        st.to_clock = to ? to->clock : c->round;
        st.intervals = npts;
        *stats = st;
    });
}

}  // extern "C"
