// ringpop_amd — the kernels of the ownership census (rp_sim_ownership /
// rp_sim_ownership_at) and their launches.  None of them is
// launched by a round.  Every store is a vector store or an integer atomic,
// and the phases are separate kernels: no block waits for another.
#include <hip/hip_runtime.h>

#include "rp_own.h"

namespace rp {

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
__global__ void __launch_bounds__(OWN_BLOCK) k_own_arcs(OwnArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t v = blockIdx.x * (OWN_BLOCK / 64) + (threadIdx.x >> 6);
    if (v >= A.n) return;  // (the whole wave)
    const uint32_t g = v / A.nl;
    if (A.dead[g][v] != 0) {  // fail-stopped, or not joined yet: no claimant
        if (lane == 0) A.claimed[v] = 0;
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
        }
        return;
    }
    const uint32_t* row = A.srv_pt + (size_t)v * OWN_REPLICAS;
    unsigned long long total = 0;
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
    }
    total = wave_sum_u64(total);
    if (lane == 0) A.claimed[v] = total;
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

static unsigned blocks_for(uint64_t items, unsigned per_block, unsigned cap) {
    const uint64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > cap ? cap : g);
}

void own_point_index(hipStream_t st, const OwnArgs& A, const uint32_t* rep_hash, uint32_t* srv_pt) {
    hipLaunchKernelGGL(k_own_point_index, dim3(blocks_for((uint64_t)A.n * OWN_REPLICAS, 256, 16384)), dim3(256), 0, st, A,
                       rep_hash, srv_pt);
}

// diff and out are zero; A.ntiles = ceil(npts / OWN_TILE)
void own_census(hipStream_t st, const OwnArgs& A) {
    hipLaunchKernelGGL(k_own_arcs, dim3((A.n + OWN_BLOCK / 64 - 1) / (OWN_BLOCK / 64)), dim3(OWN_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_own_tile_sums, dim3(A.ntiles), dim3(OWN_BLOCK), 0, st, A);
    hipLaunchKernelGGL(k_own_tile_scan, dim3(1), dim3(64), 0, st, A);
    hipLaunchKernelGGL(k_own_finish, dim3(A.ntiles), dim3(OWN_BLOCK), 0, st, A);
}

void own_at(hipStream_t st, const OwnArgs& A, const uint32_t* keys, uint32_t nk, uint32_t* claims_out) {
    hipLaunchKernelGGL(k_own_at, dim3(blocks_for(nk, 256, 16384)), dim3(256), 0, st, A, keys, nk, claims_out);
}

}  // namespace rp
