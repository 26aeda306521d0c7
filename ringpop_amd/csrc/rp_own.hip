// ringpop_amd — ownership census (rp_sim_ownership / rp_sim_ownership_at;
// DESIGN.md §13): for every interval between two ring points, how many live
// nodes claim it in their own view.  The kernels, the host side that launches
// them and the two entry points.  None of the kernels is launched by a round.
// Every store is a vector store or an integer atomic, and the phases are
// separate kernels: no block waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

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

// The census, unless no call that can change a ring ran since the last one
// (timed as "other", like a route).  Runs on the first shard's stream.
void rp_sim::own_refresh() {
    route_prepare(false);
    Shard& s0 = *sh.front();
    const uint32_t npts = s0.npts;
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
    }
    if (!own_stale && own_claims.n == npts && own_claimed.n == n) return;
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
        hipLaunchKernelGGL(rp::k_own_arcs, dim3((n + per - 1) / per), dim3(rp::OWN_BLOCK), 0, s0.st, A);
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
