// ringpop_amd — the membership census (rp_sim_membership): how
// every live node sees each member.  The views are a node-major N x N matrix
// of 16-byte cells (VEnt); the census is a column reduction of it -- per
// member the five status counts, the newest packed value vs = inc << 3 |
// status any viewer holds and how many viewers hold exactly that -- followed
// by a row pass against the result: per viewer, the members whose cell is not
// the newest.  Three phases, each a launch of its own, none launched by a
// round: k_mem_columns (a tile of columns x a slab of rows -> one 32-byte
// partial per slab and column), k_mem_combine (the slabs' partials of every
// shard, in slab order), k_mem_rows (one wave per viewer row, top[] staged in
// LDS), and k_mem_finish, one wave over the blocks' records.  Integers only,
// every store a vector store, no atomic: in-process shards give the one-shard
// result bit for bit.  A max / count reduction of 64-bit integers has no use
// for the matrix units.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rp_own.h"

namespace rp {

constexpr uint32_t MEM_BLOCK = 256;       // threads of every block here; the column pass: one column each (four 1 KB wave segments a row)
constexpr uint32_t MEM_WAVES = MEM_BLOCK / 64;
constexpr uint32_t MEM_UNROLL = 8;        // independent row loads a lane keeps in flight
constexpr uint32_t MEM_MAX_SLABS = 64;    // slabs of one shard's rows, at the most
constexpr uint32_t MEM_SLAB_DIV = 512;    // ... and n / (MEM_SLAB_DIV x shards): the partials stay below 2 / 512 of the matrix
constexpr uint32_t MEM_ONE_SLAB = 64;     // a shard of more rows than this gets at least two slabs
constexpr uint32_t MEM_ROW_TILE = 2048;   // members whose top[] a row block stages in LDS at a time (16 KB)
constexpr uint32_t MEM_ROWS_PER_WAVE = 4;
constexpr uint32_t MEM_ROWS = MEM_WAVES * MEM_ROWS_PER_WAVE;  // rows of a row-pass block
constexpr uint32_t MEM_STEP = 64 * MEM_UNROLL;                // cells of a row a wave takes per unrolled step

// a (slab, column) partial, and the fold's operand
struct alignas(16) MemPart {
    unsigned long long top;  // the largest vs among the slab's viewer rows (0: none, or nobody knows the member)
    uint32_t at_top;         // viewer rows whose cell equals it
    uint32_t seen[5];        // viewer rows by status
};
static_assert(sizeof(MemPart) == 32, "a column partial is 32 bytes");

// block records: the member side (k_mem_combine) and the viewer side (k_mem_rows)
enum : uint32_t { MR_AGREED = 0, MR_CELLS, MR_MAX, MR_UNDETECTED, MR_SUSPECTED_DEAD, MR_FALSE_FAULTY, MR_FALSE_SUSPECT,
                  MR_UNKNOWN, MR_N };
enum : uint32_t { VR_LAGGARDS = 0, VR_MAX, VR_N };
// rp_membership_stats, in words
enum : uint32_t { MS_VIEWERS = 0, MS_MEMBERS, MS_AGREED, MS_CELLS, MS_MAXM, MS_MAXM_ID, MS_LAGGARDS, MS_MAXV, MS_MAXV_ID,
                  MS_UNDETECTED, MS_SUSPECTED_DEAD, MS_FALSE_FAULTY, MS_FALSE_SUSPECT, MS_UNKNOWN, MS_N = 16 };

// "the largest value, and the first id that reaches it" as one 64-bit maximum
__device__ inline unsigned long long mem_pack(uint32_t value, uint32_t id) {
    return (unsigned long long)value << 32 | (0xFFFFFFFFu - id);
}

__device__ inline unsigned long long wave_max_u64(unsigned long long x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_down(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// one viewer's cell into a column's running state.  The whole 64-bit value is
// compared: two cells may differ in the status bits alone, or above bit 32 alone.
__device__ inline void mem_take(MemPart& p, unsigned long long x) {
    const uint32_t s = (uint32_t)x & 7u;
#pragma unroll
    for (uint32_t k = 0; k < 5; k++) p.seen[k] += s == k;
    if (x > p.top) {
        p.top = x;
        p.at_top = 1;
    } else {
        p.at_top += x == p.top;
    }
}

// The column pass over one shard: block (tile, slab) owns the 256 consecutive
// members from tile * 256 -- thread t column tile * 256 + t, so a wave's load
// of a row is 64 consecutive cells, 1 KB -- and the shard's local rows [slab *
// slab_h, min(nl, (slab + 1) * slab_h)).  A lane reads the cell's 8-byte vs at
// stride 16, not the cell: the census uses nothing of dpos and tstamp, the HBM
// lines moved are the same, and the 8-byte load returns half the bytes through
// the vector L1 and holds two registers in flight where the 16-byte one holds
// four -- eight of them outstanding cost 16 registers, not 32.  The rows'
// `dead` bytes are read 64 at a time, one per lane, and balloted: the mask is
// in scalar registers, a group of eight viewer rows is eight loads issued back
// to back before the first is used (their only dependence is through the
// accumulators), and a group with a non-viewer row branches round that row's
// load on the scalar unit.  A column past n (the ragged last tile) reads
// column n - 1 and stores nothing.
__global__ void __launch_bounds__(MEM_BLOCK) k_mem_columns(const VEnt* __restrict__ view, const uint8_t* __restrict__ dead,
                                                           uint32_t n, uint32_t lo, uint32_t nl, uint32_t slab_h,
                                                           MemPart* __restrict__ part) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t col = blockIdx.x * MEM_BLOCK + threadIdx.x;
    const uint32_t r0 = blockIdx.y * slab_h;  // (< nl: the host's grid)
    const uint32_t r1 = nl - r0 < slab_h ? nl : r0 + slab_h;
    const VEnt* cell = view + (col < n ? col : n - 1);
    MemPart p{};
    for (uint32_t rb = r0; rb < r1; rb += 64) {
        const uint32_t r = rb + lane;
        const unsigned long long live = __ballot(r < r1 && dead[lo + r] == 0);  // (bit j: row rb + j is a viewer's)
        for (uint32_t g = 0; g < 64; g += MEM_UNROLL) {
            const uint32_t bits = (uint32_t)(live >> g) & ((1u << MEM_UNROLL) - 1u);
            if (bits == 0) continue;
            const VEnt* row = cell + (size_t)(rb + g) * n;
            unsigned long long x[MEM_UNROLL];
            if (bits == (1u << MEM_UNROLL) - 1u) {
#pragma unroll
                for (uint32_t k = 0; k < MEM_UNROLL; k++) x[k] = row[(size_t)k * n].vs;
#pragma unroll
                for (uint32_t k = 0; k < MEM_UNROLL; k++) mem_take(p, x[k]);
            } else {
                // (a non-viewer row's slot reads the group's first viewer row again: a line the wave has asked
                // for already, and all eight loads still issue before the first use)
                const uint32_t first = (uint32_t)__ffs((int)bits) - 1u;
#pragma unroll
                for (uint32_t k = 0; k < MEM_UNROLL; k++) x[k] = row[(size_t)(bits >> k & 1u ? k : first) * n].vs;
#pragma unroll
                for (uint32_t k = 0; k < MEM_UNROLL; k++)
                    if (bits >> k & 1u) mem_take(p, x[k]);
            }
        }
    }
    if (col < n) {
        uint4* out = reinterpret_cast<uint4*>(part + (size_t)blockIdx.y * n + col);
        out[0] = make_uint4((uint32_t)p.top, (uint32_t)(p.top >> 32), p.at_top, p.seen[0]);
        out[1] = make_uint4(p.seen[1], p.seen[2], p.seen[3], p.seen[4]);
    }
}

// a block's record: every wave's reduced words through LDS, one store a word
template <uint32_t NW>
__device__ inline void mem_block_record(unsigned long long (&mine)[NW], uint32_t max_word, unsigned long long* __restrict__ rec) {
    __shared__ unsigned long long wsum[MEM_WAVES][NW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < NW; k++) {
        const unsigned long long x = k == max_word ? wave_max_u64(mine[k]) : wave_sum_u64(mine[k]);
        if (lane == 0) wsum[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < NW) {
        unsigned long long x = wsum[0][threadIdx.x];
        for (uint32_t w = 1; w < MEM_WAVES; w++) {
            const unsigned long long y = wsum[w][threadIdx.x];
            x = threadIdx.x == max_word ? (y > x ? y : x) : x + y;
        }
        rec[(size_t)blockIdx.x * NW + threadIdx.x] = x;
    }
}

// Combine: one thread per member folds its column's partials of every slab of
// every shard, in ascending slab order -- the larger top wins, equal tops add
// their counts; associative, so the order changes nothing, and fixed anyway --
// and stores seen, top, at_top.  The member's share of the stats goes through
// a wave reduction into the block's record.
__global__ void __launch_bounds__(MEM_BLOCK) k_mem_combine(const MemPart* __restrict__ part, uint32_t nslabs,
                                                           const uint8_t* const* __restrict__ dead, uint32_t n, uint32_t nl,
                                                           uint32_t* __restrict__ seen, unsigned long long* __restrict__ top,
                                                           uint32_t* __restrict__ at_top, unsigned long long* __restrict__ rec) {
    const uint32_t a = blockIdx.x * MEM_BLOCK + threadIdx.x;
    unsigned long long w[MR_N] = {};
    if (a < n) {
        MemPart p{};
        for (uint32_t s = 0; s < nslabs; s++) {
            const uint4* in = reinterpret_cast<const uint4*>(part + (size_t)s * n + a);
            const uint4 q0 = in[0], q1 = in[1];
            const unsigned long long t = (unsigned long long)q0.y << 32 | q0.x;
            if (t > p.top) {
                p.top = t;
                p.at_top = q0.z;
            } else if (t == p.top) {
                p.at_top += q0.z;
            }
            p.seen[0] += q0.w; p.seen[1] += q1.x; p.seen[2] += q1.y; p.seen[3] += q1.z; p.seen[4] += q1.w;
        }
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) seen[(size_t)a * 5 + k] = p.seen[k];
        top[a] = p.top;
        at_top[a] = p.at_top;
        const uint32_t viewers = p.seen[0] + p.seen[1] + p.seen[2] + p.seen[3] + p.seen[4];
        const uint32_t lag = viewers - p.at_top;
        const uint8_t d = dead[a / nl][a];
        w[MR_AGREED] = lag == 0;
        w[MR_CELLS] = lag;
        w[MR_MAX] = mem_pack(lag, a);
        w[MR_UNDETECTED] = d == 1 ? p.seen[1] : 0;
        w[MR_SUSPECTED_DEAD] = d == 1 ? p.seen[2] : 0;
        w[MR_FALSE_FAULTY] = d == 0 ? p.seen[3] : 0;
        w[MR_FALSE_SUSPECT] = d == 0 ? p.seen[2] : 0;
        w[MR_UNKNOWN] = d == 0 ? p.seen[0] : 0;
    }
    mem_block_record<MR_N>(w, MR_MAX, rec);
}

// The row pass over one shard: a block owns MEM_ROWS consecutive local rows,
// a wave four of them.  top[] is walked in tiles of MEM_ROW_TILE members, each
// staged in LDS once for all the block's rows (from L2: 8 n bytes in all), so
// that the matrix rows are the only stream to HBM; a wave takes a viewer row's
// part of the tile 64 cells a load, eight loads in flight, compares the whole
// 64-bit values and counts vs != top with a ballot.  A non-viewer row is not
// read: its behind is 0.
__global__ void __launch_bounds__(MEM_BLOCK) k_mem_rows(const VEnt* __restrict__ view, const uint8_t* __restrict__ dead,
                                                        const unsigned long long* __restrict__ top, uint32_t n, uint32_t lo,
                                                        uint32_t nl, uint32_t* __restrict__ behind,
                                                        unsigned long long* __restrict__ rec) {
    __shared__ unsigned long long stop[MEM_ROW_TILE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t rw = blockIdx.x * MEM_ROWS + wave * MEM_ROWS_PER_WAVE;  // the wave's first local row
    bool viewer[MEM_ROWS_PER_WAVE];
    uint32_t cnt[MEM_ROWS_PER_WAVE];
#pragma unroll
    for (uint32_t j = 0; j < MEM_ROWS_PER_WAVE; j++) {
        viewer[j] = rw + j < nl && __builtin_amdgcn_readfirstlane((int)dead[lo + (rw + j < nl ? rw + j : 0)]) == 0;
        cnt[j] = 0;
    }
    for (uint32_t t0 = 0; t0 < n; t0 += MEM_ROW_TILE) {
        const uint32_t m = n - t0 < MEM_ROW_TILE ? n - t0 : MEM_ROW_TILE;
        if (t0) __syncthreads();  // (every wave is done with the tile before)
        for (uint32_t i = threadIdx.x; i < m; i += MEM_BLOCK) stop[i] = top[t0 + i];
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < MEM_ROWS_PER_WAVE; j++) {
            if (!viewer[j]) continue;  // (the whole wave)
            const VEnt* row = view + (size_t)(rw + j) * n + t0;
            uint32_t i0 = 0;
            for (; i0 + MEM_STEP <= m; i0 += MEM_STEP) {
                unsigned long long x[MEM_UNROLL];
#pragma unroll
                for (uint32_t k = 0; k < MEM_UNROLL; k++) x[k] = row[i0 + 64 * k + lane].vs;
#pragma unroll
                for (uint32_t k = 0; k < MEM_UNROLL; k++) cnt[j] += __popcll(__ballot(x[k] != stop[i0 + 64 * k + lane]));
            }
            for (; i0 < m; i0 += 64) {  // the ragged end of the last tile
                const uint32_t i = i0 + lane;
                cnt[j] += __popcll(__ballot(i < m && row[i < m ? i : 0].vs != stop[i < m ? i : 0]));
            }
        }
    }
    unsigned long long w[VR_N] = {0, 0};
    if (lane == 0) {
#pragma unroll
        for (uint32_t j = 0; j < MEM_ROWS_PER_WAVE; j++) {
            if (rw + j >= nl) continue;
            behind[lo + rw + j] = cnt[j];
            w[VR_LAGGARDS] += cnt[j] != 0;
            const unsigned long long pk = mem_pack(cnt[j], lo + rw + j);
            w[VR_MAX] = pk > w[VR_MAX] ? pk : w[VR_MAX];
        }
    }
    mem_block_record<VR_N>(w, VR_MAX, rec);
}

// One wave folds the blocks' records of both sides into rp_membership_stats'
// sixteen words: sums, and the two packed maxima -- the largest value, at the
// smallest id.  viewers is any column's sum of seen.
__global__ void __launch_bounds__(64) k_mem_finish(const unsigned long long* __restrict__ mrec, uint32_t nm,
                                                   const unsigned long long* __restrict__ vrec, uint32_t nv,
                                                   const uint32_t* __restrict__ seen, uint32_t n,
                                                   unsigned long long* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    unsigned long long m[MR_N] = {}, v[VR_N] = {};
    for (uint32_t b = lane; b < nm; b += 64) {
#pragma unroll
        for (uint32_t k = 0; k < MR_N; k++) {
            const unsigned long long x = mrec[(size_t)b * MR_N + k];
            m[k] = k == MR_MAX ? (x > m[k] ? x : m[k]) : m[k] + x;
        }
    }
    for (uint32_t b = lane; b < nv; b += 64) {
#pragma unroll
        for (uint32_t k = 0; k < VR_N; k++) {
            const unsigned long long x = vrec[(size_t)b * VR_N + k];
            v[k] = k == VR_MAX ? (x > v[k] ? x : v[k]) : v[k] + x;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < MR_N; k++) m[k] = k == MR_MAX ? wave_max_u64(m[k]) : wave_sum_u64(m[k]);
#pragma unroll
    for (uint32_t k = 0; k < VR_N; k++) v[k] = k == VR_MAX ? wave_max_u64(v[k]) : wave_sum_u64(v[k]);
    if (lane != 0) return;
    out[MS_VIEWERS] = (unsigned long long)seen[0] + seen[1] + seen[2] + seen[3] + seen[4];
    out[MS_MEMBERS] = n;
    out[MS_AGREED] = m[MR_AGREED];
    out[MS_CELLS] = m[MR_CELLS];
    out[MS_MAXM] = m[MR_MAX] >> 32;
    out[MS_MAXM_ID] = 0xFFFFFFFFu - (uint32_t)m[MR_MAX];
    out[MS_LAGGARDS] = v[VR_LAGGARDS];
    out[MS_MAXV] = v[VR_MAX] >> 32;
    out[MS_MAXV_ID] = 0xFFFFFFFFu - (uint32_t)v[VR_MAX];
    out[MS_UNDETECTED] = m[MR_UNDETECTED];
    out[MS_SUSPECTED_DEAD] = m[MR_SUSPECTED_DEAD];
    out[MS_FALSE_FAULTY] = m[MR_FALSE_FAULTY];
    out[MS_FALSE_SUSPECT] = m[MR_FALSE_SUSPECT];
    out[MS_UNKNOWN] = m[MR_UNKNOWN];
    out[14] = 0;
    out[15] = 0;
}

// The slab rule: a shard's nl rows fall into min(64, n / (512 x shards)) slabs
// -- at least two once it has more than 64 rows, one below -- of equal height,
// the last one ragged.  Returns the height; the slabs are ceil(nl / height).
static uint32_t mem_slab_height(uint32_t n, uint32_t nl, uint32_t shards) {
    uint32_t slabs = std::min(MEM_MAX_SLABS, n / (MEM_SLAB_DIV * shards));
    slabs = std::max(slabs, nl > MEM_ONE_SLAB ? 2u : 1u);
    return (nl + slabs - 1) / slabs;
}

}  // namespace rp

// =====================================================================
// Host side: the column and row passes on each shard's own stream, the
// combine and the finish on the first shard's, like the censuses.
// =====================================================================
using rp::Error;
using rp::Shard;

extern "C" {

int rp_sim_membership(rp_sim* c, rp_membership_stats* stats, uint32_t* seen, uint64_t* top, uint32_t* at_top,
                      uint32_t* behind, size_t cap) {
    return rp::guarded([&] {
        static_assert(sizeof(rp_membership_stats) == 8 * rp::MS_N, "rp_membership_stats is 16 x u64");
        const bool arrays = seen || top || at_top || behind;
        if (!c || (!stats && !arrays)) throw Error(RP_ERR_INVALID, "null pointer");
        if (arrays && cap < c->n) throw Error(RP_ERR_INVALID, "a per-node array holds fewer than n entries");
        // (a rank holds its own nodes' views only: unsupported.  The shards' dead arrays; every stream is drained;
        // no census and no ring checksum is read or touched)
        c->own_prepare();
        const uint32_t n = c->n;
        Shard& s0 = *c->sh.front();
        const bool many = c->sh.size() > 1;
        // the slabs of every shard, in shard order, and the row pass' blocks
        std::vector<uint32_t> height, slab0, rblock0;
        uint32_t nslabs = 0, nrblocks = 0;
        for (auto& s : c->sh) {
            height.push_back(rp::mem_slab_height(n, s->nl, (uint32_t)c->sh.size()));
            slab0.push_back(nslabs);
            rblock0.push_back(nrblocks);
            nslabs += (s->nl + height.back() - 1) / height.back();
            nrblocks += (s->nl + rp::MEM_ROWS - 1) / rp::MEM_ROWS;
        }
        const uint32_t tiles = (n + rp::MEM_BLOCK - 1) / rp::MEM_BLOCK;
        // scratch and results, on first use: partials (32 B x slabs x n), the blocks' records, then seen (5 n),
        // at_top (n) and behind (n) in one buffer, top, and the stats
        const size_t npart = (size_t)nslabs * n, nrec = (size_t)tiles * rp::MR_N + (size_t)nrblocks * rp::VR_N;
        if (c->mem_part.n != 2 * npart) c->mem_part.alloc(2 * npart);
        if (c->mem_rec.n != nrec) c->mem_rec.alloc(nrec);
        if (c->mem_cnt.n != 7 * (size_t)n) c->mem_cnt.alloc(7 * (size_t)n);
        if (c->mem_top.n != (size_t)n + rp::MS_N) c->mem_top.alloc((size_t)n + rp::MS_N);
        rp::MemPart* part = reinterpret_cast<rp::MemPart*>(c->mem_part.p);
        unsigned long long* mrec = c->mem_rec.p;
        unsigned long long* vrec = mrec + (size_t)tiles * rp::MR_N;
        uint32_t* d_seen = c->mem_cnt.p;
        uint32_t* d_at = d_seen + 5 * (size_t)n;
        uint32_t* d_behind = d_at + n;
        unsigned long long* d_top = c->mem_top.p;
        unsigned long long* d_out = d_top + n;
        const bool rows = stats || behind;  // (nobody asked for the viewer side: the matrix is read once)

        for (size_t g = 0; g < c->sh.size(); g++) {
            Shard& s = *c->sh[g];
            s.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_mem_columns, dim3(tiles, (s.nl + height[g] - 1) / height[g]), dim3(rp::MEM_BLOCK), 0,
                                   s.st, (const rp::VEnt*)s.view.p, (const uint8_t*)s.dead.p, n, s.lo, s.nl, height[g],
                                   part + (size_t)slab0[g] * n);
            });
            RP_HIP(hipGetLastError());
        }
        if (many) c->sync_all();  // (the combine reads every shard's partials from the first shard's stream)
        s0.timed(5, [&] {
            hipLaunchKernelGGL(rp::k_mem_combine, dim3(tiles), dim3(rp::MEM_BLOCK), 0, s0.st, (const rp::MemPart*)part, nslabs,
                               (const uint8_t* const*)c->own_dead.p, n, s0.nl, d_seen, d_top, d_at, mrec);
        });
        RP_HIP(hipGetLastError());
        if (rows) {
            if (many) RP_HIP(hipStreamSynchronize(s0.st));  // (top[] is complete before any shard's rows are compared)
            for (size_t g = 0; g < c->sh.size(); g++) {
                Shard& s = *c->sh[g];
                s.timed(5, [&] {
                    hipLaunchKernelGGL(rp::k_mem_rows, dim3((s.nl + rp::MEM_ROWS - 1) / rp::MEM_ROWS), dim3(rp::MEM_BLOCK), 0,
                                       s.st, (const rp::VEnt*)s.view.p, (const uint8_t*)s.dead.p,
                                       (const unsigned long long*)d_top, n, s.lo, s.nl, d_behind,
                                       vrec + (size_t)rblock0[g] * rp::VR_N);
                });
                RP_HIP(hipGetLastError());
            }
            if (many) c->sync_all();
            s0.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_mem_finish, dim3(1), dim3(64), 0, s0.st, (const unsigned long long*)mrec, tiles,
                                   (const unsigned long long*)vrec, nrblocks, (const uint32_t*)d_seen, n, d_out);
            });
            RP_HIP(hipGetLastError());
        }
        unsigned long long h[rp::MS_N];
        if (stats) RP_HIP(hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, s0.st));
        if (seen) RP_HIP(hipMemcpyAsync(seen, d_seen, (size_t)n * 20, hipMemcpyDeviceToHost, s0.st));
        if (top) RP_HIP(hipMemcpyAsync(top, d_top, (size_t)n * 8, hipMemcpyDeviceToHost, s0.st));
        if (at_top) RP_HIP(hipMemcpyAsync(at_top, d_at, (size_t)n * 4, hipMemcpyDeviceToHost, s0.st));
        if (behind) RP_HIP(hipMemcpyAsync(behind, d_behind, (size_t)n * 4, hipMemcpyDeviceToHost, s0.st));
        RP_HIP(hipStreamSynchronize(s0.st));
        if (stats) {
            const unsigned long long* w = h;
            rp_membership_stats st{};
            st.viewers = w[rp::MS_VIEWERS]; st.members = w[rp::MS_MEMBERS]; st.agreed = w[rp::MS_AGREED];
            st.cells_behind = w[rp::MS_CELLS];
            st.max_behind_member = w[rp::MS_MAXM]; st.max_behind_member_id = w[rp::MS_MAXM_ID];
            st.laggards = w[rp::MS_LAGGARDS];
            st.max_behind_viewer = w[rp::MS_MAXV]; st.max_behind_viewer_id = w[rp::MS_MAXV_ID];
            st.undetected = w[rp::MS_UNDETECTED]; st.suspected_dead = w[rp::MS_SUSPECTED_DEAD];
            st.false_faulty = w[rp::MS_FALSE_FAULTY]; st.false_suspect = w[rp::MS_FALSE_SUSPECT];
            st.unknown = w[rp::MS_UNKNOWN];
            *stats = st;
        }
    });
}

}  // extern "C"
