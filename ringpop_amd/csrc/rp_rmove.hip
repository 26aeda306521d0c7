// ringpop_amd — replica-set movement between two instants
// (rp_replication_snapshot_* / rp_sim_replication_moved /
// rp_sim_replication_moved_at): which replicas changed hands.
// A snapshot keeps the arcs the replica census records at its R
// (k_rep_arcs<true>, rp_repl.hip): per node at most 100 disjoint arcs, each
// ending at an own point, only the first wrapping -- the row format of the
// ownership comparison, whose merge and scans (k_move_arcs, k_move_tile_sums,
// k_move_tile_scan; rp_own.hip) run on them unchanged.  This file's kernels:
// k_rmove_finish, the per-interval pass with the classes against R and the
// kept_none measures, and k_rmove_mask, the per-key query (who gained, who
// lost), whose ballots k_hold_list (rp_hold.hip) turns into lists.  None is
// launched by a round.  Every store is a vector store or an integer atomic,
// and the phases are separate kernels: no block waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>

#include "rp_repl.h"

namespace rp {

// the comparison's device results: MoveArgs::out as k_move_arcs fills it
// (MV_GAINED .. MV_MAXL), transition[3][3], same_set and the turnover where
// the ownership comparison has them, kept_none in handed_off's place and
// kept_none_regained behind
enum : uint32_t { RMV_KEPT = MV_HANDED, RMV_REGAINED = MV_NOUT, RMV_NOUT = MV_NOUT + 1 };
constexpr uint32_t RMV_SUMS = 12;  // transition[9], same_set, kept_none, kept_none_regained

// Per interval g, l and the two censuses' claims give its cell of
// transition[3][3] (under, exact, over: claims against R), same_set, kept_none
// (every holder at `from` lost it) and kept_none_regained (and some node
// gained it), the length added by selects, in registers; its turnover g + l
// packed with ~i so that a max keeps the lowest interval; per block in LDS,
// one atomic per counter and block (k_move_finish's scheme).
__global__ void __launch_bounds__(OWN_BLOCK) k_rmove_finish(MoveArgs A, uint32_t R) {
    __shared__ int32_t ws[2][OWN_BLOCK / 64];
    __shared__ unsigned long long bm[RMV_SUMS];
    __shared__ unsigned long long bmax;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < RMV_SUMS) bm[threadIdx.x] = 0;
    if (threadIdx.x == RMV_SUMS) bmax = 0;
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
    unsigned long long m[RMV_SUMS], best = 0;
#pragma unroll
    for (uint32_t k = 0; k < RMV_SUMS; k++) m[k] = 0;
#pragma unroll
    for (uint32_t j = 0; j < OWN_ITEMS; j++) {
        const uint32_t i = first + j;
        if (i < A.npts) {
            const uint32_t g = (uint32_t)(bg + cg[j]), l = (uint32_t)(bl + cl[j]);
            const uint32_t cf = A.claims[0][i], ct = A.claims[1][i];
            const unsigned long long len = i ? (unsigned long long)(A.pt_hash[i] - A.pt_hash[i - 1])
                                             : (unsigned long long)A.pt_hash[0] + (1ull << 32) - A.pt_hash[A.npts - 1];
            const uint32_t cell = ((cf >= R) + (cf > R)) * 3u + (ct >= R) + (ct > R);
#pragma unroll
            for (uint32_t k = 0; k < 9; k++) m[MV_TRANS + k] += cell == k ? len : 0ull;
            m[MV_SAME] += (g | l) == 0 ? len : 0ull;
            const bool none = cf != 0 && l == cf;
            m[RMV_KEPT] += none ? len : 0ull;
            m[RMV_KEPT + 1] += none && g != 0 ? len : 0ull;
            const unsigned long long pk = (unsigned long long)(g + l) << 32 | (uint32_t)~i;
            best = g + l != 0 && pk > best ? pk : best;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < RMV_SUMS; k++)
        if (m[k]) atomicAdd(&bm[k], m[k]);
    if (best) atomicMax(&bmax, best);
    __syncthreads();
    // (the first eleven sums lie in out as in bm; the twelfth behind the ownership comparison's words)
    if (threadIdx.x < RMV_SUMS && bm[threadIdx.x])
        atomicAdd(&A.out[threadIdx.x == RMV_KEPT + 1 ? RMV_REGAINED : threadIdx.x], bm[threadIdx.x]);
    if (threadIdx.x == RMV_SUMS && bmax) atomicMax(&A.out[MV_MAXT], bmax);
}

// ---- the per-key query: which nodes gained a key, which lost it

constexpr uint32_t RMV_BLOCK = 256;            // four waves: one tile of nodes, four batches of keys
constexpr uint32_t RMV_WAVES = RMV_BLOCK / 64;
constexpr uint32_t RMV_TILE = 32;              // nodes of a block: both sides of a node on the lanes of one wave
constexpr uint32_t RMV_BOUNDS = 2 * MV_SEGS;   // a side's boundaries of one node, at the most
// a side's rows; the other side's start one bank further, so that the two
// halves of a wave reading the same place of their rows do not collide
constexpr uint32_t RMV_SIDE = RMV_TILE * RMV_BOUNDS + 1;
constexpr uint32_t RMV_CHUNK = 1u << 16;           // keys of one set of launches, at the most
constexpr size_t RMV_BUDGET = (size_t)256 << 20;   // bytes of a chunk's two masks, and of its rows, at the most
constexpr uint32_t RMV_BLOCKS = 2048;              // blocks a launch aims at when it slices a chunk's keys

struct RMaskArgs {
    // side 0: from, side 1: to -- recorded arcs (k_rep_arcs<true>)
    const uint32_t* arc_n[2];
    const uint2* arcs[2];
    const uint32_t* pt_hash;
    const uint32_t* dir;
    uint32_t n, npts, dir_shift;
};

// One block = one tile of RMV_TILE consecutive nodes x one slice of the
// chunk's keys.  The block stages both sides of its nodes' rows once, as
// sorted boundary arrays in LDS: a row's disjoint segments [lo, hi) of
// interval indices in ascending order are lo0, hi0, lo1, hi1, ... -- arc
// (q, p) is [q + 1, p + 1), the wrapping first arc [0, p + 1) and, after every
// other, [q + 1, npts); an OWN_ARC_ALL row is [0, npts); at most RMV_BOUNDS
// words a row.  The sequence never descends (a segment may start where the
// one before ends), so interval x is covered iff the number of boundaries
// <= x is odd: one binary search a side.  Lanes 0-31 search `from` for node
// L, lanes 32-63 `to` for node L - 32; the ballot of the parities is both
// sides' coverage words at once, gain = to & ~from, loss = from & ~to.  The
// keys go through the waves in batches of 64: lane j searches key j's
// interval once (route_point), the wave takes it from lane j through a scalar
// register.  Lane 0 stores the two words to gain[key][tile] and
// loss[key][tile]; two tiles are one of k_hold_list's 64-bit words.  A tile
// past n (the host rounds the tiles up to an even number) stores zeros.
__global__ void __launch_bounds__(RMV_BLOCK) k_rmove_mask(RMaskArgs M, const uint32_t* __restrict__ keys, uint32_t nk,
                                                          uint32_t per_slice, uint32_t tiles, uint32_t* __restrict__ gain,
                                                          uint32_t* __restrict__ loss) {
    __shared__ uint32_t bnd[2 * RMV_SIDE];
    __shared__ uint32_t cnt[2 * RMV_TILE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x;
    const uint32_t npts = M.npts;
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) {
        for (uint32_t node = wave; node < RMV_TILE; node += RMV_WAVES) {  // (a row is its wave's)
            const uint32_t v = tile * RMV_TILE + node;
            uint32_t* row = bnd + s * RMV_SIDE + node * RMV_BOUNDS;
            uint32_t nb = 0;
            if (v < M.n) {
                uint32_t c = M.arc_n[s][v];
                if (c & OWN_ARC_ALL) {
                    if (lane == 0) { row[0] = 0; row[1] = npts; }
                    nb = 2;
                } else if (c) {
                    if (c > OWN_REPLICAS) c = OWN_REPLICAS;  // (never: the rows hold no more)
                    const uint2* arow = M.arcs[s] + (size_t)v * OWN_REPLICAS;
                    const uint2 a0 = arow[0];
                    const bool wraps = a0.x > a0.y;
                    for (uint32_t k = lane; k < c; k += 64) {
                        const uint2 a = arow[k];
                        row[2 * k] = k == 0 && wraps ? 0u : a.x + 1;
                        row[2 * k + 1] = a.y + 1;
                    }
                    // the wrapping arc's upper part lies after every other arc (q >= the last own point)
                    const bool tail = wraps && a0.x + 1 < npts;
                    if (tail && lane == 0) { row[2 * c] = a0.x + 1; row[2 * c + 1] = npts; }
                    nb = 2 * (c + (tail ? 1u : 0u));
                }
            }
            if (lane == 0) cnt[s * RMV_TILE + node] = nb;
        }
    }
    __syncthreads();
    const uint32_t* mine = bnd + (lane >> 5) * RMV_SIDE + (lane & 31u) * RMV_BOUNDS;
    const uint32_t nmine = cnt[lane];
    const uint32_t k0 = blockIdx.y * per_slice;  // (< nk: the host's grid)
    const uint32_t k1 = nk - k0 < per_slice ? nk : k0 + per_slice;
    for (uint32_t kb = k0 + wave * 64; kb < k1; kb += RMV_WAVES * 64) {
        uint32_t x0 = 0;
        if (kb + lane < k1) x0 = route_point(M.pt_hash, npts, M.dir, M.dir_shift, keys[kb + lane]);
        const uint32_t nb = k1 - kb < 64 ? k1 - kb : 64;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)x0, j);
            uint32_t a = 0, len = nmine;  // a: the boundaries <= x
            while (len) {
                const uint32_t half = len >> 1;
                if (mine[a + half] <= x) { a += half + 1; len -= half + 1; } else len = half;
            }
            const unsigned long long word = __ballot(a & 1u);
            if (lane == 0) {
                const uint32_t from = (uint32_t)word, to = (uint32_t)(word >> 32);
                gain[(size_t)(kb + j) * tiles + tile] = to & ~from;
                loss[(size_t)(kb + j) * tiles + tile] = from & ~to;
            }
        }
    }
}

}  // namespace rp

// =====================================================================
// Host side (on the first shard's stream, like the censuses).
// =====================================================================
using rp::DevBuf;
using rp::Error;
using rp::Shard;

// Every node's recorded arcs and the replica census' claims_R at one clock, in
// device buffers of its own: it outlives its simulation, which it names by id.
struct rp_replication_snapshot {
    uint64_t sim_id = 0, gen = 0, clock = 0;
    int dev = 0;
    uint32_t n = 0, npts = 0, replicas = 0;
    DevBuf<uint32_t> arc_n, claims;
    DevBuf<uint2> arcs;
    rp_replication_stats stats{};
};

namespace {

void check_snapshot(const rp_sim* c, const rp_replication_snapshot* s, const char* which) {
    if (s->sim_id != c->own_id) throw Error(RP_ERR_INVALID, std::string(which) + ": a snapshot of another simulation");
    if (s->gen != c->own_gen || s->n != c->n || s->npts != c->sh.front()->npts)
        throw Error(RP_ERR_STATE, std::string(which) + ": the snapshot was taken before rp_sim_load_addresses changed the points");
}

// both sides of a comparison: the checks every entry point makes, in their
// order, and the recording census at from's R when `to` is the simulation
struct Sides {
    const uint32_t* arc_n[2];
    const uint2* arcs[2];
    const uint32_t* claims[2];
};

Sides sides_of(rp_sim* c, const rp_replication_snapshot* from, const rp_replication_snapshot* to) {
    // (own_prepare rebuilt the point index if the points changed: a stale
    // snapshot's generation differs, and no kernel sees its indices)
    check_snapshot(c, from, "from");
    if (to) {
        check_snapshot(c, to, "to");
        if (to->replicas != from->replicas) throw Error(RP_ERR_INVALID, "to: a snapshot at another number of replicas");
    } else {
        c->rep_refresh(from->replicas, true);
    }
    Sides s;
    s.arc_n[0] = from->arc_n.p; s.arcs[0] = from->arcs.p; s.claims[0] = from->claims.p;
    s.arc_n[1] = to ? to->arc_n.p : c->rep_arc_n.p;
    s.arcs[1] = to ? to->arcs.p : c->rep_arcs.p;
    s.claims[1] = to ? to->claims.p : c->rep_claims.p;
    return s;
}

}  // namespace

extern "C" {

int rp_replication_snapshot_create(rp_sim* c, uint32_t replicas, rp_replication_snapshot** out) {
    return rp::guarded([&] {
        if (!c || !out) throw Error(RP_ERR_INVALID, "null pointer");
        *out = nullptr;
        if (replicas < 1 || replicas > rp::REP_MAX_R) throw Error(RP_ERR_INVALID, "replicas must be 1..8");
        c->rep_refresh(replicas, true);
        Shard& s0 = *c->sh.front();
        std::unique_ptr<rp_replication_snapshot> s(new rp_replication_snapshot());
        s->sim_id = rp::snapshot_sim_id(c); s->gen = c->own_gen; s->clock = c->round;
        s->dev = c->dev; s->n = c->n; s->npts = s0.npts; s->replicas = replicas;
        s->stats = c->rep_stats;
        s->arc_n.alloc(c->rep_arc_n.n);
        s->arcs.alloc(c->rep_arcs.n);
        s->claims.alloc(c->rep_claims.n);
        s0.timed(5, [&] {
            RP_HIP(hipMemcpyAsync(s->arc_n.p, c->rep_arc_n.p, s->arc_n.bytes(), hipMemcpyDeviceToDevice, s0.st));
            RP_HIP(hipMemcpyAsync(s->arcs.p, c->rep_arcs.p, s->arcs.bytes(), hipMemcpyDeviceToDevice, s0.st));
            RP_HIP(hipMemcpyAsync(s->claims.p, c->rep_claims.p, s->claims.bytes(), hipMemcpyDeviceToDevice, s0.st));
        });
        RP_HIP(hipStreamSynchronize(s0.st));
        *out = s.release();
    });
}

int rp_replication_snapshot_info(const rp_replication_snapshot* s, rp_replication_stats* stats, uint64_t* clock,
                                 uint32_t* replicas) {
    return rp::guarded([&] {
        if (!s) throw Error(RP_ERR_INVALID, "null pointer");
        if (stats) *stats = s->stats;
        if (clock) *clock = s->clock;
        if (replicas) *replicas = s->replicas;
    });
}

int rp_replication_snapshot_destroy(rp_replication_snapshot* s) {
    return rp::guarded([&] {
        if (!s) return;
        (void)hipSetDevice(s->dev);
        delete s;
    });
}

int rp_sim_replication_moved(rp_sim* c, const rp_replication_snapshot* from, const rp_replication_snapshot* to,
                             rp_replica_movement_stats* stats, uint64_t* gained, uint64_t* lost, size_t cap) {
    return rp::guarded([&] {
        static_assert(sizeof(rp_replica_movement_stats) == 256, "rp_replica_movement_stats is 32 x u64");
        if (!c || !stats) throw Error(RP_ERR_INVALID, "null pointer");
        // (a rank holds its own nodes' views only: unsupported, whatever else is passed)
        c->own_prepare();
        if (!from) throw Error(RP_ERR_INVALID, "null pointer");
        if ((gained || lost) && cap < c->n) throw Error(RP_ERR_INVALID, "gained / lost buffer holds fewer than n entries");
        const Sides sd = sides_of(c, from, to);
        Shard& s0 = *c->sh.front();
        const uint32_t n = c->n, npts = s0.npts, R = from->replicas;
        const uint32_t ntiles = (npts + rp::OWN_TILE - 1) / rp::OWN_TILE;
        if (c->mv_diff.n != 2 * ((size_t)npts + 1)) c->mv_diff.alloc(2 * ((size_t)npts + 1));
        if (c->mv_tile.n != 2 * (size_t)ntiles) c->mv_tile.alloc(2 * (size_t)ntiles);
        if (c->mv_gained.n != n) c->mv_gained.alloc(n);
        if (c->mv_lost.n != n) c->mv_lost.alloc(n);
        if (!c->rmv_out.p) c->rmv_out.alloc(rp::RMV_NOUT);
        rp::MoveArgs A{};
        for (int k = 0; k < 2; k++) { A.arc_n[k] = sd.arc_n[k]; A.arcs[k] = sd.arcs[k]; A.claims[k] = sd.claims[k]; }
        A.pt_hash = s0.pt_hash.p;
        A.n = n; A.npts = npts; A.ntiles = ntiles;
        A.diff = c->mv_diff.p; A.tile_sum = c->mv_tile.p;
        A.gained = c->mv_gained.p; A.lost = c->mv_lost.p; A.out = c->rmv_out.p;
        s0.timed(5, [&] {
            RP_HIP(hipMemsetAsync(c->mv_diff.p, 0, c->mv_diff.bytes(), s0.st));
            RP_HIP(hipMemsetAsync(c->rmv_out.p, 0, c->rmv_out.bytes(), s0.st));
            rp::move_scan(A, s0.st);
            hipLaunchKernelGGL(rp::k_rmove_finish, dim3(ntiles), dim3(rp::OWN_BLOCK), 0, s0.st, A, R);
        });
        RP_HIP(hipGetLastError());
        unsigned long long h[rp::RMV_NOUT];
        RP_HIP(hipMemcpyAsync(h, c->rmv_out.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
        if (gained) RP_HIP(hipMemcpyAsync(gained, c->mv_gained.p, (size_t)n * 8, hipMemcpyDeviceToHost, s0.st));
        if (lost) RP_HIP(hipMemcpyAsync(lost, c->mv_lost.p, (size_t)n * 8, hipMemcpyDeviceToHost, s0.st));
        RP_HIP(hipStreamSynchronize(s0.st));
        rp_replica_movement_stats st{};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) st.transition[a][b] = h[rp::MV_TRANS + 3 * a + b];
        st.same_set = h[rp::MV_SAME];
        st.kept_none = h[rp::RMV_KEPT]; st.kept_none_regained = h[rp::RMV_REGAINED];
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
        st.replicas = R;
        *stats = st;
    });
}

int rp_sim_replication_moved_at(rp_sim* c, const rp_replication_snapshot* from, const rp_replication_snapshot* to,
                                const uint32_t* key_hashes, size_t nk, size_t cap, int32_t* gainers, int32_t* losers,
                                uint32_t* n_gained, uint32_t* n_lost) {
    return rp::guarded([&] {
        if (!c) throw Error(RP_ERR_INVALID, "null pointer");
        c->own_prepare();
        if (!from || (nk && (!key_hashes || !n_gained || !n_lost))) throw Error(RP_ERR_INVALID, "null pointer");
        const Sides sd = sides_of(c, from, to);
        if (nk == 0) return;
        Shard& s0 = *c->sh.front();
        rp::RMaskArgs M{};
        for (int k = 0; k < 2; k++) { M.arc_n[k] = sd.arc_n[k]; M.arcs[k] = sd.arcs[k]; }
        M.pt_hash = s0.pt_hash.p; M.dir = c->route_dir.p;
        M.n = c->n; M.npts = s0.npts; M.dir_shift = c->route_dir_shift;
        // an even number of 32-node tiles: a key's row of each mask is `words` 64-bit words for k_hold_list
        const uint32_t words = (c->n + 63) / 64, tiles = 2 * words;
        // a row on the device holds min(cap, n) ids: no key has more gainers or losers, the rest of a longer row is -1 here
        int32_t* const lists[2] = {gainers, losers};
        uint32_t* const counts[2] = {n_gained, n_lost};
        const size_t dcap = gainers || losers ? std::min<size_t>(cap, c->n) : 0;
        for (int k = 0; k < 2; k++)
            if (lists[k] && dcap < cap) std::fill(lists[k], lists[k] + nk * cap, -1);
        // a chunk's two masks (8 x words bytes a key each) and two sets of rows within the budget, at most 2^16 keys
        size_t chunk = std::min<size_t>(nk, rp::RMV_CHUNK);
        chunk = std::min(chunk, std::max<size_t>(1, rp::RMV_BUDGET / (16 * (size_t)words)));
        if (dcap) chunk = std::min(chunk, std::max<size_t>(1, rp::RMV_BUDGET / (8 * dcap)));
        DevBuf<uint32_t> dh(chunk), dcnt(2 * chunk);
        DevBuf<unsigned long long> dmask(2 * chunk * words);
        DevBuf<int32_t> drow(2 * chunk * dcap);
        for (size_t first = 0; first < nk; first += chunk) {
            const uint32_t m = (uint32_t)std::min(nk - first, chunk);
            // slices of whole batches (4 waves x 64 keys), as few as fill the device: a tile's rows stay with its block
            const uint32_t want = std::max(1u, rp::RMV_BLOCKS / tiles);
            const uint32_t per = ((m + want - 1) / want + rp::RMV_BLOCK - 1) / rp::RMV_BLOCK * rp::RMV_BLOCK;
            const uint32_t slices = (m + per - 1) / per;
            unsigned long long* const mask[2] = {dmask.p, dmask.p + (size_t)m * words};
            RP_HIP(hipMemcpyAsync(dh.p, key_hashes + first, (size_t)m * 4, hipMemcpyHostToDevice, s0.st));
            s0.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_rmove_mask, dim3(tiles, slices), dim3(rp::RMV_BLOCK), 0, s0.st, M,
                                   (const uint32_t*)dh.p, m, per, tiles, (uint32_t*)mask[0], (uint32_t*)mask[1]);
                for (int k = 0; k < 2; k++)
                    rp::hold_list(mask[k], m, words, (uint32_t)dcap, drow.p + (size_t)k * m * dcap, dcnt.p + (size_t)k * m,
                                  s0.st);
            });
            RP_HIP(hipGetLastError());
            for (int k = 0; k < 2; k++) {
                const int32_t* src = drow.p + (size_t)k * m * dcap;
                if (lists[k] && dcap == cap && cap)
                    RP_HIP(hipMemcpyAsync(lists[k] + first * cap, src, (size_t)m * cap * 4, hipMemcpyDeviceToHost, s0.st));
                else if (lists[k] && dcap)
                    RP_HIP(hipMemcpy2DAsync(lists[k] + first * cap, cap * 4, src, dcap * 4, dcap * 4, m, hipMemcpyDeviceToHost,
                                            s0.st));
                RP_HIP(hipMemcpyAsync(counts[k] + first, dcnt.p + (size_t)k * m, (size_t)m * 4, hipMemcpyDeviceToHost, s0.st));
            }
            RP_HIP(hipStreamSynchronize(s0.st));
        }
    });
}

}  // extern "C"
