// ringpop_amd — the holders query (rp_sim_holders_at): for a
// batch of key hashes, which nodes believe they hold one of a key's R replicas
// in their own view -- the replica-set census' question (rp_repl.hip; §16)
// transposed: every view for a few keys, not every key for one view.  For one
// key every view walks the same global points; only the byte "is this server
// in my ring" differs.  k_hold_mask puts 64 consecutive views on the lanes of
// a wave and keeps them there while it loops over its keys, one ballot per
// (key, 64 views); k_hold_list turns a key's row of ballots into the count
// and the ascending list.  Neither is launched by a round.  Every store is a
// vector store, there is no atomic, and no output position depends on the
// order in which waves finish.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rp_repl.h"

namespace rp {

constexpr uint32_t HOLD_BLOCK = 256;                  // four waves: one tile of views, four batches of keys
constexpr uint32_t HOLD_WAVES = HOLD_BLOCK / 64;
constexpr uint32_t HOLD_SPAN = REP_MAX_R + REP_SOLO_EXTRA;  // points a lane examines alone, at the most
constexpr uint32_t HOLD_CHUNK = 1u << 16;             // keys of one pair of launches, at the most
constexpr size_t HOLD_BUDGET = (size_t)256 << 20;     // bytes of a chunk's mask, and of its rows, at the most
constexpr uint32_t HOLD_BLOCKS = 2048;                // blocks a launch aims at when it slices a chunk's keys

enum : uint32_t { HOLD_NONE = 0, HOLD_ALL = 1, HOLD_WALK = 2 };  // what a view answers without a key, or that it walks

// One point's outcome in a lane's walk: its view owns it (the key is held),
// it is the R-th distinct other owner (it is not), or the walk goes on.
__device__ inline void hold_take(OwnerSet<REP_MAX_R - 1>& u, int32_t o, int32_t self, uint32_t R, bool& done, bool& held) {
    if (done || o < 0 || (o != self && u.has(o))) return;
    if (walk_take(u, o, self, R)) {
        done = true;
        held = o == self;
    }
}

// One block = one tile of 64 consecutive views (lane L of every wave is view
// tile * 64 + L, in whichever shard holds it) x one slice of the chunk's keys.
// The views' state is read once: dead, ring_count, the base of the in_ring and
// coll_owner rows.  The keys go through the waves in batches of 64: lane j
// searches key j's point and reads the first `span` points from it (pt_coll,
// pt_server) into registers, once for the wave; key j's walk then takes them
// from lane j through scalar registers (readlane), so that a step's only
// per-lane load is in_ring[v][server] (coll_owner[v][coll] at a collision
// point).  The first min(R, span) of them are in flight at once -- a walk
// rarely ends before the R-th point --, the REP_SOLO_EXTRA further ones are
// read only while a lane still walks.  A lane that has not ended after `span`
// points belongs to a sparse view: the wave serves these one at a time with
// walk_wave, the served lane's view broadcast and its ring rebuilt from it, 64
// points a step.  A (tile, key) pair therefore costs at most span + npts +
// 64 (R + 1) wave steps whatever the views.  An empty ring and a ring of the
// view alone hold every key without a walk, a dead node and a lane past n
// none.  mask[key][tile] is the ballot of the lanes that hold the key.
__global__ void __launch_bounds__(HOLD_BLOCK) k_hold_mask(OwnArgs A, uint32_t R, const uint32_t* __restrict__ keys, uint32_t nk,
                                                          uint32_t per_slice, uint32_t tiles,
                                                          unsigned long long* __restrict__ mask) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x;
    const uint32_t v = tile * 64 + lane;
    const uint32_t npts = A.npts;
    uint32_t kind = HOLD_NONE;
    const uint8_t* in_ring = nullptr;
    const int32_t* coll_owner = nullptr;
    if (v < A.n) {
        const uint32_t g = v / A.nl;
        if (A.dead[g][v] == 0) {  // (fail-stopped, or not joined yet: no claimant)
            const RouteShard& t = A.tab[g];
            const size_t lr = v % A.nl;
            in_ring = t.in_ring + lr * A.n;
            coll_owner = t.coll_owner + lr * A.ncoll;
            const int32_t rc = t.ring_count[v];
            // an empty ring (RingPop.lookupN returns [whoami]) or a ring of v alone: everything
            kind = rc <= 0 || (rc == 1 && in_ring[v]) ? HOLD_ALL : HOLD_WALK;
        }
    }
    const RouteRing ring{in_ring, coll_owner};
    const uint32_t span = R + REP_SOLO_EXTRA < npts ? R + REP_SOLO_EXTRA : npts;
    const uint32_t lead = R < span ? R : span;
    const uint32_t k0 = blockIdx.y * per_slice;  // (< nk: the host's grid)
    const uint32_t k1 = nk - k0 < per_slice ? nk : k0 + per_slice;
    for (uint32_t kb = k0 + wave * 64; kb < k1; kb += HOLD_WAVES * 64) {
        // lane j: key kb + j's first point and the span points from it
        uint32_t p0 = 0;
        int32_t pc[HOLD_SPAN], ps[HOLD_SPAN];
        const bool mine = kb + lane < k1;
        if (mine) p0 = route_point(A.pt_hash, npts, A.dir, A.dir_shift, keys[kb + lane]);
#pragma unroll
        for (uint32_t k = 0; k < HOLD_SPAN; k++) {
            pc[k] = -1;
            ps[k] = 0;
            if (mine && k < span) {
                const uint32_t idx = walk_move<false>(p0, k, npts);  // (k < span <= npts)
                pc[k] = A.pt_coll[idx];
                ps[k] = A.pt_server[idx];
            }
        }
        const uint32_t nb = k1 - kb < 64 ? k1 - kb : 64;
        for (uint32_t j = 0; j < nb; j++) {
            bool held = kind == HOLD_ALL, done = kind != HOLD_WALK;
            OwnerSet<REP_MAX_R - 1> u;  // (the R-th other owner ends the walk: it is never stored)
            u.clear();
            int32_t o[REP_MAX_R];
#pragma unroll
            for (uint32_t k = 0; k < REP_MAX_R; k++) {
                o[k] = -1;
                if (k < lead) {
                    const int32_t c = __builtin_amdgcn_readlane(pc[k], j), s = __builtin_amdgcn_readlane(ps[k], j);
                    if (!done) o[k] = ring.owner(c, s);
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < REP_MAX_R; k++)
                if (k < lead) hold_take(u, o[k], (int32_t)v, R, done, held);
#pragma unroll
            for (uint32_t k = 1; k < HOLD_SPAN; k++) {
                if (k >= lead && k < span && __ballot(!done) != 0) {
                    const int32_t c = __builtin_amdgcn_readlane(pc[k], j), s = __builtin_amdgcn_readlane(ps[k], j);
                    if (!done) hold_take(u, ring.owner(c, s), (int32_t)v, R, done, held);
                }
            }
            if (span == npts) done = true;  // once round
            // sparse views: the wave walks for one lane at a time, from the point after the span
            unsigned long long pend = __ballot(!done);
            if (pend != 0) {
                const uint32_t first = walk_move<false>((uint32_t)__builtin_amdgcn_readlane((int)p0, j), span, npts);
                while (pend != 0) {
                    const int L = __ffsll(pend) - 1;
                    pend &= pend - 1;
                    const uint32_t vl = (uint32_t)__builtin_amdgcn_readlane((int)v, L);
                    const RouteShard& t = A.tab[vl / A.nl];
                    const size_t lr = vl % A.nl;
                    const RouteRing served{t.in_ring + lr * A.n, t.coll_owner + lr * A.ncoll};
                    uint32_t q = REP_NONE;
                    walk_wave<REP_MAX_R - 1, false>(served, A, u, first, span, lane == (uint32_t)L, q, (int32_t)vl, R, lane);
                    // (it ended at a point of vl's before the R-th other owner was kept, or it did not)
                    if (lane == (uint32_t)L) held = q != REP_NONE && u.cnt < R;
                }
            }
            const unsigned long long word = __ballot(held);
            if (lane == 0) mask[(size_t)(kb + j) * tiles + tile] = word;
        }
    }
}

// One wave per key over its row of `tiles` ballots, 64 words a pass: a word's
// popcount, the wave's exclusive scan of them over the running base of the
// earlier passes, and each lane writes its word's node ids from its rank on
// while that is below cap -- ascending, since words and bits are.  The count
// is the full one whatever cap is; the row's remaining slots get -1.
__global__ void __launch_bounds__(HOLD_BLOCK) k_hold_list(const unsigned long long* __restrict__ mask, uint32_t nk,
                                                          uint32_t tiles, uint32_t cap, int32_t* __restrict__ holders,
                                                          uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t key = blockIdx.x * HOLD_WAVES + (threadIdx.x >> 6);
    if (key >= nk) return;  // (the whole wave)
    const unsigned long long* words = mask + (size_t)key * tiles;
    int32_t* row = holders + (size_t)key * cap;  // (cap == 0: never written)
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += 64) {
        const uint32_t t = t0 + lane;
        unsigned long long w = t < tiles ? words[t] : 0ull;
        const int32_t c = __popcll(w);
        const int32_t incl = wave_scan_incl(c, lane);
        uint32_t r = base + (uint32_t)(incl - c);
        while (w != 0 && r < cap) {
            row[r++] = (int32_t)(t * 64 + (uint32_t)__ffsll(w) - 1);
            w &= w - 1;
        }
        base += (uint32_t)__builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) counts[key] = base;
    for (uint32_t i = (base < cap ? base : cap) + lane; i < cap; i += 64) row[i] = -1;
}

void hold_list(const unsigned long long* mask, uint32_t nk, uint32_t tiles, uint32_t cap, int32_t* holders, uint32_t* counts,
               hipStream_t st) {
    hipLaunchKernelGGL(k_hold_list, dim3((nk + HOLD_WAVES - 1) / HOLD_WAVES), dim3(HOLD_BLOCK), 0, st, mask, nk, tiles, cap,
                       holders, counts);
}

}  // namespace rp

// =====================================================================
// Host side (on the first shard's stream, like the censuses).
// =====================================================================
using rp::DevBuf;
using rp::Error;
using rp::Shard;

extern "C" {

int rp_sim_holders_at(rp_sim* c, uint32_t replicas, const uint32_t* key_hashes, size_t nk, size_t cap, int32_t* holders,
                      uint32_t* counts) {
    return rp::guarded([&] {
        if (!c || (nk && (!key_hashes || !counts))) throw Error(RP_ERR_INVALID, "null pointer");
        if (replicas < 1 || replicas > rp::REP_MAX_R) throw Error(RP_ERR_INVALID, "replicas must be 1..8");
        c->own_prepare();  // (the routing tables and the shards' dead arrays: neither census is read or touched)
        if (nk == 0) return;
        if (!holders) cap = 0;
        Shard& s0 = *c->sh.front();
        const rp::OwnArgs A = c->own_args();
        const uint32_t tiles = (c->n + 63) / 64;
        // a row on the device holds min(cap, n) ids: no key has more holders, the rest of a longer row is -1 here
        const size_t dcap = std::min<size_t>(cap, c->n);
        if (dcap < cap) std::fill(holders, holders + nk * cap, -1);
        // a chunk's mask (8 x tiles bytes a key) and rows within the budget, at most 2^16 keys: indices stay 32-bit
        size_t chunk = std::min<size_t>(nk, rp::HOLD_CHUNK);
        chunk = std::min(chunk, std::max<size_t>(1, rp::HOLD_BUDGET / (8 * (size_t)tiles)));
        if (dcap) chunk = std::min(chunk, std::max<size_t>(1, rp::HOLD_BUDGET / (4 * dcap)));
        DevBuf<uint32_t> dh(chunk), dcnt(chunk);
        DevBuf<unsigned long long> dmask(chunk * tiles);
        DevBuf<int32_t> drow(chunk * dcap);
        for (size_t first = 0; first < nk; first += chunk) {
            const uint32_t m = (uint32_t)std::min(nk - first, chunk);
            // slices of whole batches (4 waves x 64 keys), as few as fill the device: a tile's rows stay with its block
            const uint32_t want = std::max(1u, rp::HOLD_BLOCKS / tiles);
            const uint32_t per = ((m + want - 1) / want + rp::HOLD_BLOCK - 1) / rp::HOLD_BLOCK * rp::HOLD_BLOCK;
            const uint32_t slices = (m + per - 1) / per;
            RP_HIP(hipMemcpyAsync(dh.p, key_hashes + first, (size_t)m * 4, hipMemcpyHostToDevice, s0.st));
            s0.timed(5, [&] {
                hipLaunchKernelGGL(rp::k_hold_mask, dim3(tiles, slices), dim3(rp::HOLD_BLOCK), 0, s0.st, A, replicas,
                                   (const uint32_t*)dh.p, m, per, tiles, dmask.p);
            });
            RP_HIP(hipGetLastError());
            s0.timed(5, [&] {
                rp::hold_list(dmask.p, m, tiles, (uint32_t)dcap, drow.p, dcnt.p, s0.st);
            });
            RP_HIP(hipGetLastError());
            if (dcap == cap && cap)
                RP_HIP(hipMemcpyAsync(holders + first * cap, drow.p, (size_t)m * cap * 4, hipMemcpyDeviceToHost, s0.st));
            else if (dcap)
                RP_HIP(hipMemcpy2DAsync(holders + first * cap, cap * 4, drow.p, dcap * 4, dcap * 4, m, hipMemcpyDeviceToHost,
                                        s0.st));
            RP_HIP(hipMemcpyAsync(counts + first, dcnt.p, (size_t)m * 4, hipMemcpyDeviceToHost, s0.st));
            RP_HIP(hipStreamSynchronize(s0.st));
        }
    });
}

}  // extern "C"
