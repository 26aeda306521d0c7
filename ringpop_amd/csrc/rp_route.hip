// ringpop_amd — request routing across the simulated cluster, between rounds
// (rp_sim_ring_checksums / rp_sim_route / rp_sim_route_uniform; DESIGN.md
// §10): the ring checksum of every view and, for batches of requests, the
// outcome handleOrProxy and the request proxy would see.  The kernels, the
// host side that launches them and the three entry points.  None of the
// kernels is launched by a round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rp_block.h"
#include "rp_checksum.h"
#include "rp_cluster.h"
#include "rp_whash.h"

namespace rp {

// HashRing.checksum of one view by a whole wave (lib/ring.js:96-105): the
// structure of wave_view_checksum for the string of the in-ring members'
// addresses joined by ';'.  Pass 1 takes the length, the member count and the
// last member; the last 20 bytes come from rendering the top chunks that cover
// them; then the chunks are rendered in order into the wave's LDS buffer at
// prefix-sum offsets and their whole 20-byte blocks hashed (FhLanes), the
// leftover bytes carried to the buffer's front.  A string of <= 24 bytes is
// rendered whole and hashed by farmhash32's short branches.
constexpr uint32_t RCK_TEXT = 2240;  // > 20 carried + 64 x (1 + 32) rendered bytes; a multiple of 16
constexpr uint32_t RCK_PRE = RCK_TEXT / 20;  // >= the 20-byte blocks of one chunk
constexpr uint32_t RCK_BUF = RCK_TEXT + RCK_PRE * 48;  // + their fh_stream_pre records
static_assert(RCK_TEXT % 16 == 0 && RCK_BUF % 16 == 0, "the records are read as 16-byte words");
static_assert(RCK_TEXT >= 20 + 64 * (1 + 4 * ADDR_WORDS), "a chunk and the carried bytes fit");

// One chunk of 64 members: every lane whose member is in the ring writes
// [';'] + its address at buf + base + (the lanes' prefix sum); returns the
// chunk's bytes.
__device__ inline uint32_t ring_render_chunk(uint8_t* buf, uint32_t base, bool present, bool sep, uint32_t L,
                                             const uint4& wa, const uint4& wb) {
    const uint32_t lane = lane_id();
    const uint32_t b = present ? L + (sep ? 1u : 0u) : 0u;
    uint32_t incl = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if ((int)lane >= o) incl += y;
    }
    const uint32_t total = __shfl(incl, 63);
    if (present) {
        WordSink<LdsByteEmit> w;
        w.emit.p = buf + base + (incl - b);
        if (sep) w.put(0x3Bu, 1);
        const uint32_t aw[ADDR_WORDS] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
        for (uint32_t k = 0; k < ADDR_WORDS; k++)
            if (k * 4 < L) w.put(aw[k], L - 4 * k >= 4 ? 4 : L - 4 * k);
        for (uint32_t i = 0; i < w.bits / 8; i++) w.emit.p[i] = (uint8_t)(w.acc >> (8 * i));
    }
    return total;
}

__device__ uint32_t wave_ring_checksum(const uint8_t* row, uint32_t n, const AddrTable& at, uint8_t* buf) {
    const uint32_t lane = lane_id();
    // pass 1 (parallel): string length, server count, last server
    uint64_t len = 0, cnt = 0;
    uint32_t lastp1 = 0;
#pragma unroll 4
    for (uint32_t a = lane; a < n; a += 64) {
        const uint32_t in = row[a], L = at.len[a];
        len += in ? L : 0u;
        cnt += in ? 1u : 0u;
        lastp1 = in ? a + 1 : lastp1;
    }
    len = wave_sum64(len);
    cnt = wave_sum64(cnt);
    if (cnt == 0) return farmhash32(nullptr, 0);
    len += cnt - 1;
    const uint32_t last = ~wave_min32(~lastp1) - 1;
    const bool small = len <= 24;
    auto load = [&](uint32_t a, bool& present, uint32_t& L, uint4& wa, uint4& wb) {
        present = a < n && row[a] != 0;
        L = 0;
        wa = make_uint4(0, 0, 0, 0);
        wb = wa;
        if (a < n) {
            L = at.len[a];
            const uint4* p = (const uint4*)(at.words + (size_t)a * ADDR_WORDS);
            wa = p[0];
            wb = p[1];
        }
    };
    FhStream st;
    st.blocks_left = 0;
    if (!small) {
        // the last 20 bytes: chunks from the top down until they cover them
        // (every member with a ';' before it; only a ring's first member has
        // none, and that byte lies more than 20 bytes before the end)
        uint32_t T = 0, c_lo = last & ~63u;
        for (uint32_t c = c_lo;; c -= 64) {
            const uint32_t a = c + lane;
            const bool present = a < n && row[a] != 0;
            T += (uint32_t)wave_sum64(present ? at.len[a] + 1u : 0u);
            c_lo = c;
            if (T >= 20 || c == 0) break;
        }
        // (chunks above c_lo hold < 20 bytes, c_lo's at most 64 x 33: T < RCK_TEXT)
        uint32_t off = 0;
        for (uint32_t c = c_lo; c <= last; c += 64) {
            bool present;
            uint32_t L;
            uint4 wa, wb;
            load(c + lane, present, L, wa, wb);
            if (__ballot(present) == 0) continue;
            off += ring_render_chunk(buf, off, present, present, L, wa, wb);
        }
        wave_lds_fence();
        const uint8_t* t = buf + off - 20;
        st = fh_stream_begin5((uint32_t)len, fetch32(t), fetch32(t + 4), fetch32(t + 8), fetch32(t + 12), fetch32(t + 16));
        wave_lds_fence();
    }
    FhLanes fl;
    fl.init(st);
    uint32_t carry = 0;
    bool any_before = false;
    // the next chunk's ring bytes and addresses are in flight while this one
    // renders and hashes
    bool p_n;
    uint32_t L_n;
    uint4 wa_n, wb_n;
    load(lane, p_n, L_n, wa_n, wb_n);
    for (uint32_t c0 = 0; c0 <= last && (small || st.blocks_left); c0 += 64) {
        const bool present = p_n;
        const uint32_t L = L_n;
        const uint4 aw0 = wa_n, aw1 = wb_n;
        load(c0 + 64 + lane, p_n, L_n, wa_n, wb_n);
        const uint64_t m = __ballot(present);
        if (m == 0) continue;
        const bool sep = present && (any_before || (m & ((1ull << lane) - 1ull)) != 0);
        const uint32_t total = ring_render_chunk(buf, carry, present, sep, L, aw0, aw1);
        any_before = true;
        wave_lds_fence();
        const uint32_t avail = carry + total;
        const uint32_t nb = small ? 0u : min(avail / 20u, st.blocks_left);
        const uint32_t* wb = (const uint32_t*)buf;
        uint32_t* const pre = (uint32_t*)(buf + RCK_TEXT);
        for (uint32_t j = lane; j < nb; j += 64)
            fh_stream_pre_sliced(wb[5 * j], wb[5 * j + 1], wb[5 * j + 2], wb[5 * j + 3], wb[5 * j + 4], pre + 12 * j);
        wave_lds_fence();
        fl.run((const uint4*)pre, 0, nb);
        st.blocks_left -= nb;
        const uint32_t left = avail - 20u * nb;
        // (while blocks remain, left < 20 <= 20 nb or nb = 0: no overlapping move)
        uint8_t mv = 0;
        if (nb && st.blocks_left && lane < left) mv = buf[20u * nb + lane];
        wave_lds_fence();
        if (nb && st.blocks_left && lane < left) buf[lane] = mv;
        wave_lds_fence();
        carry = left;
    }
    if (small) return farmhash32(buf, (uint32_t)len);
    return fh_stream_end(fl.get(0));
}

// Ring checksums of this shard's views, one wave per view (grid-stride).
__global__ void __launch_bounds__(BLOCK) k_ring_checksums(SimDev S, uint32_t* out) {
    __shared__ __attribute__((aligned(16))) uint8_t bufs[NWAVE][RCK_BUF];
    const AddrTable at{S.addr_words, S.addr_len};
    for (uint32_t i = blockIdx.x * NWAVE + wave_id(); i < S.nl; i += gridDim.x * NWAVE) {
        const uint32_t v = S.lo + i;
        const uint32_t c = wave_ring_checksum(S.in_ring + S.row(v), S.n, at, bufs[wave_id()]);
        if (lane_id() == 0) out[v] = c;
    }
}

// Bucket directory over the sorted point hashes: dir[b] = lower bound of
// b << shift for b in [0, nb], dir[nb] = npts.  The points are fixed once the
// addresses are, so it is built once.
__global__ void k_route_dir(const uint32_t* pt_hash, uint32_t npts, uint32_t shift, uint32_t nb, uint32_t* dir) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    uint32_t lo = 0, hi = npts;
    if (b == nb) lo = npts;
    const uint32_t key = (uint32_t)((uint64_t)b << shift);
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (pt_hash[m] < key) lo = m + 1; else hi = m; }
    dir[b] = lo;
}

enum : uint32_t { ROUTE_LOCAL = 0, ROUTE_DELIVERED = 1, ROUTE_CHECKSUMS_DIFFER = 2, ROUTE_UNREACHABLE = 3,
                  ROUTE_ENTRY_DEAD = 4, ROUTE_MISROUTED = 5, ROUTE_NCOUNT = 6 };

// Requests [0, count): request i is (entries[i], keys[i]) or, UNIFORM, drawn
// from splitmix64 at index first + i.  One thread per request (grid-stride):
// one binary search inside the key's directory bucket, then the walk in the
// entry's view and, for a proxied request, in the destination's from the same
// point.  S carries the clock (round, partition window) and the liveness
// bytes; counts are kept per thread, summed per block in LDS and flushed with
// one atomic per counter and block.
template <bool UNIFORM>
__global__ void __launch_bounds__(256) k_route(SimDev S, const RouteShard* tab, const uint32_t* pt_hash,
                                               const int32_t* pt_server, const int32_t* pt_coll, uint32_t npts,
                                               const uint32_t* dir, uint32_t dir_shift, const uint32_t* entries,
                                               const uint32_t* keys, uint64_t seed, uint64_t first, uint64_t count,
                                               int32_t* dests, uint8_t* outcomes, uint8_t* agrees,
                                               unsigned long long* stats) {
    __shared__ unsigned long long bc[ROUTE_NCOUNT];
    if (threadIdx.x < ROUTE_NCOUNT) bc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c[ROUTE_NCOUNT] = {0, 0, 0, 0, 0, 0};
    auto ring_of = [&](uint32_t v, const RouteShard& t) { return route_ring_of(S, t, v); };
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        uint32_t e, h;
        if (UNIFORM) {
            // request first + i: splitmix64's finaliser of seed + (first + i + 1) x the golden gamma
            uint64_t s = seed + (first + i) * 0x9E3779B97F4A7C15ULL;
            const uint64_t r = splitmix_next(s);
            e = (uint32_t)(((r >> 32) * S.n) >> 32);
            h = (uint32_t)r;
        } else {
            e = entries[i];
            h = keys[i];
        }
        int32_t dest = -1;
        uint32_t oc = ROUTE_ENTRY_DEAD, ag = 0;
        if (!S.dead[e]) {
            const RouteShard& te = tab[e / S.nl];
            int32_t d = -1;
            uint32_t p = 0;
            if (te.ring_count[e] > 0) {
                p = route_point(pt_hash, npts, dir, dir_shift, h);
                d = route_walk(ring_of(e, te), pt_server, pt_coll, npts, p);
            }
            if (d < 0 || (uint32_t)d == e) {
                oc = ROUTE_LOCAL;
                dest = (int32_t)e;
            } else {
                dest = d;
                if (unreachable(S, e, (uint32_t)d)) {
                    oc = ROUTE_UNREACHABLE;
                } else {
                    const RouteShard& td = tab[(uint32_t)d / S.nl];
                    oc = te.ring_csum[e] != td.ring_csum[d] ? ROUTE_CHECKSUMS_DIFFER : ROUTE_DELIVERED;
                    const int32_t d2 =
                        td.ring_count[d] > 0 ? route_walk(ring_of((uint32_t)d, td), pt_server, pt_coll, npts, p) : -1;
                    ag = d2 == d ? 1u : 0u;
                    if (!ag) c[ROUTE_MISROUTED]++;
                }
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < ROUTE_MISROUTED; k++) c[k] += oc == k ? 1u : 0u;  // (registers: no indexed access)
        if (dests) dests[i] = dest;
        if (outcomes) outcomes[i] = (uint8_t)oc;
        if (agrees) agrees[i] = (uint8_t)ag;
    }
#pragma unroll
    for (uint32_t k = 0; k < ROUTE_NCOUNT; k++)
        if (c[k]) atomicAdd(&bc[k], (unsigned long long)c[k]);
    __syncthreads();
    if (threadIdx.x < ROUTE_NCOUNT && bc[threadIdx.x]) atomicAdd(&stats[threadIdx.x], bc[threadIdx.x]);
}

}  // namespace rp

using rp::DevBuf;
using rp::Error;
using rp::Shard;

// =====================================================================
// Host side.
// =====================================================================
// Every local view's ring checksum into its shard's ring_csum, unless no call
// that can change a ring ran since the last time (timed as "checksum").
void rp_sim::refresh_ring_checksums() {
    bool have = !ring_csum_stale;
    for (auto& s : sh) have = have && s->ring_csum.p;
    if (have) return;
    for (auto& sp : sh) {
        Shard& s = *sp;
        if (!s.ring_csum.p) {
            s.ring_csum.alloc(s.n);
            RP_HIP(hipMemsetAsync(s.ring_csum.p, 0, s.ring_csum.bytes(), s.st));
        }
        s.timed(4, [&] {
            hipLaunchKernelGGL(rp::k_ring_checksums, dim3(std::min(rp::grid_for(s.nl, rp::NWAVE), 8192u)), dim3(rp::BLOCK),
                               0, s.st, s.d, s.ring_csum.p);
        });
        RP_HIP(hipGetLastError());
    }
    ring_csum_stale = false;
}

// What a route needs besides the simulation state: fresh ring checksums, the
// shards' base pointers and the bucket directory (about one point per bucket).
void rp_sim::route_prepare(bool checksums) {
    if (comm)
        throw Error(RP_ERR_UNSUPPORTED, "routing needs every node's view: not available on one rank of a multi-process "
                                        "or loop cluster");
    RP_HIP(hipSetDevice(dev));
    check_errors();
    if (checksums) refresh_ring_checksums();
    // (the census reads no checksum, but the pointer table below names the buffers)
    for (auto& s : sh)
        if (!s->ring_csum.p) {
            s->ring_csum.alloc(s->n);
            RP_HIP(hipMemsetAsync(s->ring_csum.p, 0, s->ring_csum.bytes(), s->st));
        }
    Shard& s0 = *sh.front();
    if (!route_dir.p) {
        uint32_t bits = 0;
        while (bits < 22 && (2ull << bits) <= s0.npts) bits++;
        const uint32_t nb = 1u << bits;
        route_dir.alloc((size_t)nb + 1);
        route_dir_shift = 32 - bits;
        hipLaunchKernelGGL(rp::k_route_dir, dim3(rp::grid_for((uint64_t)nb + 1, 256)), dim3(256), 0, s0.st,
                           (const uint32_t*)s0.pt_hash.p, s0.npts, route_dir_shift, nb, route_dir.p);
        RP_HIP(hipGetLastError());
    }
    if (!route_tab.p) {
        std::vector<rp::RouteShard> h;
        for (auto& s : sh) h.push_back(rp::RouteShard{s->in_ring.p, s->coll_owner.p, s->ring_count.p, s->ring_csum.p});
        route_tab.alloc(h.size());
        RP_HIP(hipMemcpy(route_tab.p, h.data(), h.size() * sizeof(rp::RouteShard), hipMemcpyHostToDevice));
    }
    sync_all();  // the route reads every shard's rows from the first shard's stream
}

template <bool UNIFORM>
void rp_sim::route_launch(const uint32_t* entries, const uint32_t* keys, uint64_t seed, uint64_t count, int32_t* dests,
                          uint8_t* outcomes, uint8_t* agrees, rp_route_stats* stats) {
    Shard& s0 = *sh.front();
    rp::SimDev S = s0.d;
    S.round = round;  // the clock of the next round, as the wire bridge
    S.part_start = part[0]; S.part_end = part[1]; S.part_split = part[2];
    DevBuf<unsigned long long> dst(rp::ROUTE_NCOUNT);
    RP_HIP(hipMemsetAsync(dst.p, 0, dst.bytes(), s0.st));
    // (launches of at most 2^31 requests: a thread's counters are 32-bit)
    for (uint64_t first = 0; first < count; first += 1ull << 31) {
        const uint64_t m = std::min<uint64_t>(count - first, 1ull << 31);
        s0.timed(5, [&] {
            hipLaunchKernelGGL(rp::k_route<UNIFORM>, dim3(std::min(rp::grid_for(m, 256), 16384u)), dim3(256), 0, s0.st, S,
                               (const rp::RouteShard*)route_tab.p, (const uint32_t*)s0.pt_hash.p,
                               (const int32_t*)s0.pt_server.p, (const int32_t*)s0.pt_coll.p, s0.npts,
                               (const uint32_t*)route_dir.p, route_dir_shift, UNIFORM ? nullptr : entries + first,
                               UNIFORM ? nullptr : keys + first, seed, first, m, dests ? dests + first : nullptr,
                               outcomes ? outcomes + first : nullptr, agrees ? agrees + first : nullptr, dst.p);
        });
        RP_HIP(hipGetLastError());
    }
    unsigned long long h[rp::ROUTE_NCOUNT];
    RP_HIP(hipMemcpyAsync(h, dst.p, sizeof h, hipMemcpyDeviceToHost, s0.st));
    RP_HIP(hipStreamSynchronize(s0.st));
    if (stats) {
        stats->local = h[rp::ROUTE_LOCAL];
        stats->delivered = h[rp::ROUTE_DELIVERED];
        stats->checksums_differ = h[rp::ROUTE_CHECKSUMS_DIFFER];
        stats->unreachable = h[rp::ROUTE_UNREACHABLE];
        stats->entry_dead = h[rp::ROUTE_ENTRY_DEAD];
        stats->misrouted = h[rp::ROUTE_MISROUTED];
        stats->requests = stats->local + stats->delivered + stats->checksums_differ + stats->unreachable + stats->entry_dead;
        stats->reserved = 0;
    }
}

extern "C" {

int rp_sim_ring_checksums(rp_sim* c, uint32_t* out, size_t cap) {
    return rp::guarded([&] {
        if (!c || !out) throw Error(RP_ERR_INVALID, "null pointer");
        if (cap < c->n) throw Error(RP_ERR_INVALID, "checksum buffer holds fewer than n entries");
        RP_HIP(hipSetDevice(c->dev));
        memset(out, 0, (size_t)c->n * 4);  // nodes of other processes' shards stay 0
        c->refresh_ring_checksums();
        for (auto& s : c->sh) {
            RP_HIP(hipMemcpyAsync(out + s->lo, s->ring_csum.p + s->lo, (size_t)s->nl * 4, hipMemcpyDeviceToHost, s->st));
            RP_HIP(hipStreamSynchronize(s->st));
        }
    });
}

int rp_sim_route(rp_sim* c, const uint32_t* entries, const uint32_t* key_hashes, size_t nk, int32_t* dests,
                 uint8_t* outcomes, uint8_t* owner_agrees, rp_route_stats* stats) {
    return rp::guarded([&] {
        if (!c || (nk && (!entries || !key_hashes))) throw Error(RP_ERR_INVALID, "null pointer");
        for (size_t i = 0; i < nk; i++)
            if (entries[i] >= c->n) throw Error(RP_ERR_INVALID, "request " + std::to_string(i) + ": entry node out of range");
        c->route_prepare();
        if (stats) memset(stats, 0, sizeof *stats);
        if (nk == 0) return;
        Shard& s0 = *c->sh.front();
        DevBuf<uint32_t> de(nk), dh(nk);
        DevBuf<int32_t> dd(dests ? nk : 0);
        DevBuf<uint8_t> dout(outcomes ? nk : 0), dag(owner_agrees ? nk : 0);
        RP_HIP(hipMemcpyAsync(de.p, entries, nk * 4, hipMemcpyHostToDevice, s0.st));
        RP_HIP(hipMemcpyAsync(dh.p, key_hashes, nk * 4, hipMemcpyHostToDevice, s0.st));
        c->route_launch<false>(de.p, dh.p, 0, nk, dd.p, dout.p, dag.p, stats);  // (ends with the stream drained)
        if (dests) RP_HIP(hipMemcpyAsync(dests, dd.p, nk * 4, hipMemcpyDeviceToHost, s0.st));
        if (outcomes) RP_HIP(hipMemcpyAsync(outcomes, dout.p, nk, hipMemcpyDeviceToHost, s0.st));
        if (owner_agrees) RP_HIP(hipMemcpyAsync(owner_agrees, dag.p, nk, hipMemcpyDeviceToHost, s0.st));
        RP_HIP(hipStreamSynchronize(s0.st));
    });
}

int rp_sim_route_uniform(rp_sim* c, uint64_t seed, uint64_t count, rp_route_stats* stats) {
    return rp::guarded([&] {
        if (!c || !stats) throw Error(RP_ERR_INVALID, "null pointer");
        c->route_prepare();
        memset(stats, 0, sizeof *stats);
        if (count) c->route_launch<true>(nullptr, nullptr, seed, count, nullptr, nullptr, nullptr, stats);
    });
}

}  // extern "C"
