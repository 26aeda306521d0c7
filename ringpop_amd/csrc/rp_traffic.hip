// ringpop_amd — the request tracker (rp_traffic_*): the kernels
// that advance the device-resident request table, the tracker that launches
// them and its C ABI.  None of the kernels is launched by a round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rp_block.h"
#include "rp_cluster.h"

namespace rp {

// ---- the request table

// rp_traffic_stats, then by_retries[outcome][0..8]
enum : uint32_t {
    TS_SUBMITTED = 0, TS_LOCAL = 1, TS_DELIVERED = 2, TS_REROUTED_LOCAL = 3, TS_FAILED = 4, TS_ENTRY_DEAD = 5,
    TS_PROXIED = 6, TS_SEND_UNREACHABLE = 7, TS_CHECKSUMS_DIFFER = 8, TS_RETRY_SCHEDULED = 9, TS_RETRY_ATTEMPTED = 10,
    TS_RETRY_REROUTED = 11, TS_RETRY_SUCCEEDED = 12, TS_RETRY_FAILED = 13, TS_MISROUTED = 14, TS_RESERVED = 15,
    TS_NSTATS = 16, TS_NREG = 15, TS_RETRY_SLOTS = 9, TS_NOUTCOMES = 5, TS_NSLOTS = TS_NSTATS + TS_NOUTCOMES * TS_RETRY_SLOTS
};
enum : uint32_t { TO_LOCAL = 0, TO_DELIVERED = 1, TO_REROUTED_LOCAL = 2, TO_FAILED = 3, TO_ENTRY_DEAD = 4, TO_PENDING = 255 };
// control words of a tracker (device): the pending count, the count the last
// compaction started from, where the last batch's survivors were appended,
// an overflow flag (a survivor that found no room: the host presizes the
// table, so it stays 0) and the largest pending count seen
enum : uint32_t { TC_COUNT = 0, TC_PREV = 1, TC_BASE = 2, TC_OVERFLOW = 3, TC_PEAK = 4, TC_NWORDS = 8 };
constexpr uint32_t TRAFFIC_TILE = 256;
constexpr uint32_t TRAFFIC_SCAN = 1024;
constexpr uint32_t TRAFFIC_MAX_SCHEDULE = 8;

// A pending record is two 16-byte words (rp_request_pending):
//   {id lo, id hi, entry, key_hash} {first_dest, due, submit_clock, retries}
// A final record is one (rp_request_result):
//   {dest, outcome | retries << 8, submit_clock, done_clock}
struct TrafficArgs {
    const RouteShard* tab;
    const uint32_t* pt_hash;
    const int32_t* pt_server;
    const int32_t* pt_coll;
    const uint32_t* dir;
    uint32_t npts, dir_shift;
    uint32_t max_retries, nschedule, enforce;
    uint32_t schedule[TRAFFIC_MAX_SCHEDULE];
    unsigned long long* cum;  // TS_NSLOTS cumulative counters
    unsigned long long* row;  // TS_NSTATS: the clock's history row
    uint4* results;           // by id, or null (not tracking)
    uint64_t results_cap;
    uint32_t* ctl;            // TC_*
    uint32_t* tile_count;     // survivors per tile of 256 records
    uint32_t* tile_off;       // their exclusive prefix sums
    uint32_t tiles_cap;
};

enum : int { TRAFFIC_PENDING = 0, TRAFFIC_BATCH = 1, TRAFFIC_UNIFORM = 2 };

// HashRing.lookup(h) in v's view from point p on; an empty ring gives -1
__device__ inline int32_t traffic_lookup(const SimDev& S, const TrafficArgs& A, uint32_t v, uint32_t p) {
    const RouteShard& t = A.tab[v / S.nl];
    if (t.ring_count[v] <= 0) return -1;
    return route_walk(route_ring_of(S, t, v), A.pt_server, A.pt_coll, A.npts, p);
}

// One step of the request table at clock S.round, one thread per record, a
// block per tile of 256 (grid-stride over tiles).
//   TRAFFIC_PENDING: the records of the pending table `recs` (ctl[TC_COUNT] of
//     them) that are due make their retry, in place;
//   TRAFFIC_BATCH / TRAFFIC_UNIFORM: requests [0, count) -- (entries[i],
//     keys[i]), or request first_index + i of k_route's generator -- get ids
//     first_id + i and make their first attempt; `recs` is a staging buffer.
// A request loops through send / error / retry (send.js's state machine,
// DESIGN.md §11) until it is final or due at a later clock.  The tile's
// surviving records are written at the front of the tile in their order
// (wave ballots and the waves' counts in LDS) and counted in tile_count; every
// thread has read its record before the first barrier, so the pending table
// is compacted in place.  Counters are kept per thread, summed per block in
// LDS and flushed with one atomic per counter and block to the cumulative row
// and to the clock's.
template <int MODE>
__global__ void __launch_bounds__(256) k_traffic_step(SimDev S, TrafficArgs A, uint4* recs, uint32_t cap,
                                                      const uint32_t* entries, const uint32_t* keys, uint64_t seed,
                                                      uint64_t first_index, uint64_t first_id, uint32_t count_in) {
    __shared__ unsigned long long bc[TS_NSLOTS];
    __shared__ uint32_t wcnt[TRAFFIC_TILE / 64];
    if (threadIdx.x < TS_NSLOTS) bc[threadIdx.x] = 0;
    const uint32_t count = min(MODE == TRAFFIC_PENDING ? A.ctl[TC_COUNT] : count_in, cap);
    const uint32_t ntiles = min((count + TRAFFIC_TILE - 1) / TRAFFIC_TILE, A.tiles_cap);
    const uint32_t clock = S.round;
    uint32_t c[TS_NREG];
#pragma unroll
    for (uint32_t k = 0; k < TS_NREG; k++) c[k] = 0;
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * TRAFFIC_TILE + threadIdx.x;
        bool alive = false, changed = false;
        uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
        if (i < count) {
            uint64_t id;
            uint32_t e, h, due = 0, submit = clock, retries = 0;
            int32_t d0 = -1;
            if (MODE == TRAFFIC_PENDING) {
                w0 = recs[2 * (size_t)i];
                w1 = recs[2 * (size_t)i + 1];
                id = (uint64_t)w0.x | (uint64_t)w0.y << 32;
                e = w0.z; h = w0.w;
                d0 = (int32_t)w1.x; due = w1.y; submit = w1.z; retries = w1.w;
            } else {
                id = first_id + i;
                if (MODE == TRAFFIC_UNIFORM) {
                    uint64_t s = seed + (first_index + i) * 0x9E3779B97F4A7C15ULL;
                    const uint64_t r = splitmix_next(s);
                    e = (uint32_t)(((r >> 32) * S.n) >> 32);
                    h = (uint32_t)r;
                } else {
                    e = entries[i];
                    h = keys[i];
                }
                c[TS_SUBMITTED]++;
            }
            if (MODE == TRAFFIC_PENDING && due > clock) {
                alive = true;
            } else {
                changed = true;
                uint32_t oc = TO_PENDING;
                int32_t dest = -1, target = -1;
                bool attempt = false;  // a send to `target` is ready
                const uint32_t p = route_point(A.pt_hash, A.npts, A.dir, A.dir_shift, h);
                if (MODE != TRAFFIC_PENDING) {
                    if (S.dead[e]) {
                        oc = TO_ENTRY_DEAD;
                    } else {
                        d0 = traffic_lookup(S, A, e, p);
                        if (d0 < 0 || (uint32_t)d0 == e) {
                            oc = TO_LOCAL;
                            dest = (int32_t)e;
                        } else {
                            c[TS_PROXIED]++;
                            target = d0;
                            attempt = true;
                        }
                    }
                }
                // (each pass ends a request or makes one more attempt: at most max_retries + 1)
                while (oc == TO_PENDING) {
                    if (!attempt) {  // a retry is due
                        if (S.dead[e]) { oc = TO_ENTRY_DEAD; break; }
                        retries++;
                        c[TS_RETRY_ATTEMPTED]++;
                        int32_t nd = traffic_lookup(S, A, e, p);
                        if (nd < 0) nd = (int32_t)e;
                        if (nd != d0) {
                            c[TS_RETRY_REROUTED]++;
                            if ((uint32_t)nd == e) { oc = TO_REROUTED_LOCAL; dest = (int32_t)e; break; }
                        }
                        c[TS_PROXIED]++;
                        target = nd;
                    }
                    attempt = false;
                    bool err = true;
                    if (unreachable(S, e, (uint32_t)target)) {
                        c[TS_SEND_UNREACHABLE]++;
                    } else {
                        const bool differ =
                            A.tab[e / S.nl].ring_csum[e] != A.tab[(uint32_t)target / S.nl].ring_csum[target];
                        if (differ) c[TS_CHECKSUMS_DIFFER]++;
                        err = differ && A.enforce;
                    }
                    dest = target;
                    if (!err) {
                        oc = TO_DELIVERED;
                        if (retries) c[TS_RETRY_SUCCEEDED]++;
                        if (traffic_lookup(S, A, (uint32_t)target, p) != target) c[TS_MISROUTED]++;
                        break;
                    }
                    if (retries >= A.max_retries) {
                        oc = TO_FAILED;
                        if (A.max_retries) c[TS_RETRY_FAILED]++;
                        break;
                    }
                    c[TS_RETRY_SCHEDULED]++;
                    // (retries differs per thread: a select over the unrolled entries keeps the schedule,
                    // a kernel argument, in scalar registers and out of scratch)
                    uint32_t delay = 0;
#pragma unroll
                    for (uint32_t k = 0; k < TRAFFIC_MAX_SCHEDULE; k++)
                        if (k == min(retries, A.nschedule - 1)) delay = A.schedule[k];
                    due = clock + delay;
                    if (due > clock) break;
                }
                alive = oc == TO_PENDING;
                if (alive) {
                    w0 = make_uint4((uint32_t)id, (uint32_t)(id >> 32), e, h);
                    w1 = make_uint4((uint32_t)d0, due, submit, retries);
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < TS_NOUTCOMES; k++) c[TS_LOCAL + k] += oc == k ? 1u : 0u;
                    atomicAdd(&bc[TS_NSTATS + oc * TS_RETRY_SLOTS + min(retries, TS_RETRY_SLOTS - 1)], 1ull);
                }
                if (A.results && id < A.results_cap && (!alive || MODE != TRAFFIC_PENDING))
                    A.results[id] = alive ? make_uint4((uint32_t)d0, TO_PENDING, submit, 0u)
                                          : make_uint4((uint32_t)dest, oc | retries << 8, submit, clock);
            }
        }
        const uint64_t m = __ballot(alive);
        const uint32_t lane = lane_id(), w = wave_id();
        const uint32_t rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[w] = __popcll(m);
        __syncthreads();
        uint32_t off = 0, total = 0;
#pragma unroll
        for (uint32_t q = 0; q < TRAFFIC_TILE / 64; q++) {
            const uint32_t v = wcnt[q];
            off += q < w ? v : 0u;
            total += v;
        }
        if (alive) {
            const size_t j = (size_t)tile * TRAFFIC_TILE + off + rank;
            if (MODE != TRAFFIC_PENDING || changed || j != i) {
                recs[2 * j] = w0;
                recs[2 * j + 1] = w1;
            }
        }
        if (threadIdx.x == 0) A.tile_count[tile] = total;
        __syncthreads();  // (wcnt is rewritten by the next tile)
    }
#pragma unroll
    for (uint32_t k = 0; k < TS_NREG; k++)
        if (c[k]) atomicAdd(&bc[k], (unsigned long long)c[k]);
    __syncthreads();
    if (threadIdx.x < TS_NSLOTS && bc[threadIdx.x]) {
        atomicAdd(&A.cum[threadIdx.x], bc[threadIdx.x]);
        if (threadIdx.x < TS_NSTATS) atomicAdd(&A.row[threadIdx.x], bc[threadIdx.x]);
    }
}

// Exclusive prefix sums of the tiles' survivor counts by one block (the tiles
// in chunks of 1024: a shuffle scan per wave, the waves' sums through LDS),
// then the control words.  APPEND (a submitted batch of count_in requests):
// the survivors go after the pending records, ctl[TC_BASE] = the old count;
// otherwise (the pending table of ctl[TC_COUNT] records) they replace them.
template <bool APPEND>
__global__ void __launch_bounds__(TRAFFIC_SCAN) k_traffic_scan(TrafficArgs A, uint32_t count_in, uint32_t cap_src,
                                                               uint32_t cap_table) {
    __shared__ uint32_t wsum[TRAFFIC_SCAN / 64];
    const uint32_t old = A.ctl[TC_COUNT];
    const uint32_t count = min(APPEND ? count_in : old, cap_src);
    const uint32_t ntiles = min((count + TRAFFIC_TILE - 1) / TRAFFIC_TILE, A.tiles_cap);
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    uint32_t running = 0;
    __syncthreads();  // (every thread has read the count before it is replaced)
    for (uint32_t base = 0; base < ntiles; base += TRAFFIC_SCAN) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < ntiles ? A.tile_count[t] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o);
            if ((int)lane >= o) incl += y;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t woff = 0, total = 0;
#pragma unroll
        for (uint32_t q = 0; q < TRAFFIC_SCAN / 64; q++) {
            const uint32_t s = wsum[q];
            woff += q < w ? s : 0u;
            total += s;
        }
        if (t < ntiles) A.tile_off[t] = running + woff + incl - v;
        running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        uint32_t now;
        if (APPEND) {
            A.ctl[TC_BASE] = old;
            now = old + running;
            if (now > cap_table || now < old) {
                A.ctl[TC_OVERFLOW] = 1;
                now = cap_table;
            }
        } else {
            A.ctl[TC_PREV] = count;
            now = running;
        }
        A.ctl[TC_COUNT] = now;
        if (now > A.ctl[TC_PEAK]) A.ctl[TC_PEAK] = now;
    }
}

// The tiles' survivors (at the front of each tile of `src`) to their places
// in `dst`: tile_off[tile] + rank, after ctl[TC_BASE] records when APPEND.
template <bool APPEND>
__global__ void __launch_bounds__(256) k_traffic_scatter(TrafficArgs A, const uint4* src, uint4* dst, uint32_t count_in,
                                                         uint32_t cap_src, uint32_t cap_dst) {
    const uint32_t count = min(APPEND ? count_in : A.ctl[TC_PREV], cap_src);
    const uint32_t ntiles = min((count + TRAFFIC_TILE - 1) / TRAFFIC_TILE, A.tiles_cap);
    const uint64_t base = APPEND ? A.ctl[TC_BASE] : 0u;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t cnt = min(A.tile_count[tile], TRAFFIC_TILE);
        if (threadIdx.x >= cnt) continue;
        const uint64_t j = base + A.tile_off[tile] + threadIdx.x;
        if (j >= cap_dst) continue;  // (k_traffic_scan raised TC_OVERFLOW)
        const size_t i = (size_t)tile * TRAFFIC_TILE + threadIdx.x;
        dst[2 * j] = src[2 * i];
        dst[2 * j + 1] = src[2 * i + 1];
    }
}

}  // namespace rp

using rp::DevBuf;
using rp::Error;
using rp::Shard;

// =====================================================================
// Host side.  A tracker keeps its request table on its simulation's device
// and runs on the first shard's stream, like a route.
// =====================================================================
struct rp_traffic {
    rp_sim* sim = nullptr;
    rp_traffic_config cfg{};
    uint64_t lifetime = 0;             // rounds a request can stay pending: the delays of its max_retries retries
    DevBuf<uint4> tab[2];              // the pending table and the buffer the next compaction writes (2 words a record)
    int cur = 0;
    uint64_t alloc = 0;                // records each holds (<= cfg.capacity)
    DevBuf<uint4> stage;               // a submitted chunk's surviving records, tile by tile
    DevBuf<uint32_t> tile_count, tile_off, ctl;
    DevBuf<unsigned long long> cum, hist;
    uint64_t hist_rows = 0;
    DevBuf<uint4> results;             // by id (tracking)
    uint64_t results_cap = 0;
    uint64_t next_id = 0, run_index = 0;
    uint64_t bound = 0;                // >= the device's pending count
    uint32_t h_ctl[rp::TC_NWORDS] = {0};
    rp::SpanTimer tm;                  // cfg.timing: 0 poll, 1 submit
    double ms[2] = {0, 0};
    uint64_t calls[2] = {0, 0};
    static constexpr uint64_t CHUNK = 1ull << 20;  // requests per submit launch

    hipStream_t st() const { return sim->sh.front()->st; }

    // `count` elements with the first `keep` kept and the rest set to `fill` bytes
    template <class T>
    void grow(DevBuf<T>& b, uint64_t count, uint64_t keep, int fill) {
        DevBuf<T> nb((size_t)count);
        if (keep) RP_HIP(hipMemcpyAsync(nb.p, b.p, (size_t)keep * sizeof(T), hipMemcpyDeviceToDevice, st()));
        if (count > keep) RP_HIP(hipMemsetAsync(nb.p + keep, fill, (size_t)(count - keep) * sizeof(T), st()));
        RP_HIP(hipStreamSynchronize(st()));
        b = std::move(nb);
    }
    // room for `need` pending records, or RP_ERR_CAPACITY (nothing changed)
    void ensure_table(uint64_t need) {
        if (need > cfg.capacity)
            throw Error(RP_ERR_CAPACITY, "the pending table would need " + std::to_string(need) + " records, capacity is " +
                                             std::to_string(cfg.capacity));
        if (need > alloc) {
            const uint64_t na = std::min<uint64_t>(cfg.capacity, std::max<uint64_t>({need, alloc * 2, 1024}));
            grow(tab[cur], 2 * na, 2 * bound, 0);
            tab[cur ^ 1].alloc((size_t)(2 * na));
            alloc = na;
        }
        const uint64_t tiles = (std::max(alloc, CHUNK) + rp::TRAFFIC_TILE - 1) / rp::TRAFFIC_TILE;
        if (tile_count.n < tiles) { tile_count.alloc((size_t)tiles); tile_off.alloc((size_t)tiles); }
    }
    void ensure_history(uint64_t rows) {
        if (rows <= hist_rows) return;
        const uint64_t nr = std::max<uint64_t>({rows, hist_rows * 2, 64});
        grow(hist, nr * rp::TS_NSTATS, hist_rows * rp::TS_NSTATS, 0);
        hist_rows = nr;
    }
    void ensure_results(uint64_t ids) {
        if (!cfg.track || ids <= results_cap) return;
        const uint64_t nr = std::max<uint64_t>({ids, results_cap * 2, 1024});
        grow(results, nr, results_cap, 0xFF);
        results_cap = nr;
    }
    void ensure_stage(uint64_t n) {
        const uint64_t m = std::min(n, CHUNK);
        if (stage.n < 2 * m) stage.alloc((size_t)(2 * m));
    }
    // the control words; a survivor that found no room is an error (the table is presized: never expected)
    void read_ctl() {
        RP_HIP(hipMemcpyAsync(h_ctl, ctl.p, sizeof h_ctl, hipMemcpyDeviceToHost, st()));
        RP_HIP(hipStreamSynchronize(st()));
        bound = h_ctl[rp::TC_COUNT];
        if (h_ctl[rp::TC_OVERFLOW]) throw Error(RP_ERR_STATE, "the pending table overflowed on the device");
    }
    // fresh ring checksums and routing tables, then the pending count
    void prepare() {
        sim->route_prepare();
        read_ctl();
    }
    rp::TrafficArgs args() {
        Shard& s0 = *sim->sh.front();
        rp::TrafficArgs A{};
        A.tab = sim->route_tab.p;
        A.pt_hash = s0.pt_hash.p; A.pt_server = s0.pt_server.p; A.pt_coll = s0.pt_coll.p;
        A.dir = sim->route_dir.p;
        A.npts = s0.npts; A.dir_shift = sim->route_dir_shift;
        A.max_retries = (uint32_t)cfg.max_retries; A.nschedule = cfg.nschedule;
        A.enforce = cfg.enforce_consistency ? 1u : 0u;
        for (uint32_t i = 0; i < rp::TRAFFIC_MAX_SCHEDULE; i++) A.schedule[i] = cfg.schedule[i];
        A.cum = cum.p;
        A.row = hist.p + (size_t)sim->round * rp::TS_NSTATS;
        A.results = results.p; A.results_cap = results_cap;
        A.ctl = ctl.p;
        A.tile_count = tile_count.p; A.tile_off = tile_off.p;
        A.tiles_cap = (uint32_t)tile_count.n;
        return A;
    }
    rp::SimDev clocked() {
        rp::SimDev S = sim->sh.front()->d;
        S.round = sim->round;  // the clock of the next round, as a route
        S.part_start = sim->part[0]; S.part_end = sim->part[1]; S.part_split = sim->part[2];
        return S;
    }
    template <class F>
    void timed(int cat, F&& launch) {
        tm.timed(st(), cat, cfg.timing != 0, launch);
    }
    static unsigned tile_grid(uint64_t records) {
        return std::min(rp::grid_for(std::max<uint64_t>(records, 1), rp::TRAFFIC_TILE), 8192u);
    }
    // every due pending record retries; the survivors, in order, become the table (history row presized)
    void launch_poll() {
        if (!alloc) return;  // nothing was ever submitted
        const rp::TrafficArgs A = args();
        const rp::SimDev S = clocked();
        const uint32_t cap = (uint32_t)alloc;
        timed(0, [&] {
            const dim3 grid(tile_grid(bound));
            hipLaunchKernelGGL(rp::k_traffic_step<rp::TRAFFIC_PENDING>, grid, dim3(256), 0, st(), S, A, tab[cur].p, cap,
                               (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint64_t)0, (uint64_t)0, (uint64_t)0, 0u);
            hipLaunchKernelGGL(rp::k_traffic_scan<false>, dim3(1), dim3(rp::TRAFFIC_SCAN), 0, st(), A, 0u, cap, cap);
            hipLaunchKernelGGL(rp::k_traffic_scatter<false>, grid, dim3(256), 0, st(), A, (const uint4*)tab[cur].p,
                               tab[cur ^ 1].p, 0u, cap, cap);
        });
        RP_HIP(hipGetLastError());
        cur ^= 1;
    }
    // first attempts of n requests (device arrays, or the generator from index `first`); survivors are appended
    void launch_submit(const uint32_t* entries, const uint32_t* keys, uint64_t seed, uint64_t first, uint64_t n) {
        const rp::TrafficArgs A = args();
        const rp::SimDev S = clocked();
        const uint32_t cap_stage = (uint32_t)(stage.n / 2), cap = (uint32_t)alloc;
        timed(1, [&] {
            for (uint64_t off = 0; off < n; off += CHUNK) {
                const uint32_t m = (uint32_t)std::min(n - off, CHUNK);
                const dim3 grid(tile_grid(m));
                if (entries)
                    hipLaunchKernelGGL(rp::k_traffic_step<rp::TRAFFIC_BATCH>, grid, dim3(256), 0, st(), S, A, stage.p,
                                       cap_stage, entries + off, keys + off, seed, first + off, next_id + off, m);
                else
                    hipLaunchKernelGGL(rp::k_traffic_step<rp::TRAFFIC_UNIFORM>, grid, dim3(256), 0, st(), S, A, stage.p,
                                       cap_stage, (const uint32_t*)nullptr, (const uint32_t*)nullptr, seed, first + off,
                                       next_id + off, m);
                hipLaunchKernelGGL(rp::k_traffic_scan<true>, dim3(1), dim3(rp::TRAFFIC_SCAN), 0, st(), A, m, cap_stage, cap);
                hipLaunchKernelGGL(rp::k_traffic_scatter<true>, grid, dim3(256), 0, st(), A, (const uint4*)stage.p,
                                   tab[cur].p, m, cap_stage, cap);
            }
        });
        RP_HIP(hipGetLastError());
        next_id += n;
    }
    void submit(const uint32_t* d_entries, const uint32_t* d_keys, uint64_t seed, uint64_t first, uint64_t n) {
        ensure_table(bound + n);
        ensure_results(next_id + n);
        ensure_history((uint64_t)sim->round + 1);
        ensure_stage(n);
        launch_submit(d_entries, d_keys, seed, first, n);
        read_ctl();
    }
    void collect_timing() {
        RP_HIP(hipStreamSynchronize(st()));
        tm.collect([&](int cat, float t) {
            ms[cat] += t;
            calls[cat]++;
        });
    }
};

extern "C" {

int rp_traffic_create(rp_sim* sim, const rp_traffic_config* cfg, rp_traffic** out) {
    return rp::guarded([&] {
        if (!sim || !out) throw Error(RP_ERR_INVALID, "null pointer");
        if (sim->comm)
            throw Error(RP_ERR_UNSUPPORTED, "request traffic needs every node's view: not available on one rank of a "
                                            "multi-process or loop cluster");
        RP_HIP(hipSetDevice(sim->dev));
        std::unique_ptr<rp_traffic> t(new rp_traffic());
        t->sim = sim;
        rp_traffic_config c{};
        c.max_retries = -1;
        c.enforce_consistency = -1;
        if (cfg) c = *cfg;
        if (c.max_retries < 0) c.max_retries = 3;
        if (c.enforce_consistency < 0) c.enforce_consistency = 1;
        if (c.nschedule == 0) {
            // RETRY_SCHEDULE [0, 1, 3.5] s (send.js:49) in 200 ms periods, rounded up
            c.nschedule = 3;
            c.schedule[0] = 0; c.schedule[1] = 5; c.schedule[2] = 18;
        }
        if (c.capacity == 0) c.capacity = 1ull << 20;
        if (c.max_retries > (int32_t)(rp::TS_RETRY_SLOTS - 1)) throw Error(RP_ERR_INVALID, "max_retries is at most 8");
        if (c.nschedule > rp::TRAFFIC_MAX_SCHEDULE) throw Error(RP_ERR_INVALID, "the schedule has at most 8 entries");
        if (c.capacity > (1ull << 30)) throw Error(RP_ERR_INVALID, "capacity is at most 2^30 records");
        for (uint32_t i = 0; i < c.nschedule; i++)
            if (c.schedule[i] > (1u << 20)) throw Error(RP_ERR_INVALID, "a retry delay is at most 2^20 rounds");
        for (uint32_t i = c.nschedule; i < rp::TRAFFIC_MAX_SCHEDULE; i++) c.schedule[i] = 0;
        t->cfg = c;
        for (int32_t r = 0; r < c.max_retries; r++) t->lifetime += c.schedule[std::min<uint32_t>((uint32_t)r, c.nschedule - 1)];
        t->ctl.alloc(rp::TC_NWORDS);
        t->cum.alloc(64);
        RP_HIP(hipMemsetAsync(t->ctl.p, 0, t->ctl.bytes(), t->st()));
        RP_HIP(hipMemsetAsync(t->cum.p, 0, t->cum.bytes(), t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
        *out = t.release();
    });
}

int rp_traffic_destroy(rp_traffic* t) {
    return rp::guarded([&] {
        delete t;  // (its buffers only: hipFree waits for the device; the simulation is not touched)
    });
}

int rp_traffic_submit(rp_traffic* t, const uint32_t* entries, const uint32_t* key_hashes, size_t n, uint64_t* first_id) {
    return rp::guarded([&] {
        if (!t || (n && (!entries || !key_hashes))) throw Error(RP_ERR_INVALID, "null pointer");
        for (size_t i = 0; i < n; i++)
            if (entries[i] >= t->sim->n) throw Error(RP_ERR_INVALID, "request " + std::to_string(i) + ": entry node out of range");
        t->prepare();
        if (first_id) *first_id = t->next_id;
        if (n == 0) return;
        t->ensure_table(t->bound + n);  // (RP_ERR_CAPACITY before anything is copied or changed)
        DevBuf<uint32_t> de(n), dh(n);
        RP_HIP(hipMemcpyAsync(de.p, entries, n * 4, hipMemcpyHostToDevice, t->st()));
        RP_HIP(hipMemcpyAsync(dh.p, key_hashes, n * 4, hipMemcpyHostToDevice, t->st()));
        t->submit(de.p, dh.p, 0, 0, n);  // (ends with the stream drained)
    });
}

int rp_traffic_submit_uniform(rp_traffic* t, uint64_t seed, uint64_t first, uint64_t count) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        t->prepare();
        if (count) t->submit(nullptr, nullptr, seed, first, count);
    });
}

int rp_traffic_poll(rp_traffic* t) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        t->prepare();
        t->ensure_history((uint64_t)t->sim->round + 1);
        t->launch_poll();
        t->read_ctl();
    });
}

int rp_traffic_run(rp_traffic* t, int k_rounds, int churn_active, uint64_t per_round, uint64_t seed) {
    return rp::guarded([&] {
        if (!t || k_rounds < 0) throw Error(RP_ERR_INVALID, "bad argument");
        RP_HIP(hipSetDevice(t->sim->dev));
        t->read_ctl();
        // a batch stays at most `lifetime` rounds: at most that many earlier batches beside the newest
        const uint64_t batches = std::min<uint64_t>((uint64_t)k_rounds, t->lifetime + 1);
        if (per_round && batches > (1ull << 31) / per_round) throw Error(RP_ERR_CAPACITY, "per_round x rounds overflows");
        const uint64_t need = t->bound + per_round * batches;
        if (per_round || t->bound) t->ensure_table(need);
        t->ensure_results(t->next_id + per_round * (uint64_t)k_rounds);
        t->ensure_history((uint64_t)t->sim->round + (uint64_t)k_rounds + 1);
        t->ensure_stage(per_round);
        uint64_t host_bound = t->bound;
        for (int r = 0; r < k_rounds; r++) {
            t->sim->rings_changed();
            t->sim->run(1, churn_active != 0);
            t->sim->route_prepare();  // (rp_sim_round's error check; no other readback)
            t->bound = host_bound;
            t->launch_poll();
            if (per_round) {
                t->launch_submit(nullptr, nullptr, seed, t->run_index, per_round);
                t->run_index += per_round;
                host_bound = std::min(need, host_bound + per_round);
            }
        }
        t->read_ctl();
    });
}

int rp_traffic_read_stats(rp_traffic* t, rp_traffic_stats* cumulative, uint64_t* by_retries) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        RP_HIP(hipSetDevice(t->sim->dev));
        unsigned long long h[64];
        RP_HIP(hipMemcpyAsync(h, t->cum.p, sizeof h, hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
        static_assert(sizeof(rp_traffic_stats) == rp::TS_NSTATS * 8, "rp_traffic_stats is 16 x u64");
        if (cumulative) memcpy(cumulative, h, sizeof *cumulative);
        if (by_retries)
            for (uint32_t i = 0; i < rp::TS_NOUTCOMES * rp::TS_RETRY_SLOTS; i++) by_retries[i] = h[rp::TS_NSTATS + i];
    });
}

int rp_traffic_history(rp_traffic* t, uint32_t first_clock, uint32_t count, rp_traffic_stats* rows) {
    return rp::guarded([&] {
        if (!t || (count && !rows)) throw Error(RP_ERR_INVALID, "null pointer");
        RP_HIP(hipSetDevice(t->sim->dev));
        if (!count) return;
        memset(rows, 0, (size_t)count * sizeof *rows);  // (clocks without a call: zero rows)
        if (first_clock >= t->hist_rows) return;
        const uint64_t m = std::min<uint64_t>(count, t->hist_rows - first_clock);
        RP_HIP(hipMemcpyAsync(rows, t->hist.p + (size_t)first_clock * rp::TS_NSTATS, (size_t)m * sizeof *rows,
                              hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
    });
}

int rp_traffic_pending(rp_traffic* t, rp_request_pending* out, size_t cap, uint64_t* count) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        RP_HIP(hipSetDevice(t->sim->dev));
        t->read_ctl();
        if (count) *count = t->bound;
        if (!out) return;
        if (cap < t->bound) throw Error(RP_ERR_INVALID, "pending buffer too small");
        static_assert(sizeof(rp_request_pending) == 32, "a pending record is two 16-byte words");
        if (t->bound)
            RP_HIP(hipMemcpyAsync(out, t->tab[t->cur].p, (size_t)t->bound * 32, hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
    });
}

int rp_traffic_results(rp_traffic* t, uint64_t first_id, size_t n, rp_request_result* out) {
    return rp::guarded([&] {
        if (!t || (n && !out)) throw Error(RP_ERR_INVALID, "null pointer");
        if (!t->cfg.track) throw Error(RP_ERR_INVALID, "the tracker was created without `track`");
        if (first_id > t->next_id || n > t->next_id - first_id) throw Error(RP_ERR_INVALID, "ids beyond the last submitted");
        RP_HIP(hipSetDevice(t->sim->dev));
        static_assert(sizeof(rp_request_result) == 16, "a final record is one 16-byte word");
        if (n) RP_HIP(hipMemcpyAsync(out, t->results.p + first_id, n * 16, hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
    });
}

int rp_traffic_times(rp_traffic* t, double* ms2, uint64_t* calls2, uint64_t* peak_pending) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        RP_HIP(hipSetDevice(t->sim->dev));
        t->collect_timing();
        t->read_ctl();
        for (int i = 0; i < 2; i++) {
            if (ms2) ms2[i] = t->ms[i];
            if (calls2) calls2[i] = t->calls[i];
        }
        if (peak_pending) *peak_pending = t->h_ctl[rp::TC_PEAK];
    });
}

}  // extern "C"
