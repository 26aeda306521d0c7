// ringpop_amd — the kernels of the request tracker (rp_traffic_*; DESIGN.md
// §11) and their launches.  None of them is launched by a round.
#include <hip/hip_runtime.h>

#include "rp_block.h"
#include "rp_common.h"
#include "rp_sim.h"
#include "rp_traffic.h"

namespace rp {

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

void traffic_step(int mode, unsigned grid, hipStream_t st, const SimDev& S, const TrafficArgs& A, uint4* recs, uint32_t cap,
                  const uint32_t* entries, const uint32_t* keys, uint64_t seed, uint64_t first_index, uint64_t first_id,
                  uint32_t count) {
    if (mode == TRAFFIC_PENDING)
        hipLaunchKernelGGL(k_traffic_step<TRAFFIC_PENDING>, dim3(grid), dim3(256), 0, st, S, A, recs, cap, entries, keys,
                           seed, first_index, first_id, count);
    else if (mode == TRAFFIC_BATCH)
        hipLaunchKernelGGL(k_traffic_step<TRAFFIC_BATCH>, dim3(grid), dim3(256), 0, st, S, A, recs, cap, entries, keys, seed,
                           first_index, first_id, count);
    else
        hipLaunchKernelGGL(k_traffic_step<TRAFFIC_UNIFORM>, dim3(grid), dim3(256), 0, st, S, A, recs, cap, entries, keys,
                           seed, first_index, first_id, count);
}

void traffic_scan(bool append, hipStream_t st, const TrafficArgs& A, uint32_t count, uint32_t cap_src, uint32_t cap_table) {
    if (append)
        hipLaunchKernelGGL(k_traffic_scan<true>, dim3(1), dim3(TRAFFIC_SCAN), 0, st, A, count, cap_src, cap_table);
    else
        hipLaunchKernelGGL(k_traffic_scan<false>, dim3(1), dim3(TRAFFIC_SCAN), 0, st, A, count, cap_src, cap_table);
}

void traffic_scatter(bool append, unsigned grid, hipStream_t st, const TrafficArgs& A, const uint4* src, uint4* dst,
                     uint32_t count, uint32_t cap_src, uint32_t cap_dst) {
    if (append)
        hipLaunchKernelGGL(k_traffic_scatter<true>, dim3(grid), dim3(256), 0, st, A, src, dst, count, cap_src, cap_dst);
    else
        hipLaunchKernelGGL(k_traffic_scatter<false>, dim3(grid), dim3(256), 0, st, A, src, dst, count, cap_src, cap_dst);
}

}  // namespace rp
