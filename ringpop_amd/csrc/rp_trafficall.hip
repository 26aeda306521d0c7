// ringpop_amd — the multi-key request tracker (rp_traffic_all_*; DESIGN.md
// §23): RingPop.handleOrProxyAll's requests across rounds.  A request's keys are
// grouped at submission as rp_sim_route_all groups them; every group is a send
// that goes through the request proxy's retry machine (rp_traffic's rules), and
// a retry whose keys no longer share one owner in the entry's view aborts
// (send.js:105-113).  The kernels that advance the device-resident request
// table, the tracker that launches them and its C ABI.  None of the kernels is
// launched by a round; every store is a vector store or an integer atomic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rp_block.h"
#include "rp_routeall.h"

namespace rp {

// rp_traffic_all_stats as words, then by_retries[outcome][0..8]
enum : uint32_t {
    TA_REQUESTS = 0, TA_REQ_ENTRY_DEAD, TA_REQ_EMPTY, TA_REQ_OK, TA_REQ_FAILED, TA_KEYS, TA_SENDS,
    TA_LOCAL = 7, TA_DELIVERED, TA_REROUTED_LOCAL, TA_FAILED, TA_ENTRY_DEAD, TA_ABORTED,
    TA_PROXIED = 13, TA_SEND_UNREACHABLE, TA_CHECKSUMS_DIFFER, TA_RETRY_SCHEDULED, TA_RETRY_ATTEMPTED, TA_RETRY_REROUTED,
    TA_RETRY_SUCCEEDED, TA_RETRY_FAILED, TA_MISROUTED_KEYS,
    TA_NSTATS = 24, TA_RETRY_SLOTS = 9, TA_NOUTCOMES = 6, TA_NSLOTS = TA_NSTATS + TA_NOUTCOMES * TA_RETRY_SLOTS
};
enum : uint32_t { AO_LOCAL = 0, AO_DELIVERED = 1, AO_REROUTED_LOCAL = 2, AO_FAILED = 3, AO_ENTRY_DEAD = 4, AO_ABORTED = 5,
                  AO_PENDING = 255 };
// control words of a tracker (device): pending requests and their keys, the
// request count the last compaction started from, where the last batch's
// survivors were appended, an overflow flag (the host presizes: it stays 0)
enum : uint32_t { AC_COUNT = 0, AC_KEYS = 1, AC_PREV = 2, AC_BASE = 3, AC_BASE_KEYS = 4, AC_OVERFLOW = 5, AC_NWORDS = 8 };
constexpr uint32_t TA_BLOCK = 256;
constexpr uint32_t TA_TILE = 256;   // requests of a compaction tile: one block's, in 256 / (256 / W) passes
constexpr uint32_t TA_SCAN = 1024;
constexpr uint32_t TA_MAX_SCHEDULE = 8;
constexpr uint32_t TA_NEVER = 0xFFFFFFFFu;

// Device state.  A pending request is two 16-byte words
//   {id lo, id hi, entry, key offset} {nkeys | ngroups << 16, submit clock, next_due, first_error_clock}
// (next_due: the minimum over its open sends).  Its keys lie in the key arena
// from its key offset, group-major: group 0's keys in input order, then group
// 1's.  Group j is the 16-byte word at key offset + j of the group arena:
//   {d0, due, retries | outcome << 8, key begin | key count << 16}
// Final sends of a pending request are kept: its outcome, fanout and largest
// retry count are derived from them.
struct TallArgs {
    OwnArgs own;  // the routing tables and the points
    uint32_t max_retries, nschedule, enforce;
    uint32_t schedule[TA_MAX_SCHEDULE];
    unsigned long long* cum;  // TA_NSLOTS
    uint4* results;           // by id, or null (not tracking)
    uint64_t results_cap;
    uint32_t* ctl;            // AC_*
    uint32_t* keep;           // per request of the step: its keys if it survives, else 0
    uint2* tile_sum;          // {survivors, their keys} per tile of 256 requests
    uint2* tile_off;          // their exclusive prefix sums
    uint32_t tiles_cap;
};
// a table of requests with its arenas
struct TallTable {
    uint4* req;
    uint32_t* keys;
    uint4* groups;
    uint32_t cap_req, cap_keys;
};
// a submitted batch (CSR, or the generator: uniform_k keys a request)
struct TallBatch {
    const uint32_t* entries;
    const uint64_t* offsets;
    const uint32_t* keys;
    uint64_t seed, first_index, first_id;
    uint32_t uniform_k;
};

enum : int { TALL_PENDING = 0, TALL_BATCH = 1, TALL_UNIFORM = 2 };

// A lane's counters: named fields, set and flushed one by one, so that each is
// a register (the kernels use no scratch; see tall_send on alternatives).
#define TALL_COUNTERS(X)                                                                                              \
    X(requests, TA_REQUESTS) X(req_entry_dead, TA_REQ_ENTRY_DEAD) X(req_empty, TA_REQ_EMPTY) X(req_ok, TA_REQ_OK)      \
    X(req_failed, TA_REQ_FAILED) X(keys, TA_KEYS) X(sends, TA_SENDS) X(proxied, TA_PROXIED)                            \
    X(send_unreachable, TA_SEND_UNREACHABLE) X(checksums_differ, TA_CHECKSUMS_DIFFER)                                  \
    X(retry_scheduled, TA_RETRY_SCHEDULED) X(retry_attempted, TA_RETRY_ATTEMPTED) X(retry_rerouted, TA_RETRY_REROUTED) \
    X(retry_succeeded, TA_RETRY_SUCCEEDED) X(retry_failed, TA_RETRY_FAILED) X(misrouted_keys, TA_MISROUTED_KEYS)
struct TallCounts {
#define X(name, slot) uint32_t name = 0;
    TALL_COUNTERS(X)
#undef X
    __device__ inline void flush(unsigned long long* bc) const {
#define X(name, slot) if (name) atomicAdd(&bc[slot], (unsigned long long)name);
        TALL_COUNTERS(X)
#undef X
    }
};

// A request of more than 64 keys: one wave's LDS.  Submission: an open-
// addressing table owner -> group rank (rp_routeall.hip's), the groups' owners
// and key counts, and each key's group and place in it.  Poll: the groups' key
// begins and due flags, each key's group and owner in the entry's view.
struct TallLds {
    int32_t dest[2 * RA_MAX_K];   // -1: free
    uint16_t rank[2 * RA_MAX_K];
    int32_t gdest[RA_MAX_K];      // poll: 1 = the send's keys diverge
    int32_t gres[RA_MAX_K];       // where the send was delivered in this call, else -1
    int32_t own[RA_MAX_K];
    uint32_t p0[RA_MAX_K];
    uint16_t gcnt[RA_MAX_K], gbeg[RA_MAX_K], kgrp[RA_MAX_K], widx[RA_MAX_K];
    uint8_t gflag[RA_MAX_K];
};

// what the lanes of a request know of it
struct TallRequest {
    uint64_t id;
    uint32_t e, K, ng, off, submit, first_err, cse;
    int32_t rce;
    bool active, live;  // live: the entry has not fail-stopped
};

struct TallSend {
    int32_t d0, dest;
    uint32_t due, retries, oc;
};

// One send from its next event to its end or to a later clock: rp_traffic's
// rules 2-5 with the multi-key retry (send.js:105-127).  attempt: a send to d0
// is ready (submission); otherwise a retry is due.  The entry's view does not
// change within a call, so what a retry's lookups give -- diverge: the send's
// keys have more than one owner; nd: the one owner -- holds for every retry of
// a zero delay too.
__device__ __forceinline__ void tall_send(const SimDev& S, const TallArgs& A, const TallRequest& q, bool attempt, bool diverge,
                                 int32_t nd, TallSend& s, TallCounts& c) {
    const uint32_t clock = S.round;
    int32_t target = s.d0;
    // (each pass ends the send or makes one more attempt: at most max_retries + 1)
    while (s.oc == AO_PENDING) {
        if (!attempt) {
            if (!q.live) { s.oc = AO_ENTRY_DEAD; s.dest = -1; break; }
            s.retries++;
            if (diverge) { s.oc = AO_ABORTED; s.dest = s.d0; break; }
            c.retry_attempted++;
            if (nd != s.d0) {
                c.retry_rerouted++;
                if ((uint32_t)nd == q.e) { s.oc = AO_REROUTED_LOCAL; s.dest = (int32_t)q.e; break; }
            }
            c.proxied++;
            target = nd;
        }
        attempt = false;
        // (the counters of alternatives are added branch-free: inside this function they are fields behind a
        // reference, and a store to one of two of them chosen by a branch becomes one store through a selected
        // address, which keeps them out of registers after inlining)
        const bool cutoff = unreachable(S, q.e, (uint32_t)target);
        const bool differ = !cutoff && A.own.tab[(uint32_t)target / A.own.nl].ring_csum[target] != q.cse;
        c.send_unreachable += cutoff ? 1u : 0u;
        c.checksums_differ += differ ? 1u : 0u;
        const bool err = cutoff || (differ && A.enforce);
        s.dest = target;
        const bool last = s.retries >= A.max_retries;
        c.retry_succeeded += !err && s.retries ? 1u : 0u;
        c.retry_failed += err && last && A.max_retries ? 1u : 0u;
        c.retry_scheduled += err && !last ? 1u : 0u;
        if (!err) {
            s.oc = AO_DELIVERED;
            break;
        }
        if (last) {
            s.oc = AO_FAILED;
            break;
        }
        // (a select over the unrolled entries keeps the schedule in scalar registers and out of scratch)
        uint32_t delay = 0;
#pragma unroll
        for (uint32_t k = 0; k < TA_MAX_SCHEDULE; k++)
            if (k == min(s.retries, A.nschedule - 1)) delay = A.schedule[k];
        s.due = clock + delay;
        if (s.due > clock) break;
    }
}

// a send became final: its by_retries slot (bc: the block's LDS counters; the host sums an outcome's slots into
// its counter)
__device__ inline void tall_count_final(const TallSend& s, unsigned long long* bc) {
    atomicAdd(&bc[TA_NSTATS + s.oc * TA_RETRY_SLOTS + min(s.retries, TA_RETRY_SLOTS - 1)], 1ull);
}

__device__ inline uint4 tall_pack_group(const TallSend& s, uint32_t kbeg, uint32_t kcnt) {
    return make_uint4((uint32_t)s.d0, s.due, s.retries | s.oc << 8, kbeg | kcnt << 16);
}

// max over the lanes of a W-lane segment
template <uint32_t W>
__device__ inline uint32_t tall_seg_max(uint32_t v) {
#pragma unroll
    for (int o = 1; o < (int)W; o <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, (int)W));
    return v;
}

// What a request's sends amount to after a step, reduced over its lanes:
// open: a send is still open; ndue: the least due clock of the open ones;
// worst, maxret: over the final ones; err: a send ended with an outcome >= 3 in
// this call.  The leader lane then writes the request's words (tab.req[at]),
// its survival (keep[at]), its record and its counters.
struct TallSummary {
    uint32_t open, ndue, worst, maxret, err;
    __device__ inline void add(const TallSend& s, bool changed) {
        const bool fin = s.oc != AO_PENDING;
        open |= fin ? 0u : 1u;
        ndue = min(ndue, fin ? TA_NEVER : s.due);
        worst = max(worst, fin ? s.oc : 0u);
        maxret = max(maxret, s.retries);
        err |= fin && changed && s.oc >= AO_FAILED ? 1u : 0u;
    }
};
template <uint32_t W>
__device__ inline TallSummary tall_reduce(const TallSummary& x) {
    TallSummary r;
    r.open = tall_seg_max<W>(x.open);
    r.ndue = ~tall_seg_max<W>(~x.ndue);
    r.worst = tall_seg_max<W>(x.worst);
    r.maxret = tall_seg_max<W>(x.maxret);
    r.err = tall_seg_max<W>(x.err);
    return r;
}
template <int MODE>
__device__ __forceinline__ void tall_finish(const SimDev& S, const TallArgs& A, const TallTable& tab, TallRequest& q, uint32_t at,
                                   const TallSummary& m, TallCounts& c, uint32_t* tile_lds) {
    const uint32_t clock = S.round;
    if (m.err && q.first_err == TA_NEVER) q.first_err = clock;
    uint32_t oc = m.open ? AO_PENDING : m.worst;
    if (MODE != TALL_PENDING) {
        const uint32_t live = q.live ? 1u : 0u;
        if (!q.live) oc = AO_ENTRY_DEAD;
        c.requests++;
        c.req_entry_dead += 1u - live;
        c.req_empty += q.K == 0 ? live : 0u;
        c.keys += q.live ? q.K : 0u;
        c.sends += q.live ? q.ng : 0u;
    }
    if (m.open) {
        tab.req[2 * (size_t)at] = make_uint4((uint32_t)q.id, (uint32_t)(q.id >> 32), q.e, q.off);
        tab.req[2 * (size_t)at + 1] = make_uint4(q.K | q.ng << 16, q.submit, m.ndue, q.first_err);
        atomicAdd(&tile_lds[0], 1u);
        atomicAdd(&tile_lds[1], q.K);
    }
    const uint32_t retired = m.open ? 0u : 1u, ok = oc <= AO_REROUTED_LOCAL ? retired : 0u;
    c.req_ok += ok;
    c.req_failed += retired - ok;
    A.keep[at] = m.open ? q.K : 0u;
    if (A.results && q.id < A.results_cap)
        A.results[q.id] = make_uint4(oc | m.maxret << 8 | q.ng << 16, q.submit, q.first_err, m.open ? 0u : clock);
}

// A request of at most W keys on the W lanes of a segment (lane j: key slot j,
// then group j).
//  Submission: every key lane walks e's row, ra_group_by groups them, and a
//  key's slot in the arena is its group's begin (the exclusive scan of the
//  groups' sizes over the group lanes) plus its rank among the group's members
//  -- the store does the regrouping.
//  Poll: group lane j loads send j; the heads of the due sends' key segments,
//  OR-ed over the wave, tell every key lane its group (a popcount); only the
//  keys of due sends are looked up; "my owner is not my left neighbour's" off
//  the heads, one ballot, is the divergence of every send at once.
//  Then the group lanes run their sends, one per lane, and the key lanes of a
//  delivered send count their agreement in the destination's view.
template <uint32_t W, int MODE>
__device__ __forceinline__ void tall_segment(const SimDev& S, const TallArgs& A, const TallTable& tab, const TallBatch& B,
                                    TallRequest& q, uint32_t at, uint32_t j, uint32_t sshift, TallCounts& c,
                                    unsigned long long* bc, uint32_t* tile_lds) {
    constexpr uint64_t SEG = ~0ull >> (64 - W);
    const uint32_t clock = S.round, L = sshift + j;
    const uint64_t below = (1ull << L) - 1ull;
    const bool kslot = q.active && j < q.K;
    uint32_t p0 = 0, gi = 0, kbeg = 0, kcnt = 0;
    int32_t o = (int32_t)q.e;
    bool isg, run = false, diverge = false;  // run: the group lane's send has an event now
    TallSend s{-1, -1, 0, 0, AO_PENDING};
    int32_t nd;
    if (MODE != TALL_PENDING) {
        const bool has = kslot && q.live;
        uint32_t h = 0;
        if (MODE == TALL_UNIFORM) h = (uint32_t)ra_draw(B.seed, (B.first_index + at) * B.uniform_k + j);
        else if (has) h = B.keys[B.offsets[at] + j];
        if (has) o = ra_entry_dest(A.own, q.e, q.rce, h, p0);
        int32_t gd;
        uint64_t gm;
        q.ng = ra_group_by<W>(has, o, j, sshift, gi, gd, gm);
        isg = j < q.ng;
        kcnt = (uint32_t)__popcll(gm);
        uint32_t incl = kcnt;
#pragma unroll
        for (int d = 1; d < (int)W; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, d, (int)W);
            if ((int)j >= d) incl += y;
        }
        kbeg = incl - kcnt;
        const uint32_t src = sshift + (has ? gi : 0u);
        const uint32_t mybeg = (uint32_t)__shfl((int)kbeg, (int)src);
        const uint64_t mygm = (uint64_t)__shfl((unsigned long long)gm, (int)src);
        if (has) tab.keys[q.off + mybeg + (uint32_t)__popcll(mygm & ((1ull << j) - 1ull))] = h;
        s.d0 = gd;
        nd = gd;
        if (isg && (uint32_t)gd == q.e) {
            s.oc = AO_LOCAL;
            s.dest = gd;
            tall_count_final(s, bc);
        } else if (isg) {
            c.proxied++;
            run = true;
        }
    } else {
        isg = q.active && j < q.ng;
        uint4 g = make_uint4(0, 0, 0, 0);
        if (isg) g = tab.groups[q.off + j];
        s.d0 = (int32_t)g.x; s.due = g.y; s.retries = g.z & 0xFFu; s.oc = isg ? g.z >> 8 : AO_LOCAL;
        s.dest = s.d0;
        kbeg = g.w & 0xFFFFu; kcnt = g.w >> 16;
        run = isg && s.oc == AO_PENDING && s.due <= clock;
        uint64_t heads = isg ? 1ull << (sshift + kbeg) : 0ull;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) heads |= (uint64_t)__shfl_xor((unsigned long long)heads, d);
        // (key slot 0 is group 0's head: a key lane has a head at or below it)
        gi = kslot ? (uint32_t)__popcll(heads & (SEG << sshift) & (below | 1ull << L)) - 1u : 0u;
        const bool kdue = __shfl((int)run, (int)(sshift + gi)) != 0 && kslot && q.live;
        if (kdue) o = ra_entry_dest(A.own, q.e, q.rce, tab.keys[q.off + j], p0);
        const int32_t left = __shfl_up(o, 1);
        const uint64_t dm = __ballot(kdue && !((heads >> L) & 1ull) && o != left);
        const uint64_t mine = (kcnt >= 64 ? ~0ull : (1ull << kcnt) - 1ull) << (sshift + kbeg);
        diverge = (dm & mine) != 0;
        nd = __shfl(o, (int)(isg ? sshift + kbeg : L));
    }
    if (run) {
        tall_send(S, A, q, MODE != TALL_PENDING, diverge, nd, s, c);
        if (s.oc != AO_PENDING) tall_count_final(s, bc);
    }
    if (isg && (run || MODE != TALL_PENDING)) tab.groups[q.off + j] = tall_pack_group(s, kbeg, kcnt);
    // the key lanes of a send delivered in this call: does its destination, in its own view, own the key
    const int32_t res = run && s.oc == AO_DELIVERED ? s.dest : -1;
    const int32_t kres = __shfl(res, (int)(sshift + gi));
    if (kslot && q.live && kres >= 0 && !ra_agrees(A.own, kres, p0)) c.misrouted_keys++;
    TallSummary m{0, TA_NEVER, 0, 0, 0};
    if (isg) m.add(s, run || MODE != TALL_PENDING);
    m = tall_reduce<W>(m);
    if (q.active && j == 0) tall_finish<MODE>(S, A, tab, q, at, m, c, tile_lds);
}

// A request of 65 .. 256 keys on a whole wave, 64 keys or 64 groups a pass,
// with its groups in the wave's LDS (TallLds).
//  Submission: a chunk of keys is grouped as a segment is; its groups probe the
//  table (an owner an earlier chunk met keeps its rank, new ones take the next
//  ranks in lane order); every key notes its group and its place among the
//  group's members so far.  After the last chunk the groups' sizes are scanned
//  into their begins and every key is stored at begin + place.
//  Poll: the groups' begins and due flags go to LDS; a key finds its group by
//  bisection of the begins, the keys of due sends are looked up, and a key whose
//  owner differs from the key before it in the same send marks the send.
template <int MODE>
__device__ __forceinline__ void tall_chunked(const SimDev& S, const TallArgs& A, const TallTable& tab, const TallBatch& B,
                                    TallRequest& q, uint32_t at, TallLds& T, uint32_t lane, TallCounts& c,
                                    unsigned long long* bc, uint32_t* tile_lds) {
    const uint32_t clock = S.round;
    const uint64_t below = (1ull << lane) - 1ull;
    if (MODE != TALL_PENDING) {
        for (uint32_t t = lane; t < 2 * RA_MAX_K; t += 64) T.dest[t] = -1;
        ra_fence();
        uint32_t ng = 0;
        const uint64_t src0 = MODE == TALL_UNIFORM ? (B.first_index + at) * B.uniform_k : B.offsets[at];
        for (uint32_t c0 = 0; c0 < q.K; c0 += 64) {
            const uint32_t k = c0 + lane;
            const bool has = k < q.K;  // (a dead entry's request never comes here)
            uint32_t h = 0, p0 = 0, lr;
            if (MODE == TALL_UNIFORM) h = (uint32_t)ra_draw(B.seed, src0 + k);
            else if (has) h = B.keys[src0 + k];
            int32_t d = (int32_t)q.e, gd;
            if (has) d = ra_entry_dest(A.own, q.e, q.rce, h, p0);
            uint64_t gm;
            const uint32_t nc = ra_group_by<64>(has, d, lane, 0, lr, gd, gm);
            const bool isg = lane < nc;
            uint32_t slot = 0;
            bool fresh = false;
            if (isg) {
                // (the chunk's groups have distinct owners; at most RA_MAX_K of the slots are ever taken)
                slot = ((uint32_t)gd * 0x9E3779B1u) >> 23;
                for (;;) {
                    const int32_t old = atomicCAS(&T.dest[slot], -1, gd);
                    fresh = old == -1;
                    if (fresh || old == gd) break;
                    slot = (slot + 1) & (2 * RA_MAX_K - 1);
                }
            }
            const uint64_t fm = __ballot(fresh);
            uint32_t r = 0, before = 0;
            if (fresh) {
                r = ng + (uint32_t)__popcll(fm & below);  // (r < the keys seen so far <= RA_MAX_K)
                T.rank[slot] = (uint16_t)r;
                T.gdest[r] = gd;
            } else if (isg) {
                r = T.rank[slot];
                before = T.gcnt[r];
            }
            ng += (uint32_t)__popcll(fm);
            const int from = (int)(has ? lr : 0u);
            const uint32_t kr = (uint32_t)__shfl((int)r, from), kb = (uint32_t)__shfl((int)before, from);
            const uint64_t kgm = (uint64_t)__shfl((unsigned long long)gm, from);
            if (has) {
                T.kgrp[k] = (uint16_t)kr;
                T.widx[k] = (uint16_t)(kb + (uint32_t)__popcll(kgm & below));
                T.p0[k] = p0;
            }
            if (isg) T.gcnt[r] = (uint16_t)(before + (uint32_t)__popcll(gm));
            ra_fence();
        }
        q.ng = ng;
        uint32_t carry = 0;
        for (uint32_t g0 = 0; g0 < ng; g0 += 64) {
            const uint32_t g = g0 + lane, v = g < ng ? T.gcnt[g] : 0u;
            uint32_t incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
                if ((int)lane >= d) incl += y;
            }
            if (g < ng) T.gbeg[g] = (uint16_t)(carry + incl - v);
            carry += (uint32_t)__shfl((int)incl, 63);
        }
        ra_fence();
        for (uint32_t k = lane; k < q.K; k += 64) {
            const uint32_t h = MODE == TALL_UNIFORM ? (uint32_t)ra_draw(B.seed, src0 + k) : B.keys[src0 + k];
            tab.keys[q.off + T.gbeg[T.kgrp[k]] + T.widx[k]] = h;
        }
    } else {
        for (uint32_t g = lane; g < q.ng; g += 64) {
            const uint4 w = tab.groups[q.off + g];
            T.gbeg[g] = (uint16_t)(w.w & 0xFFFFu);
            T.gflag[g] = (w.z >> 8) == AO_PENDING && w.y <= clock ? 1 : 0;
            T.gdest[g] = 0;
        }
        ra_fence();
        for (uint32_t k = lane; k < q.K; k += 64) {
            uint32_t lo = 0, hi = q.ng;  // the last group whose begin is <= k
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (T.gbeg[mid] <= k) lo = mid; else hi = mid;
            }
            T.kgrp[k] = (uint16_t)lo;
            if (T.gflag[lo] && q.live) {
                uint32_t p0;
                T.own[k] = ra_entry_dest(A.own, q.e, q.rce, tab.keys[q.off + k], p0);
                T.p0[k] = p0;
            }
        }
        ra_fence();
        for (uint32_t k = lane; k < q.K; k += 64) {
            const uint32_t g = T.kgrp[k];
            if (T.gflag[g] && q.live && k > T.gbeg[g] && T.own[k] != T.own[k - 1]) T.gdest[g] = 1;
        }
        ra_fence();
    }
    TallSummary m{0, TA_NEVER, 0, 0, 0};
    for (uint32_t g = lane; g < q.ng; g += 64) {
        TallSend s{-1, -1, 0, 0, AO_PENDING};
        uint32_t kbeg, kcnt;
        bool run, diverge = false;
        int32_t nd;
        if (MODE != TALL_PENDING) {
            kbeg = T.gbeg[g]; kcnt = T.gcnt[g];
            s.d0 = nd = T.gdest[g];
            run = (uint32_t)s.d0 != q.e;
            if (run) {
                c.proxied++;
            } else {
                s.oc = AO_LOCAL;
                s.dest = s.d0;
                tall_count_final(s, bc);
            }
        } else {
            const uint4 w = tab.groups[q.off + g];
            s.d0 = s.dest = (int32_t)w.x; s.due = w.y; s.retries = w.z & 0xFFu; s.oc = w.z >> 8;
            kbeg = w.w & 0xFFFFu; kcnt = w.w >> 16;
            run = T.gflag[g] != 0;
            diverge = T.gdest[g] != 0;
            nd = run && q.live ? T.own[kbeg] : (int32_t)q.e;
        }
        if (run) {
            tall_send(S, A, q, MODE != TALL_PENDING, diverge, nd, s, c);
            if (s.oc != AO_PENDING) tall_count_final(s, bc);
        }
        if (run || MODE != TALL_PENDING) tab.groups[q.off + g] = tall_pack_group(s, kbeg, kcnt);
        T.gres[g] = run && s.oc == AO_DELIVERED ? s.dest : -1;
        m.add(s, run || MODE != TALL_PENDING);
    }
    ra_fence();
    for (uint32_t k = lane; k < q.K; k += 64) {
        const int32_t res = T.gres[T.kgrp[k]];
        if (res >= 0 && !ra_agrees(A.own, res, T.p0[k])) c.misrouted_keys++;
    }
    ra_fence();  // (the next request rewrites the table)
    m = tall_reduce<64>(m);
    if (lane == 0) tall_finish<MODE>(S, A, tab, q, at, m, c, tile_lds);
}

// One step of the request table at clock S.round.
//   TALL_PENDING: the requests of the pending table `tab` (ctl[AC_COUNT]) whose
//     next_due has come retry their due sends, in place;
//   TALL_BATCH / TALL_UNIFORM: requests [0, count_in) of the batch get ids
//     first_id + i and make their first sends; `tab` is a staging table, a
//     request's keys at its offset in the batch.
// W lanes a request; a block takes a tile of 256 requests in W passes of
// 256 / W (grid-stride over tiles), counts the tile's survivors and their keys
// in LDS and writes them to tile_sum: k_tall_scan and k_tall_compact move the
// survivors.  Every request has at most W keys, but with BIG (W == 64; chosen
// when a request of more than 64 keys was ever submitted), where such a request
// takes the chunked path with its LDS table: the other instantiations carry
// neither.  A pending request that is not due
// costs its leader one 16-byte load.  Counters: lane registers, then LDS, then
// one atomic per counter and block.
template <uint32_t W, int MODE, bool BIG>
__global__ void __launch_bounds__(TA_BLOCK) k_traffic_all_step(SimDev S, TallArgs A, TallTable tab, TallBatch B,
                                                               uint32_t count_in) {
    constexpr uint32_t PER_PASS = TA_BLOCK / W;
    __shared__ unsigned long long bc[TA_NSLOTS];
    __shared__ uint32_t tile_lds[2];
    if (threadIdx.x < TA_NSLOTS) bc[threadIdx.x] = 0;
    if (threadIdx.x < 2) tile_lds[threadIdx.x] = 0;
    const uint32_t count = min(MODE == TALL_PENDING ? A.ctl[AC_COUNT] : count_in, tab.cap_req);
    const uint32_t ntiles = min((count + TA_TILE - 1) / TA_TILE, A.tiles_cap);
    const uint32_t lane = threadIdx.x & 63u, j = lane & (W - 1), sshift = lane & ~(W - 1);
    const uint32_t clock = S.round;
    TallCounts c;
    __syncthreads();
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        for (uint32_t pass = 0; pass < W; pass++) {
            const uint32_t at = tile * TA_TILE + pass * PER_PASS + threadIdx.x / W;
            TallRequest q;
            q.active = at < count;
            uint32_t id_lo = 0, id_hi = 0, e = 0, off = 0, kng = 0, submit = clock, first_err = TA_NEVER, cse = 0, dead = 1;
            uint32_t skip = 0;
            int32_t rce = 0;
            if (q.active && j == 0) {
                if (MODE == TALL_PENDING) {
                    const uint4 w1 = tab.req[2 * (size_t)at + 1];
                    kng = w1.x; submit = w1.y; first_err = w1.w;
                    skip = w1.z > clock ? 1u : 0u;
                    if (skip) {  // not due: it survives as it is
                        A.keep[at] = kng & 0xFFFFu;
                        atomicAdd(&tile_lds[0], 1u);
                        atomicAdd(&tile_lds[1], kng & 0xFFFFu);
                    } else {
                        const uint4 w0 = tab.req[2 * (size_t)at];
                        id_lo = w0.x; id_hi = w0.y; e = w0.z; off = w0.w;
                    }
                } else {
                    const uint64_t id = B.first_id + at;
                    id_lo = (uint32_t)id; id_hi = (uint32_t)(id >> 32);
                    if (MODE == TALL_UNIFORM) {
                        kng = B.uniform_k;
                        off = at * B.uniform_k;
                        e = (uint32_t)(((ra_draw(B.seed, (B.first_index + at) * B.uniform_k) >> 32) * S.n) >> 32);
                    } else {
                        e = B.entries[at];
                        off = (uint32_t)(B.offsets[at] - B.offsets[0]);
                        kng = (uint32_t)(B.offsets[at + 1] - B.offsets[at]);
                    }
                }
                if (!skip) {
                    dead = S.dead[e];
                    const RouteShard& te = A.own.tab[e / A.own.nl];
                    rce = te.ring_count[e];
                    cse = te.ring_csum[e];
                }
            }
            q.active = q.active && __shfl((int)skip, 0, (int)W) == 0;
            q.id = (uint64_t)(uint32_t)__shfl((int)id_lo, 0, (int)W) | (uint64_t)(uint32_t)__shfl((int)id_hi, 0, (int)W) << 32;
            q.e = (uint32_t)__shfl((int)e, 0, (int)W);
            q.off = (uint32_t)__shfl((int)off, 0, (int)W);
            kng = (uint32_t)__shfl((int)kng, 0, (int)W);
            q.K = kng & 0xFFFFu;
            q.ng = kng >> 16;
            q.submit = (uint32_t)__shfl((int)submit, 0, (int)W);
            q.first_err = (uint32_t)__shfl((int)first_err, 0, (int)W);
            q.cse = (uint32_t)__shfl((int)cse, 0, (int)W);
            q.rce = __shfl(rce, 0, (int)W);
            q.live = q.active && __shfl((int)dead, 0, (int)W) == 0;
            if (!q.active) q.K = q.ng = 0;
            if constexpr (BIG) {
                static_assert(W == 64, "the chunked path takes a whole wave");
                __shared__ TallLds lds[TA_BLOCK / 64];
                // (the wave's one request; a dead entry's submission has no groups: the segment path counts it)
                if (q.K > 64 && (q.live || MODE == TALL_PENDING))
                    tall_chunked<MODE>(S, A, tab, B, q, at, lds[threadIdx.x >> 6], lane, c, bc, tile_lds);
                else
                    tall_segment<W, MODE>(S, A, tab, B, q, at, j, sshift, c, bc, tile_lds);
            } else {
                tall_segment<W, MODE>(S, A, tab, B, q, at, j, sshift, c, bc, tile_lds);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            A.tile_sum[tile] = make_uint2(tile_lds[0], tile_lds[1]);
            tile_lds[0] = tile_lds[1] = 0;
        }
        __syncthreads();
    }
    c.flush(bc);
    __syncthreads();
    if (threadIdx.x < TA_NSLOTS && bc[threadIdx.x]) atomicAdd(&A.cum[threadIdx.x], bc[threadIdx.x]);
}

__device__ inline unsigned long long tall_pair(uint2 v) { return (unsigned long long)v.x << 32 | v.y; }

// inclusive scan of a {count, keys} pair (count in the high word: the keys of a tracker stay below 2^32) over the wave
__device__ inline unsigned long long tall_wave_scan(unsigned long long x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o);
        if ((int)lane >= o) x += y;
    }
    return x;
}

// Exclusive prefix sums of the tiles' {survivors, keys} by one block (the tiles
// in chunks of 1024), then the control words.  APPEND (a submitted batch of
// count_in requests): the survivors go after the pending requests and their
// keys after the pending keys; otherwise they replace the table.
template <bool APPEND>
__global__ void __launch_bounds__(TA_SCAN) k_tall_scan(TallArgs A, uint32_t count_in, uint32_t cap_src, uint32_t cap_req,
                                                       uint32_t cap_keys) {
    __shared__ unsigned long long wsum[TA_SCAN / 64];
    const uint32_t old = A.ctl[AC_COUNT], old_keys = A.ctl[AC_KEYS];
    const uint32_t count = min(APPEND ? count_in : old, cap_src);
    const uint32_t ntiles = min((count + TA_TILE - 1) / TA_TILE, A.tiles_cap);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long running = 0;
    __syncthreads();  // (every thread has read the counts before they are replaced)
    for (uint32_t base = 0; base < ntiles; base += TA_SCAN) {
        const uint32_t t = base + threadIdx.x;
        const unsigned long long v = t < ntiles ? tall_pair(A.tile_sum[t]) : 0ull;
        const unsigned long long incl = tall_wave_scan(v, lane);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        unsigned long long woff = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < TA_SCAN / 64; k++) {
            const unsigned long long s = wsum[k];
            woff += k < w ? s : 0ull;
            total += s;
        }
        const unsigned long long ex = running + woff + incl - v;
        if (t < ntiles) A.tile_off[t] = make_uint2((uint32_t)(ex >> 32), (uint32_t)ex);
        running += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        uint64_t now = running >> 32, now_keys = (uint32_t)running;
        if (APPEND) {
            A.ctl[AC_BASE] = old;
            A.ctl[AC_BASE_KEYS] = old_keys;
            now += old;
            now_keys += old_keys;
            if (now > cap_req || now_keys > cap_keys) {
                A.ctl[AC_OVERFLOW] = 1;
                now = min(now, (uint64_t)cap_req);
                now_keys = min(now_keys, (uint64_t)cap_keys);
            }
        } else {
            A.ctl[AC_PREV] = count;
        }
        A.ctl[AC_COUNT] = (uint32_t)now;
        A.ctl[AC_KEYS] = (uint32_t)now_keys;
    }
}

// The survivors of each tile of `src`, with their key and group segments, to
// `dst` in order: request r of the tile goes to tile_off + its rank (a block
// scan of keep[]), its keys to the exclusive sum of the keys of the survivors
// before it, and its key offset is rewritten.  The tile's segments are
// contiguous in dst, so the block copies them as one flat range: a thread finds
// an element's request by bisection of the survivors' begins in LDS.  Group j
// of a request travels with its key j (a request has no more groups than keys).
template <bool APPEND>
__global__ void __launch_bounds__(TA_TILE) k_tall_compact(TallArgs A, TallTable src, TallTable dst, uint32_t count_in) {
    __shared__ unsigned long long wsum[TA_TILE / 64];
    __shared__ uint32_t sbeg[TA_TILE + 1], soff[TA_TILE], sng[TA_TILE];
    const uint32_t count = min(APPEND ? count_in : A.ctl[AC_PREV], src.cap_req);
    const uint32_t ntiles = min((count + TA_TILE - 1) / TA_TILE, A.tiles_cap);
    const uint32_t base = APPEND ? A.ctl[AC_BASE] : 0u, base_keys = APPEND ? A.ctl[AC_BASE_KEYS] : 0u;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * TA_TILE + threadIdx.x;
        const uint32_t nk = i < count ? A.keep[i] : 0u;
        const unsigned long long v = nk ? 1ull << 32 | nk : 0ull;
        const unsigned long long incl = tall_wave_scan(v, lane);
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        unsigned long long woff = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < TA_TILE / 64; k++) {
            const unsigned long long s = wsum[k];
            woff += k < w ? s : 0ull;
            total += s;
        }
        const unsigned long long ex = woff + incl - v;
        const uint32_t rank = (uint32_t)(ex >> 32), kbeg = (uint32_t)ex;
        const uint32_t nsurv = (uint32_t)(total >> 32), nkeys = (uint32_t)total;
        const uint2 toff = A.tile_off[tile];
        const uint64_t to_req = (uint64_t)base + toff.x, to_keys = (uint64_t)base_keys + toff.y;
        if (nk) {
            uint4 w0 = src.req[2 * (size_t)i];
            const uint4 w1 = src.req[2 * (size_t)i + 1];
            soff[rank] = w0.w;
            sbeg[rank] = kbeg;
            sng[rank] = w1.x >> 16;
            w0.w = (uint32_t)(to_keys + kbeg);
            // (k_tall_scan raised AC_OVERFLOW where a survivor finds no room)
            if (to_req + rank < dst.cap_req && to_keys + kbeg + nk <= dst.cap_keys) {
                dst.req[2 * (to_req + rank)] = w0;
                dst.req[2 * (to_req + rank) + 1] = w1;
            }
        }
        if (threadIdx.x == 0) sbeg[nsurv] = nkeys;
        __syncthreads();
        for (uint32_t f = threadIdx.x; f < nkeys; f += TA_TILE) {
            uint32_t lo = 0, hi = nsurv;  // the last survivor whose begin is <= f
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sbeg[mid] <= f) lo = mid; else hi = mid;
            }
            const uint32_t jk = f - sbeg[lo];
            const size_t from = (size_t)soff[lo] + jk;
            if (to_keys + f >= dst.cap_keys) continue;
            dst.keys[to_keys + f] = src.keys[from];
            if (jk < sng[lo]) dst.groups[to_keys + f] = src.groups[from];
        }
        __syncthreads();  // (the LDS arrays are rewritten by the next tile)
    }
}

}  // namespace rp

using rp::DevBuf;
using rp::Error;
using rp::Shard;

// =====================================================================
// Host side.  A tracker keeps its tables on its simulation's device and runs on
// the first shard's stream, like a route.
// =====================================================================
struct rp_traffic_all {
    rp_sim* sim = nullptr;
    rp_traffic_config cfg{};
    uint64_t key_capacity = 0;
    uint64_t lifetime = 0;  // rounds a request can stay pending: the delays of its max_retries retries
    struct Table {
        DevBuf<uint4> req, groups;
        DevBuf<uint32_t> keys;
        rp::TallTable dev(uint64_t cap_req, uint64_t cap_keys) {
            return rp::TallTable{req.p, keys.p, groups.p, (uint32_t)cap_req, (uint32_t)cap_keys};
        }
    };
    Table tab[2], stage;  // the pending table, the one the next compaction writes, a submitted chunk's
    int cur = 0;
    uint64_t alloc = 0, alloc_keys = 0;  // requests and keys each of tab[] holds
    uint64_t stage_req = 0, stage_keys = 0;
    DevBuf<uint32_t> keep, ctl;
    DevBuf<uint2> tile_sum, tile_off;
    DevBuf<unsigned long long> cum;
    DevBuf<uint4> results;
    uint64_t results_cap = 0;
    uint64_t next_id = 0, run_index = 0;
    uint64_t bound = 0, bound_keys = 0;  // >= the device's pending requests and keys
    uint32_t max_k = 0;                  // the largest request ever submitted: the lanes of a poll
    uint32_t h_ctl[rp::AC_NWORDS] = {0};
    static constexpr uint64_t CHUNK_REQ = 1ull << 20;   // requests ...
    static constexpr uint64_t CHUNK_KEYS = 1ull << 22;  // ... and keys of a submit launch, at the most

    hipStream_t st() const { return sim->sh.front()->st; }

    template <class T>
    void grow(DevBuf<T>& b, uint64_t count, uint64_t keep_n) {
        DevBuf<T> nb((size_t)count);
        if (keep_n) RP_HIP(hipMemcpyAsync(nb.p, b.p, (size_t)keep_n * sizeof(T), hipMemcpyDeviceToDevice, st()));
        RP_HIP(hipStreamSynchronize(st()));
        b = std::move(nb);
    }
    void ensure_tiles(uint64_t requests) {
        if (keep.n < requests) keep.alloc((size_t)requests);
        const uint64_t tiles = (requests + rp::TA_TILE - 1) / rp::TA_TILE;
        if (tile_sum.n < tiles) { tile_sum.alloc((size_t)tiles); tile_off.alloc((size_t)tiles); }
    }
    // room for need_req pending requests with need_keys keys, or RP_ERR_CAPACITY (nothing changed)
    void ensure_table(uint64_t need_req, uint64_t need_keys) {
        if (need_req > cfg.capacity)
            throw Error(RP_ERR_CAPACITY, "the pending table would need " + std::to_string(need_req) +
                                             " requests, capacity is " + std::to_string(cfg.capacity));
        if (need_keys > key_capacity)
            throw Error(RP_ERR_CAPACITY, "the key arena would need " + std::to_string(need_keys) +
                                             " keys, key_capacity is " + std::to_string(key_capacity));
        if (need_req > alloc) {
            const uint64_t na = std::min<uint64_t>(cfg.capacity, std::max<uint64_t>({need_req, alloc * 2, 1024}));
            grow(tab[cur].req, 2 * na, 2 * bound);
            tab[cur ^ 1].req.alloc((size_t)(2 * na));
            alloc = na;
        }
        if (need_keys > alloc_keys) {
            const uint64_t na = std::min<uint64_t>(key_capacity, std::max<uint64_t>({need_keys, alloc_keys * 2, 16384}));
            grow(tab[cur].keys, na, bound_keys);
            grow(tab[cur].groups, na, bound_keys);
            tab[cur ^ 1].keys.alloc((size_t)na);
            tab[cur ^ 1].groups.alloc((size_t)na);
            alloc_keys = na;
        }
        ensure_tiles(std::max(alloc, stage_req));
    }
    void ensure_results(uint64_t ids) {
        if (!cfg.track || ids <= results_cap) return;
        const uint64_t nr = std::max<uint64_t>({ids, results_cap * 2, 1024});
        DevBuf<uint4> nb((size_t)nr);
        if (results_cap)
            RP_HIP(hipMemcpyAsync(nb.p, results.p, (size_t)results_cap * 16, hipMemcpyDeviceToDevice, st()));
        RP_HIP(hipMemsetAsync(nb.p + results_cap, 0xFF, (size_t)(nr - results_cap) * 16, st()));
        RP_HIP(hipStreamSynchronize(st()));
        results = std::move(nb);
        results_cap = nr;
    }
    // a chunk of at most n requests and keys_total keys
    void ensure_stage(uint64_t n, uint64_t keys_total) {
        const uint64_t r = std::min(n, CHUNK_REQ), k = std::min<uint64_t>(keys_total, CHUNK_KEYS + rp::RA_MAX_K);
        if (stage_req < r) { stage.req.alloc((size_t)(2 * r)); stage_req = r; }
        if (stage_keys < k) { stage.keys.alloc((size_t)k); stage.groups.alloc((size_t)k); stage_keys = k; }
        ensure_tiles(std::max(alloc, stage_req));
    }
    void read_ctl() {
        RP_HIP(hipMemcpyAsync(h_ctl, ctl.p, sizeof h_ctl, hipMemcpyDeviceToHost, st()));
        RP_HIP(hipStreamSynchronize(st()));
        bound = h_ctl[rp::AC_COUNT];
        bound_keys = h_ctl[rp::AC_KEYS];
        if (h_ctl[rp::AC_OVERFLOW]) throw Error(RP_ERR_STATE, "the pending table overflowed on the device");
    }
    void prepare() {
        sim->route_prepare();
        read_ctl();
    }
    rp::TallArgs args() {
        rp::TallArgs A{};
        A.own = sim->own_args();  // (the routing tables and the points: no census buffer is read)
        A.max_retries = (uint32_t)cfg.max_retries; A.nschedule = cfg.nschedule;
        A.enforce = cfg.enforce_consistency ? 1u : 0u;
        for (uint32_t i = 0; i < rp::TA_MAX_SCHEDULE; i++) A.schedule[i] = cfg.schedule[i];
        A.cum = cum.p;
        A.results = results.p; A.results_cap = results_cap;
        A.ctl = ctl.p;
        A.keep = keep.p;
        A.tile_sum = tile_sum.p; A.tile_off = tile_off.p;
        A.tiles_cap = (uint32_t)tile_sum.n;
        return A;
    }
    rp::SimDev clocked() {
        rp::SimDev S = sim->sh.front()->d;
        S.round = sim->round;  // the clock of the next round, as a route
        S.part_start = sim->part[0]; S.part_end = sim->part[1]; S.part_split = sim->part[2];
        return S;
    }
    static unsigned tile_grid(uint64_t requests) {
        return std::min(rp::grid_for(std::max<uint64_t>(requests, 1), rp::TA_TILE), 8192u);
    }
    // the lanes of a request; 128: a wave with the chunked path
    static uint32_t lanes(uint32_t k) { return k > 64 ? 128u : rp::ra_lanes_for(k); }
    template <int MODE>
    void launch_step(uint32_t W, dim3 grid, const rp::SimDev& S, const rp::TallArgs& A, const rp::TallTable& t,
                     const rp::TallBatch& B, uint32_t m) {
        switch (W) {
            case 8: hipLaunchKernelGGL((rp::k_traffic_all_step<8, MODE, false>), grid, dim3(rp::TA_BLOCK), 0, st(), S, A, t, B, m); break;
            case 16: hipLaunchKernelGGL((rp::k_traffic_all_step<16, MODE, false>), grid, dim3(rp::TA_BLOCK), 0, st(), S, A, t, B, m); break;
            case 32: hipLaunchKernelGGL((rp::k_traffic_all_step<32, MODE, false>), grid, dim3(rp::TA_BLOCK), 0, st(), S, A, t, B, m); break;
            case 64: hipLaunchKernelGGL((rp::k_traffic_all_step<64, MODE, false>), grid, dim3(rp::TA_BLOCK), 0, st(), S, A, t, B, m); break;
            default: hipLaunchKernelGGL((rp::k_traffic_all_step<64, MODE, true>), grid, dim3(rp::TA_BLOCK), 0, st(), S, A, t, B, m); break;
        }
    }
    // every due send of the pending requests retries; the surviving requests, in order, become the table
    void launch_poll() {
        if (!alloc || !alloc_keys) return;  // nothing with a send was ever submitted
        const rp::TallArgs A = args();
        const rp::SimDev S = clocked();
        const rp::TallTable src = tab[cur].dev(alloc, alloc_keys), dst = tab[cur ^ 1].dev(alloc, alloc_keys);
        const dim3 grid(tile_grid(bound));
        launch_step<rp::TALL_PENDING>(lanes(max_k), grid, S, A, src, rp::TallBatch{}, 0u);
        hipLaunchKernelGGL(rp::k_tall_scan<false>, dim3(1), dim3(rp::TA_SCAN), 0, st(), A, 0u, (uint32_t)alloc, (uint32_t)alloc,
                           (uint32_t)alloc_keys);
        hipLaunchKernelGGL(rp::k_tall_compact<false>, grid, dim3(rp::TA_TILE), 0, st(), A, src, dst, 0u);
        RP_HIP(hipGetLastError());
        cur ^= 1;
    }
    // first sends of n requests (B: device arrays, or the generator); host_offsets: the CSR offsets (null: uniform).
    // Launches of at most CHUNK_REQ requests and CHUNK_KEYS keys; the survivors are appended.
    void launch_submit(rp::TallBatch B, const uint64_t* host_offsets, uint64_t n, uint32_t batch_max_k) {
        const rp::TallArgs A = args();
        const rp::SimDev S = clocked();
        const rp::TallTable stg = stage.dev(stage_req, stage_keys), dst = tab[cur].dev(alloc, alloc_keys);
        const uint32_t W = lanes(batch_max_k);
        const rp::TallBatch B0 = B;
        for (uint64_t first = 0; first < n;) {
            uint64_t m = std::min(n - first, CHUNK_REQ);
            if (host_offsets) {  // the requests whose keys end within CHUNK_KEYS of this launch's first key (at least one)
                const uint64_t* end = std::upper_bound(host_offsets + first + 1, host_offsets + first + m + 1,
                                                       host_offsets[first] + CHUNK_KEYS);
                m = std::max<uint64_t>(1, (uint64_t)(end - (host_offsets + first + 1)));
            } else {
                m = std::min<uint64_t>(m, std::max<uint64_t>(1, CHUNK_KEYS / B.uniform_k));
            }
            B = B0;
            if (B.entries) { B.entries += first; B.offsets += first; }
            B.first_index = B0.first_index + first;
            B.first_id = next_id + first;
            const dim3 grid(tile_grid(m));
            if (host_offsets) launch_step<rp::TALL_BATCH>(W, grid, S, A, stg, B, (uint32_t)m);
            else launch_step<rp::TALL_UNIFORM>(W, grid, S, A, stg, B, (uint32_t)m);
            hipLaunchKernelGGL(rp::k_tall_scan<true>, dim3(1), dim3(rp::TA_SCAN), 0, st(), A, (uint32_t)m, (uint32_t)stage_req,
                               (uint32_t)alloc, (uint32_t)alloc_keys);
            hipLaunchKernelGGL(rp::k_tall_compact<true>, grid, dim3(rp::TA_TILE), 0, st(), A, stg, dst, (uint32_t)m);
            first += m;
        }
        RP_HIP(hipGetLastError());
        next_id += n;
        max_k = std::max(max_k, batch_max_k);
    }
    void submit(const rp::TallBatch& B, const uint64_t* host_offsets, uint64_t n, uint64_t total_keys, uint32_t batch_max_k) {
        ensure_table(bound + n, bound_keys + total_keys);
        ensure_results(next_id + n);
        ensure_stage(n, total_keys);
        launch_submit(B, host_offsets, n, batch_max_k);
        read_ctl();
    }
};

extern "C" {

int rp_traffic_all_create(rp_sim* sim, const rp_traffic_config* cfg, uint64_t key_capacity, rp_traffic_all** out) {
    return rp::guarded([&] {
        if (!sim || !out) throw Error(RP_ERR_INVALID, "null pointer");
        if (sim->comm)
            throw Error(RP_ERR_UNSUPPORTED, "request traffic needs every node's view: not available on one rank of a "
                                            "multi-process or loop cluster");
        RP_HIP(hipSetDevice(sim->dev));
        std::unique_ptr<rp_traffic_all> t(new rp_traffic_all());
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
        if (key_capacity == 0) key_capacity = 16 * c.capacity;
        if (c.max_retries > (int32_t)(rp::TA_RETRY_SLOTS - 1)) throw Error(RP_ERR_INVALID, "max_retries is at most 8");
        if (c.nschedule > rp::TA_MAX_SCHEDULE) throw Error(RP_ERR_INVALID, "the schedule has at most 8 entries");
        if (c.capacity > (1ull << 26)) throw Error(RP_ERR_INVALID, "capacity is at most 2^26 requests");
        if (key_capacity > (1ull << 31)) throw Error(RP_ERR_INVALID, "key_capacity is at most 2^31 keys");
        for (uint32_t i = 0; i < c.nschedule; i++)
            if (c.schedule[i] > (1u << 20)) throw Error(RP_ERR_INVALID, "a retry delay is at most 2^20 rounds");
        for (uint32_t i = c.nschedule; i < rp::TA_MAX_SCHEDULE; i++) c.schedule[i] = 0;
        t->cfg = c;
        t->key_capacity = key_capacity;
        for (int32_t r = 0; r < c.max_retries; r++) t->lifetime += c.schedule[std::min<uint32_t>((uint32_t)r, c.nschedule - 1)];
        t->ctl.alloc(rp::AC_NWORDS);
        t->cum.alloc(rp::TA_NSLOTS);
        RP_HIP(hipMemsetAsync(t->ctl.p, 0, t->ctl.bytes(), t->st()));
        RP_HIP(hipMemsetAsync(t->cum.p, 0, t->cum.bytes(), t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
        *out = t.release();
    });
}

int rp_traffic_all_destroy(rp_traffic_all* t) {
    return rp::guarded([&] {
        delete t;  // (its buffers only: hipFree waits for the device; the simulation is not touched)
    });
}

int rp_traffic_all_submit(rp_traffic_all* t, const uint32_t* entries, const uint64_t* offsets, const uint32_t* key_hashes,
                          size_t n, uint64_t* first_id) {
    return rp::guarded([&] {
        if (!t || (n && (!entries || !offsets))) throw Error(RP_ERR_INVALID, "null pointer");
        uint32_t max_k = 0;
        if (n && offsets[0] != 0) throw Error(RP_ERR_INVALID, "offsets[0] must be 0");
        for (size_t i = 0; i < n; i++) {
            const std::string at = "request " + std::to_string(i);
            if (entries[i] >= t->sim->n) throw Error(RP_ERR_INVALID, at + ": entry node out of range");
            if (offsets[i + 1] < offsets[i]) throw Error(RP_ERR_INVALID, at + ": offsets decrease");
            if (offsets[i + 1] - offsets[i] > rp::RA_MAX_K) throw Error(RP_ERR_INVALID, at + ": more than 256 keys");
            max_k = std::max(max_k, (uint32_t)(offsets[i + 1] - offsets[i]));
        }
        const size_t T = n ? (size_t)offsets[n] : 0;
        if (T && !key_hashes) throw Error(RP_ERR_INVALID, "null pointer");
        t->prepare();
        if (first_id) *first_id = t->next_id;
        if (n == 0) return;
        t->ensure_table(t->bound + n, t->bound_keys + T);  // (RP_ERR_CAPACITY before anything is copied or changed)
        DevBuf<uint32_t> de(n), dh(T);
        DevBuf<uint64_t> doff(n + 1);
        RP_HIP(hipMemcpyAsync(de.p, entries, n * 4, hipMemcpyHostToDevice, t->st()));
        RP_HIP(hipMemcpyAsync(doff.p, offsets, (n + 1) * 8, hipMemcpyHostToDevice, t->st()));
        if (T) RP_HIP(hipMemcpyAsync(dh.p, key_hashes, T * 4, hipMemcpyHostToDevice, t->st()));
        t->submit(rp::TallBatch{de.p, doff.p, dh.p, 0, 0, 0, 0}, offsets, n, T, max_k);  // (ends with the stream drained)
    });
}

int rp_traffic_all_submit_uniform(rp_traffic_all* t, uint64_t seed, uint64_t first, uint64_t count, uint32_t keys_per_request) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        if (keys_per_request < 1 || keys_per_request > rp::RA_MAX_K)
            throw Error(RP_ERR_INVALID, "keys_per_request must be 1..256");
        t->prepare();
        if (count == 0) return;
        if (count > (1ull << 31) / keys_per_request) throw Error(RP_ERR_CAPACITY, "count x keys_per_request overflows");
        t->submit(rp::TallBatch{nullptr, nullptr, nullptr, seed, first, 0, keys_per_request}, nullptr, count,
                  count * keys_per_request, keys_per_request);
    });
}

int rp_traffic_all_poll(rp_traffic_all* t) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        t->prepare();
        t->launch_poll();
        t->read_ctl();
    });
}

int rp_traffic_all_run(rp_traffic_all* t, int k_rounds, int churn_active, uint64_t per_round, uint32_t keys_per_request,
                       uint64_t seed) {
    return rp::guarded([&] {
        if (!t || k_rounds < 0) throw Error(RP_ERR_INVALID, "bad argument");
        if (per_round && (keys_per_request < 1 || keys_per_request > rp::RA_MAX_K))
            throw Error(RP_ERR_INVALID, "keys_per_request must be 1..256");
        RP_HIP(hipSetDevice(t->sim->dev));
        t->read_ctl();
        // a batch stays at most `lifetime` rounds: at most that many earlier batches beside the newest
        const uint64_t batches = std::min<uint64_t>((uint64_t)k_rounds, t->lifetime + 1);
        const uint64_t K = per_round ? keys_per_request : 0;
        if (per_round && batches > (1ull << 31) / (per_round * K)) throw Error(RP_ERR_CAPACITY, "per_round x rounds overflows");
        const uint64_t need = t->bound + per_round * batches, need_keys = t->bound_keys + per_round * K * batches;
        if (per_round || t->bound) t->ensure_table(need, need_keys);
        t->ensure_results(t->next_id + per_round * (uint64_t)k_rounds);
        if (per_round) t->ensure_stage(per_round, per_round * K);
        uint64_t host_bound = t->bound, host_keys = t->bound_keys;
        for (int r = 0; r < k_rounds; r++) {
            t->sim->rings_changed();
            t->sim->run(1, churn_active != 0);
            t->sim->route_prepare();  // (rp_sim_round's error check; no other readback)
            t->bound = host_bound;
            t->bound_keys = host_keys;
            t->launch_poll();
            if (per_round) {
                t->launch_submit(rp::TallBatch{nullptr, nullptr, nullptr, seed, t->run_index, 0, keys_per_request}, nullptr,
                                 per_round, keys_per_request);
                t->run_index += per_round;
                host_bound = std::min(need, host_bound + per_round);
                host_keys = std::min(need_keys, host_keys + per_round * K);
            }
        }
        t->read_ctl();
    });
}

int rp_traffic_all_read_stats(rp_traffic_all* t, rp_traffic_all_stats* cumulative, uint64_t* by_retries) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        RP_HIP(hipSetDevice(t->sim->dev));
        unsigned long long h[rp::TA_NSLOTS];
        RP_HIP(hipMemcpyAsync(h, t->cum.p, sizeof h, hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
        static_assert(sizeof(rp_traffic_all_stats) == rp::TA_NSTATS * 8, "rp_traffic_all_stats is 24 x u64");
        static_assert(offsetof(rp_traffic_all_stats, local) == 8 * rp::TA_LOCAL &&
                          offsetof(rp_traffic_all_stats, proxied) == 8 * rp::TA_PROXIED &&
                          offsetof(rp_traffic_all_stats, misrouted_keys) == 8 * rp::TA_MISROUTED_KEYS,
                      "the device counters are the struct's fields, in order");
        for (uint32_t o = 0; o < rp::TA_NOUTCOMES; o++)  // (the kernels count final sends by outcome and retries only)
            for (uint32_t r = 0; r < rp::TA_RETRY_SLOTS; r++) h[rp::TA_LOCAL + o] += h[rp::TA_NSTATS + o * rp::TA_RETRY_SLOTS + r];
        if (cumulative) memcpy(cumulative, h, sizeof *cumulative);
        if (by_retries)
            for (uint32_t i = 0; i < rp::TA_NOUTCOMES * rp::TA_RETRY_SLOTS; i++) by_retries[i] = h[rp::TA_NSTATS + i];
    });
}

int rp_traffic_all_pending(rp_traffic_all* t, rp_send_pending* sends, size_t cap, uint64_t* nsends, uint32_t* keys,
                           size_t key_cap, uint64_t* nkeys) {
    return rp::guarded([&] {
        if (!t) throw Error(RP_ERR_INVALID, "null tracker");
        RP_HIP(hipSetDevice(t->sim->dev));
        t->read_ctl();
        const size_t nr = (size_t)t->bound, nk = (size_t)t->bound_keys;
        std::vector<uint4> req(2 * nr), groups(nk);
        std::vector<uint32_t> hk(nk);
        auto& tb = t->tab[t->cur];
        if (nr) RP_HIP(hipMemcpyAsync(req.data(), tb.req.p, nr * 32, hipMemcpyDeviceToHost, t->st()));
        if (nk) RP_HIP(hipMemcpyAsync(groups.data(), tb.groups.p, nk * 16, hipMemcpyDeviceToHost, t->st()));
        if (nk) RP_HIP(hipMemcpyAsync(hk.data(), tb.keys.p, nk * 4, hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
        // two passes: the counts (and the buffers' sizes checked before anything is written), then the records
        for (int pass = 0; pass < 2; pass++) {
            uint64_t ns = 0, nkk = 0;
            for (size_t i = 0; i < nr; i++) {
                const uint4 w0 = req[2 * i], w1 = req[2 * i + 1];
                const uint32_t ng = w1.x >> 16;
                for (uint32_t g = 0; g < ng; g++) {
                    const uint4 s = groups[(size_t)w0.w + g];
                    if ((s.z >> 8) != rp::AO_PENDING) continue;
                    const uint32_t kbeg = s.w & 0xFFFFu, kcnt = s.w >> 16;
                    if (pass && sends)
                        sends[ns] = rp_send_pending{(uint64_t)w0.x | (uint64_t)w0.y << 32, w0.z, (uint16_t)g, (uint16_t)kcnt,
                                                    (int32_t)s.x, s.y, w1.y, s.z & 0xFFu};
                    if (pass && keys) memcpy(keys + nkk, hk.data() + w0.w + kbeg, (size_t)kcnt * 4);
                    ns++;
                    nkk += kcnt;
                }
            }
            if (!pass) {
                if (nsends) *nsends = ns;
                if (nkeys) *nkeys = nkk;
                if ((sends && cap < ns) || (keys && key_cap < nkk)) throw Error(RP_ERR_INVALID, "pending buffer too small");
            }
        }
    });
}

int rp_traffic_all_results(rp_traffic_all* t, uint64_t first_id, size_t n, rp_request_all_result* out) {
    return rp::guarded([&] {
        if (!t || (n && !out)) throw Error(RP_ERR_INVALID, "null pointer");
        if (!t->cfg.track) throw Error(RP_ERR_INVALID, "the tracker was created without `track`");
        if (first_id > t->next_id || n > t->next_id - first_id) throw Error(RP_ERR_INVALID, "ids beyond the last submitted");
        RP_HIP(hipSetDevice(t->sim->dev));
        static_assert(sizeof(rp_request_all_result) == 16, "a request's record is one 16-byte word");
        if (n) RP_HIP(hipMemcpyAsync(out, t->results.p + first_id, n * 16, hipMemcpyDeviceToHost, t->st()));
        RP_HIP(hipStreamSynchronize(t->st()));
    });
}

}  // extern "C"
