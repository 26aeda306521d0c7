// ringpop_amd — what the replica-set census (rp_repl.hip) shares
// with the holders query (rp_hold.hip; §17): the limits of a replica walk, the
// set of distinct owners a walk keeps in registers, and the walkers over the
// global points in one view.  Each feature stays a translation unit of its
// own, so that neither changes the other's code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rp_own.h"

namespace rp {

constexpr uint32_t REP_MAX_R = 8;        // replicas of the census
constexpr uint32_t REP_MAX_N = 16;       // owners of a per-view lookupN
constexpr uint32_t REP_SOLO_EXTRA = 3;   // a lane examines target + 3 points alone before the wave walks for it
constexpr uint32_t REP_NONE = 0xFFFFFFFFu;  // a walk that went once round without ending

// k_hold_list (rp_hold.hip) on st: one wave per key over its row of `tiles`
// 64-bit words, bit b of word t standing for node t * 64 + b -- counts[key] =
// the bits set, holders[key * cap ..] the first `cap` of their nodes in
// ascending order, the remaining slots -1.  The holders query's second kernel,
// which replica-set movement (rp_rmove.hip; §19) runs on its gain and loss masks.
void hold_list(const unsigned long long* mask, uint32_t nk, uint32_t tiles, uint32_t cap, int32_t* holders, uint32_t* counts,
               hipStream_t st);

// The distinct owners a walk has kept, in order of first appearance: K
// registers, written and compared by unrolled chains of selects (constant
// indices only: nothing spills to scratch).  Empty slots hold -2, which no
// owner (>= 0) equals.  add() past K only counts: the walk ends there.
template <int K>
struct OwnerSet {
    int32_t s[K];
    uint32_t cnt;
    __device__ inline void clear() {
#pragma unroll
        for (int j = 0; j < K; j++) s[j] = -2;
        cnt = 0;
    }
    __device__ inline bool has(int32_t o) const {
        bool f = false;
#pragma unroll
        for (int j = 0; j < K; j++) f |= s[j] == o;
        return f;
    }
    __device__ inline void add(int32_t o) {
#pragma unroll
        for (int j = 0; j < K; j++) s[j] = cnt == (uint32_t)j ? o : s[j];
        cnt++;
    }
    // lane L's set, in scalar registers (L is wave-uniform)
    __device__ inline OwnerSet of(int L) const {
        OwnerSet w;
#pragma unroll
        for (int j = 0; j < K; j++) w.s[j] = __builtin_amdgcn_readlane(s[j], L);
        w.cnt = (uint32_t)__builtin_amdgcn_readlane((int)cnt, L);
        return w;
    }
};

// A walk over the global points in one view, backwards (the arc kernel) or
// forwards (lookupN): `pos` is the next point to examine, `dist` the points
// examined so far.  A present point's owner o is kept the first time it
// appears; the walk ends at the point where o == stop (the arc kernel: the
// view's own node; lookupN: -1, never) or where the set reaches `target`
// owners (q = that point), or after npts points (q = REP_NONE).

template <int K>
__device__ inline bool walk_take(OwnerSet<K>& u, int32_t o, int32_t stop, uint32_t target) {
    if (o == stop) return true;
    u.add(o);
    return u.cnt >= target;
}

template <bool BACK>
__device__ inline uint32_t walk_move(uint32_t pos, uint32_t d, uint32_t npts) {  // (d < npts)
    if (BACK) return pos >= d ? pos - d : pos + npts - d;
    return pos + d < npts ? pos + d : pos + d - npts;
}

// a lane alone, at most `steps` points
template <int K, bool BACK>
__device__ inline void walk_solo(const RouteRing& ring, const OwnArgs& A, OwnerSet<K>& u, uint32_t& pos, uint32_t& dist,
                                 bool& done, uint32_t& q, int32_t stop, uint32_t target, uint32_t steps) {
    for (uint32_t k = 0; k < steps && !done; k++) {
        const int32_t o = ring.owner(A.pt_coll[pos], A.pt_server[pos]);
        dist++;
        if (o >= 0 && (o == stop || !u.has(o)) && walk_take(u, o, stop, target)) {
            done = true;
            q = pos;
        } else if (dist >= A.npts) {
            done = true;
            q = REP_NONE;
        } else {
            pos = walk_move<BACK>(pos, 1, A.npts);
        }
    }
}

// The wave serves its lanes that are still walking (`pending`) one after the
// other, the lowest first, each to its end.  The served lane's set, position
// and distance go to scalar registers; a step examines the next 64 points, one
// per lane, and takes a ballot of those that are present and whose owner is
// not in the set yet (or is `stop`).  The hits are consumed nearest first,
// the owner read from its lane; a kept owner's other points in the step are
// struck from the ballot, so a step consumes at most `target` hits and a walk
// over m points costs m / 64 + target steps' work at the most.  The whole wave
// must call this together.  Returns the steps taken.
template <int K, bool BACK>
__device__ inline uint32_t walk_wave(const RouteRing& ring, const OwnArgs& A, OwnerSet<K>& u, uint32_t pos, uint32_t dist,
                                     bool pending, uint32_t& q, int32_t stop, uint32_t target, uint32_t lane) {
    const uint32_t npts = A.npts;
    uint32_t steps = 0;
    unsigned long long pend;
    while ((pend = __ballot(pending)) != 0) {
        const int L = __ffsll(pend) - 1;
        OwnerSet<K> w = u.of(L);
        uint32_t bpos = (uint32_t)__builtin_amdgcn_readlane((int)pos, L);
        uint32_t bdist = (uint32_t)__builtin_amdgcn_readlane((int)dist, L);  // (< npts: the walk goes on)
        uint32_t end = REP_NONE;
        bool fin = false;
        while (!fin) {
            steps++;
            // lanes past a whole turn sit out: lane < npts - bdist <= npts
            const bool valid = bdist + lane < npts;
            uint32_t idx = 0;
            int32_t o = -1;
            if (valid) {
                idx = walk_move<BACK>(bpos, lane, npts);
                o = ring.owner(A.pt_coll[idx], A.pt_server[idx]);
            }
            unsigned long long hits = __ballot(o >= 0 && (o == stop || !w.has(o)));
            while (hits != 0 && !fin) {
                const int h = __ffsll(hits) - 1;
                const int32_t oh = __builtin_amdgcn_readlane(o, h);
                const uint32_t ih = (uint32_t)__builtin_amdgcn_readlane((int)idx, h);
                if (walk_take(w, oh, stop, target)) {
                    fin = true;
                    end = ih;
                } else {
                    hits &= ~__ballot(o == oh);
                }
            }
            if (!fin) {
                bdist += 64;
                if (bdist >= npts) fin = true;  // once round: end stays REP_NONE
                else bpos = walk_move<BACK>(bpos, 64, npts);  // (npts > 64 here)
            }
        }
        if (lane == (uint32_t)L) {
            u = w;
            q = end;
            pending = false;
        }
    }
    return steps;
}

}  // namespace rp
