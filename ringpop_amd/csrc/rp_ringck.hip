// ringpop_amd — ring checksums of many views, one view per lane
// (k_ring_checksums_pl).  HashRing.checksum (lib/ring.js:
// 96-105) is farmhash32 of the in-ring members' addresses in id order joined
// by ';'.  k_ring_checksums (rp_route.hip) gives a wave to each view; here a
// wave takes 64 views, lane l the view i0 + l, and walks the members once for
// all of them: member a's text, ';' + its address, is the same for every lane
// (scalar loads, scalar shifts), the only per-lane input is the member's
// presence bit, and each lane keeps its own farmhash chain (h, g, f, blocks
// left) in registers and its own byte stream in LDS.  A code object of its
// own; launched by rp_sim::refresh_ring_checksums for shards of at least
// ring_ck_lane_min views.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rp_block.h"
#include "rp_checksum.h"
#include "rp_cluster.h"

namespace rp {

constexpr uint32_t RPL_GRP = 4;                 // members per phase (one drain of the lanes' buffers each)
constexpr uint32_t RPL_PHASES = 64 / RPL_GRP;   // phases per tile of 64 members
constexpr uint32_t RPL_TW = ADDR_WORDS + 1;     // words of a member's text: ';' + up to 32 bytes
constexpr uint32_t RPL_MAXBLK = (16 + 3 + RPL_GRP * (1 + 4 * ADDR_WORDS)) / 20;  // blocks a phase can complete: 7
// A lane's buffer, in words: word 0 takes the discarded start of the stream,
// block j of a drain is words 1 + 5j .. 5 + 5j.  A phase starts with at most
// 4 complete words and 3 bytes carried, its last member starts at most
// (16 + 3 + (RPL_GRP - 1) x 33) / 4 words in and writes RPL_TW + 1 words from
// there; the drain reads one block past the last one it hashes.
constexpr uint32_t RPL_STRIDE = 1 + 5 * (RPL_MAXBLK + 1);  // 41: odd, so the lanes' words fall in different banks
static_assert(1 + (16 + 3 + (RPL_GRP - 1) * (1 + 4 * ADDR_WORDS)) / 4 + RPL_TW + 1 <= RPL_STRIDE, "lane buffer too short");
static_assert(RPL_STRIDE % 2 == 1 && 64 % RPL_GRP == 0, "odd stride; a phase's members lie in one tile");

typedef __attribute__((address_space(4))) const uint32_t rpl_kconst_u32;  // through the scalar cache (s_load)

// The presence bytes of 64 views x 64 members become one 64-bit mask per lane
// (bit j of lane r: member a0 + j is in view r's ring).  Rows are n bytes
// apart and aligned to nothing, so each row's 64 bytes are one byte per lane
// -- a single contiguous segment per load instruction -- and the wave's
// ballot of "non-zero" is the row's mask, which lane r keeps.  `RowLoads` is
// a batch of NR rows in flight.
template <uint32_t NR>
struct RowLoads {
    uint32_t b[NR];
    // rows r0 .. r0 + NR of the tile at member a0.  Every load is issued, at
    // an address clamped into the group's rows (no per-row condition to keep):
    // `into` drops the rows past nv and the members past n.
    // (r0 is made opaque: hoisted out of the tile loops, the 64 rows' offsets
    // and lane masks would take more scalar registers than there are)
    __device__ inline void issue(const uint8_t* rows, uint32_t n, uint32_t nv, uint32_t a0, uint32_t r0) {
        asm volatile("" : "+s"(r0));
        const uint8_t* const col = rows + min(a0 + lane_id(), n - 1);
#pragma unroll
        for (uint32_t k = 0; k < NR; k++) b[k] = col[(size_t)min(r0 + k, nv - 1) * n];
    }
    // valid: the ballot of the tile's members below n
    __device__ inline void into(uint32_t& mlo, uint32_t& mhi, uint32_t r0, uint32_t nv, uint64_t valid) const {
        asm volatile("" : "+s"(r0));
#pragma unroll
        for (uint32_t k = 0; k < NR; k++) {
            const uint64_t bal = r0 + k < nv ? __ballot(b[k] != 0) & valid : 0ull;
            const bool mine = lane_id() == (int)(r0 + k);
            mlo = mine ? (uint32_t)bal : mlo;
            mhi = mine ? (uint32_t)(bal >> 32) : mhi;
        }
    }
};

// A lane's byte stream by whole words (the append of rp_sim.hip's LaneStream
// for the one kind of piece a ring has).  `acc` holds the nb (0-3) bytes of
// the incomplete word; a piece of K uniform bytes in uniform words c[0 .. W)
// is written as acc | c[0] << 8 nb and then the funnel shifts of c[i - 1] :
// c[i], unconditionally, at the write position, which moves only where `on`
// (a word written past it is overwritten by the next append before a drain
// reads it).  No branch depends on the lane.
struct RingLane {
    uint32_t* buf;  // the lane's RPL_STRIDE words
    uint32_t acc, nb, wp;
    __device__ inline void piece(const uint32_t (&c)[RPL_TW], uint32_t K, uint32_t W, bool on) {
        // (one byte permute: selector byte m = 4 - nb + m; 4..7 name the high word's bytes, 0..3 the low's)
        const uint32_t sel = 0x07060504u - nb * 0x01010101u;
        uint32_t prev = acc | (c[0] << (8 * nb)), cur = prev;
        buf[wp] = prev;
#pragma unroll
        for (uint32_t i = 1; i <= RPL_TW; i++) {
            if (i > W) break;  // (uniform)
            const uint32_t ci = i < W ? c[i < RPL_TW ? i : 0] : 0u;  // (W <= RPL_TW)
            prev = cur;
            cur = __builtin_amdgcn_perm(ci, c[i - 1], sel);
            buf[wp + i] = cur;
        }
        const uint32_t tot = nb + (on ? K : 0u), nout = tot >> 2;
        acc = on ? (nout == W ? cur : prev) & ((1u << (8 * (tot & 3))) - 1u) : acc;
        wp += nout;
        nb = tot & 3;
    }
};

// Ring checksums of views [lo, lo + nl): rows = their in_ring rows (nl x n),
// out indexed by node id.  One wave per 64 views (grid-stride).
//
// Pass 1 walks the tiles from the top down and takes, per lane, the string's
// length and member count and its last 20 bytes -- farmhash's > 24-byte
// branch needs both before the first block, and a ring has no stored length.
// The tail is written backwards, byte by byte, while fewer than 20 bytes are
// covered: at most 20 bytes and 10 members per lane, whatever n is.  Pass 2
// walks the tiles upwards in phases of RPL_GRP members: every lane appends
// the member's text where its bit is set, then drains the whole 20-byte
// blocks of its buffer into its chain and moves the < 5 words left to the
// buffer's front.  A lane's first member has no ';': its stream starts three
// bytes into the discarded word 0, which the first ';' completes.  Strings of
// <= 24 bytes are never drained; they are hashed at the end by farmhash32's
// short branches from the buffer.
//
// The presence rows of the next tile are loaded RPL_GRP per phase, at the
// phase's start, and packed into the next masks at its end, so their latency
// lies behind the phase's appends and chain steps; pass 1 keeps two batches
// of 16 rows in flight.  No lane reads another's LDS words: no barrier.
__global__ void __launch_bounds__(64) k_ring_checksums_pl(const uint8_t* in_ring, uint32_t n, uint32_t lo, uint32_t nl,
                                                          const uint32_t* addr_words, const uint8_t* addr_len,
                                                          uint32_t* out) {
    __shared__ uint32_t bufs[64 * RPL_STRIDE];
    const uint32_t lane = lane_id();
    const uint32_t NT = (n + 63) / 64;
    uint32_t* const B = bufs + lane * RPL_STRIDE;
    for (uint32_t i0 = blockIdx.x * 64; i0 < nl; i0 += gridDim.x * 64) {
        const uint32_t nv = min(64u, nl - i0);  // this group's views
        const uint8_t* const rows = in_ring + (size_t)i0 * n;
        const bool act = lane < nv;

        // ---- pass 1: length, count, last 20 bytes
        uint32_t len = 0, cnt = 0, T = 0;  // len: every member's bytes + 1; T: bytes covered from the end
        uint8_t* const tl = (uint8_t*)B;   // the tail, bytes [0, 20)
        RowLoads<16> ra, rb;
        ra.issue(rows, n, nv, (NT - 1) * 64, 0);
        // lane j: the bytes of member a0 + j's address, loaded one tile ahead
        auto len_at = [&](uint32_t a) -> uint32_t { return a < n ? addr_len[a] : 0u; };
        uint32_t Ln = len_at((NT - 1) * 64 + lane);
        for (uint32_t t = NT; t-- > 0;) {
            const uint32_t a0 = t * 64;
            uint32_t mlo = 0, mhi = 0;
            const uint32_t Lv = a0 + lane < n ? Ln + 1u : 0u;  // (+ 1: the member's ';')
            Ln = t > 0 ? len_at(a0 - 64 + lane) : 0u;
            const uint64_t valid = __ballot(a0 + lane < n);
            rb.issue(rows, n, nv, a0, 16);
            ra.into(mlo, mhi, 0, nv, valid);
            ra.issue(rows, n, nv, a0, 32);
            rb.into(mlo, mhi, 16, nv, valid);
            rb.issue(rows, n, nv, a0, 48);
            ra.into(mlo, mhi, 32, nv, valid);
            ra.issue(rows, n, nv, t > 0 ? a0 - 64 : 0u, 0);  // (the next tile down; at the bottom, unused)
            rb.into(mlo, mhi, 48, nv, valid);
            const uint64_t m = ((uint64_t)mhi << 32) | mlo;
            cnt += (uint32_t)__popcll(m);
            if (__ballot(m != valid && act) == 0) {
                // (every view of the group holds the whole tile; summed by all lanes, then kept by the views')
                const uint32_t whole = (uint32_t)wave_sum64(Lv);
                len += act ? whole : 0u;
            } else {
#pragma unroll 4
                for (uint32_t j = 0; j < 64; j++) {
                    const uint32_t Lj = __builtin_amdgcn_readlane(Lv, j);
                    len += ((m >> j) & 1u) ? Lj : 0u;
                }
            }
            uint64_t mm = m;
            while (T < 20 && mm) {
                const uint32_t j = 63u - (uint32_t)__builtin_clzll(mm);
                mm &= ~(1ull << j);
                const uint32_t a = a0 + j, L = addr_len[a];
                const uint8_t* const ab = (const uint8_t*)(addr_words + (size_t)a * ADDR_WORDS);
                // the member's text from its end: L address bytes, then its ';'
                for (uint32_t k = 0; k <= L && T + k < 20; k++) tl[19 - (T + k)] = k < L ? ab[L - 1 - k] : (uint8_t)0x3B;
                T += L + 1;
            }
        }
        const uint32_t slen = cnt ? len - 1 : 0u;
        const bool small = act && slen <= 24;
        FhStream st = fh_stream_begin5(slen, B[0], B[1], B[2], B[3], B[4]);
        st.blocks_left = act && slen > 24 ? st.blocks_left : 0u;

        // ---- pass 2: the members in order
        RingLane ls;
        ls.buf = B;
        ls.acc = 0;
        ls.nb = 3;
        ls.wp = 0;
        uint32_t mlo = 0, mhi = 0;
        const uint64_t valid0 = __ballot(lane < n);
        rb.issue(rows, n, nv, 0, 16);  // (rows 0 .. 15 of tile 0 are in ra: pass 1's last prefetch)
        ra.into(mlo, mhi, 0, nv, valid0);
        ra.issue(rows, n, nv, 0, 32);
        rb.into(mlo, mhi, 16, nv, valid0);
        rb.issue(rows, n, nv, 0, 48);
        ra.into(mlo, mhi, 32, nv, valid0);
        rb.into(mlo, mhi, 48, nv, valid0);
        Ln = len_at(lane);
        for (uint32_t t = 0; t < NT; t++) {
            if (__ballot(small || st.blocks_left != 0) == 0) break;  // (the rest is in the tails)
            const uint32_t a0 = t * 64;
            const bool more = t + 1 < NT;
            const uint32_t Lv = Ln;
            Ln = len_at(a0 + 64 + lane);
            uint32_t nlo = 0, nhi = 0;
            const uint64_t nvalid = __ballot(a0 + 64 + lane < n);
            for (uint32_t p = 0; p < RPL_PHASES; p++) {
                RowLoads<RPL_GRP> nx;
                nx.issue(rows, n, nv, a0 + 64, p * RPL_GRP);  // (past the top tile: clamped, unused)
                const uint32_t ap = a0 + p * RPL_GRP;
                if (ap < n) {
                    const bool live = small || st.blocks_left != 0;
                    const uint32_t mw = (p < RPL_PHASES / 2 ? mlo : mhi) >> ((p * RPL_GRP) & 31u);
#pragma unroll
                    for (uint32_t k = 0; k < RPL_GRP; k++) {
                        const uint32_t a = ap + k;
                        if (a >= n) break;  // (uniform)
                        const uint32_t L = __builtin_amdgcn_readlane(Lv, (p * RPL_GRP + k) & 63u);
                        const rpl_kconst_u32* const aw = (const rpl_kconst_u32*)(addr_words + (size_t)a * ADDR_WORDS);
                        uint32_t w[ADDR_WORDS], c[RPL_TW];
#pragma unroll
                        for (uint32_t q = 0; q < ADDR_WORDS; q++) w[q] = aw[q];
                        c[0] = 0x3Bu | (w[0] << 8);
#pragma unroll
                        for (uint32_t q = 1; q < ADDR_WORDS; q++) c[q] = (w[q - 1] >> 24) | (w[q] << 8);
                        c[ADDR_WORDS] = w[ADDR_WORDS - 1] >> 24;
                        ls.piece(c, L + 1, (L + 4) >> 2, live && ((mw >> k) & 1u));
                    }
                    // drain: the whole blocks the chain still takes, the next
                    // block's words read while this one's chain step runs
                    const uint32_t avail = max(ls.wp, 1u) - 1u;
                    const uint32_t nbk = min(avail / 5u, st.blocks_left);
                    uint32_t x0 = B[1], x1 = B[2], x2 = B[3], x3 = B[4], x4 = B[5];
                    for (uint32_t j = 0; __ballot(j < nbk) != 0; j++) {
                        const uint32_t* const nb5 = B + 6 + 5 * j;
                        const uint32_t y0 = nb5[0], y1 = nb5[1], y2 = nb5[2], y3 = nb5[3], y4 = nb5[4];
                        FhStream s2 = st;
                        fh_stream_block(s2, x0, x1, x2, x3, x4);
                        const bool take = j < nbk;
                        st.h = take ? s2.h : st.h;
                        st.g = take ? s2.g : st.g;
                        st.f = take ? s2.f : st.f;
                        x0 = y0; x1 = y1; x2 = y2; x3 = y3; x4 = y4;
                    }
                    st.blocks_left -= nbk;
                    if (nbk) {
                        // (a chain that took its last block renders nothing more: its position is parked)
                        const uint32_t* const src = B + 1 + 5 * nbk;
                        const uint32_t m0 = src[0], m1 = src[1], m2 = src[2], m3 = src[3];
                        B[1] = m0; B[2] = m1; B[3] = m2; B[4] = m3;
                        ls.wp = st.blocks_left ? 1u + (avail - 5u * nbk) : 1u;
                    }
                }
                if (more) nx.into(nlo, nhi, p * RPL_GRP, nv, nvalid);
            }
            mlo = nlo;
            mhi = nhi;
        }
        B[ls.wp] = ls.acc;  // (a short string's last bytes)
        uint32_t res = fh_stream_end(st);
        if (__ballot(small) != 0) {
            if (small) res = farmhash32((const uint8_t*)(B + 1), slen);
        }
        if (act) out[lo + i0 + lane] = res;
    }
}

void launch_ring_checksums_pl(const uint8_t* in_ring, uint32_t n, uint32_t lo, uint32_t nl, const uint32_t* addr_words,
                              const uint8_t* addr_len, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(k_ring_checksums_pl, dim3(grid_for(nl, 64)), dim3(64), 0, st, in_ring, n, lo, nl, addr_words,
                       addr_len, out);
}

}  // namespace rp
