// ringpop_amd — the simulated cluster's host types, shared by the translation
// units that hold its entry points: a shard and its device
// buffers (Shard), the transport between ranks (Xport) and the cluster
// (rp_sim).  Member functions that launch a round kernel are declared here and
// defined beside the kernels in rp_sim.hip; a feature that adds no round
// kernel lives in a file of its own (rp_route.hip, rp_traffic.hip, rp_own.hip,
// rp_xport.hip) and reaches the cluster through this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "rp_internal.h"
#include "rp_sim.h"
#include "rp_traffic.h"

struct rp_loop;

namespace rp {

struct OwnArgs;  // rp_own.hip

constexpr int NCAT = 7;  // churn, issue, merge_ping, merge_resp, checksum, other, exchange
constexpr int CAT_SIDE = NCAT;  // a span of a shard's side stream (Shard::side_ms; no stage of its own)
constexpr uint32_t CHURN_SLOTS = 1024;  // rounds of churn ids staged per copy

struct TimedSpan {
    int cat;
    hipEvent_t a, b;
};

// Device time of launches, by category: timed() brackets a launch with two
// events on its stream, collect() -- once the streams are drained -- hands
// every span's (category, ms) to the caller.  Events are reused: creating
// one costs a driver call.
struct SpanTimer {
    std::vector<TimedSpan> spans;
    std::vector<hipEvent_t> pool;
    SpanTimer() = default;
    SpanTimer(const SpanTimer&) = delete;
    SpanTimer& operator=(const SpanTimer&) = delete;
    ~SpanTimer() {
        for (auto& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
    hipEvent_t take() {
        hipEvent_t e = nullptr;
        if (!pool.empty()) { e = pool.back(); pool.pop_back(); return e; }
        RP_HIP(hipEventCreate(&e));
        return e;
    }
    template <class F>
    void timed(hipStream_t st, int cat, bool on, F&& launch) {
        if (!on) { launch(); return; }
        TimedSpan s{cat, take(), take()};
        RP_HIP(hipEventRecord(s.a, st));
        launch();
        RP_HIP(hipEventRecord(s.b, st));
        spans.push_back(s);
    }
    template <class G>
    void collect(G&& got) {
        for (auto& s : spans) {
            float ms = 0;
            RP_HIP(hipEventElapsedTime(&ms, s.a, s.b));
            got(s.cat, ms);
            pool.push_back(s.a);
            pool.push_back(s.b);
        }
        spans.clear();
    }
};

struct Shard {
    rp_sim_config cfg{};
    uint32_t n = 0, k = 0;
    uint32_t lo = 0, nl = 0, rank = 0, G = 1;  // this shard holds nodes [lo, lo + nl) of G shards
    bool one_per_process = false;  // exchanges over RCCL (rp_sim_create_rank)
    hipStream_t st = nullptr;
    bool own_stream = false;
    hipEvent_t xev = nullptr;  // in-process clusters: this shard's stream reached an exchange step
    rp::SimDev d{};
    DevBuf<rp::VEnt> view;
    DevBuf<uint64_t> fp, rng, snd_inc, snd_fp, msg_off, snaps, pr_inc, pr_fp, pq_off, rl_off, rl_inc, rl_fp;
    DevBuf<uint32_t> mcount, snap_ord, snap_m;
    DevBuf<uint32_t> order, dhead, dtail, csum, csum_valid, addr_words, msg_len, msg_plen, snd_csum, g_cnt, g_fill, g_base,
        g_list, snap_count, pend_slot, pend_csum, origin_count, err, conv, pr_n, pr_errors, pr_bad, pr_done, pr_csum,
        pq_len, rl_len, rl_csum, thead, ttail;
    DevBuf<Change> arena;
    DevBuf<uint32_t> dko;
    DevBuf<uint32_t> dad;
    DevBuf<uint32_t> p2_list, p2_len;  // k_p2_lists: receivers per ping rank
    DevBuf<uint64_t> p2_msg;           // ... and their pings' bodies (k_p2_apply)
    DevBuf<rp::P2Rec> p2_rec;          // k_p2_pre: one rank's respond records (k_p2_respond)
    DevBuf<uint64_t> dvs;
    DevBuf<rp::Resp> resp;
    DevBuf<uint2> tfifo;
    DevBuf<int32_t> storm;  // CHURN_SLOTS x 2 x storm_kmax: per round, accusers then victims (k_storm)
    uint32_t storm_kmax = 0;
    DevBuf<int32_t> max_pb, ring_count, coll_owner, coll_of, iter_index, iter_round, npingable, target, churn_ids,
        pt_server, pt_coll, w3_dest, w4_dest, w5_dest, w6_dest, dead_ids;
    DevBuf<uint64_t> sv_word;  // k_phase1: same-view decisions
    DevBuf<uint8_t> in_ring, dead, addr_len, need_shuffle, need_csum, pend_done, w4_err;
    DevBuf<uint32_t> shuf_list, shuf_count, g_tile, g_bloc;  // k_iterate: nodes whose iterator wrapped this round
    DevBuf<uint64_t> min_l1, min_l2;
    DevBuf<uint32_t> min_safe, min_cnt, dangerous, dlive, icount, seen, oc_snap, coll_off, coll_ids, rbatch, self_origin;
    DevBuf<uint32_t> cmem_off, cmem;  // per collision group, its servers (ascending): rp_sim_set_views' ring owners
    DevBuf<uint64_t> self_inc;
    DevBuf<int64_t> slen;
    DevBuf<uint32_t> ck_list, ck_count;  // views queued for k_checksums
    DevBuf<uint32_t> ring_csum;          // n: this shard's nodes' ring checksums (rp_sim_ring_checksums; on first use)
    DevBuf<unsigned long long> hkey;      // Shard::checksums: fingerprint table
    DevBuf<uint32_t> hval, ck_lead, ck_nlead, ck_slot;
    DevBuf<rp::CkEntry> ck_cache;
    // the round's sender checksums and fullSync decisions on a side stream
    // (one shard: k_ck_snapcopy, k_checksums_snap beside the ping merge,
    // k_pending beside the response merge's pass 1)
    bool ck_side = false;                      // the side stream exists (one shard)
    // ... and this round uses it: fault runs (fail-stops, storms, partitions),
    // whose distinct views make the checksum stage a few hundred long chains;
    // without faults the stage is a handful of short ones and splitting the
    // response merge around k_pending costs more than it hides
    bool side_round() const { return ck_side && fault_mode; }
    hipStream_t st2 = nullptr;
    hipEvent_t ev_ck_copy = nullptr, ev_ck_done = nullptr, ev_merge_done = nullptr, ev_pend_done = nullptr;
    uint32_t ck_cap = 0;                       // leader rows of the snapshot
    DevBuf<uint64_t> ck_rows;                  // ck_cap x n view values
    DevBuf<unsigned long long> ck_lfp;         // the leaders' fingerprints
    DevBuf<uint32_t> ck_lres, ck_hlead;        // their checksums; leader index by fingerprint slot
    double side_ms = 0;                        // device time of the side stream's work (timing on)
    DevBuf<rp::Origin> origins;
    DevBuf<unsigned long long> arena_cursor, stats, totals, fp_mm, bstats;
    DevBuf<uint32_t> pt_hash;
    // exchange (G > 1)
    DevBuf<rp::PingMeta> meta;
    DevBuf<uint64_t> soff, seoff, psoff, pseoff, rx_off, rx_eoff;
    DevBuf<uint32_t> rr_idx, rs_idx, msg_nesc;
    DevBuf<rp::RespRec> rsend, rrecv;
    DevBuf<uint32_t> sendw, rxw, psendw, rx2w;  // cross-shard messages: words ...
    DevBuf<rp::Esc> sende, rxe, psende, rx2e;  // ... and escapes (SimDev::rxw)
    DevBuf<Change> rxc;                         // received pings, W3-W5 lists decoded (responses, W6: from rx2w)
    DevBuf<unsigned long long> xcnt, sgather, xrow, ltotals;  // ltotals: this shard's own counters
    DevBuf<uint32_t> gseen, gs_range, gsettled;
    // ping-req waves across shards (k_xs_*)
    DevBuf<uint8_t> pr_ckv;
    DevBuf<uint32_t> w3cnt, w4b;  // k_pr_need's per-relay bounds
    DevBuf<uint32_t> fdecl_bits, fdecl_count;
    DevBuf<uint32_t> fdecl_all;  // G: every shard's k_fdecl_share, all-gathered (sharded fault rounds)
    bool fd_shared = false;      // fdecl_all holds this round's counts
    // a view may hold faulty or leave members no k_timers declared (views set
    // from given statuses, changes applied through the node bridge): k_pr_need
    // then bounds its relays' ring shrink by all n (k_pr_hist)
    bool faulty_unbounded = false;
    DevBuf<uint32_t> pq_nesc, rl_nesc, xs_rec, xs_w, xs_e, xs_list, xs_nlist, lorigin_count, lorigin_sent;
    DevBuf<rp::Origin> og;  // origin all-gather: G blocks of 1 + og_cap records (k_origin_pack)
    uint32_t og_cap = 0;
    DevBuf<uint64_t> xs_wabs, xs_eabs;
    DevBuf<rp::SlotRec> xsend, xrecv;
    DevBuf<unsigned long long> xsrow;
    unsigned long long* h_xsrow = nullptr;  // pinned: the all-gathered G x 3 x G send counts, then the pack count
    unsigned long long* h_xcnt = nullptr;  // pinned: XC_NCAT x G counts of the round
    unsigned long long* h_xrow = nullptr;  // pinned: G x 2 x G response payload counts (words, escapes)
    uint32_t npts = 0, ncoll = 0, seen_words = 0;
    bool join_mode = false;  // views may lack members: the JOIN merge kernels
    bool life_mode = false;  // graceful leaves scheduled (with join_mode): k_iterate / k_round_end skip gossip-off nodes
    DevBuf<uint32_t> life_ev, tcount;  // a round's events (k_lifecycle); k_timer_count's result
    bool fault_mode = false;  // fail-stops, storms or partitions scheduled: the settled-filter issue kernels
    bool issue_wave = RP_ISSUE_WAVE != 0;  // rp_sim_config.issue_wave: the one-wave issue kernels where eligible
    // k_phase1 / k_p2_respond as one wave per node (wave_issue): runs without
    // faults or joins, rows of whole 64-entry groups, a seen window that fits its LDS
    bool wave_issue_ok() const {
        return issue_wave && !fault_mode && !join_mode && n % 64 == 0 && seen_words <= rp::SEEN_STAGE_WORDS;
    }
    // join replies of a round (rp_sim_join): per pair its seed's view, member
    // order / count and checksum (filled on the seed's shard, then shared)
    DevBuf<uint64_t> jvs;
    DevBuf<uint32_t> jord, jm, jcs, j_ids, j_poff, j_pidx, j_pjoin, j_seedof;
    DevBuf<int32_t> j_pseed;
    std::vector<std::string> addrs;  // in sort order; preset by rp_sim_load_addresses, else the sim scheme
    uint32_t timing = 0;  // bit cat: stage cat's spans are timed (rp_sim_enable_timing_stages)
    uint64_t xsent = 0;  // bytes this shard sent to other shards (all-gathers, all-to-alls, all-reduces) since enable_timing
    SpanTimer tm;  // both streams' spans, one event pool
    double kms[NCAT] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t klaunch[NCAT] = {0, 0, 0, 0, 0, 0, 0};

    ~Shard() {
        if (h_xcnt) (void)hipHostFree(h_xcnt);
        if (h_xrow) (void)hipHostFree(h_xrow);
        if (h_xsrow) (void)hipHostFree(h_xsrow);
        if (xev) (void)hipEventDestroy(xev);
        for (hipEvent_t e : {ev_ck_copy, ev_ck_done, ev_merge_done, ev_pend_done})
            if (e) (void)hipEventDestroy(e);
        if (st2) (void)hipStreamDestroy(st2);
        if (st && own_stream) (void)hipStreamDestroy(st);
    }
    // side-stream work, timed on its own stream (kernel_ms "checksum_side")
    template <class F>
    void side_timed(F&& launch) {
        tm.timed(st2, CAT_SIDE, (timing >> 4) & 1u, launch);
    }
    template <class F>
    void timed(int cat, F&& launch) {
        tm.timed(st, cat, (timing >> cat) & 1u, launch);
    }
    void collect_timing() {
        tm.collect([&](int cat, float ms) {
            if (cat == CAT_SIDE) { side_ms += ms; return; }
            kms[cat] += ms;
            klaunch[cat]++;
        });
    }
    // buffer resets queued for one k_fill_batch launch (fill_flush)
    std::vector<rp::FillDesc> fills;
    void fill(void* dst, uint64_t bytes, uint8_t byte) {
        if (bytes % 4) throw Error(RP_ERR_STATE, "fill: size not a multiple of 4");
        if (bytes) fills.push_back(rp::FillDesc{dst, bytes, byte * 0x01010101u, 0});
    }
    // seen_clear: the last batch also clears the round's seen bits (k_round_start)
    void fill_flush(bool seen_clear = false);

    void setup();
    // prefilled: counts reset by stage_start; counted: and counted already (k_phase1, one shard)
    void group(const int32_t* dest, uint32_t nslots, bool prefilled = false, bool counted = false);
    // the pending fullSync decisions (k_pending)
    void launch_pending(hipStream_t s);
    // one round = these stages in order; a cluster exchanges between them
    void stage_start(uint32_t round, bool churn_active, uint32_t slot, const std::vector<int32_t>& dead_now,
                     bool faults, const uint32_t part[3], uint32_t storm_k);
    void stage_churn(bool churn_active, uint32_t slot, uint32_t storm_k, uint64_t now);
    // the set() bootstrap of nodes [node_lo, node_lo + count) from views (st/inc
    // rows, or every member of member_map alive at INC0 + id) (rp_sim_set_views)
    void bootstrap_views(uint32_t node_lo, uint32_t count, const uint8_t* st, const uint64_t* inc,
                         const uint8_t* member_map, uint64_t seed);
    void stage_issue();
    void stage_checksums();
    void stage_ping_merge(uint64_t now);
    void stage_resp_merge(uint64_t now, bool faults);
    void stage_pr_need();
    void stage_wave(int w, uint64_t now);  // ping-req waves W3..W6 (faults)
    void checksums(uint32_t* out, bool prefilled = false);  // ck_list's views -> out[v] (and the cache), one per distinct view
    void ensure_ck_side();                 // the side stream's leader rows (allocated when faults are scheduled)
    void checksums_side(uint32_t* out, bool prefilled = false);  // the same, the chains on st2 (ck_side; ready at ev_ck_done)
    // exchange buffers sized to a round's traffic (escapes dominate once
    // suspect/faulty updates circulate); direction 0: pings and W3/W4,
    // 1: responses and W5/W6
    void fit_exchange(int dir, uint64_t send_w, uint64_t send_e, uint64_t recv_w, uint64_t recv_e);
    // every exchange buffer to at least e elements (rp_sim::presize_exchange)
    void presize(uint64_t e) {
        for (auto* b : {&sendw, &rxw, &psendw, &rx2w}) b->reserve(e);
        for (auto* b : {&sende, &rxe, &psende, &rx2e}) b->reserve(e);
        rxc.reserve(e);
        d.rxw = rxw.p; d.rxe = rxe.p; d.rx2w = rx2w.p; d.rx2e = rx2e.p; d.rxc = rxc.p;
    }
    uint64_t xsum(int cat) const {
        uint64_t t = 0;
        for (uint32_t q = 0; q < G; q++) t += h_xcnt[(size_t)cat * G + q];
        return t;
    }
    void stage_end();
    uint32_t read_err();
};

// ---------------------------------------------------------------- rank transports
// A process that holds one shard of a G-rank cluster exchanges with the other
// ranks through a transport (rp_xport.hip): RCCL, or a loopback among the
// host threads of one process on one device.
struct Xfer {
    uint32_t peer;
    void* ptr;
    size_t bytes;
};
struct Xport {
    virtual ~Xport() = default;
    // in place: this rank's chunk is base + rank * bytes, the others arrive
    virtual void allgather(uint8_t* base, size_t bytes, uint32_t rank, hipStream_t st) = 0;
    virtual void allreduce_u32(uint32_t* buf, size_t count, hipStream_t st) = 0;
    // matching pairs: this rank's send to q is q's receive from this rank
    virtual void sendrecv(const std::vector<Xfer>& sends, const std::vector<Xfer>& recvs, hipStream_t st) = 0;
    virtual void broadcast(uint8_t* p, size_t bytes, uint32_t root, hipStream_t st) = 0;
};
// the RCCL transport of `rank` in the communicator `id` names (rp_comm_unique_id)
std::unique_ptr<Xport> nccl_xport(int nranks, int rank, const uint8_t* id);
// the loopback transport of `rank` in `group`, and the group's size
std::unique_ptr<Xport> loop_xport(rp_loop* group, int rank);
uint32_t loop_ranks(const rp_loop* group);

// launches of rp_sim.hip's copy and add kernels, for exchanges done on one device
// (every segment copy of a collective in launches of COPY_BATCH; dst[i] += src[i])
void copy_batches(const std::vector<CopyDesc>& segs, hipStream_t st);
void add_u32(uint32_t* dst, const uint32_t* src, size_t count, hipStream_t st);

}  // namespace rp

// A simulated cluster: G shards of N/G nodes each.  Either all shards live in
// this process on one device (exchanges are device copies; used by the tests
// and for single-GPU runs, G = 1), or this process holds one shard of a
// G-process cluster and exchanges over RCCL (one process per GPU).
struct rp_sim {
    rp_sim_config cfg{};
    uint32_t n = 0, k = 0, G = 1;
    int dev = 0;  // the HIP device it lives on (entry points may come from any host thread)
    std::vector<std::unique_ptr<rp::Shard>> sh;  // local shards (all G, or one)
    std::unique_ptr<rp::Xport> comm;         // RCCL (or loopback): this process holds shard `rank` only
    uint32_t rank = 0;
    hipStream_t st = nullptr;                // shared by in-process shards
    std::vector<int32_t> fail_round;         // per node: round of its fail-stop, -1 none
    struct JoinEv { uint32_t round, joiner; std::vector<int32_t> seeds; };
    std::vector<JoinEv> joins;               // rp_sim_join's schedule, in order
    std::vector<int32_t> join_round;         // per node: round it joins at, -1 = a member from the start
    // rp_sim_leave / rp_sim_rejoin: per node the rounds of its events, strictly
    // increasing, leave (even index) and rejoin (odd) in turn; by round, the
    // events (node, bit 31: a rejoin) in call order
    std::vector<std::vector<uint32_t>> life;
    std::map<uint32_t, std::vector<uint32_t>> life_at;
    // the node's gossip runs during round r: a function of the schedule, like
    // live_at (an event before the node's join is skipped)
    bool gossiping_at(uint32_t i, uint32_t r) const {
        if (life.empty()) return true;
        bool on = true;
        const std::vector<uint32_t>& e = life[i];
        for (size_t j = 0; j < e.size() && e[j] <= r; j++)
            if (join_round[i] < 0 || e[j] >= (uint32_t)join_round[i]) on = (j & 1) != 0;
        return on;
    }
    // neither failed nor still outside the cluster at round r, and gossiping:
    // the nodes churn and storms draw from
    bool live_at(uint32_t i, uint32_t r) const {
        return (fail_round[i] < 0 || (uint32_t)fail_round[i] > r) && (join_round[i] < 0 || (uint32_t)join_round[i] <= r) &&
               gossiping_at(i, r);
    }
    void schedule_life(uint32_t node, uint32_t r, bool rejoin);
    void join_step(uint32_t r, uint64_t now);
    void life_step(uint32_t r, uint64_t now);
    bool faults = false;
    bool views_set = false;                  // rp_sim_set_views ran (rp_sim_load_addresses must come first)
    uint32_t part[3] = {0, 0, 0};
    uint64_t churn_rng = 0;
    uint32_t round = 0;
    int32_t* h_churn = nullptr;              // pinned staging for churn ids
    // false-suspicion storm: rounds [start, end), ceil(live * ppm / 1e6) victims per round
    uint32_t storm_start = 0, storm_end = 0, storm_ppm = 0, storm_kmax = 0;
    uint64_t storm_rng = 0;
    int32_t* h_storm = nullptr;              // pinned staging: CHURN_SLOTS x 2 x storm_kmax
    std::vector<uint32_t> storm_k;           // pairs per staged round
    uint64_t xbytes = 0, xcalls = 0;         // bytes this process sent in exchanges
    // request routing (rp_sim_ring_checksums / rp_sim_route): the shards'
    // ring_csum buffers are recomputed when an entry point that can change a
    // ring ran since (host flag only: the round kernels know nothing of it);
    // the per-shard pointer table and the bucket directory over the point
    // hashes are built on first use and dropped with the shards
    // (rp_sim_load_addresses)
    bool ring_csum_stale = true;
    // an entry point that can change a ring ran: both caches (this one and
    // the census') are stale
    void rings_changed() {
        ring_csum_stale = true;
        own_stale = true;
    }
    rp::DevBuf<rp::RouteShard> route_tab;
    rp::DevBuf<uint32_t> route_dir;
    uint32_t route_dir_shift = 32;
    void refresh_ring_checksums();
    void route_prepare(bool checksums = true);
    // ownership census (rp_sim_ownership / rp_sim_ownership_at; DESIGN.md
    // §13): the same cache rule with a flag of its own -- the counts per
    // interval, per node and the stats stay until an entry point that can
    // change a ring ran.  The server -> point index and the shards' dead
    // arrays are built on first use and dropped with the shards.
    bool own_stale = true;
    rp::DevBuf<uint32_t> own_srv_pt, own_claims;
    rp::DevBuf<int32_t> own_diff, own_tile;
    rp::DevBuf<unsigned long long> own_claimed, own_out;
    rp::DevBuf<const uint8_t*> own_dead;
    rp_ownership_stats own_stats{};
    rp::OwnArgs own_args();
    void own_prepare();
    void own_refresh(bool record = false);
    // ownership movement (rp_ownership_snapshot_* / rp_sim_ownership_moved;
    // DESIGN.md §15).  A census run for a snapshot or a comparison also
    // records every node's arcs (own_arcs_valid: they are the cached census');
    // the plain census never does.  own_id names this simulation in its
    // snapshots (given at the first one); own_gen counts the builds of the
    // server -> point index, so that a snapshot of other points is refused.
    bool own_arcs_valid = false;
    uint64_t own_id = 0, own_gen = 0;
    rp::DevBuf<uint32_t> own_arc_n;  // n: arcs recorded, or OWN_ARC_ALL
    rp::DevBuf<uint2> own_arcs;      // n x REPLICAS: (q, p) by ascending p
    rp::DevBuf<int32_t> mv_diff, mv_tile;
    rp::DevBuf<unsigned long long> mv_gained, mv_lost, mv_out;
    template <bool UNIFORM>
    void route_launch(const uint32_t* entries, const uint32_t* keys, uint64_t seed, uint64_t count, int32_t* dests,
                      uint8_t* outcomes, uint8_t* agrees, rp_route_stats* stats);

    // f(shard) for every shard this process holds, in shard order.  (One host
    // thread per in-process shard was measured: no faster, and it varied
    // more -- 39.6-75 against 39.1-39.3 ms/round at 65,536 nodes on 4 shards.)
    template <class F>
    void each(F&& f) {
        for (auto& s : sh) f(*s);
    }

    ~rp_sim() {
        sh.clear();
        if (xdone) (void)hipEventDestroy(xdone);
        comm.reset();
        if (h_churn) (void)hipHostFree(h_churn);
        if (h_storm) (void)hipHostFree(h_storm);
        if (st) (void)hipStreamDestroy(st);
    }
    rp::Shard& owner_of(uint32_t node) {
        for (auto& s : sh)
            if (node - s->lo < s->nl) return *s;
        throw rp::Error(RP_ERR_INVALID, "node " + std::to_string(node) + " is not held by this process");
    }
    void choose_churn(int32_t* out, uint32_t r);
    uint32_t choose_storm(int32_t* out, uint32_t r);
    void enqueue_round(bool churn_active, uint32_t slot);
    void run(int k_rounds, bool churn_active);
    void check_errors();
    // exchanges
    template <class T>
    void allgather_nodes(rp::DevBuf<T> rp::Shard::*buf, size_t per_node);
    template <class T>
    void allgather_block(rp::DevBuf<T> rp::Shard::*buf, size_t per_shard);
    void allreduce_sum(rp::DevBuf<uint32_t> rp::Shard::*buf, size_t count);
    void alltoallv(rp::DevBuf<rp::Change> rp::Shard::*sendb, rp::DevBuf<rp::Change> rp::Shard::*recvb, int cat_send,
                   int cat_recv, size_t elem);
    template <class T>
    void alltoallv_t(rp::DevBuf<T> rp::Shard::*sendb, rp::DevBuf<T> rp::Shard::*recvb, int cat_send, int cat_recv);
    void read_counts();
    void origin_exchange();
    template <int W>
    void slot_exchange();
    void sync_all() { for (auto& s : sh) RP_HIP(hipStreamSynchronize(s->st)); }
    bool presized = false;
    bool loop_rank = false;  // a loopback rank: its G - 1 peers share this device
    void presize_exchange();
    // In-process clusters run each shard on a stream of its own, so that the
    // shards' kernels overlap as one-GPU-per-shard ranks would; an exchange
    // step (device copies on the cluster stream st) starts after every
    // shard's earlier work (xbegin) and every shard's later work waits for it
    // (xend).  One shard per process (RCCL): the shard's stream orders both.
    hipEvent_t xdone = nullptr;
    // segment copies of the current in-process exchange (k_copy_batch at xend)
    std::vector<rp::CopyDesc> cbatch;
    void copy(void* dst, const void* src, size_t bytes) {
        if (bytes) cbatch.push_back(rp::CopyDesc{src, dst, (uint64_t)bytes});
    }
    void copy_flush() {
        rp::copy_batches(cbatch, st);
        cbatch.clear();
    }
    bool overlap() const { return !comm && sh.size() > 1 && sh.front()->st != st; }
    // (nested scopes: consecutive collectives with no shard work between
    // them share one ordering step and one copy launch)
    int xdepth = 0;
    void xbegin() {
        if (xdepth++ > 0 || !overlap()) return;
        for (auto& s : sh) {
            RP_HIP(hipEventRecord(s->xev, s->st));
            RP_HIP(hipStreamWaitEvent(st, s->xev, 0));
        }
    }
    void xend() {
        if (--xdepth > 0) return;
        copy_flush();
        if (!overlap()) return;
        RP_HIP(hipEventRecord(xdone, st));
        for (auto& s : sh) RP_HIP(hipStreamWaitEvent(s->st, xdone, 0));
    }
};
