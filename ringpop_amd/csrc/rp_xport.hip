// ringpop_amd — rank transports (rp::Xport, rp_cluster.h).  A process that
// holds one shard of a G-rank cluster exchanges with the other ranks through
// a transport: RCCL (one process per GPU, rp_sim_create_rank), or a loopback
// among the host threads of one process on one device
// (rp_sim_create_rank_loop): the same rank code -- plans, counts, offsets,
// buffer sizes -- with the collectives done as device copies, so that the
// rank path runs and is compared with the in-process shards where one GPU is
// all there is.  Also the RCCL self-test and the rp_loop group's C ABI.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>

#include "rp_cluster.h"

using rp::DevBuf;
using rp::Error;

#define RP_NCCL(expr)                                                                               \
    do {                                                                                            \
        ncclResult_t r_ = (expr);                                                                   \
        if (r_ != ncclSuccess) throw Error(RP_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

namespace rp {
struct NcclXport : Xport {
    ncclComm_t comm = nullptr;
    ~NcclXport() override { if (comm) (void)ncclCommDestroy(comm); }
    void allgather(uint8_t* base, size_t bytes, uint32_t rank, hipStream_t st) override {
        RP_NCCL(ncclAllGather(base + (size_t)rank * bytes, base, bytes, ncclUint8, comm, st));
    }
    void allreduce_u32(uint32_t* buf, size_t count, hipStream_t st) override {
        RP_NCCL(ncclAllReduce(buf, buf, count, ncclUint32, ncclSum, comm, st));
    }
    void sendrecv(const std::vector<Xfer>& sends, const std::vector<Xfer>& recvs, hipStream_t st) override {
        RP_NCCL(ncclGroupStart());
        for (const Xfer& x : sends) RP_NCCL(ncclSend(x.ptr, x.bytes, ncclUint8, (int)x.peer, comm, st));
        for (const Xfer& x : recvs) RP_NCCL(ncclRecv(x.ptr, x.bytes, ncclUint8, (int)x.peer, comm, st));
        RP_NCCL(ncclGroupEnd());
    }
    void broadcast(uint8_t* p, size_t bytes, uint32_t root, hipStream_t st) override {
        RP_NCCL(ncclBroadcast(p, p, bytes, ncclUint8, (int)root, comm, st));
    }
};

// The loopback group: every collective is a rendezvous of all G rank threads.
// Each rank posts its transfers and records an event after its earlier work;
// the last rank to arrive leads: on the group's own stream it waits for every
// rank's event, moves all G x (G - 1) segments with batched copy launches
// (k_copy_batch, as the in-process exchanges do) and records one done event,
// then releases the others; every rank's stream waits on that one event.  Per
// collective that is 2 API calls per rank plus G + 2 for the leader, where a
// copy and two waits per segment (~180 calls at G = 8, with eight threads
// contending for the runtime) left the GPU idle a third of each round.
struct LoopGroup {
    uint32_t G;
    std::mutex m;
    std::condition_variable cv;
    uint32_t arrived = 0;
    uint64_t gen = 0;
    bool broken = false;  // a rank threw: the others stop waiting
    struct Post {
        std::vector<Xfer> sends, recvs;
        hipEvent_t ready = nullptr;
    };
    std::vector<Post> post;
    hipStream_t xs = nullptr;    // the leader's copies (created by the first leader)
    hipEvent_t done = nullptr;   // recorded on xs after each collective's copies
    explicit LoopGroup(uint32_t g) : G(g), post(g) {}
    ~LoopGroup() {
        if (xs) (void)hipStreamSynchronize(xs);
        if (done) (void)hipEventDestroy(done);
        if (xs) (void)hipStreamDestroy(xs);
    }
    // true for the last rank to arrive, which then leads and calls release()
    bool arrive() {
        std::unique_lock<std::mutex> l(m);
        if (broken) throw Error(RP_ERR_STATE, "loopback cluster: another rank failed");
        const uint64_t g0 = gen;
        if (++arrived == G) {
            arrived = 0;
            return true;
        }
        if (!cv.wait_for(l, std::chrono::seconds(120), [&] { return gen != g0 || broken; }) || broken) {
            broken = true;
            cv.notify_all();
            throw Error(RP_ERR_STATE, "loopback cluster: a rank did not reach the collective");
        }
        return false;
    }
    void release() {
        std::lock_guard<std::mutex> l(m);
        gen++;
        cv.notify_all();
    }
    void fail() {
        std::lock_guard<std::mutex> l(m);
        broken = true;
        cv.notify_all();
    }
    // (the leader, all posts in) every receive matched to its send, the
    // segments copied on xs once every rank's earlier work is done
    void lead() {
        if (!xs) {
            RP_HIP(hipStreamCreateWithFlags(&xs, hipStreamNonBlocking));
            RP_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        }
        for (const Post& p : post) RP_HIP(hipStreamWaitEvent(xs, p.ready, 0));
        std::vector<CopyDesc> segs;
        size_t nsend = 0, nrecv = 0;
        for (const Post& p : post) nsend += p.sends.size();
        for (uint32_t r = 0; r < G; r++) {
            for (const Xfer& x : post[r].recvs) {
                const Xfer* src = nullptr;
                for (const Xfer& y : post[x.peer].sends)
                    if (y.peer == r) { src = &y; break; }
                if (!src || src->bytes != x.bytes)
                    throw Error(RP_ERR_STATE, "loopback cluster: a receive has no matching send");
                nrecv++;
                if (!x.bytes) continue;
                segs.push_back(CopyDesc{src->ptr, x.ptr, (uint64_t)x.bytes});
            }
        }
        if (nrecv != nsend) throw Error(RP_ERR_STATE, "loopback cluster: a send has no matching receive");
        copy_batches(segs, xs);
        RP_HIP(hipGetLastError());
        RP_HIP(hipEventRecord(done, xs));
    }
};

struct LoopXport : Xport {
    LoopGroup* g;
    uint32_t rank;
    hipEvent_t ready = nullptr;
    DevBuf<uint32_t> stage, tmp;  // all-reduce: this rank's input, then every other rank's
    LoopXport(LoopGroup* grp, uint32_t r) : g(grp), rank(r) {
        RP_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    }
    ~LoopXport() override {
        if (ready) (void)hipEventDestroy(ready);
    }
    void exchange(const std::vector<Xfer>& sends, const std::vector<Xfer>& recvs, hipStream_t st) {
        try {
            RP_HIP(hipEventRecord(ready, st));
            g->post[rank].sends = sends;
            g->post[rank].recvs = recvs;
            g->post[rank].ready = ready;
            if (g->arrive()) {
                try {
                    g->lead();
                } catch (...) {
                    g->fail();
                    throw;
                }
                g->release();
            }
            // (the posts are read by the leader before its release: this
            // rank may post again once it is past here)
            RP_HIP(hipStreamWaitEvent(st, g->done, 0));
        } catch (...) {
            g->fail();
            throw;
        }
    }
    void allgather(uint8_t* base, size_t bytes, uint32_t r, hipStream_t st) override {
        std::vector<Xfer> sends, recvs;
        for (uint32_t q = 0; q < g->G; q++)
            if (q != r) {
                sends.push_back(Xfer{q, base + (size_t)r * bytes, bytes});
                recvs.push_back(Xfer{q, base + (size_t)q * bytes, bytes});
            }
        exchange(sends, recvs, st);
    }
    void allreduce_u32(uint32_t* buf, size_t count, hipStream_t st) override {
        stage.reserve(count);
        tmp.reserve(count * g->G);
        RP_HIP(hipMemcpyAsync(stage.p, buf, count * 4, hipMemcpyDeviceToDevice, st));
        std::vector<Xfer> sends, recvs;
        for (uint32_t q = 0; q < g->G; q++)
            if (q != rank) {
                sends.push_back(Xfer{q, stage.p, count * 4});
                recvs.push_back(Xfer{q, tmp.p + (size_t)q * count, count * 4});
            }
        exchange(sends, recvs, st);
        for (uint32_t q = 0; q < g->G; q++)
            if (q != rank)
                add_u32(buf, tmp.p + (size_t)q * count, count, st);
    }
    void sendrecv(const std::vector<Xfer>& sends, const std::vector<Xfer>& recvs, hipStream_t st) override {
        exchange(sends, recvs, st);
    }
    void broadcast(uint8_t* p, size_t bytes, uint32_t root, hipStream_t st) override {
        std::vector<Xfer> sends, recvs;
        if (rank == root) {
            for (uint32_t q = 0; q < g->G; q++)
                if (q != root) sends.push_back(Xfer{q, p, bytes});
        } else {
            recvs.push_back(Xfer{root, p, bytes});
        }
        exchange(sends, recvs, st);
    }
};
}  // namespace rp

struct rp_loop {
    rp::LoopGroup grp;
    explicit rp_loop(uint32_t g) : grp(g) {}
};

namespace rp {
std::unique_ptr<Xport> nccl_xport(int nranks, int rank, const uint8_t* id) {
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    std::unique_ptr<NcclXport> x(new NcclXport());
    RP_NCCL(ncclCommInitRank(&x->comm, nranks, u, rank));
    return x;
}
std::unique_ptr<Xport> loop_xport(rp_loop* group, int rank) {
    return std::unique_ptr<Xport>(new LoopXport(&group->grp, (uint32_t)rank));
}
uint32_t loop_ranks(const rp_loop* group) { return group->grp.G; }
}  // namespace rp

extern "C" {

int rp_comm_unique_id(uint8_t* id, size_t cap) {
    return rp::guarded([&] {
        if (!id || cap < sizeof(ncclUniqueId)) throw Error(RP_ERR_INVALID, "id buffer must hold 128 bytes");
        ncclUniqueId u;
        RP_NCCL(ncclGetUniqueId(&u));
        memcpy(id, &u, sizeof u);
    });
}

// The RCCL transport on its own (rp::NcclXport, the four calls the rank path
// makes), on small buffers whose contents every rank can predict: rank r's
// all-gather chunk, all-reduce input and sends are functions of (r, peer, i).
// nranks = 1 runs every call on one GPU (the sends and receives go to the
// rank itself), so the library's RCCL linkage, communicator set-up and call
// arguments are exercised where only one GPU is available.
static uint32_t selftest_word(uint32_t from, uint32_t to, uint32_t i) {
    return 0x9E3779B1u * (from + 1) ^ 0x85EBCA6Bu * (to + 7) ^ (i * 2654435761u);
}
int rp_comm_selftest(int nranks, int rank, const uint8_t* id, uint32_t words, uint32_t* failures) {
    return rp::guarded([&] {
        if (!id || !failures || nranks < 1 || rank < 0 || rank >= nranks || words == 0 || words > (1u << 24))
            throw Error(RP_ERR_INVALID, "bad argument");
        RP_HIP(hipSetDevice(rp::current_device()));
        rp::NcclXport x;
        ncclUniqueId u;
        memcpy(&u, id, sizeof u);
        RP_NCCL(ncclCommInitRank(&x.comm, nranks, u, rank));
        const uint32_t G = (uint32_t)nranks, r = (uint32_t)rank, W = words;
        struct StreamGuard {  // (destroyed on every exit, a throw included)
            hipStream_t s = nullptr;
            ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
        } sg;
        RP_HIP(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
        const hipStream_t st = sg.s;
        DevBuf<uint32_t> ag, ar, sb, rb;
        ag.alloc((size_t)G * W); ar.alloc(W); sb.alloc((size_t)G * W); rb.alloc((size_t)G * W);
        std::vector<uint32_t> h((size_t)G * W, 0u);
        // all-gather in place: this rank's chunk at base + r * bytes
        for (uint32_t i = 0; i < W; i++) h[(size_t)r * W + i] = selftest_word(r, rp::NONE, i);
        RP_HIP(hipMemcpyAsync(ag.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
        x.allgather((uint8_t*)ag.p, (size_t)W * 4, r, st);
        // all-reduce (sum) of u32
        std::vector<uint32_t> a(W);
        for (uint32_t i = 0; i < W; i++) a[i] = selftest_word(r, 0, i) & 0xFFFFu;
        RP_HIP(hipMemcpyAsync(ar.p, a.data(), (size_t)W * 4, hipMemcpyHostToDevice, st));
        x.allreduce_u32(ar.p, W, st);
        // one grouped send/recv with every rank (itself included), a
        // different length per pair as the exchanges have
        std::vector<uint32_t> sbh((size_t)G * W);
        std::vector<rp::Xfer> sends, recvs;
        for (uint32_t q = 0; q < G; q++) {
            const uint32_t len_s = W - (r + 2 * q) % W, len_r = W - (q + 2 * r) % W;
            for (uint32_t i = 0; i < W; i++) sbh[(size_t)q * W + i] = selftest_word(r, q, i);
            sends.push_back(rp::Xfer{q, sb.p + (size_t)q * W, (size_t)len_s * 4});
            recvs.push_back(rp::Xfer{q, rb.p + (size_t)q * W, (size_t)len_r * 4});
        }
        RP_HIP(hipMemcpyAsync(sb.p, sbh.data(), sbh.size() * 4, hipMemcpyHostToDevice, st));
        RP_HIP(hipMemsetAsync(rb.p, 0, (size_t)G * W * 4, st));
        x.sendrecv(sends, recvs, st);
        std::vector<uint32_t> hag((size_t)G * W), har(W), hrb((size_t)G * W), hbc(W);
        RP_HIP(hipMemcpyAsync(hag.data(), ag.p, hag.size() * 4, hipMemcpyDeviceToHost, st));
        RP_HIP(hipMemcpyAsync(har.data(), ar.p, har.size() * 4, hipMemcpyDeviceToHost, st));
        RP_HIP(hipMemcpyAsync(hrb.data(), rb.p, hrb.size() * 4, hipMemcpyDeviceToHost, st));
        // broadcast from the last rank (reuses ar on the device; the payload
        // has a host vector of its own, so the pageable all-reduce input
        // copied above is never rewritten while that copy may be pending)
        const uint32_t root = G - 1;
        std::vector<uint32_t> bc(W, 0u);
        if (r == root)
            for (uint32_t i = 0; i < W; i++) bc[i] = selftest_word(root, root, i);
        RP_HIP(hipMemcpyAsync(ar.p, bc.data(), (size_t)W * 4, hipMemcpyHostToDevice, st));
        x.broadcast((uint8_t*)ar.p, (size_t)W * 4, root, st);
        RP_HIP(hipMemcpyAsync(hbc.data(), ar.p, hbc.size() * 4, hipMemcpyDeviceToHost, st));
        RP_HIP(hipStreamSynchronize(st));
        uint32_t bad = 0;
        for (uint32_t q = 0; q < G; q++)
            for (uint32_t i = 0; i < W; i++) {
                bad += hag[(size_t)q * W + i] != selftest_word(q, rp::NONE, i);
                const uint32_t len_r = W - (q + 2 * r) % W;
                bad += hrb[(size_t)q * W + i] != (i < len_r ? selftest_word(q, r, i) : 0u);
            }
        for (uint32_t i = 0; i < W; i++) {
            uint32_t want = 0;
            for (uint32_t q = 0; q < G; q++) want += selftest_word(q, 0, i) & 0xFFFFu;
            bad += har[i] != want;
            bad += hbc[i] != selftest_word(root, root, i);
        }
        *failures = bad;
    });
}

int rp_loop_create(int nranks, rp_loop** out) {
    return rp::guarded([&] {
        if (!out || nranks < 2 || nranks > (int)rp::MAXG) throw Error(RP_ERR_INVALID, "nranks must be in [2, 64]");
        *out = new rp_loop((uint32_t)nranks);
    });
}
int rp_loop_destroy(rp_loop* g) {
    delete g;
    return RP_OK;
}

}  // extern "C"
