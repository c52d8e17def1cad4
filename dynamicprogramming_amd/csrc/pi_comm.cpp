// pi_comm.cpp — the multi-GPU half of libpi_mi355.so: transports, the exchange plan and the
// sharded sweep driver (SURVEY.md section 8e / 8b "must export": pi_comm_init, pi_allgather_V,
// pi_allreduce_*).  The reference has no counterpart: src/cuda_policy_iteration.py:300-336 is a
// single-device loop.
//
// Partition: contiguous flat-index shards of `per` = ceil(n / world) states (slabs along
// dimension 0); every rank keeps a full-size V, sweeps its shard and then makes the new values
// visible where other ranks will read them, either
//   * halo exchange — exactly the dimension-0 plane runs each peer can reach (measured once for
//     ALL actions with pi_reach_planes_kernel), as grouped ncclSend/ncclRecv in place in V', the
//     planes peers wait for swept first and sent on a second HIP stream while the interior is
//     swept; or
//   * all-gather of the shards (ncclAllGather, in place) when the reachable bands cover most
//     of the grid anyway.
// Two transports implement the same small interface: RCCL (one process per GPU, xGMI), and an
// in-process one (several handles of ONE process, one host thread each, device-to-device copies
// ordered by HIP events) that exists so the stream ordering of the overlapped exchange can be
// tested with real kernels on a single GPU.

#include "pi_internal.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <numeric>

using pi::fail;

namespace pi {

struct ShardPlan {
    int64_t per = 0, s_begin = 0, s_end = 0;
    bool halo = false;
    int depth = 1;                                           // granularity of the reach probe
    struct Seg { int src, dst; int64_t a, b; };
    std::vector<Seg> segs;                                   // only those that involve this rank
    std::vector<std::pair<int64_t, int64_t>> send_ranges, interior;
    int64_t recv_elems = 0, send_elems = 0;
    bool broken = false;            // a sharded sweep failed half-way: streams were drained; new communicator + plan needed
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
    // What an overlapped halo plan sweeps first, beyond the coarse ranges above (every such plan has those).  The Push
    // kinds belong to the fused exchange of transports that can_push(): entry k of what is swept first goes to the peers
    // named by the bits of its destination mask — bit j = push_peers[j] — stored by pi_eval_push_kernel itself.
    enum class SweptFirst {
        Ranges,         // nothing more; the exchange on the second stream
        Lists,          // no terminal states: d_first / d_inner split the shard (plan_row_lists)
        PushLists,      // the same with d_first_dest: fused, every sweep (plan_state_lists, plan_row_lists)
        // terminal states (plan_live_masks): fused from a batch's second sweep on, while the handle's live-state list is live_list
        PushLiveLists,  // d_first / d_inner / d_first_dest split the shard's LIVE states
        PushLiveSpans,  // d_live_dest: one byte per entry of the shard's live span, for the live spans of send_ranges
    };
    SweptFirst swept_first = SweptFirst::Ranges;
    bool row_lists() const { return swept_first == SweptFirst::Lists || swept_first == SweptFirst::PushLists; }
    bool live_push() const { return swept_first == SweptFirst::PushLiveLists || swept_first == SweptFirst::PushLiveSpans; }
    bool fused() const { return swept_first == SweptFirst::PushLists || live_push(); }
    bool has_lists() const { return row_lists() || swept_first == SweptFirst::PushLiveLists; }
    bool overlapped() const { return halo && comm_stream != nullptr; }
    std::vector<std::pair<int64_t, int64_t>> first_exact, inner_exact;      // row-exact lists as ranges, for pi_plan_ranges
    int32_t *d_first = nullptr, *d_inner = nullptr;
    int64_t n_first = 0, n_inner = 0;
    std::vector<int> push_peers, push_senders;
    uint8_t *d_first_dest = nullptr, *d_live_dest = nullptr;
    const int32_t* live_list = nullptr;
    int64_t live_list_count = 0, live_dest_base = 0;
    bool pair_exact = false;            // destination masks cut down to the pairs (i_0, i_v) each peer reads
    int64_t fused_send_elems = -1;      // (state, receiver) pairs one fused sweep delivers; -1: not counted for this plan
    ~ShardPlan() {
        if (d_live_dest) (void)hipFree(d_live_dest);
        if (d_first_dest) (void)hipFree(d_first_dest);
        if (d_first) (void)hipFree(d_first);
        if (d_inner) (void)hipFree(d_inner);
        if (ev_ready) (void)hipEventDestroy(ev_ready);
        if (ev_done) (void)hipEventDestroy(ev_done);
        if (comm_stream) (void)hipStreamDestroy(comm_stream);
    }
};

void drop_plan(pi_handle* h) {
    delete h->plan;
    h->plan = nullptr;
}
void release_comm(pi_handle* h) {
    drop_plan(h);
    delete h->comm;
    h->comm = nullptr;
    drop_p2p_pending(h);
}

}  // namespace pi

namespace {

#define PI_NCCL(expr)                                                                      \
    do {                                                                                   \
        ncclResult_t r_ = (expr);                                                          \
        if (r_ != ncclSuccess)                                                             \
            return fail(std::string(#expr) + ": " + ncclGetErrorString(r_));               \
    } while (0)

using pi::Knob;

// ---- RCCL ------------------------------------------------------------------------------
// Failure handling ("RCCL error -> abort with message"): every RCCL call goes
// through check(); on the first error an open group is closed (a group left open would swallow
// every later call of the thread), the communicator is aborted (ncclCommAbort frees the peers'
// resources and unblocks kernels that wait for this rank) and the handle refuses further
// collectives with the recorded message.  After every group / collective the communicator's
// asynchronous error state is polled once (ncclCommGetAsyncError): a peer that died shows up there.
struct RcclComm : pi::Comm {
    ncclComm_t comm = nullptr;
    bool in_group = false;
    std::string dead;                       // non-empty once the communicator has been aborted
    ~RcclComm() override {
        if (comm) (void)ncclCommDestroy(comm);
    }
    int transport() const override { return PI_TRANSPORT_RCCL; }
    int abort_with(const std::string& why) {
        if (in_group) { (void)ncclGroupEnd(); in_group = false; }
        if (comm) { (void)ncclCommAbort(comm); comm = nullptr; }
        dead = "RCCL communicator aborted (rank " + std::to_string(rank) + " of " + std::to_string(world) + "): " + why;
        return fail(dead);
    }
    int check(ncclResult_t r, const char* what) {
        if (r == ncclSuccess) return 0;
        return abort_with(std::string(what) + ": " + ncclGetErrorString(r));
    }
    int alive() { return dead.empty() && comm ? 0 : fail(dead.empty() ? "no RCCL communicator" : dead); }
    int poll_async() {
        ncclResult_t st = ncclSuccess;
        if (check(ncclCommGetAsyncError(comm, &st), "ncclCommGetAsyncError")) return 1;
        if (st != ncclSuccess && st != ncclInProgress)
            return abort_with(std::string("asynchronous error: ") + ncclGetErrorString(st));
        return 0;
    }
    int group_begin() override {
        if (alive()) return 1;
        if (check(ncclGroupStart(), "ncclGroupStart")) return 1;
        in_group = true;
        return 0;
    }
    int send(const void* p, size_t bytes, int peer, hipStream_t st) override {
        if (alive()) return 1;
        return check(ncclSend(p, bytes, ncclChar, peer, comm, st), "ncclSend");
    }
    int recv(void* p, size_t bytes, int peer, hipStream_t st) override {
        if (alive()) return 1;
        return check(ncclRecv(p, bytes, ncclChar, peer, comm, st), "ncclRecv");
    }
    int group_end(hipStream_t) override {
        if (alive()) return 1;
        in_group = false;
        if (check(ncclGroupEnd(), "ncclGroupEnd")) return 1;
        return poll_async();
    }
    int allgather(void* full, size_t bytes, hipStream_t st) override {
        if (alive()) return 1;
        if (check(ncclAllGather(static_cast<const char*>(full) + (size_t)rank * bytes, full, bytes, ncclChar,
                                comm, st), "ncclAllGather")) return 1;
        return poll_async();
    }
    int allreduce_scalar(void* d, ncclDataType_t type, ncclRedOp_t op, const char* what, hipStream_t st) {
        if (alive()) return 1;
        if (check(ncclAllReduce(d, d, 1, type, op, comm, st), what)) return 1;
        return poll_async();
    }
    int allreduce_max_f32(float* d, hipStream_t st) override { return allreduce_scalar(d, ncclFloat, ncclMax, "ncclAllReduce(max)", st); }
    int allreduce_sum_u32(uint32_t* d, hipStream_t st) override { return allreduce_scalar(d, ncclUint32, ncclSum, "ncclAllReduce(sum)", st); }
};

// ---- in-process transport (test transport: N handles, N host threads, one process) -------
// send(): records an event on the sender's stream and posts {pointer, bytes, event} in the
// mailbox of the (src, dst) pair.  recv() (deferred to group_end): waits on the host for the
// posting, makes the receiver's stream wait for the sender's event, enqueues the device copy and
// records a completion event.  group_end() finally makes the SENDER's stream wait for those
// completion events, so a later kernel cannot overwrite a buffer that is still being copied —
// the same stream semantics an RCCL send has.
struct LocalGroup {
    std::mutex mu;
    std::condition_variable cv;
    int world = 0, joined = 0, left = 0;
    bool failed = false;                                     // a member gave up: nobody waits any longer
    struct Msg {
        const void* src = nullptr;
        size_t bytes = 0;
        hipEvent_t ready = nullptr, done = nullptr;
        bool copied = false;
    };
    std::vector<std::deque<std::shared_ptr<Msg>>> box;        // [src * world + dst]
    // host-side scalar reductions
    std::vector<double> red;
    int red_arrived = 0, red_epoch = 0;
    double red_result = 0.0;
};
std::mutex g_groups_mu;
std::map<std::string, std::shared_ptr<LocalGroup>> g_groups;

struct LocalComm : pi::Comm {
    std::shared_ptr<LocalGroup> grp;
    std::string name;
    struct PendingRecv { void* p; size_t bytes; int peer; hipStream_t st; };
    std::vector<PendingRecv> recvs;
    std::vector<std::shared_ptr<LocalGroup::Msg>> sent, retired;
    void drop_retired() {
        for (auto& m : retired) {
            (void)hipEventDestroy(m->ready);
            (void)hipEventDestroy(m->done);
        }
        retired.clear();
    }
    ~LocalComm() override {
        (void)hipDeviceSynchronize();
        drop_retired();
        std::lock_guard<std::mutex> lk(g_groups_mu);
        if (grp && ++grp->left == grp->world) g_groups.erase(name);
    }
    int transport() const override { return PI_TRANSPORT_IN_PROCESS; }
    // Every host wait of this transport is bounded: a peer that failed (or never arrives) turns into
    // an error on all members after PI_MI355_COMM_TIMEOUT seconds instead of a hang.
    template <typename Pred>
    int wait_for(std::unique_lock<std::mutex>& lk, Pred ready, const char* what) {
        const auto limit = std::chrono::duration<double>(pi::knob_seconds(Knob::COMM_TIMEOUT));
        if (!grp->cv.wait_for(lk, limit, [&] { return grp->failed || ready(); }) || grp->failed) {
            grp->failed = true;
            grp->cv.notify_all();
            return fail(std::string("local transport: rank ") + std::to_string(rank) + " gave up waiting for " + what);
        }
        return 0;
    }
    void give_up() override {
        std::lock_guard<std::mutex> lk(grp->mu);
        grp->failed = true;
        grp->cv.notify_all();
    }
    int group_begin() override { return 0; }
    int send(const void* p, size_t bytes, int peer, hipStream_t st) override {
        auto m = std::make_shared<LocalGroup::Msg>();
        m->src = p;
        m->bytes = bytes;
        PI_HIP(hipEventCreateWithFlags(&m->ready, hipEventDisableTiming));
        PI_HIP(hipEventCreateWithFlags(&m->done, hipEventDisableTiming));
        PI_HIP(hipEventRecord(m->ready, st));
        {
            std::lock_guard<std::mutex> lk(grp->mu);
            grp->box[(size_t)rank * world + peer].push_back(m);
        }
        grp->cv.notify_all();
        sent.push_back(m);
        return 0;
    }
    int recv(void* p, size_t bytes, int peer, hipStream_t st) override {
        recvs.push_back({p, bytes, peer, st});
        return 0;
    }
    int group_end(hipStream_t st) override {
        for (const PendingRecv& r : recvs) {
            std::shared_ptr<LocalGroup::Msg> m;
            {
                std::unique_lock<std::mutex> lk(grp->mu);
                auto& q = grp->box[(size_t)r.peer * world + rank];
                if (wait_for(lk, [&] { return !q.empty(); }, "a send of its peer")) { recvs.clear(); return 1; }
                m = q.front();
                q.pop_front();
            }
            if (m->bytes != r.bytes) {
                give_up();
                recvs.clear();
                return fail("local transport: send/recv size mismatch");
            }
            PI_HIP(hipStreamWaitEvent(r.st, m->ready, 0));
            PI_HIP(hipMemcpyAsync(r.p, m->src, r.bytes, hipMemcpyDeviceToDevice, r.st));
            PI_HIP(hipEventRecord(m->done, r.st));
            {
                std::lock_guard<std::mutex> lk(grp->mu);
                m->copied = true;
            }
            grp->cv.notify_all();
        }
        recvs.clear();
        for (auto& m : sent) {
            {
                std::unique_lock<std::mutex> lk(grp->mu);
                if (wait_for(lk, [&] { return m->copied; }, "its peer to receive")) return 1;
            }
            PI_HIP(hipStreamWaitEvent(st, m->done, 0));
        }
        // both streams have enqueued their waits; the events are destroyed in batches, after a
        // synchronisation, so none is released while a stream still refers to it
        for (auto& m : sent) retired.push_back(m);
        sent.clear();
        if (retired.size() >= 512) {
            PI_HIP(hipDeviceSynchronize());
            drop_retired();
        }
        return 0;
    }
    int allgather(void* full, size_t bytes, hipStream_t st) override {
        for (int p = 0; p < world; ++p)
            if (p != rank && send(static_cast<const char*>(full) + (size_t)rank * bytes, bytes, p, st)) return 1;
        for (int p = 0; p < world; ++p)
            if (p != rank && recv(static_cast<char*>(full) + (size_t)p * bytes, bytes, p, st)) return 1;
        return group_end(st);
    }
    // scalar reductions go through the host (this transport only exists for tests)
    int reduce_host(double mine, bool is_max, double* out) {
        std::unique_lock<std::mutex> lk(grp->mu);
        const int epoch = grp->red_epoch;
        grp->red.push_back(mine);
        if (++grp->red_arrived == world) {
            double r = is_max ? grp->red[0] : 0.0;
            for (double v : grp->red) r = is_max ? std::max(r, v) : r + v;
            grp->red_result = r;
            grp->red_arrived = 0;
            grp->red.clear();
            ++grp->red_epoch;
            grp->cv.notify_all();
        } else if (wait_for(lk, [&] { return grp->red_epoch != epoch; }, "the other ranks of a reduction")) {
            return 1;
        }
        *out = grp->red_result;
        return 0;
    }
    template <typename T> int allreduce_scalar(T* d, bool is_max, hipStream_t st) {
        T v;
        PI_HIP(hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, st));
        PI_HIP(hipStreamSynchronize(st));
        double r;
        if (reduce_host((double)v, is_max, &r)) return 1;
        v = (T)r;
        PI_HIP(hipMemcpyAsync(d, &v, sizeof v, hipMemcpyHostToDevice, st));
        PI_HIP(hipStreamSynchronize(st));
        return 0;
    }
    int allreduce_max_f32(float* d, hipStream_t st) override { return allreduce_scalar(d, true, st); }
    int allreduce_sum_u32(uint32_t* d, hipStream_t st) override { return allreduce_scalar(d, false, st); }
};

int need_comm(pi_handle* h) {
    if (pi::check_ready(h)) return 1;
    if (!h->comm) return fail("no communicator on this handle: call pi_comm_init first");
    return 0;
}
int need_plan(pi_handle* h) {
    if (need_comm(h)) return 1;
    if (!h->plan) return fail("no exchange plan on this handle: call pi_exchange_plan first");
    if (h->plan->broken)
        return fail("a sharded sweep failed on this handle and its exchange was abandoned; the communicator is not usable "
                    "any more (RCCL: aborted; in-process: its group gave up).  Recover on EVERY rank: pi_comm_destroy, a new "
                    "pi_comm_init (fresh id) / pi_comm_init_local (fresh group name), then pi_exchange_plan");
    return 0;
}

// Post the halo sends/receives of one freshly swept buffer on `st` (one transport group).
int post_exchange(pi_handle* h, float* full, hipStream_t st) {
    pi::Comm* c = h->comm;
    const pi::ShardPlan* p = h->plan;
    if (c->group_begin()) return 1;
    for (const auto& s : p->segs) {
        const size_t bytes = (size_t)(s.b - s.a) * sizeof(float);
        const int rc = s.src == c->rank ? c->send(full + s.a, bytes, s.dst, st) : c->recv(full + s.a, bytes, s.src, st);
        if (rc) {                       // the transport has closed its group (RCCL: and aborted); keep its message
            const std::string why = pi::last_error();
            (void)c->group_end(st);
            return fail(why);
        }
    }
    return c->group_end(st);
}

// Fault injection for the tests (PI_MI355_DEBUG_DROP_DELIVERY=k): every k-th destination mask of a fused plan is cleared —
// the state is still swept, its value is just not delivered — so that a test can show its poisoning check FAILS when a
// delivery is missing (tests/test_gpu_p2p.py).  Off unless the variable is set.
void drop_deliveries_for_tests(std::vector<uint8_t>& dest) {
    const int k = pi::knob_int(Knob::DEBUG_DROP_DELIVERY);
    if (k > 0)
        for (size_t i = (size_t)k - 1; i < dest.size(); i += (size_t)k) dest[i] = 0;
}

// This rank's reach bitmap (`units` bits on the device, produced by `probe`) -> one byte per unit -> every rank's, through
// the transport: out[r * units + u] != 0 <=> rank r reads unit u.  Collective; blocks on `st` (planning is one-off).
template <typename Probe>
int gather_reach(pi::Comm* c, int64_t units, Probe probe, hipStream_t st, std::vector<uint8_t>& out, const char* what) {
    const size_t words = (size_t)(units + 31) / 32;
    uint32_t* d_bits = nullptr;
    uint8_t* d_all = nullptr;
    PI_HIP(hipMalloc((void**)&d_bits, words * sizeof(uint32_t)));
    std::vector<uint32_t> bits(words, 0u);
    int rc = hipMemsetAsync(d_bits, 0, words * sizeof(uint32_t), st) == hipSuccess ? probe(d_bits) : 1;
    if (!rc && hipMemcpyAsync(bits.data(), d_bits, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess) rc = 1;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = 1;
    (void)hipFree(d_bits);
    if (rc) return fail(std::string(what) + ": reach probe failed: " + pi::last_error());
    const size_t row = (size_t)(units + 3) / 4 * 4;              // padded to whole words for the transport
    std::vector<uint8_t> all((size_t)c->world * row, 0);
    for (int64_t u = 0; u < units; ++u) all[(size_t)c->rank * row + (size_t)u] = (bits[(size_t)u >> 5] >> (u & 31)) & 1u;
    PI_HIP(hipMalloc((void**)&d_all, all.size()));
    hipError_t e = hipMemcpyAsync(d_all, all.data(), all.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = c->allgather(d_all, row, st);
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(all.data(), d_all, all.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
    (void)hipFree(d_all);
    if (e != hipSuccess) return fail(std::string(what) + ": " + hipGetErrorString(e));
    if (rc) return 1;
    out.resize((size_t)c->world * (size_t)units);
    for (int r = 0; r < c->world; ++r) std::memcpy(&out[(size_t)r * units], &all[(size_t)r * row], (size_t)units);
    return 0;
}

// ---- the steps of pi_exchange_plan, in the order it takes them -----------------------------------------------------------
using Ranges = std::vector<std::pair<int64_t, int64_t>>;
using SweptFirst = pi::ShardPlan::SweptFirst;
// Units the reach is measured in: rows (i0, i1) where the grid has them (2-4x fewer values to
// exchange than whole planes of dimension 0), planes otherwise; PI_MI355_REACH_DEPTH overrides.
int reach_depth(pi_handle* h) {
    return pi::knob_clamped(Knob::REACH_DEPTH, pi_reach_depth_max(h));
}
// Reach bitmap of this shard -> all ranks -> who sends what to whom -> halo or all-gather (`mode`; PI_PLAN_NONE: halo
// unless a rank would receive > 60 % of an all-gather).  A halo plan keeps the segments that involve this rank.  Collective.
int plan_halo_segments(pi_handle* h, const uint8_t* term, int mode, hipStream_t st, pi::ShardPlan* plan) {
    pi::Comm* c = h->comm;
    int64_t g0 = 1;
    for (int d = 0; d < plan->depth; ++d) g0 *= h->shape[d];
    const int64_t n = h->n_states, stride0 = n / g0;
    std::vector<uint8_t> reach;
    auto probe = [&](uint32_t* d_bits) { return pi_reach_units(h, term, plan->s_begin, plan->s_end, plan->depth, d_bits, st); };
    if (gather_reach(c, g0, probe, st, reach, "exchange plan")) return 1;
    const int64_t count = pi_plan_segments(c->world, g0, stride0, n, plan->per, reach.data(), nullptr, 0);
    std::vector<int64_t> segs((size_t)count * 4);
    pi_plan_segments(c->world, g0, stride0, n, plan->per, reach.data(), segs.data(), count);
    std::vector<int64_t> recv(c->world, 0);
    for (int64_t i = 0; i < count; ++i) recv[segs[4 * i + 1]] += segs[4 * i + 3] - segs[4 * i + 2];
    const int64_t worst = *std::max_element(recv.begin(), recv.end()), full = plan->per * (c->world - 1);
    plan->halo = mode == PI_PLAN_HALO || (double)worst <= 0.6 * (double)full;
    if (!plan->halo) return 0;
    for (int64_t i = 0; i < count; ++i) {
        pi::ShardPlan::Seg s = {(int)segs[4 * i], (int)segs[4 * i + 1], segs[4 * i + 2], segs[4 * i + 3]};
        if (s.src == c->rank) { plan->segs.push_back(s); plan->send_elems += s.b - s.a; }
        else if (s.dst == c->rank) { plan->segs.push_back(s); plan->recv_elems += s.b - s.a; }
    }
    return 0;
}

// Sorted ranges, those at most `gap` apart merged | what ascending ranges leave of [lo, hi).
Ranges merge_ranges(const Ranges& sorted, int64_t gap) {
    Ranges out;
    for (const auto& r : sorted) {
        if (!out.empty() && r.first <= out.back().second + gap) out.back().second = std::max(out.back().second, r.second);
        else out.push_back(r);
    }
    return out;
}
Ranges ranges_between(const Ranges& ranges, int64_t lo, int64_t hi) {
    Ranges out;
    for (const auto& r : ranges) {
        if (r.first > lo) out.push_back({lo, r.first});
        lo = std::max(lo, r.second);
    }
    if (lo < hi) out.push_back({lo, hi});
    return out;
}
// The coarse launch ranges of the shard [s_begin, s_end): `cuts` (what travels, sorted) merged into what is swept first,
// and the rest.  What is swept first may be coarser than what is sent: pieces less than two planes of dimension 0 (at
// least 2^16 states) apart become ONE launch, so a shard is still swept in about three launches (low boundary planes, high
// boundary planes, interior) although the segments that travel are single rows.  The gap is bounded by an eighth of the
// shard: with shards of ~10 planes (C4 at 8 ranks) two planes would merge every send range into the whole shard and leave
// nothing to sweep while the halo travels (profiles/r02/halo_granularity.txt: "1 / 0").
void coarse_ranges(const Ranges& cuts, int64_t s_begin, int64_t s_end, int64_t n, int64_t shape0, Ranges* first, Ranges* interior) {
    const int64_t gap = std::min(std::max<int64_t>(int64_t(1) << 16, 2 * (n / shape0)), std::max<int64_t>((s_end - s_begin) / 8, 1));
    *first = merge_ranges(cuts, gap);
    // a sliver between the shard's edge and its first / last send range joins that range
    if (!first->empty()) {
        if (first->front().first - s_begin < gap) first->front().first = s_begin;
        if (s_end - first->back().second < gap) first->back().second = s_end;
    }
    *interior = ranges_between(*first, s_begin, s_end);
}
// Does the plan get what a transport that can deliver from inside the sweep (can_push) adds to it?  Wanted here: the
// transport can, PI_MI355_P2P_FUSED is not 0 and the second module builds.  Every rank must take the fused steps or none: a
// rank whose second module did not build (a failed hipRTC compile, a corrupt cache entry) would otherwise leave its peers
// waiting in the pair probe until the communicator's time limit.  One scalar sum, collective where can_push().
int agree_on_fused(pi_handle* h, hipStream_t st, bool* fused) {
    pi::Comm* c = h->comm;
    *fused = false;
    if (!c->can_push()) return 0;
    const uint32_t mine = pi::knob_flag(Knob::P2P_FUSED) && pi::ensure_push_module(h) == 0 ? 1u : 0u;
    uint32_t* d_votes = nullptr;
    PI_HIP(hipMalloc((void**)&d_votes, sizeof(uint32_t)));
    uint32_t all = 0;
    hipError_t e = hipMemcpyAsync(d_votes, &mine, sizeof mine, hipMemcpyHostToDevice, st);
    int rc = e == hipSuccess ? c->allreduce_sum_u32(d_votes, st) : 1;
    if (!rc && hipMemcpyAsync(&all, d_votes, sizeof all, hipMemcpyDeviceToHost, st) != hipSuccess) rc = 1;
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = 1;
    (void)hipFree(d_votes);
    if (rc) return fail("exchange plan: the ranks could not agree on the fused exchange");
    *fused = all == (uint32_t)c->world;
    return 0;
}
// Pair refinement.  With the velocity that moves coordinate 0 somewhere else than in memory dimension 1 (the fast
// single-GPU orders put it along the lanes) the rows (i0, i1) of the segments are all reachable and the segments are whole
// bands of planes; the fused exchange delivers per STATE, so its destination masks are cut down to the pairs (i_0, i_v)
// every peer really reads (pi_reach_pairs_kernel) — the triangle again, in any memory order.  The segments stay as they are:
// the unfused exchanges (a batch's first sweep on grids with terminal states, value iteration, all-gathers) travel whole.
struct PairReach {
    std::vector<uint8_t> need;                  // [rank * units + i_0 * gv + i_v]; empty: not measured, every state is wanted
    int64_t units = 0, gv = 1, stv = 1, st0 = 1;
    bool measured() const { return !need.empty(); }
    bool wanted_by(int dst, int64_t q) const {   // does rank dst read state q at all (pair level)?
        return need.empty() || need[(size_t)dst * (size_t)units + (size_t)((q / st0) * gv + (q / stv) % gv)] != 0;
    }
};
// Measured where it can be and PI_MI355_PAIR_REACH is not 0.  Collective: every rank measures or none (same grid, same
// order, same transport, same environment).
int gather_pair_reach(pi_handle* h, const uint8_t* term, const pi::ShardPlan& plan, hipStream_t st, PairReach* pr) {
    const int v = h->D >= 2 ? h->mem_of_user[1] : 0;
    if (!pi::pairs_possible(h) || v == 1 || !pi::knob_flag(Knob::PAIR_REACH)) return 0;
    pr->st0 = h->n_states / h->shape[0];
    pr->gv = h->shape[v];
    for (int d = v + 1; d < h->D; ++d) pr->stv *= h->shape[d];
    pr->units = (int64_t)h->shape[0] * pr->gv;
    return gather_reach(h->comm, pr->units, [&](uint32_t* d_bits) { return pi::reach_pairs(h, term, plan.s_begin, plan.s_end, d_bits, st); },
                        st, pr->need, "exchange plan (pairs)");
}
// One walk over the plan's segments for the fused exchange: the senders of incoming ones are noted (push_senders); for every
// outgoing one the receiver gets its bit in the destination masks — the j-th distinct receiver bit j (push_peers), at most 8
// (more: keep the copy kernel) — and visit(segment, bit) marks what it delivers, or refuses.  Returns whether everything
// fitted; if not, the plan names no receivers and no senders.
template <typename Visit> bool mark_deliveries(pi::ShardPlan* plan, int rank, Visit visit) {
    auto index_in = [](std::vector<int>& v, int x) {           // position of x in v, appended if it is new
        auto it = std::find(v.begin(), v.end(), x);
        return (size_t)((it == v.end() ? v.insert(it, x) : it) - v.begin());
    };
    for (const auto& sg : plan->segs) {
        if (sg.dst == rank) { index_in(plan->push_senders, sg.src); continue; }
        const size_t j = index_in(plan->push_peers, sg.dst);
        if (j >= 8 || !visit(sg, (uint8_t)(1u << j))) {
            plan->push_peers.clear(); plan->push_senders.clear();
            return false;
        }
    }
    return true;
}
int64_t count_deliveries(const std::vector<uint8_t>& dest) {     // (state, receiver) pairs
    return std::accumulate(dest.begin(), dest.end(), int64_t(0), [](int64_t n, uint8_t m) { return n + __builtin_popcount(m); });
}
template <typename T> int copy_up(const std::vector<T>& v, T** d, hipStream_t st) {   // asynchronous: synchronise `st` while v is alive
    PI_HIP(hipMalloc((void**)d, std::max<size_t>(v.size(), 1) * sizeof(T)));
    PI_HIP(hipMemcpyAsync(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return 0;
}
// Ends an upload, failed (rc) or not: copies queued so far still read the host vectors, so the stream is drained either way.
int finish_upload(int rc, hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    if (!rc) PI_HIP(e);
    return rc;
}
// The swept-first list, the interior list and — fused plans; null otherwise — the destination mask of every swept-first entry
// go to the device and the plan becomes `kind`.  count: the plan reports what one sweep delivers (PI_COMM_INFO_FUSED_VALUES).
int upload_lists(pi::ShardPlan* plan, SweptFirst kind, const std::vector<int32_t>& first, const std::vector<int32_t>& inner,
                 std::vector<uint8_t>* dest, bool count, hipStream_t st) {
    plan->n_first = (int64_t)first.size();
    plan->n_inner = (int64_t)inner.size();
    int rc = copy_up(first, &plan->d_first, st) || copy_up(inner, &plan->d_inner, st);
    if (!rc && dest) {
        drop_deliveries_for_tests(*dest);
        rc = copy_up(*dest, &plan->d_first_dest, st);
        if (count) plan->fused_send_elems = count_deliveries(*dest);
    }
    if (finish_upload(rc, st)) return 1;
    plan->swept_first = kind;
    return 0;
}

// State-exact lists (grids without terminal states, pair reach measured): swept first = the states of this shard some
// peer reads, each with the mask of those peers; the rest is the interior.  Only the fused exchange can deliver them.
// Leaves the plan as it is when more than 8 peers read from this shard or the split is trivial.
int plan_state_lists(pi_handle* h, const PairReach& pairs, hipStream_t st, pi::ShardPlan* plan) {
    const int64_t len = plan->s_end - plan->s_begin;
    std::vector<uint8_t> mark((size_t)len, 0);
    if (!mark_deliveries(plan, h->comm->rank, [&](const pi::ShardPlan::Seg& sg, uint8_t bit) {
            for (int64_t q = sg.a; q < sg.b; ++q)
                if (pairs.wanted_by(sg.dst, q)) mark[(size_t)(q - plan->s_begin)] |= bit;
            return true;
        }))
        return 0;
    std::vector<int32_t> first, inner;
    std::vector<uint8_t> dest;
    for (int64_t q = plan->s_begin; q < plan->s_end; ++q) {
        const uint8_t m = mark[(size_t)(q - plan->s_begin)];
        if (m) { first.push_back((int32_t)q); dest.push_back(m); }
        else inner.push_back((int32_t)q);
    }
    if (first.empty() || (int64_t)first.size() == len) { plan->push_peers.clear(); plan->push_senders.clear(); return 0; }
    return upload_lists(plan, SweptFirst::PushLists, first, inner, &dest, true, st);
}

// Row-exact lists (grids without terminal states: the list kernel visits listed states only and copies nothing): the union
// of the rows that travel (`cuts`), nothing merged across gaps.  Taken when it moves at least a quarter of the coarse
// swept-first states into the interior or PI_MI355_ROW_EXACT = 1 (`want`).  `fused`: who reads which listed row, a byte per entry.
int plan_row_lists(pi_handle* h, const Ranges& cuts, int want, bool fused, hipStream_t st, pi::ShardPlan* plan) {
    const Ranges exact = merge_ranges(cuts, 0);
    int64_t exact_states = 0, coarse_states = 0;
    for (const auto& r : exact) exact_states += r.second - r.first;
    for (const auto& r : plan->send_ranges) coarse_states += r.second - r.first;
    const bool possible = !exact.empty() && exact_states < plan->s_end - plan->s_begin;
    const bool pays = exact.size() > plan->send_ranges.size() && 4 * exact_states <= 3 * coarse_states;
    if (!possible || !(want == 1 || pays)) return 0;
    plan->first_exact = exact;
    plan->inner_exact = ranges_between(exact, plan->s_begin, plan->s_end);
    std::vector<int32_t> first, inner;
    std::vector<int64_t> start;                                 // position of every range of `exact` in the list
    first.reserve((size_t)exact_states);
    inner.reserve((size_t)(plan->s_end - plan->s_begin - exact_states));
    for (const auto& r : exact) {
        start.push_back((int64_t)first.size());
        for (int64_t q = r.first; q < r.second; ++q) first.push_back((int32_t)q);
    }
    for (const auto& r : plan->inner_exact)
        for (int64_t q = r.first; q < r.second; ++q) inner.push_back((int32_t)q);
    std::vector<uint8_t> dest(first.size(), 0);
    fused = fused && mark_deliveries(plan, h->comm->rank, [&](const pi::ShardPlan::Seg& sg, uint8_t bit) {
        // the range of `exact` that holds [a, b): the last one that starts at or before a
        const size_t i = (size_t)(std::upper_bound(exact.begin(), exact.end(), std::make_pair(sg.a, INT64_MAX)) - exact.begin()) - 1;
        if (i >= exact.size() || sg.a < exact[i].first || sg.b > exact[i].second) return false;
        for (int64_t q = sg.a; q < sg.b; ++q) dest[(size_t)(start[i] + (q - exact[i].first))] |= bit;
        return true;
    });
    // fused_send_elems is NOT counted for this plan: PI_COMM_INFO_FUSED_VALUES has always answered -1 for it (recorded runs hold that)
    return upload_lists(plan, fused ? SweptFirst::PushLists : SweptFirst::Lists, first, inner, fused ? &dest : nullptr, false, st);
}

// Live-state masks (grids WITH terminal states whose shard keeps a live-state list): later sweeps of a batch visit the
// shard's live states only — who reads which of them.  Where some are read by nobody the plan gets state-exact lists for
// these sweeps too: swept first = the live states some peer reads (with their masks), interior = the shard's other live states
// — instead of the coarse ranges, which in the orders that keep the coupling velocity off memory dimension 1 are bands of planes.
int plan_live_masks(pi_handle* h, const PairReach& pairs, hipStream_t st, pi::ShardPlan* plan) {
    int64_t base = 0, total = 0;
    pi::live_span(h, plan->s_begin, plan->s_end, &base, &total);
    if (total <= 0) return 0;
    std::vector<uint8_t> dest((size_t)total, 0);
    std::vector<int32_t> states;
    if (!mark_deliveries(plan, h->comm->rank, [&](const pi::ShardPlan::Seg& sg, uint8_t bit) {
            int64_t first = 0, count = 0;
            pi::live_span(h, sg.a, sg.b, &first, &count);
            states.clear();
            if (pairs.measured()) pi::live_states(h, sg.a, sg.b, states);      // the listed states of [a, b), ascending
            for (int64_t k = 0; k < count; ++k)
                if (!pairs.measured() || pairs.wanted_by(sg.dst, states[(size_t)k])) dest[(size_t)(first - base + k)] |= bit;
            return true;
        }))
        return 0;
    plan->live_list = h->d_live;
    plan->live_list_count = h->live_count;
    plan->fused_send_elems = count_deliveries(dest);
    std::vector<int32_t> every, first, inner;
    std::vector<uint8_t> dfirst;
    pi::live_states(h, plan->s_begin, plan->s_end, every);
    if ((int64_t)every.size() == total) {
        for (int64_t k = 0; k < total; ++k) {
            if (dest[(size_t)k]) { first.push_back(every[(size_t)k]); dfirst.push_back(dest[(size_t)k]); }
            else inner.push_back(every[(size_t)k]);
        }
    }
    if (!first.empty() && !inner.empty()) return upload_lists(plan, SweptFirst::PushLiveLists, first, inner, &dfirst, false, st);
    if (finish_upload(copy_up(dest, &plan->d_live_dest, st), st)) return 1;
    plan->live_dest_base = base;
    plan->swept_first = SweptFirst::PushLiveSpans;
    return 0;
}

// ---- one sharded evaluation sweep: what peers wait for, the hand-over, the interior ------------------------------------
struct ShardSweep {
    const float* src; float* dst;   // the buffers of this sweep: dst = V'(src)
    const int32_t* policy; const uint8_t* term;
    float gamma;
    bool want;          // this sweep leaves its residual in the accumulator slots
    int k;              // index in its batch
    bool live, fused;   // the handle holds a live-state list for `term` that covers the shard | the swept-first kernel delivers
    hipStream_t st;
};
// Does sweep k of a batch go through the fused exchange?  Lists with masks: every sweep.  Live-state masks: the later sweeps,
// over the list they were built from (terminal states' values never change: every rank holds them since the first sweep).
bool fused_sweep(const pi_handle* h, const uint8_t* term, int k, bool live) {
    const pi::ShardPlan* p = h->plan;
    if (!p->overlapped()) return false;
    if (p->swept_first == SweptFirst::PushLists) return term == nullptr;
    return p->live_push() && k >= 1 && live && p->live_list == h->d_live && p->live_list_count == h->live_count;
}
// Is the sweep split into the plan's two state lists (otherwise: into its coarse ranges)?  Live lists hold no terminal state,
// and a batch's first sweep (k = 0, never fused) has to copy the terminal values: it takes the coarse ranges like any unfused sweep.
bool swept_by_lists(const pi::ShardPlan* p, const ShardSweep& s) {
    return p->row_lists() ? s.term == nullptr : s.fused && p->swept_first == SweptFirst::PushLiveLists;
}
// One launch range of one sweep: the later sweeps of a batch (k >= 1) visit only the range's live states when
// the handle holds a list for this mask (pi_prepare_mask) — the first one copies the terminal values.
int sweep_range(pi_handle* h, const ShardSweep& s, int64_t a, int64_t b) {
    if (s.k >= 1 && s.live) {
        int64_t first = 0, count = 0;
        pi::live_span(h, a, b, &first, &count);
        return pi::launch_eval_live(h, s.src, s.dst, s.policy, first, count, s.gamma, s.want, s.st);
    }
    return pi::launch_eval(h, s.src, s.dst, s.policy, s.term, a, b, s.gamma, s.want, s.st, s.k >= 1);
}
// What peers wait for (no overlap: the whole shard).  `table`: the peers' addresses of s.dst for the push kernel, fused sweeps only.
int sweep_first_part(pi_handle* h, const ShardSweep& s, float* const* table) {
    const pi::ShardPlan* p = h->plan;
    if (!p->overlapped()) return sweep_range(h, s, p->s_begin, p->s_end);
    const int n_peers = (int)p->push_peers.size();
    if (swept_by_lists(p, s))
        return s.fused ? pi::launch_eval_push(h, s.src, s.dst, s.policy, p->d_first, p->d_first_dest, table, n_peers, p->n_first,
                                              s.gamma, s.want, s.st)
                       : pi::launch_eval_live(h, s.src, s.dst, s.policy, 0, p->n_first, s.gamma, s.want, s.st, p->d_first);
    for (const auto& r : p->send_ranges) {
        int64_t first = 0, count = 0;                       // fused: the live states of the range, with their masks
        if (s.fused) pi::live_span(h, r.first, r.second, &first, &count);
        if (s.fused ? pi::launch_eval_push(h, s.src, s.dst, s.policy, h->d_live + first, p->d_live_dest + (first - p->live_dest_base),
                                           table, n_peers, count, s.gamma, s.want, s.st)
                    : sweep_range(h, s, r.first, r.second)) return 1;
    }
    return 0;
}
// The rest of the shard, swept while the first part travels.
int sweep_interior_part(pi_handle* h, const ShardSweep& s) {
    const pi::ShardPlan* p = h->plan;
    if (!p->overlapped()) return 0;
    if (swept_by_lists(p, s)) return pi::launch_eval_live(h, s.src, s.dst, s.policy, 0, p->n_inner, s.gamma, s.want, s.st, p->d_inner);
    for (const auto& r : p->interior)
        if (sweep_range(h, s, r.first, r.second)) return 1;
    return 0;
}

}  // namespace

extern "C" {

int pi_comm_unique_id(void* id128) {
    if (!id128) return fail("null argument");
    ncclUniqueId id;
    PI_NCCL(ncclGetUniqueId(&id));
    static_assert(sizeof id == 128, "RCCL unique id is 128 bytes");
    std::memcpy(id128, &id, sizeof id);
    return 0;
}

int pi_comm_init(pi_handle* h, int rank, int world, const void* id128) {
    if (!h || !id128) return fail("null argument");
    if (h->device < 0) return fail("host-only handle cannot own a communicator");
    if (world < 1 || rank < 0 || rank >= world) return fail("rank/world out of range");
    pi::DeviceGuard guard(h->device);
    std::unique_ptr<RcclComm> c(new RcclComm);
    c->rank = rank;
    c->world = world;
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof id);
    PI_NCCL(ncclCommInitRank(&c->comm, world, id, rank));
    pi::release_comm(h);
    h->comm = c.release();
    return 0;
}

int pi_comm_init_local(pi_handle* h, int rank, int world, const char* group_name) {
    if (!h || !group_name) return fail("null argument");
    if (h->device < 0) return fail("host-only handle cannot own a communicator");
    if (world < 1 || rank < 0 || rank >= world) return fail("rank/world out of range");
    std::unique_ptr<LocalComm> c(new LocalComm);
    c->rank = rank;
    c->world = world;
    c->name = group_name;
    {
        std::lock_guard<std::mutex> lk(g_groups_mu);
        auto& g = g_groups[c->name];
        if (!g) {
            g = std::make_shared<LocalGroup>();
            g->world = world;
            g->box.resize((size_t)world * world);
        }
        if (g->world != world) return fail("local group exists with a different world size");
        ++g->joined;
        c->grp = g;
    }
    pi::release_comm(h);
    h->comm = c.release();
    return 0;
}

int pi_comm_destroy(pi_handle* h) {
    if (!h) return fail("null handle");
    pi::DeviceGuard guard(h->device);
    pi::release_comm(h);
    return 0;
}

int pi_comm_info(pi_handle* h, int what) {
    if (!h || !h->comm) return -1;
    const pi::ShardPlan* p = h->plan;
    auto clip = [](int64_t v) { return (int)std::min<int64_t>(v, INT32_MAX); };
    switch (what) {
        case PI_COMM_INFO_RANK: return h->comm->rank;
        case PI_COMM_INFO_WORLD: return h->comm->world;
        case PI_COMM_INFO_TRANSPORT: return h->comm->transport();
        case PI_COMM_INFO_PLAN: return p ? (p->halo ? PI_PLAN_HALO : PI_PLAN_ALLGATHER) : PI_PLAN_NONE;
        case PI_COMM_INFO_REACH_UNITS: return p ? p->depth : 0;
        case PI_COMM_INFO_ROW_EXACT: return p && p->row_lists() ? 1 : 0;
        case PI_COMM_INFO_FUSED: return p && p->fused() ? 1 : 0;
        case PI_COMM_INFO_PAIR_EXACT: return p && p->pair_exact ? 1 : 0;
        case PI_COMM_INFO_FUSED_VALUES: return p ? clip(p->fused_send_elems) : -1;
        case PI_COMM_INFO_FIRST_ENTRIES: return p && p->has_lists() ? clip(p->n_first) : -1;
        case PI_COMM_INFO_INTERIOR_ENTRIES: return p && p->has_lists() ? clip(p->n_inner) : -1;
        default: return -1;
    }
}

int pi_allgather_V(pi_handle* h, float* V_full, int64_t shard_elems, void* stream) {
    if (need_comm(h)) return 1;
    if (!V_full || shard_elems < 0) return fail("bad argument");
    pi::DeviceGuard guard(h->device);
    return h->comm->allgather(V_full, (size_t)shard_elems * sizeof(float), (hipStream_t)stream);
}

int pi_allgather_policy(pi_handle* h, int32_t* policy_full, int64_t shard_elems, void* stream) {
    if (need_comm(h)) return 1;
    if (!policy_full || shard_elems < 0) return fail("bad argument");
    pi::DeviceGuard guard(h->device);
    return h->comm->allgather(policy_full, (size_t)shard_elems * sizeof(int32_t), (hipStream_t)stream);
}

int pi_allreduce_max_f32(pi_handle* h, float* d_value, void* stream) {
    if (need_comm(h)) return 1;
    pi::DeviceGuard guard(h->device);
    return h->comm->allreduce_max_f32(d_value, (hipStream_t)stream);
}

int pi_allreduce_sum_u32(pi_handle* h, uint32_t* d_value, void* stream) {
    if (need_comm(h)) return 1;
    pi::DeviceGuard guard(h->device);
    return h->comm->allreduce_sum_u32(d_value, (hipStream_t)stream);
}

// Pure host logic (no GPU, no communicator): which pieces of V' must travel between ranks.
//   reach[r * g0 + p] != 0  <=>  rank r's shard can read dimension-0 plane p (any action)
// Output: up to `cap` segments {src, dst, a, b} = "src sends V'[a, b) to dst" (every rank derives
// the same list from the same bitmaps).  Returns the number of segments (may exceed cap: call
// again with a larger buffer), or -1 on bad arguments.
int64_t pi_plan_segments(int world, int64_t g0, int64_t stride0, int64_t n_states, int64_t per,
                         const uint8_t* reach, int64_t* segs, int64_t cap) {
    if (world < 1 || g0 < 1 || stride0 < 1 || per < 1 || !reach) { fail("bad argument"); return -1; }
    int64_t count = 0;
    for (int dst = 0; dst < world; ++dst) {
        const uint8_t* need = reach + (size_t)dst * g0;
        int64_t p = 0;
        while (p < g0) {
            if (!need[p]) { ++p; continue; }
            int64_t q = p;
            while (q < g0 && need[q]) ++q;
            const int64_t lo = p * stride0, hi = std::min(q * stride0, n_states);
            for (int src = 0; src < world; ++src) {
                const int64_t a = std::max(lo, (int64_t)src * per);
                const int64_t b = std::min(hi, std::min(((int64_t)src + 1) * per, n_states));
                if (src != dst && a < b) {
                    if (segs && count < cap) {
                        segs[4 * count + 0] = src;
                        segs[4 * count + 1] = dst;
                        segs[4 * count + 2] = a;
                        segs[4 * count + 3] = b;
                    }
                    ++count;
                }
            }
            p = q;
        }
    }
    return count;
}

// mode: PI_PLAN_NONE = choose (halo unless a rank would receive > 60 % of an all-gather), PI_PLAN_ALLGATHER,
// PI_PLAN_HALO.  `overlap` = 0 disables the send-first / interior-while-travelling split.
// info[0] = mode chosen (PI_PLAN_ALLGATHER | PI_PLAN_HALO), info[1] = elements this rank receives per sweep,
// info[2] = elements it sends, info[3] = number of send ranges, info[4] = interior ranges.
int pi_exchange_plan(pi_handle* h, const uint8_t* term, int64_t per, int mode, int overlap, int64_t* info, void* stream) {
    if (need_comm(h)) return 1;
    if (per < 1) return fail("bad argument");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    pi::Comm* c = h->comm;
    const int64_t n = h->n_states;
    if (per * c->world < n) return fail("per * world < n_states");
    std::unique_ptr<pi::ShardPlan> plan(new pi::ShardPlan);
    plan->per = per;
    plan->depth = reach_depth(h);
    plan->s_begin = std::min((int64_t)c->rank * per, n);
    plan->s_end = std::min(plan->s_begin + per, n);
    if (mode != PI_PLAN_ALLGATHER && plan_halo_segments(h, term, mode, st, plan.get())) return 1;
    if (plan->halo && overlap) {
        // sub-ranges of this shard that peers wait for (swept first), and the rest
        Ranges cuts;
        for (const auto& s : plan->segs)
            if (s.src == c->rank) cuts.push_back({s.a, s.b});
        std::sort(cuts.begin(), cuts.end());
        coarse_ranges(cuts, plan->s_begin, plan->s_end, n, h->shape[0], &plan->send_ranges, &plan->interior);
        // the collectives of the fused exchange, in this order on every rank
        bool fused = false;
        PairReach pairs;
        if (agree_on_fused(h, st, &fused)) return 1;
        if (fused && gather_pair_reach(h, term, *plan, st, &pairs)) return 1;
        plan->pair_exact = pairs.measured();
        // What is swept first, beyond the coarse ranges — the first of these that yields something:
        //   state-exact lists   no terminal states, pair reach measured, this shard sends something; always fused
        //   row-exact lists     no terminal states, where they pay or PI_MI355_ROW_EXACT = 1 (= 0: neither kind of list)
        //   live-state masks    the shard keeps a live-state list for this mask; fused exchange only
        const int want = pi::knob_flag(Knob::ROW_EXACT);
        const bool lists_possible = term == nullptr && want != 0;
        if (lists_possible && plan->pair_exact && !cuts.empty() && plan_state_lists(h, pairs, st, plan.get())) return 1;
        if (lists_possible && plan->swept_first == SweptFirst::Ranges && plan_row_lists(h, cuts, want, fused, st, plan.get())) return 1;
        const bool live = fused && pi::live_usable(h, term, plan->s_begin, plan->s_end);
        if (live && plan->swept_first == SweptFirst::Ranges && plan_live_masks(h, pairs, st, plan.get())) return 1;
        PI_HIP(hipStreamCreateWithFlags(&plan->comm_stream, hipStreamNonBlocking));
        PI_HIP(hipEventCreateWithFlags(&plan->ev_ready, hipEventDisableTiming));
        PI_HIP(hipEventCreateWithFlags(&plan->ev_done, hipEventDisableTiming));
    }
    if (!plan->halo) {
        plan->recv_elems = per * (c->world - 1);
        plan->send_elems = per;
    }
    if (info) {
        info[0] = plan->halo ? PI_PLAN_HALO : PI_PLAN_ALLGATHER;
        info[1] = plan->recv_elems;
        info[2] = plan->send_elems;
        info[3] = (int64_t)plan->send_ranges.size();
        info[4] = (int64_t)plan->interior.size();
    }
    pi::drop_plan(h);
    h->plan = plan.release();
    return 0;
}

// The launch ranges of the current plan: up to `cap` triples {kind, begin, end} — kind 0 = swept
// first (peers wait for rows inside it), kind 1 = interior (swept while the halo travels); a plan
// without overlap (all-gather, or overlap disabled) reports the whole shard as one kind-0 range.
int64_t pi_plan_ranges(pi_handle* h, int64_t* ranges, int64_t cap) {
    if (need_plan(h)) return -1;
    const pi::ShardPlan* p = h->plan;
    std::vector<std::array<int64_t, 3>> all;
    const bool rows = !p->first_exact.empty();              // row-exact lists: the ranges they were made from
    if (p->overlapped()) {
        for (const auto& r : rows ? p->first_exact : p->send_ranges) all.push_back({0, r.first, r.second});
        for (const auto& r : rows ? p->inner_exact : p->interior) all.push_back({1, r.first, r.second});
    } else if (p->s_end > p->s_begin) {
        all.push_back({0, p->s_begin, p->s_end});
    }
    for (size_t i = 0; ranges && i < all.size() && (int64_t)i < cap; ++i)
        for (int k = 0; k < 3; ++k) ranges[3 * i + k] = all[i][k];
    return (int64_t)all.size();
}

// One part of a sharded evaluation sweep WITHOUT the exchange, launched by the functions pi_eval_sweeps_sharded
// launches the first sweep of a batch with: part 0 = what peers wait for (swept first), part 1 = the interior.  For
// measurements and tests: both parts together are one sweep of the shard.  A plan without overlap has everything in part 0.
int pi_eval_sweep_part(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, const uint8_t* term, int part,
                       float gamma, void* stream) {
    if (need_plan(h)) return 1;
    if (!V || !Vnew || !policy || V == Vnew) return fail("bad device pointer");
    if (part != 0 && part != 1) return fail("part must be 0 (swept first) or 1 (interior)");
    pi::DeviceGuard guard(h->device);
    const ShardSweep s = {V, Vnew, policy, term, gamma, false, 0, false, false, (hipStream_t)stream};
    return part == 0 ? sweep_first_part(h, s, nullptr) : sweep_interior_part(h, s);
}

// Make this rank's freshly written shard of `V_full` visible where the other ranks read it.
int pi_exchange_V(pi_handle* h, float* V_full, void* stream) {
    if (need_plan(h)) return 1;
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (!h->plan->halo) return h->comm->allgather(V_full, (size_t)h->plan->per * sizeof(float), st);
    return post_exchange(h, V_full, st);
}

// n_sweeps evaluation sweeps of this rank's shard, ping-ponging between Va and Vb exactly like
// pi_eval_sweeps, with the exchange after every sweep; d_delta (nullable) receives the residual of
// the LAST sweep, already reduced (MAX) over all ranks.  Nothing returns to the host in between.
int pi_eval_sweeps_sharded(pi_handle* h, float* Va, float* Vb, const int32_t* policy, const uint8_t* term, float gamma,
                           int n_sweeps, float* d_delta, void* stream) {
    if (need_plan(h)) return 1;
    if (n_sweeps < 0) return fail("n_sweeps < 0");
    if (!Va || !Vb || !policy) return fail("null device pointer");
    if (Va == Vb) return fail("Va and Vb must be different buffers (Jacobi sweep)");
    if (n_sweeps == 0) return 0;
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    pi::ShardPlan* p = h->plan;
    pi::Comm* c = h->comm;
    const bool overlap = p->overlapped();
    const bool live = pi::live_usable(h, term, p->s_begin, p->s_end);
    auto batch = [&]() -> int {
        for (int k = 0; k < n_sweeps; ++k) {
            const float* src = (k & 1) ? Vb : Va;
            float* dst = (k & 1) ? Va : Vb;
            const bool want = k == n_sweeps - 1 && d_delta != nullptr;
            // How the swept-first part reaches the peers: fused (everything on this stream: the swept-first kernel stores
            // its states into the peers' buffers itself, one-wave kernels hand-shake in front of it and behind it), as an
            // exchange on the second stream while the interior is swept, or — no overlap — as a plain exchange after.
            const ShardSweep s = {src, dst, policy, term, gamma, want, k, live, fused_sweep(h, term, k, live), st};
            float* const* table = nullptr;
            if (s.fused && c->push_begin(p->push_peers, p->push_senders, dst, &table, st)) return 1;
            if (sweep_first_part(h, s, table)) return 1;
            if (s.fused) {
                if (c->push_signal(st)) return 1;
            } else if (overlap) {
                PI_HIP(hipEventRecord(p->ev_ready, st));
                PI_HIP(hipStreamWaitEvent(p->comm_stream, p->ev_ready, 0));
                if (post_exchange(h, dst, p->comm_stream)) return 1;
                PI_HIP(hipEventRecord(p->ev_done, p->comm_stream));
            } else if (pi_exchange_V(h, dst, stream)) {
                return 1;
            }
            if (sweep_interior_part(h, s)) return 1;
            if (s.fused) {
                // a fused sweep is followed by fused sweeps only: the next one's push_begin waits for this one's data
                if (k + 1 < n_sweeps ? c->push_wait_deferred(st) : c->push_wait(st)) return 1;
            } else if (overlap) {
                PI_HIP(hipStreamWaitEvent(st, p->ev_done, 0));
            }
        }
        if (d_delta) {
            if (p->s_end == p->s_begin) PI_HIP(hipMemsetAsync(d_delta, 0, sizeof(float), st));
            else if (pi::finalize(h, d_delta, nullptr, st)) return 1;
            return h->comm->allreduce_max_f32(d_delta, st);
        }
        return 0;
    };
    if (batch() == 0) return 0;
    // Failure half-way through the batch: leave a DEFINED state behind.  Drain both streams (a launch or an event may be
    // pending on either), clear the residual slots a finished sweep may have filled, and retire the plan — the peers are at
    // an unknown sweep, so the next sharded call must be preceded by a new communicator and a collective pi_exchange_plan
    // (need_plan says how).  The error of the failing call is kept.
    const std::string why = pi::last_error();
    h->comm->give_up();                                                      // in-process peers stop waiting at once
    if (p->comm_stream) (void)hipStreamSynchronize(p->comm_stream);
    (void)hipStreamSynchronize(st);
    (void)hipMemsetAsync(h->d_slots, 0, 2 * pi::kSlots * sizeof(unsigned int), st);
    (void)hipGetLastError();
    p->broken = true;
    return fail("pi_eval_sweeps_sharded abandoned (streams drained, exchange plan retired): " + why);
}

// Greedy improvement of this rank's shard; d_changed (nullable) = entries changed, summed over ranks.
int pi_improve_sweep_sharded(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term,
                             float gamma, uint32_t* d_changed, void* stream) {
    if (need_plan(h)) return 1;
    if (pi_improve_sweep(h, V, policy, term, h->plan->s_begin, h->plan->s_end, gamma, d_changed, stream)) return 1;
    if (d_changed) {
        pi::DeviceGuard guard(h->device);
        return h->comm->allreduce_sum_u32(d_changed, (hipStream_t)stream);
    }
    return 0;
}

}  // extern "C"
