// pi_live.cpp — the lists of states a sweep visits instead of the whole grid: the live (non-terminal) states of
// pi_prepare_mask with their host-side index (live_span, live_states), and the per-evaluation list of pi_eval_begin.
// Both are built on the device by one two-pass procedure (count_and_scan, then pass 1 of the list kernel).

#include "pi_internal.h"

#include <algorithm>

using pi::Knob;
using pi::knob_int;
using pi::fail;

namespace pi {

bool live_usable(const pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end) {
    return h->live_count > 0 && term != nullptr && term == h->live_term && s_begin >= h->live_lo && s_end <= h->live_hi;
}

void live_span(const pi_handle* h, int64_t s_begin, int64_t s_end, int64_t* first, int64_t* count) {
    const int64_t word0 = h->live_lo >> 6;
    auto position = [&](int64_t s) {                      // listed live states below s
        if (s <= h->live_lo) return int64_t(0);
        if (s >= h->live_hi) return h->live_count;
        const uint64_t word = h->live_bits[(size_t)((s >> 6) - word0)];
        const uint64_t below = (s & 63) ? word & ((uint64_t(1) << (s & 63)) - 1) : 0;
        return h->live_before[(size_t)((s >> 6) - word0)] + (int64_t)__builtin_popcountll(below);
    };
    *first = position(s_begin);
    *count = position(s_end) - *first;
}

void live_states(const pi_handle* h, int64_t s_begin, int64_t s_end, std::vector<int32_t>& out) {
    const int64_t a = std::max(s_begin, h->live_lo), b = std::min(s_end, h->live_hi);
    const int64_t word0 = h->live_lo >> 6;
    for (int64_t w = a >> 6; w <= (b - 1) >> 6 && a < b; ++w) {
        uint64_t word = h->live_bits[(size_t)(w - word0)];
        while (word) {
            const int bit = __builtin_ctzll(word);
            word &= word - 1;
            const int64_t s = (w << 6) + bit;
            if (s >= a && s < b) out.push_back((int32_t)s);
        }
    }
}

// What a list of `entries` states spread over the listed range [live_lo, live_hi) would have over the whole grid
// (plan_launch's `total`: the strip schedule cuts a list into the same shares as the planes it stands for).
int64_t live_list_total(const pi_handle* h, int64_t entries) {
    const int64_t range = h->live_hi - h->live_lo;
    if (range <= 0 || entries <= 0) return 0;
    return (int64_t)((double)entries * ((double)h->n_states / (double)range));
}

void drop_eval_list(pi_handle* h) {
    h->eval_count = -1;
    h->eval_policy = nullptr;
    h->eval_holds.clear();
}

}  // namespace pi

namespace {

// "Count per block, scan, write in order": pass(0) of a list kernel leaves one count per block in slots[0, nblocks),
// pi_scan_slots_kernel turns them into offsets with the total behind them, and the total comes back to the host.
// pass(1) — the same launch, the caller's second step — then writes the list in order.
template <typename Pass>
hipError_t count_and_scan(pi_handle* h, Pass pass, long long nblocks, unsigned long long* slots, hipStream_t st,
                          unsigned long long* total) {
    hipError_t err = pass(0);
    if (err == hipSuccess) err = pi::launch(h->f_scan_slots, {1, 1}, 1024, st, slots, nblocks);
    if (err == hipSuccess) err = hipMemcpyAsync(total, slots + nblocks, sizeof *total, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    return err;
}

}  // namespace

extern "C" {

int pi_prepare_mask(pi_handle* h, const uint8_t* d_term, void* stream) {
    if (pi::check_ready(h)) return 1;
    return pi_prepare_mask_range(h, d_term, 0, h->n_states, stream);
}

int pi_prepare_mask_range(pi_handle* h, const uint8_t* d_term, int64_t s_begin, int64_t s_end, void* stream) {
    if (pi::check_ready(h) || pi::check_range(h, s_begin, s_end)) return 1;
    pi::DeviceGuard guard(h->device);
    if (h->d_live) { (void)hipFree(h->d_live); h->d_live = nullptr; }
    if (h->d_eval_list) { (void)hipFree(h->d_eval_list); h->d_eval_list = nullptr; }
    if (h->d_eval_cursor) { (void)hipFree(h->d_eval_cursor); h->d_eval_cursor = nullptr; }
    pi::drop_eval_list(h);
    h->live_term = nullptr;
    h->live_count = 0;
    h->live_bits.clear();
    h->live_bits.shrink_to_fit();
    h->live_before.clear();
    h->live_before.shrink_to_fit();
    h->live_lo = h->live_hi = 0;
    if (!d_term || s_end == s_begin) return 0;
    // Only [s_begin, s_end) is listed: a rank of a sharded run lists its shard (the only states its launches visit),
    // not the grid — 1 / world of the device list, of the host index and of the host pass (at 25^6 on 8 ranks:
    // 80 MB instead of 630 MB of list per rank).
    const int64_t n = s_end - s_begin;
    if (h->n_states < knob_int(Knob::LIVE_MIN) || !knob_int(Knob::LIVE)) return 0;
    // Built on the device (pi_mask_list_kernel: bitmap + per-block counts, scan, ordered write); the host keeps the
    // bitmap only — 1 bit per state, 30 MB at 25^6 — and derives the live states in front of every 64-state block from it,
    // which is what positions of sub-ranges (live_span) and the sharded planner (live_states) need.
    hipStream_t st = (hipStream_t)stream;
    const int64_t w0 = s_begin & ~int64_t(63);
    const size_t nwords = (size_t)((s_end - w0 + 63) / 64);
    const long long nblocks = (long long)((nwords * 64 + pi::kProbeBlock - 1) / pi::kProbeBlock);
    unsigned long long* d_bits = nullptr;
    unsigned long long* d_slots = nullptr;
    PI_HIP(hipMalloc((void**)&d_bits, nwords * sizeof(unsigned long long)));
    if (hipMalloc((void**)&d_slots, (size_t)(nblocks + 1) * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipFree(d_bits);
        return fail("pi_prepare_mask: out of device memory");
    }
    auto cleanup = [&]() { (void)hipFree(d_bits); (void)hipFree(d_slots); };
    int32_t* out = nullptr;
    auto pass = [&](int which) {
        return pi::launch(h->f_mask_list, {(unsigned)nblocks, 1}, pi::kProbeBlock, st, d_term, (long long)s_begin, (long long)s_end,
                          (long long)w0, d_bits, d_slots, out, which);
    };
    unsigned long long packed = 0;
    hipError_t err = count_and_scan(h, pass, nblocks, d_slots, st, &packed);
    if (err != hipSuccess) { cleanup(); return fail(std::string("pi_prepare_mask: ") + hipGetErrorString(err)); }
    const int64_t n_live = (int64_t)(packed & 0xFFFFFFFFull), waves_with_a_live_lane = (int64_t)(packed >> 32);
    // idle lanes the state-order sweep carries through its gathers, as a share of the listed range
    const double idle = (double)(waves_with_a_live_lane * 64 - n_live) / (double)n;
    if (n_live == 0 || (idle < 0.03 && !h->live_force)) { cleanup(); return 0; }   // nothing to win: keep sweeping in state order
    if (hipMalloc((void**)&h->d_live, (size_t)n_live * sizeof(int32_t)) != hipSuccess) { cleanup(); return fail("pi_prepare_mask: out of device memory"); }
    out = h->d_live;
    std::vector<uint64_t> bits(nwords);
    err = pass(1);
    if (err == hipSuccess) err = hipMemcpyAsync(bits.data(), d_bits, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    cleanup();
    if (err != hipSuccess) {
        (void)hipFree(h->d_live);
        h->d_live = nullptr;
        return fail(std::string("pi_prepare_mask: ") + hipGetErrorString(err));
    }
    std::vector<int64_t> before_block(nwords + 1, 0);
    for (size_t k = 0; k < nwords; ++k) before_block[k + 1] = before_block[k] + (int64_t)__builtin_popcountll(bits[k]);
    if (before_block[nwords] != n_live) {
        (void)hipFree(h->d_live);
        h->d_live = nullptr;
        return fail("pi_prepare_mask: the bitmap and the list disagree");
    }
    h->live_term = d_term;
    h->live_lo = s_begin;
    h->live_hi = s_end;
    h->live_count = n_live;
    h->live_bits = std::move(bits);
    h->live_before = std::move(before_block);
    return 0;
}

int64_t pi_live_list(pi_handle* h, int32_t* d_out, int64_t capacity, void* stream) {
    if (pi::check_ready(h)) return -1;
    if (h->live_count <= 0 || !h->d_live) return 0;
    if (!d_out) return h->live_count;
    if (capacity < h->live_count) { fail("pi_live_list: capacity below the list's length"); return -1; }
    pi::DeviceGuard guard(h->device);
    if (hipMemcpyAsync(d_out, h->d_live, (size_t)h->live_count * sizeof(int32_t), hipMemcpyDeviceToDevice,
                       (hipStream_t)stream) != hipSuccess) { fail("pi_live_list: copy failed"); return -1; }
    return h->live_count;
}

int pi_eval_begin(pi_handle* h, const int32_t* policy, const uint8_t* term, void* stream) {
    if (pi::check_ready(h)) return 1;
    if (!policy) return fail("null device pointer");
    pi::drop_eval_list(h);
    if (!pi::live_usable(h, term, 0, h->n_states) || !knob_int(Knob::EVAL_LIST)) return 0;   // nothing to shorten
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const long long nblocks = (h->live_count + pi::kProbeBlock - 1) / pi::kProbeBlock;
    if (!h->d_eval_list) PI_HIP(hipMalloc((void**)&h->d_eval_list, (size_t)h->live_count * sizeof(int32_t)));
    if (!h->d_eval_cursor) PI_HIP(hipMalloc((void**)&h->d_eval_cursor, (size_t)(nblocks + 1) * sizeof(unsigned long long)));
    auto pass = [&](int which) {
        return pi::launch(h->f_policy_list, {(unsigned)nblocks, 1}, pi::kProbeBlock, st, (const int32_t*)h->d_live,
                          (long long)h->live_count, policy, (const float*)h->d_tab, h->d_eval_cursor, h->d_eval_list, which);
    };
    unsigned long long kept = 0;
    PI_HIP(count_and_scan(h, pass, nblocks, h->d_eval_cursor, st, &kept));
    PI_HIP(pass(1));
    PI_HIP(hipStreamSynchronize(st));                         // the list is complete when this call returns
    // worth a second list only when it is noticeably shorter
    if ((double)kept > 0.97 * (double)h->live_count) return 0;
    h->eval_count = (int64_t)kept;
    h->eval_policy = policy;
    return 0;
}

int pi_eval_end(pi_handle* h) {
    if (!h) return fail("null handle");
    pi::drop_eval_list(h);
    return 0;
}


}  // extern "C"
