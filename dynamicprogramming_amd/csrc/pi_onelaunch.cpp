// pi_onelaunch.cpp — the one-launch families of launch-bound grids (csrc/pi_onelaunch_kernels.hip): a whole policy
// evaluation (pi_policy_evaluation: XCD-local, dataflow or LDS-resident kernel) or a whole run (pi_policy_iteration) per
// launch, and the zeroed scratch blocks and wait limits the XCD-local and dataflow kernels need.

#include "pi_internal.h"

#include <algorithm>

using pi::check_ready;
using pi::fail;
using pi::kXcdCtlWords;
using pi::kXcds;
using pi::launch;

namespace {

// The device block of a one-launch kernel (d_flow / d_xcd, owned by the handle): at least `bytes`, and all of it zero
// on `st` — control, progress and check words start from zero, and the ring's tags of an earlier launch must not match
// either (tags are version + 1 >= 1); ~3 us for the 5 MB of a 200 x 200 grid.
int scratch_block(void** block, size_t* have, size_t bytes, hipStream_t st) {
    if (!*block || *have < bytes) {                   // more sweeps or more frequent looks than last time
        if (*block) {
            PI_HIP(hipStreamSynchronize(st));         // an earlier launch may still be using it
            PI_HIP(hipFree(*block));
            *block = nullptr;
        }
        PI_HIP(hipMalloc(block, bytes));
        *have = bytes;
    }
    PI_HIP(hipMemsetAsync(*block, 0, bytes, st));
    return 0;
}

// How long a wave of these kernels waits for another: the knob's seconds in ticks of wall_clock64 (100 MHz)
unsigned long long timeout_ticks(pi::Knob k) {
    return std::max<unsigned long long>((unsigned long long)(pi::knob_seconds(k) * 1e8), 1ull);
}

// pi_xcd_kernel + pi_xcd_finish_kernel on `st`: one policy evaluation (max_pi_iter == 0) or the whole run.  Device
// block (owned by the handle): ring of kXcdRing (PI_XCD_RING) granule versions of V (whole 128-byte lines each) |
// scratch policy | kXcdCtlWords control words (tickets, status, result, two banks of 64 flag granules: the kernel's
// PI_XCD_CTL_WORDS, checked against this constant by a static_assert in the generated unit).
int launch_xcd(pi_handle* h, float* V, int32_t* policy, const uint8_t* term, float gamma, double theta, int max_sweeps,
               int check_interval, int max_pi_iter, int32_t* d_out, float* d_delta, float* d_residual_log, uint32_t* d_iter_log,
               hipStream_t st) {
    const size_t n = (size_t)h->n_states;
    const unsigned wgs = (unsigned)((h->n_states + h->xcd_states - 1) / h->xcd_states);
    const size_t ring_bytes = (size_t)pi::kXcdRing * ((n + 15) & ~size_t(15)) * sizeof(unsigned long long);   // PI_XCD_RING versions
    const size_t pol_bytes = ((n * sizeof(int32_t)) + 255) & ~size_t(255);
    if (scratch_block(&h->d_xcd, &h->xcd_bytes, ring_bytes + pol_bytes + (size_t)kXcdCtlWords * sizeof(unsigned int), st)) return 1;
    unsigned long long* ring = (unsigned long long*)h->d_xcd;
    int32_t* pol_out = (int32_t*)((char*)h->d_xcd + ring_bytes);
    unsigned int* ctl = (unsigned int*)((char*)h->d_xcd + ring_bytes + pol_bytes);
    // placement is checked, not assumed: a quarter of a second is ample for a sweep and short for a wrong guess
    const unsigned long long ticks = timeout_ticks(pi::Knob::XCD_TIMEOUT);
    const unsigned grid = (unsigned)kXcds * (wgs + std::max(wgs / 4, 2u));        // spare workgroups: the first `wgs` on XCD 0 take part
    PI_HIP(launch(h->f_xcd, {grid, 1}, 1024, st, (const float*)V, (const int32_t*)policy, term, (const float*)h->d_tab, gamma,
                  max_sweeps, theta, check_interval, max_pi_iter, d_residual_log, d_iter_log, ring, pol_out, ctl, ticks));
    const int whole_run = max_pi_iter > 0 ? 1 : 0;
    PI_HIP(launch(h->f_xcd_finish, {(unsigned)((n + 255) / 256), 1}, 256, st, V, policy, (const unsigned long long*)ring,
                  (const int32_t*)pol_out, (const unsigned int*)ctl, whole_run, d_out, d_delta));
    return 0;
}

}  // namespace

extern "C" {

int pi_policy_evaluation(pi_handle* h, float* V, const int32_t* policy, const uint8_t* term, float gamma,
                         double theta, int max_sweeps, int check_interval, int32_t* d_sweeps, float* d_delta,
                         float* d_residual_log, void* stream) {
    if (check_ready(h)) return 1;
    const bool lds = h->f_resident && h->use_resident;
    if (!lds && !h->f_flow)
        return fail("pi_policy_evaluation: this grid has no one-launch evaluation kernel "
                    "(PI_INFO_RESIDENT_STATES_PER_THREAD: LDS-resident, PI_INFO_FLOW_WORKGROUPS: dataflow)");
    if (!V || !policy || !d_sweeps || !d_residual_log) return fail("null device pointer");
    if (max_sweeps < 1 || check_interval < 1) return fail("max_sweeps and check_interval must be positive");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const float* tab = h->d_tab;
    if (h->f_xcd && !h->xcd_off) {
        // XCD-local kernel first (also on the bigger ones of the grids one CU holds); V is untouched when it did not go through: the placement-independent kernel below runs
        // this evaluation then.  Repeated failures (placement, a wait that ran out) switch the form off for the handle.
        if (launch_xcd(h, V, const_cast<int32_t*>(policy), term, gamma, theta, max_sweeps, check_interval, 0, d_sweeps, d_delta,
                       d_residual_log, nullptr, st))
            return 1;
        int32_t done = 0;                                          // the caller reads it next anyway: one small copy
        PI_HIP(hipMemcpyAsync(&done, d_sweeps, sizeof done, hipMemcpyDeviceToHost, st));
        PI_HIP(hipStreamSynchronize(st));
        ++h->xcd_used;
        if (done >= 0) return 0;
        if (++h->xcd_failed >= 2) h->xcd_off = true;
    }
    if (!lds) {
        // dataflow kernel: ring of 16 granule versions | progress words + status word | one check slot per look
        const size_t n = (size_t)h->n_states;
        const unsigned int wgs = (unsigned)((h->n_states + h->flow_block - 1) / h->flow_block);
        const size_t ring_bytes = 16 * n * sizeof(unsigned long long);
        const size_t progress_words = ((size_t)wgs + 1 + 31) & ~size_t(31);
        const size_t looks = ((size_t)max_sweeps / (size_t)check_interval + 2 + 31) & ~size_t(31);
        if (scratch_block(&h->d_flow, &h->flow_bytes, ring_bytes + (progress_words + looks) * sizeof(unsigned int), st)) return 1;
        unsigned long long* ring = (unsigned long long*)h->d_flow;
        unsigned int* progress = (unsigned int*)((char*)h->d_flow + ring_bytes);
        unsigned int* checks = progress + progress_words;
        const unsigned long long ticks = timeout_ticks(pi::Knob::FLOW_TIMEOUT);
        PI_HIP(launch(h->f_flow, {wgs, 1}, h->flow_block, st, V, policy, term, tab, gamma, max_sweeps, d_delta, theta,
                      check_interval, d_sweeps, d_residual_log, ring, progress, checks, ticks));
        // the finish kernel is the only writer of V: the last version out of the ring when no wave gave up, nothing otherwise
        PI_HIP(launch(h->f_flow_finish, {(unsigned)((n + 255) / 256), 1}, 256, st, progress, wgs, d_sweeps, ring, V));
        return 0;
    }
    PI_HIP(launch(h->f_resident, {1, 1}, h->resident_block, st, V, (float*)nullptr, policy, term, tab, gamma, max_sweeps,
                  d_delta, theta, check_interval, d_sweeps, d_residual_log));
    return 0;
}

int pi_policy_iteration(pi_handle* h, float* V, int32_t* policy, const uint8_t* term, float gamma, double theta,
                        int max_eval_sweeps, int check_interval, int max_pi_iter, int32_t* d_result, uint32_t* d_iter_log,
                        void* stream) {
    if (check_ready(h)) return 1;
    const bool xcd = h->f_xcd && !h->xcd_off;
    const bool resident = !xcd && h->f_run_resident && h->use_resident;
    if (!resident && !xcd) return fail("pi_policy_iteration: this grid has no one-launch run (PI_INFO_WHOLE_RUN_AVAILABLE)");
    if (!V || !policy || !d_result || !d_iter_log) return fail("null device pointer");
    if (max_eval_sweeps < 1 || check_interval < 1 || max_pi_iter < 1) return fail("limits and check_interval must be positive");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    pi::drop_eval_list(h);                                   // the policy is about to change
    if (resident) {
        // one CU holds V and the policy in LDS: one workgroup, nothing to wait for
        PI_HIP(launch(h->f_run_resident, {1, 1}, h->resident_block, st, V, policy, term, (const float*)h->d_tab, gamma,
                      max_eval_sweeps, theta, check_interval, max_pi_iter, d_result, d_iter_log));
        ++h->whole_runs;
        return 0;
    }
    if (launch_xcd(h, V, policy, term, gamma, theta, max_eval_sweeps, check_interval, max_pi_iter, d_result, nullptr, nullptr,
                   d_iter_log, st))
        return 1;
    ++h->whole_runs;
    return 0;
}

}  // extern "C"
