// pi_expect.cpp — noise-aware solving: the disturbance set of a handle, the expectation sweeps over it and the worst-case
// sweeps over it (csrc/pi_expect_kernels.hip; the semantics are written out in include/pi_mi355.h at pi_set_disturbances
// and pi_robust_eval_sweeps).

#include "pi_internal.h"

#include <algorithm>
#include <cmath>

using namespace pi;

namespace {

constexpr int kMaxPoints = pi::kMaxDisturbances;
constexpr int kBlock = 256;         // PI_BLOCK_EXPECT: one chunk per workgroup

// What every expectation and worst-case sweep checks before it looks at its own arguments.  The set comes first, so that a caller who
// forgot it is told so on any handle.
int check_expect(const pi_handle* h, const char* who, int64_t s_begin, int64_t s_end) {
    if (!h) return fail("null handle");
    if (h->dist_k == 0) return fail(std::string(who) + ": no disturbance set is installed: call pi_set_disturbances first");
    return check_ready(h) || check_range(h, s_begin, s_end);
}

unsigned int* delta_slots(pi_handle* h, bool want) { return want ? h->d_slots : nullptr; }
unsigned int* changed_slots(pi_handle* h, bool want) { return want ? h->d_slots + kSlots : nullptr; }
Grid2 blocks_for(int64_t count) { return {launch_blocks(kBlock, count, 1), 1u}; }

// The three sweeps, each ONE host function for the expectation and the worst case: `kernel` is the instantiation of the
// handle's expectation module that the entry point `who` launches (pi_expect_*_kernel or pi_robust_*_kernel: same
// arguments, same chunking).
int eval_sweeps(pi_handle* h, const char* who, hipFunction_t kernel, float* Va, float* Vb, const int32_t* policy,
                const uint8_t* term, int64_t s_begin, int64_t s_end, float gamma, int n_sweeps, float* d_delta, void* stream) {
    if (check_expect(h, who, s_begin, s_end)) return 1;
    if (n_sweeps < 0) return fail("n_sweeps < 0");
    if (!Va || !Vb || !policy) return fail("null device pointer");
    if (Va == Vb) return fail("Va and Vb must be different buffers (Jacobi sweep)");
    if (n_sweeps == 0) return 0;
    drop_eval_list(h);                                       // ends a pi_eval_begin bracket
    DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(d_delta, nullptr, st);
    for (int i = 0; i < n_sweeps; ++i) {
        const float* src = (i & 1) ? Vb : Va;
        float* dst = (i & 1) ? Va : Vb;
        // every sweep copies the terminal states' values: both buffers hold them after the first, as pi_eval_sweeps leaves them
        PI_HIP(launch(kernel, blocks_for(s_end - s_begin), kBlock, st, src, dst, policy, term, (const float*)h->d_tab,
                      (const float*)h->d_dist, h->dist_k, h->dist_a_min, h->dist_a_max, (long long)s_begin, (long long)s_end,
                      gamma, delta_slots(h, i == n_sweeps - 1 && d_delta)));
    }
    return finalize(h, d_delta, nullptr, st);
}

int improve_sweep(pi_handle* h, const char* who, hipFunction_t kernel, const float* V, int32_t* policy, const uint8_t* term,
                  int64_t s_begin, int64_t s_end, float gamma, uint32_t* d_changed, void* stream) {
    if (check_expect(h, who, s_begin, s_end)) return 1;
    if (!V || !policy) return fail("null device pointer");
    drop_eval_list(h);                                       // the policy is about to change
    DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(nullptr, d_changed, st);
    PI_HIP(launch(kernel, blocks_for(s_end - s_begin), kBlock, st, V, policy, term, (const float*)h->d_tab,
                  (const float*)h->d_dist, h->dist_k, h->dist_a_min, h->dist_a_max, (long long)s_begin, (long long)s_end, gamma,
                  changed_slots(h, d_changed != nullptr)));
    return finalize(h, nullptr, d_changed, st);
}

int value_sweep(pi_handle* h, const char* who, hipFunction_t kernel, const float* V, float* Vnew, int32_t* policy,
                const uint8_t* term, int64_t s_begin, int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed,
                void* stream) {
    if (check_expect(h, who, s_begin, s_end)) return 1;
    if (!V || !Vnew || !policy) return fail("null device pointer");
    if (V == Vnew) return fail("V and Vnew must be different buffers (Jacobi sweep)");
    drop_eval_list(h);                                       // the policy is about to change
    DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(d_delta, d_changed, st);
    PI_HIP(launch(kernel, blocks_for(s_end - s_begin), kBlock, st, V, Vnew, policy, term, (const float*)h->d_tab,
                  (const float*)h->d_dist, h->dist_k, h->dist_a_min, h->dist_a_max, (long long)s_begin, (long long)s_end, gamma,
                  delta_slots(h, d_delta != nullptr), changed_slots(h, d_changed != nullptr)));
    return finalize(h, d_delta, d_changed, st);
}

}  // namespace

int pi::build_disturbance_table(const char* who_c, int D, int K, const float* action_offsets, const float* state_offsets,
                                const float* weights, std::vector<float>& table) {
    const std::string who(who_c);
    table.clear();
    if (K < 0 || K > kMaxPoints) return fail(who + ": K must be in [0, " + std::to_string(kMaxPoints) + "]");
    if (K == 0) return 0;
    if (!weights) return fail(who + ": null weights");
    const int row = D + 2;
    table.assign((size_t)K * row, 0.0f);
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        float* r = &table[(size_t)k * row];
        if (action_offsets) r[0] = action_offsets[k];
        for (int d = 0; d < D && state_offsets; ++d) r[1 + d] = state_offsets[(size_t)k * D + d];
        r[row - 1] = weights[k];
        for (int j = 0; j < row; ++j)
            if (!std::isfinite(r[j])) return fail(who + ": point " + std::to_string(k) + " holds a value that is not finite");
        if (r[row - 1] < 0.0f) return fail(who + ": weight " + std::to_string(k) + " is negative");
        sum += (double)r[row - 1];
    }
    if (!(std::fabs(sum - 1.0) <= 1e-4))
        return fail(who + ": the weights sum to " + std::to_string(sum) + ", not to 1 within 1e-4");
    return 0;
}

extern "C" {

int pi_set_disturbances(pi_handle* h, int K, const float* action_offsets, const float* state_offsets, const float* weights) {
    pi::fail("");
    if (!h) return fail("null handle");
    if (h->n_states >= (int64_t(1) << 30))
        return fail("pi_set_disturbances: grids of 2^30 states or more are not served (the expectation sweeps have no 64-bit "
                    "addressing path)");
    if (!h->compiled) return fail("pi_set_disturbances: pi_compile has not been called on this handle");
    const int row = h->D + 2;
    std::vector<float> table;
    if (build_disturbance_table("pi_set_disturbances", h->D, K, action_offsets, state_offsets, weights, table)) return 1;
    if (K == 0) {
        h->dist_k = 0;
        return 0;
    }
    if (ensure_expect_module(h)) return 1;
    const auto ends = std::minmax_element(h->tab.begin(), h->tab.begin() + h->n_actions);
    if (h->device >= 0) {
        DeviceGuard guard(h->device);
        if (!h->d_dist) {
            float* p = nullptr;
            PI_HIP(hipMalloc((void**)&p, sizeof(float) * kMaxPoints * row));
            h->d_dist = p;
        }
        PI_HIP(hipDeviceSynchronize());                      // a sweep in flight may still read the table of the set before
        PI_HIP(hipMemcpy(h->d_dist, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    h->dist_a_min = *ends.first;
    h->dist_a_max = *ends.second;
    h->dist_k = K;
    return 0;
}

int pi_expect_eval_sweeps(pi_handle* h, float* Va, float* Vb, const int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, int n_sweeps, float* d_delta, void* stream) {
    return eval_sweeps(h, "pi_expect_eval_sweeps", h ? h->f_expect_eval : nullptr, Va, Vb, policy, term, s_begin, s_end, gamma,
                       n_sweeps, d_delta, stream);
}

int pi_robust_eval_sweeps(pi_handle* h, float* Va, float* Vb, const int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, int n_sweeps, float* d_delta, void* stream) {
    return eval_sweeps(h, "pi_robust_eval_sweeps", h ? h->f_robust_eval : nullptr, Va, Vb, policy, term, s_begin, s_end, gamma,
                       n_sweeps, d_delta, stream);
}

int pi_expect_improve_sweep(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term, int64_t s_begin,
                            int64_t s_end, float gamma, uint32_t* d_changed, void* stream) {
    return improve_sweep(h, "pi_expect_improve_sweep", h ? h->f_expect_improve : nullptr, V, policy, term, s_begin, s_end,
                         gamma, d_changed, stream);
}

int pi_robust_improve_sweep(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term, int64_t s_begin,
                            int64_t s_end, float gamma, uint32_t* d_changed, void* stream) {
    return improve_sweep(h, "pi_robust_improve_sweep", h ? h->f_robust_improve : nullptr, V, policy, term, s_begin, s_end,
                         gamma, d_changed, stream);
}

int pi_expect_value_sweep(pi_handle* h, const float* V, float* Vnew, int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed, void* stream) {
    return value_sweep(h, "pi_expect_value_sweep", h ? h->f_expect_value : nullptr, V, Vnew, policy, term, s_begin, s_end,
                       gamma, d_delta, d_changed, stream);
}

int pi_robust_value_sweep(pi_handle* h, const float* V, float* Vnew, int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed, void* stream) {
    return value_sweep(h, "pi_robust_value_sweep", h ? h->f_robust_value : nullptr, V, Vnew, policy, term, s_begin, s_end,
                       gamma, d_delta, d_changed, stream);
}

}  // extern "C"
