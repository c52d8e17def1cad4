// pi_greedy.cpp — value-greedy control on the inference handle (include/pi_mi355.h, "Inference" block): the one-step
// lookahead a*(s) = argmax_a [ r(s, a) + gamma * E[V](s') ] on the handle's value function at arbitrary states.
// pi_infer_set_greedy uploads the action table and builds the handle's greedy module — its grid, pi_math.h, the plugin
// pi_infer_set_dynamics was given, the helpers of csrc/pi_rollout_kernels.hip and csrc/pi_greedy_kernels.hip in one
// translation unit; pi_infer_greedy answers a batch of query points and pi_infer_rollout_greedy runs whole episodes of a
// batch of start states under that controller, one launch each.

#include "pi_internal.h"

#include <cmath>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_greedy\n"
    "pi_embedded_greedy:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_greedy_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_greedy[];

using pi::fail;

namespace {

constexpr int kBlock = 256;               // PI_GR_BLOCK, PI_RO_BLOCK

// what both launching entry points refuse about the handle
int check_module(const char* who, const pi_infer* h) {
    if (!h->greedy.ready)
        return fail(std::string(who) + ": no greedy module: call pi_infer_set_greedy (again after every pi_infer_set_dynamics)");
    return 0;
}

}  // namespace

extern "C" {

int pi_infer_set_greedy(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h) return fail("null handle");
    pi::ActionTable table;
    // any value goes: the lookahead never clamps to the table's extremes, and a NaN or infinite entry never wins the argmax
    if (pi::check_action_table("pi_infer_set_greedy", false, action_space, n_actions, &table)) return 1;
    if (!h->has_values) return fail("pi_infer_set_greedy: pi_infer_set_values was never called");
    if (!h->rollout.ready) return fail("pi_infer_set_greedy: pi_infer_set_dynamics was never called");
    std::vector<char> image;
    if (pi::build_infer_module(h, "#define PI_GREEDY 1\n" + h->grid_defines, h->dynamics_src,
                               {{"rollout helpers", pi_embedded_rollout}, {"greedy kernels", pi_embedded_greedy}}, log, log_len, image))
        return 1;
    return pi::install(h, h->greedy, image, &table, "pi_greedy_rollout_kernel", "pi_greedy_kernel");
}

int pi_infer_greedy(pi_infer* h, const float* d_points, int64_t m, float gamma, int32_t* d_best, float* d_action,
                    float* d_q_best, float* d_q_all, void* stream) {
    if (!h) return fail("null handle");
    if (check_module("pi_infer_greedy", h)) return 1;
    if (std::isnan(gamma)) return fail("pi_infer_greedy: gamma is NaN");
    if (m < 0) return fail("m < 0");
    if (m == 0) return 0;                           // nothing to do: an empty batch has no buffers either
    if (!d_best && !d_action && !d_q_best && !d_q_all) return fail("pi_infer_greedy: all four outputs are null");
    int64_t q_floats = 0;
    if (__builtin_mul_overflow(m, (int64_t)h->greedy.n_actions, &q_floats) || q_floats > (INT64_MAX >> 2))
        return fail("m * n_actions does not fit 63 bits");
    const int64_t blocks = (m + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX) return fail("m is too large for one launch");
    if (h->device < 0 || !h->greedy.f_query) return fail("host-only handle (device = -1) cannot launch kernels");
    if (!d_points) return fail("null device pointer (d_points)");
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->greedy.f_query, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_points, (long long)m,
                      (const float*)h->d_values, (const float*)h->greedy.d_actions, h->greedy.n_actions, gamma, d_best,
                      d_action, d_q_best, d_q_all));
    return 0;
}

int pi_infer_rollout_greedy(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float lookahead_gamma,
                            float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj,
                            int traj_every, void* stream) {
    if (!h) return fail("null handle");
    if (check_module("pi_infer_rollout_greedy", h)) return 1;
    if (std::isnan(gamma)) return fail("pi_infer_rollout_greedy: gamma is NaN");
    if (std::isnan(lookahead_gamma)) return fail("pi_infer_rollout_greedy: lookahead_gamma is NaN");
    if (h->device < 0 || !h->greedy.f_rollout) return fail("host-only handle (device = -1) cannot launch kernels");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->greedy.f_rollout, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_start, (long long)m, n_steps,
                      gamma, lookahead_gamma, (const float*)h->d_values, (const float*)h->greedy.d_actions,
                      h->greedy.n_actions, d_final, d_return, d_length, d_terminated,
                      traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

}  // extern "C"
