// pi_adversary.cpp — the robust lookahead and the adversary rollout on the inference handle (include/pi_mi355.h,
// "Inference" block): the worst-case fold over the set of pi_infer_set_disturbances at arbitrary states.
// pi_infer_set_robust uploads the action table and builds the handle's adversary module — its grid, pi_math.h, the plugin
// pi_infer_set_dynamics was given, the helpers of csrc/pi_rollout_kernels.hip, the functions of csrc/pi_greedy_kernels.hip
// and csrc/pi_adversary_kernels.hip in one translation unit; pi_infer_robust answers a batch of query points and
// pi_infer_rollout_adversary runs whole episodes in which the disturbance is chosen against the controller, one launch each.

#include "pi_internal.h"

#include <cmath>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_adversary\n"
    "pi_embedded_adversary:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_adversary_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_adversary[];

using pi::fail;

namespace {

constexpr int kBlock = 256;               // PI_ADV_BLOCK, PI_RO_BLOCK

// what both launching entry points refuse about the handle: the module first, then the set
int check_ready(const char* who, const pi_infer* h) {
    if (!h->robust.ready)
        return fail(std::string(who) + ": no adversary module: call pi_infer_set_robust (again after every "
                                       "pi_infer_set_dynamics)");
    if (h->dist_k == 0)
        return fail(std::string(who) + ": no disturbance set is installed: call pi_infer_set_disturbances first");
    return 0;
}

}  // namespace

extern "C" {

int pi_infer_set_robust(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h) return fail("null handle");
    pi::ActionTable table;
    if (pi::check_action_table("pi_infer_set_robust", true, action_space, n_actions, &table)) return 1;
    if (!h->has_values) return fail("pi_infer_set_robust: pi_infer_set_values was never called");
    if (!h->rollout.ready) return fail("pi_infer_set_robust: pi_infer_set_dynamics was never called");
    std::vector<char> image;
    if (pi::build_infer_module(h, "#define PI_ADVERSARY 1\n#define PI_GREEDY 1\n" + h->grid_defines, h->dynamics_src,
                               {{"rollout helpers", pi_embedded_rollout}, {"greedy functions", pi_embedded_greedy},
                                {"adversary kernels", pi_embedded_adversary}},
                               log, log_len, image))
        return 1;
    return pi::install(h, h->robust, image, &table, "pi_adversary_rollout_kernel", "pi_robust_greedy_kernel");
}

int pi_infer_robust(pi_infer* h, const float* d_points, int64_t m, float gamma, int32_t* d_best, float* d_action,
                    float* d_q_best, float* d_q_all, int32_t* d_worst, void* stream) {
    if (!h) return fail("null handle");
    if (check_ready("pi_infer_robust", h)) return 1;
    if (std::isnan(gamma)) return fail("pi_infer_robust: gamma is NaN");
    if (m < 0) return fail("m < 0");
    if (m == 0) return 0;                           // nothing to do: an empty batch has no buffers either
    if (!d_best && !d_action && !d_q_best && !d_q_all && !d_worst) return fail("pi_infer_robust: all five outputs are null");
    int64_t q_floats = 0;
    if (__builtin_mul_overflow(m, (int64_t)h->robust.n_actions, &q_floats) || q_floats > (INT64_MAX >> 2))
        return fail("m * n_actions does not fit 63 bits");
    const int64_t blocks = (m + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX) return fail("m is too large for one launch");
    if (h->device < 0 || !h->robust.f_query || !h->d_dist) return fail("host-only handle (device = -1) cannot launch kernels");
    if (!d_points) return fail("null device pointer (d_points)");
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->robust.f_query, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_points, (long long)m,
                      (const float*)h->d_values, (const float*)h->robust.d_actions, h->robust.n_actions, h->robust.a_min,
                      h->robust.a_max, (const float*)h->d_dist, h->dist_k, gamma, d_best, d_action, d_q_best, d_q_all, d_worst));
    return 0;
}

int pi_infer_rollout_adversary(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float lookahead_gamma,
                               int controller, float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated,
                               float* d_traj, int traj_every, void* stream) {
    const char* who = "pi_infer_rollout_adversary";
    if (!h) return fail("null handle");
    if (check_ready(who, h)) return 1;
    if (std::isnan(gamma)) return fail(std::string(who) + ": gamma is NaN");
    if (std::isnan(lookahead_gamma)) return fail(std::string(who) + ": lookahead_gamma is NaN");
    if (controller != 0 && controller != 1)
        return fail(std::string(who) + ": controller must be 0 (the policy table) or 1 (the robust lookahead)");
    if (controller == 0 && !h->d_policy)
        return fail(std::string(who) + ": controller 0 needs a policy: pi_infer_set_policy was never called");
    if (h->device < 0 || !h->robust.f_rollout || !h->d_dist) return fail("host-only handle (device = -1) cannot launch kernels");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->robust.f_rollout, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_start, (long long)m, n_steps,
                      gamma, lookahead_gamma, controller, (const int*)h->d_policy, (const float*)h->d_actions,
                      (const float*)h->d_values, (const float*)h->robust.d_actions, h->robust.n_actions, h->robust.a_min,
                      h->robust.a_max, (const float*)h->d_dist, h->dist_k, d_final, d_return, d_length, d_terminated,
                      traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

}  // extern "C"
