// pi_expect_greedy.cpp — expected-value greedy control on the inference handle (include/pi_mi355.h, "Inference" block):
// the one-step lookahead a*(s) = argmax_a sum_k p_k [ r_k + gamma * E[V](f(s, a (+) da_k) + dx_k) ] over a disturbance set
// on the handle's value function at arbitrary states.  pi_infer_set_expect_greedy uploads the action table and builds
// the handle's seventh module — its grid, pi_math.h, the plugin pi_infer_set_dynamics was given, the helpers of
// csrc/pi_rollout_kernels.hip, the functions of csrc/pi_greedy_kernels.hip and csrc/pi_stochastic_kernels.hip and
// csrc/pi_expect_greedy_kernels.hip in one translation unit; pi_infer_set_disturbances uploads the set (run-time data:
// never a build); pi_infer_expect_greedy answers a batch of query points and pi_infer_rollout_expect_greedy runs whole
// episodes of a batch of start states under that controller with the stochastic rollouts' noise, one launch each.

#include "pi_internal.h"

#include <cmath>
#include <sstream>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_expect_greedy\n"
    "pi_embedded_expect_greedy:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_expect_greedy_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_expect_greedy[];

using pi::fail;

namespace {

constexpr int kBlock = 256;               // PI_EG_BLOCK

struct StateNoise {                       // PiStateNoise
    float v[6];
};

// what both launching entry points refuse about the handle: the module first, then the set
int check_ready(const char* who, const pi_infer* h) {
    if (!h->has_expect_greedy)
        return fail(std::string(who) + ": no expected-greedy module: call pi_infer_set_expect_greedy (again after every "
                                       "pi_infer_set_dynamics)");
    if (h->dist_k == 0)
        return fail(std::string(who) + ": no disturbance set is installed: call pi_infer_set_disturbances first");
    return 0;
}

}  // namespace

int pi::drop_expect_greedy(pi_infer* h) {
    if (h->module_expect_greedy) {                  // launches already enqueued have to finish first
        pi::DeviceGuard guard(h->device);
        PI_HIP(hipDeviceSynchronize());
        PI_HIP(hipModuleUnload(h->module_expect_greedy));
    }
    h->module_expect_greedy = nullptr;
    h->f_expect_greedy = nullptr;
    h->f_expect_greedy_rollout = nullptr;
    h->has_expect_greedy = false;
    return 0;
}

extern "C" {

int pi_infer_set_expect_greedy(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h) return fail("null handle");
    if (!action_space) return fail("null argument (action_space)");
    if (n_actions < 1) return fail("need at least one action");
    float a_min = action_space[0], a_max = action_space[0];
    for (int i = 0; i < n_actions; ++i) {
        if (!std::isfinite(action_space[i]))
            return fail("pi_infer_set_expect_greedy: action_space[" + std::to_string(i) + "] is not finite");
        a_min = std::fmin(a_min, action_space[i]);
        a_max = std::fmax(a_max, action_space[i]);
    }
    if (!h->has_values) return fail("pi_infer_set_expect_greedy: pi_infer_set_values was never called");
    if (!h->has_dynamics) return fail("pi_infer_set_expect_greedy: pi_infer_set_dynamics was never called");
    std::ostringstream src;
    src << "#define PI_EXPECT_GREEDY 1\n#define PI_GREEDY 1\n#define PI_STOCHASTIC 1\n";
    src << h->grid_defines;
    src << pi_embedded_math << "\n";
    src << "#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n";
    src << "// ---- env plugin (user string) ----\n";
    src << h->dynamics_src << "\n";
    src << "// ---- rollout helpers ----\n";
    src << pi_embedded_rollout << "\n";
    src << "// ---- greedy functions ----\n";
    src << pi_embedded_greedy << "\n";
    src << "// ---- stochastic functions ----\n";
    src << pi_embedded_stochastic << "\n";
    src << "// ---- expected-greedy kernels ----\n";
    src << pi_embedded_expect_greedy << "\n";
    std::vector<char> image;
    if (pi::compile_image(src.str(), h->has_cache_dir ? h->cache_dir.c_str() : nullptr, log, log_len, image, nullptr)) return 1;
    if (pi::drop_expect_greedy(h)) return 1;
    if (h->device >= 0) {
        pi::DeviceGuard guard(h->device);
        // drop_expect_greedy has waited for the launches that read the previous table, if there was one
        if (h->d_expect_greedy_actions) { (void)hipFree(h->d_expect_greedy_actions); h->d_expect_greedy_actions = nullptr; }
        PI_HIP(hipMalloc((void**)&h->d_expect_greedy_actions, (size_t)n_actions * sizeof(float)));
        PI_HIP(hipMemcpy(h->d_expect_greedy_actions, action_space, (size_t)n_actions * sizeof(float), hipMemcpyHostToDevice));
        PI_HIP(hipModuleLoadData(&h->module_expect_greedy, image.data()));
        PI_HIP(hipModuleGetFunction(&h->f_expect_greedy, h->module_expect_greedy, "pi_expect_greedy_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_expect_greedy_rollout, h->module_expect_greedy, "pi_expect_greedy_rollout_kernel"));
    }
    h->n_expect_greedy_actions = n_actions;
    h->expect_greedy_a_min = a_min;
    h->expect_greedy_a_max = a_max;
    h->has_expect_greedy = true;
    return 0;
}

int pi_infer_set_disturbances(pi_infer* h, int K, const float* action_offsets, const float* state_offsets,
                              const float* weights) {
    pi::fail("");
    if (!h) return fail("null handle");
    std::vector<float> table;
    if (pi::build_disturbance_table("pi_infer_set_disturbances", h->D, K, action_offsets, state_offsets, weights, table))
        return 1;
    if (K == 0) {
        h->dist_k = 0;
        return 0;
    }
    if (h->device >= 0) {
        pi::DeviceGuard guard(h->device);
        if (!h->d_dist)
            PI_HIP(hipMalloc((void**)&h->d_dist, sizeof(float) * pi::kMaxDisturbances * (h->D + 2)));
        PI_HIP(hipDeviceSynchronize());                      // a launch in flight may still read the table of the set before
        PI_HIP(hipMemcpy(h->d_dist, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    h->dist_k = K;
    return 0;
}

int pi_infer_expect_greedy(pi_infer* h, const float* d_points, int64_t m, float gamma, int32_t* d_best, float* d_action,
                           float* d_q_best, float* d_q_all, void* stream) {
    if (!h) return fail("null handle");
    if (check_ready("pi_infer_expect_greedy", h)) return 1;
    if (std::isnan(gamma)) return fail("pi_infer_expect_greedy: gamma is NaN");
    if (m < 0) return fail("m < 0");
    if (m == 0) return 0;                           // nothing to do: an empty batch has no buffers either
    if (!d_best && !d_action && !d_q_best && !d_q_all) return fail("pi_infer_expect_greedy: all four outputs are null");
    int64_t q_floats = 0;
    if (__builtin_mul_overflow(m, (int64_t)h->n_expect_greedy_actions, &q_floats) || q_floats > (INT64_MAX >> 2))
        return fail("m * n_actions does not fit 63 bits");
    const int64_t blocks = (m + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX) return fail("m is too large for one launch");
    if (h->device < 0 || !h->f_expect_greedy || !h->d_dist) return fail("host-only handle (device = -1) cannot launch kernels");
    if (!d_points) return fail("null device pointer (d_points)");
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->f_expect_greedy, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_points, (long long)m,
                      (const float*)h->d_values, (const float*)h->d_expect_greedy_actions, h->n_expect_greedy_actions,
                      h->expect_greedy_a_min, h->expect_greedy_a_max, (const float*)h->d_dist, h->dist_k, gamma, d_best,
                      d_action, d_q_best, d_q_all));
    return 0;
}

int pi_infer_rollout_expect_greedy(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma,
                                   float lookahead_gamma, float epsilon, float action_noise, const float* state_noise,
                                   uint64_t seed, uint64_t first_episode, float* d_final, float* d_return,
                                   int32_t* d_length, uint8_t* d_terminated, float* d_traj, int traj_every, void* stream) {
    const char* who = "pi_infer_rollout_expect_greedy";
    if (!h) return fail("null handle");
    if (check_ready(who, h)) return 1;
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(std::string(who) + ": epsilon must lie in [0, 1]");
    if (!(action_noise >= 0.0f) || !std::isfinite(action_noise))
        return fail(std::string(who) + ": action_noise must be finite and not negative");
    StateNoise noise = {};
    int any_noise = 0;
    for (int d = 0; state_noise && d < h->D; ++d) {
        if (!(state_noise[d] >= 0.0f) || !std::isfinite(state_noise[d]))
            return fail(std::string(who) + ": state_noise[" + std::to_string(d) + "] must be finite and not negative");
        noise.v[d] = state_noise[d];
        any_noise |= state_noise[d] != 0.0f;
    }
    if (std::isnan(gamma)) return fail(std::string(who) + ": gamma is NaN");
    if (std::isnan(lookahead_gamma)) return fail(std::string(who) + ": lookahead_gamma is NaN");
    if (h->device < 0 || !h->f_expect_greedy_rollout || !h->d_dist)
        return fail("host-only handle (device = -1) cannot launch kernels");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    const unsigned int eps24 = (unsigned int)std::llrint((double)epsilon * 16777216.0);
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->f_expect_greedy_rollout, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_start, (long long)m,
                      n_steps, gamma, lookahead_gamma, (const float*)h->d_values, (const float*)h->d_expect_greedy_actions,
                      h->n_expect_greedy_actions, h->expect_greedy_a_min, h->expect_greedy_a_max, (const float*)h->d_dist,
                      h->dist_k, eps24, action_noise, noise, any_noise, (unsigned long long)seed,
                      (unsigned long long)first_episode, d_final, d_return, d_length, d_terminated,
                      traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

}  // extern "C"
