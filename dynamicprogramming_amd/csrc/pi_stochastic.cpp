// pi_stochastic.cpp — stochastic rollouts on the inference handle (include/pi_mi355.h, "Inference" block): the
// random-policy baseline, epsilon-random actions, action noise and state noise from a counter-based random stream
// (Philox4x32-10 keyed by seed, episode and step) inside the rollout kernel.  pi_infer_set_stochastic uploads the action
// table and builds the handle's stochastic module — its grid, pi_math.h, the plugin pi_infer_set_dynamics was given, the
// helpers of csrc/pi_rollout_kernels.hip and csrc/pi_stochastic_kernels.hip in one translation unit;
// pi_infer_rollout_stochastic runs whole episodes of a batch of start states in one launch and pi_infer_random_words
// reads the stream itself.

#include "pi_internal.h"

#include <cmath>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_stochastic\n"
    "pi_embedded_stochastic:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_stochastic_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_stochastic[];

using pi::fail;

namespace {

constexpr int kBlock = 256;               // PI_ST_BLOCK, PI_RO_BLOCK

// what both launching entry points refuse about the handle
int check_module(const char* who, const pi_infer* h) {
    if (!h->stochastic.ready)
        return fail(std::string(who) +
                    ": no stochastic module: call pi_infer_set_stochastic (again after every pi_infer_set_dynamics)");
    return 0;
}

}  // namespace

int pi::check_stochastic_args(const char* who, int D, float epsilon, float action_noise, const float* state_noise,
                              float gamma, StochasticArgs* out) {
    const std::string w = std::string(who) + ": ";
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail(w + "epsilon must lie in [0, 1]");
    if (!(action_noise >= 0.0f) || !std::isfinite(action_noise)) return fail(w + "action_noise must be finite and not negative");
    *out = {};
    for (int d = 0; state_noise && d < D; ++d) {
        if (!(state_noise[d] >= 0.0f) || !std::isfinite(state_noise[d]))
            return fail(w + "state_noise[" + std::to_string(d) + "] must be finite and not negative");
        out->noise.v[d] = state_noise[d];
        out->any_noise |= state_noise[d] != 0.0f;
    }
    if (std::isnan(gamma)) return fail(w + "gamma is NaN");
    out->eps24 = (unsigned int)std::llrint((double)epsilon * 16777216.0);
    return 0;
}

extern "C" {

int pi_infer_set_stochastic(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h) return fail("null handle");
    pi::ActionTable table;
    if (pi::check_action_table("pi_infer_set_stochastic", true, action_space, n_actions, &table)) return 1;
    if (!h->rollout.ready) return fail("pi_infer_set_stochastic: pi_infer_set_dynamics was never called");
    std::vector<char> image;
    if (pi::build_infer_module(h, "#define PI_STOCHASTIC 1\n" + h->grid_defines, h->dynamics_src,
                               {{"rollout helpers", pi_embedded_rollout}, {"stochastic kernels", pi_embedded_stochastic}}, log,
                               log_len, image))
        return 1;
    return pi::install(h, h->stochastic, image, &table, "pi_stochastic_rollout_kernel", "pi_random_words_kernel");
}

int pi_infer_rollout_stochastic(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float epsilon,
                                float action_noise, const float* state_noise, uint64_t seed, uint64_t first_episode,
                                float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj,
                                int traj_every, void* stream) {
    if (!h) return fail("null handle");
    if (check_module("pi_infer_rollout_stochastic", h)) return 1;
    pi::StochasticArgs args;
    if (pi::check_stochastic_args("pi_infer_rollout_stochastic", h->D, epsilon, action_noise, state_noise, gamma, &args)) return 1;
    if (h->device < 0 || !h->stochastic.f_rollout) return fail("host-only handle (device = -1) cannot launch kernels");
    // a handle without a policy serves the random baseline only
    const int use_policy = h->d_policy != nullptr && epsilon != 1.0f;
    if (epsilon != 1.0f && !h->d_policy)
        return fail("pi_infer_rollout_stochastic: epsilon < 1 acts on the policy, but pi_infer_set_policy was never called");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->stochastic.f_rollout, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_start, (long long)m,
                      n_steps, gamma, (const int32_t*)h->d_policy, (const float*)h->d_actions, use_policy,
                      (const float*)h->stochastic.d_actions, h->stochastic.n_actions, h->stochastic.a_min,
                      h->stochastic.a_max, args.eps24, action_noise, args.noise, args.any_noise, (unsigned long long)seed,
                      (unsigned long long)first_episode, d_final, d_return, d_length, d_terminated,
                      traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

int pi_infer_random_words(pi_infer* h, uint64_t seed, uint64_t first_episode, int64_t m, uint32_t step, uint32_t block,
                          uint32_t* d_words, void* stream) {
    if (!h) return fail("null handle");
    if (check_module("pi_infer_random_words", h)) return 1;
    if (m < 0) return fail("m < 0");
    if (m > (INT64_MAX >> 4)) return fail("m * 16 bytes does not fit 63 bits");
    const int64_t blocks = (m + kBlock - 1) / kBlock;
    if (blocks > INT32_MAX) return fail("m is too large for one launch");
    if (h->device < 0 || !h->stochastic.f_query) return fail("host-only handle (device = -1) cannot launch kernels");
    if (m == 0) return 0;                           // nothing to do: an empty batch has no buffer either
    if (!d_words) return fail("null device pointer (d_words)");
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->stochastic.f_query, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, (unsigned long long)seed,
                      (unsigned long long)first_episode, (long long)m, (unsigned int)step, (unsigned int)block, d_words));
    return 0;
}

}  // extern "C"
