// pi_stochastic.cpp — stochastic rollouts on the inference handle (include/pi_mi355.h, "Inference" block): the
// random-policy baseline, epsilon-random actions, action noise and state noise from a counter-based random stream
// (Philox4x32-10 keyed by seed, episode and step) inside the rollout kernel.  pi_infer_set_stochastic uploads the action
// table and builds the handle's sixth module — its grid, pi_math.h, the plugin pi_infer_set_dynamics was given, the
// helpers of csrc/pi_rollout_kernels.hip and csrc/pi_stochastic_kernels.hip in one translation unit;
// pi_infer_rollout_stochastic runs whole episodes of a batch of start states in one launch and pi_infer_random_words
// reads the stream itself.

#include "pi_internal.h"

#include <cmath>
#include <sstream>

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

constexpr int kBlock = 256;               // PI_ST_BLOCK

struct StateNoise {                       // PiStateNoise
    float v[6];
};

// what both launching entry points refuse about the handle
int check_module(const char* who, const pi_infer* h) {
    if (!h->has_stochastic)
        return fail(std::string(who) +
                    ": no stochastic module: call pi_infer_set_stochastic (again after every pi_infer_set_dynamics)");
    return 0;
}

}  // namespace

int pi::drop_stochastic(pi_infer* h) {
    if (h->module_stochastic) {                     // launches already enqueued have to finish first
        pi::DeviceGuard guard(h->device);
        PI_HIP(hipDeviceSynchronize());
        PI_HIP(hipModuleUnload(h->module_stochastic));
    }
    h->module_stochastic = nullptr;
    h->f_stochastic_rollout = nullptr;
    h->f_random_words = nullptr;
    h->has_stochastic = false;
    return 0;
}

extern "C" {

int pi_infer_set_stochastic(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h) return fail("null handle");
    if (!action_space) return fail("null argument (action_space)");
    if (n_actions < 1) return fail("need at least one action");
    float a_min = action_space[0], a_max = action_space[0];
    for (int i = 0; i < n_actions; ++i) {
        if (!std::isfinite(action_space[i]))
            return fail("pi_infer_set_stochastic: action_space[" + std::to_string(i) + "] is not finite");
        a_min = std::fmin(a_min, action_space[i]);
        a_max = std::fmax(a_max, action_space[i]);
    }
    if (!h->has_dynamics) return fail("pi_infer_set_stochastic: pi_infer_set_dynamics was never called");
    std::ostringstream src;
    src << "#define PI_STOCHASTIC 1\n";
    src << h->grid_defines;
    src << pi_embedded_math << "\n";
    src << "#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n";
    src << "// ---- env plugin (user string) ----\n";
    src << h->dynamics_src << "\n";
    src << "// ---- rollout helpers ----\n";
    src << pi_embedded_rollout << "\n";
    src << "// ---- stochastic kernels ----\n";
    src << pi_embedded_stochastic << "\n";
    std::vector<char> image;
    if (pi::compile_image(src.str(), h->has_cache_dir ? h->cache_dir.c_str() : nullptr, log, log_len, image, nullptr)) return 1;
    if (pi::drop_stochastic(h)) return 1;
    if (h->device >= 0) {
        pi::DeviceGuard guard(h->device);
        // drop_stochastic has waited for the launches that read the previous table, if there was one
        if (h->d_stochastic_actions) { (void)hipFree(h->d_stochastic_actions); h->d_stochastic_actions = nullptr; }
        PI_HIP(hipMalloc((void**)&h->d_stochastic_actions, (size_t)n_actions * sizeof(float)));
        PI_HIP(hipMemcpy(h->d_stochastic_actions, action_space, (size_t)n_actions * sizeof(float), hipMemcpyHostToDevice));
        PI_HIP(hipModuleLoadData(&h->module_stochastic, image.data()));
        PI_HIP(hipModuleGetFunction(&h->f_stochastic_rollout, h->module_stochastic, "pi_stochastic_rollout_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_random_words, h->module_stochastic, "pi_random_words_kernel"));
    }
    h->n_stochastic_actions = n_actions;
    h->stochastic_a_min = a_min;
    h->stochastic_a_max = a_max;
    h->has_stochastic = true;
    return 0;
}

int pi_infer_rollout_stochastic(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float epsilon,
                                float action_noise, const float* state_noise, uint64_t seed, uint64_t first_episode,
                                float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj,
                                int traj_every, void* stream) {
    if (!h) return fail("null handle");
    if (check_module("pi_infer_rollout_stochastic", h)) return 1;
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail("pi_infer_rollout_stochastic: epsilon must lie in [0, 1]");
    if (!(action_noise >= 0.0f) || !std::isfinite(action_noise))
        return fail("pi_infer_rollout_stochastic: action_noise must be finite and not negative");
    StateNoise noise = {};
    int any_noise = 0;
    for (int d = 0; state_noise && d < h->D; ++d) {
        if (!(state_noise[d] >= 0.0f) || !std::isfinite(state_noise[d]))
            return fail("pi_infer_rollout_stochastic: state_noise[" + std::to_string(d) + "] must be finite and not negative");
        noise.v[d] = state_noise[d];
        any_noise |= state_noise[d] != 0.0f;
    }
    if (std::isnan(gamma)) return fail("pi_infer_rollout_stochastic: gamma is NaN");
    if (h->device < 0 || !h->f_stochastic_rollout) return fail("host-only handle (device = -1) cannot launch kernels");
    // a handle without a policy serves the random baseline only
    const int use_policy = h->d_policy != nullptr && epsilon != 1.0f;
    if (epsilon != 1.0f && !h->d_policy)
        return fail("pi_infer_rollout_stochastic: epsilon < 1 acts on the policy, but pi_infer_set_policy was never called");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    const unsigned int eps24 = (unsigned int)std::llrint((double)epsilon * 16777216.0);
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->f_stochastic_rollout, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, d_start, (long long)m,
                      n_steps, gamma, (const int32_t*)h->d_policy, (const float*)h->d_actions, use_policy,
                      (const float*)h->d_stochastic_actions, h->n_stochastic_actions, h->stochastic_a_min,
                      h->stochastic_a_max, eps24, action_noise, noise, any_noise, (unsigned long long)seed,
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
    if (h->device < 0 || !h->f_random_words) return fail("host-only handle (device = -1) cannot launch kernels");
    if (m == 0) return 0;                           // nothing to do: an empty batch has no buffer either
    if (!d_words) return fail("null device pointer (d_words)");
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->f_random_words, {(unsigned)blocks, 1}, kBlock, (hipStream_t)stream, (unsigned long long)seed,
                      (unsigned long long)first_episode, (long long)m, (unsigned int)step, (unsigned int)block, d_words));
    return 0;
}

}  // extern "C"
