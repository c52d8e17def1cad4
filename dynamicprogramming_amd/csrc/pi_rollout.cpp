// pi_rollout.cpp — closed-loop rollouts on the inference handle (include/pi_mi355.h, "Inference" block):
// pi_infer_set_dynamics builds the handle's second module — its grid, pi_math.h, the env plugin and
// csrc/pi_rollout_kernels.hip in one translation unit — and pi_infer_rollout runs whole episodes of a batch
// of start states in one launch.  The plugin string is kept for the third module (pi_hybrid.cpp).

#include "pi_internal.h"

#include <cstdio>
#include <sstream>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_rollout\n"
    "pi_embedded_rollout:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_rollout_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_rollout[];

using pi::fail;

int pi::check_rollout_args(int D, const float* d_start, int64_t m, int n_steps, const float* d_final, const float* d_traj,
                           int traj_every, int64_t* blocks) {
    if (m < 0) return fail("m < 0");
    if (n_steps < 0) return fail("n_steps < 0");
    if (traj_every < 0) return fail("traj_every < 0");
    if (n_steps > 0 && traj_every > n_steps) return fail("traj_every > n_steps");
    if (traj_every > 0 && !d_traj) return fail("traj_every > 0 needs a trajectory buffer (d_traj is null)");
    const int64_t rows = traj_every > 0 ? n_steps / traj_every + 1 : 1;
    int64_t per_row = 0, floats = 0;
    if (__builtin_mul_overflow(m, (int64_t)D, &per_row) || __builtin_mul_overflow(per_row, rows, &floats) ||
        floats > (INT64_MAX >> 2))
        return fail("m * rows * D does not fit 63 bits");
    if (m == 0) return 2;
    if (!d_start) return fail("null device pointer (d_start)");
    // the kernel stores states as float2 (2-D, 6-D) or float4 (4-D) per episode
    const uintptr_t align = D == 4 ? 16 : 8;
    if (((uintptr_t)d_final | (uintptr_t)d_traj) % align)
        return fail("d_final and d_traj must be aligned to " + std::to_string(align) + " bytes");
    *blocks = (m + 255) / 256;
    if (*blocks > INT32_MAX) return fail("m is too large for one launch");
    return 0;
}

extern "C" {

int pi_infer_set_dynamics(pi_infer* h, const char* dynamics_src, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h || !dynamics_src) return fail("null argument");
    std::ostringstream src;
    src << h->grid_defines;
    src << pi_embedded_math << "\n";
    src << "#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n";
    src << "// ---- env plugin (user string) ----\n";
    src << dynamics_src << "\n";
    src << "// ---- rollout kernel ----\n";
    src << pi_embedded_rollout << "\n";
    std::vector<char> image;
    if (pi::compile_image(src.str(), h->has_cache_dir ? h->cache_dir.c_str() : nullptr, log, log_len, image, nullptr)) return 1;
    if (pi::drop_hybrid(h)) return 1;               // the hybrid module holds the previous plugin
    if (pi::drop_greedy(h)) return 1;               // ... and so does the greedy one
    if (pi::drop_stochastic(h)) return 1;           // ... and the stochastic one
    if (pi::drop_expect_greedy(h)) return 1;        // ... and the expected-greedy one
    h->dynamics_src = dynamics_src;
    if (h->device < 0) {                            // host-only handle: compile check
        h->has_dynamics = true;
        return 0;
    }
    pi::DeviceGuard guard(h->device);
    if (h->module_rollout) {                        // replaced: launches already enqueued have to finish first
        PI_HIP(hipDeviceSynchronize());
        PI_HIP(hipModuleUnload(h->module_rollout));
        h->module_rollout = nullptr;
        h->f_rollout = nullptr;
        h->has_dynamics = false;
    }
    PI_HIP(hipModuleLoadData(&h->module_rollout, image.data()));
    PI_HIP(hipModuleGetFunction(&h->f_rollout, h->module_rollout, "pi_rollout_kernel"));
    h->has_dynamics = true;
    return 0;
}

int pi_infer_rollout(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float* d_final,
                     float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj, int traj_every,
                     void* stream) {
    if (!h) return fail("null handle");
    if (h->device < 0) return fail("host-only handle (device = -1) cannot launch kernels");
    if (!h->d_policy) return fail("pi_infer_rollout: pi_infer_set_policy was never called");
    if (!h->has_dynamics || !h->f_rollout) return fail("pi_infer_rollout: pi_infer_set_dynamics was never called");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->f_rollout, {(unsigned)blocks, 1}, 256, (hipStream_t)stream, d_start, (long long)m, n_steps, gamma,
                      h->d_policy, h->d_actions, d_final, d_return, d_length, d_terminated,
                      traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

}  // extern "C"
