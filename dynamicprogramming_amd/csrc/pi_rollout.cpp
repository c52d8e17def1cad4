// pi_rollout.cpp — closed-loop rollouts on the inference handle (include/pi_mi355.h, "Inference" block):
// pi_infer_set_dynamics builds the handle's rollout module — its grid, pi_math.h, the env plugin and
// csrc/pi_rollout_kernels.hip in one translation unit — and pi_infer_rollout runs whole episodes of a batch
// of start states in one launch.  The plugin string is kept for the modules of the other controllers, and what all of
// them share on the host lives here: the unit builder, the action-table rules, unloading and installing a module.

#include "pi_internal.h"

#include <cmath>
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

int pi::build_infer_module(const pi_infer* h, const std::string& leading, const std::string& plugin,
                           std::initializer_list<UnitPart> parts, char* log, size_t log_len, std::vector<char>& image) {
    std::ostringstream src;
    src << leading;
    src << pi_embedded_math << "\n";
    src << "#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n";
    src << "// ---- env plugin (user string) ----\n";
    src << plugin << "\n";
    for (const UnitPart& part : parts) src << "// ---- " << part.section << " ----\n" << part.text << "\n";
    return pi::compile_image(src.str(), h->has_cache_dir ? h->cache_dir.c_str() : nullptr, log, log_len, image, nullptr);
}

int pi::check_action_table(const char* who, bool finite, const float* action_space, int n_actions, ActionTable* table) {
    if (!action_space) return fail("null argument (action_space)");
    if (n_actions < 1) return fail("need at least one action");
    *table = {action_space, n_actions, action_space[0], action_space[0]};
    for (int i = 0; i < n_actions; ++i) {
        if (finite && !std::isfinite(action_space[i]))
            return fail(std::string(who) + ": action_space[" + std::to_string(i) + "] is not finite");
        table->a_min = std::fmin(table->a_min, action_space[i]);
        table->a_max = std::fmax(table->a_max, action_space[i]);
    }
    return 0;
}

int pi::unload(pi_infer* h, InferModule& mod) {
    if (mod.module) {                               // launches already enqueued have to finish first
        pi::DeviceGuard guard(h->device);
        PI_HIP(hipDeviceSynchronize());
        PI_HIP(hipModuleUnload(mod.module));
    }
    mod.module = nullptr;
    mod.f_rollout = mod.f_query = nullptr;
    mod.ready = false;
    return 0;
}

int pi::install(pi_infer* h, InferModule& mod, const std::vector<char>& image, const ActionTable* table,
                const char* rollout, const char* query) {
    if (pi::unload(h, mod)) return 1;
    if (h->device >= 0) {
        pi::DeviceGuard guard(h->device);
        if (table) {                                // unload has waited for the launches that read the previous table
            if (mod.d_actions) { (void)hipFree(mod.d_actions); mod.d_actions = nullptr; }
            PI_HIP(hipMalloc((void**)&mod.d_actions, (size_t)table->n * sizeof(float)));
            PI_HIP(hipMemcpy(mod.d_actions, table->values, (size_t)table->n * sizeof(float), hipMemcpyHostToDevice));
        }
        PI_HIP(hipModuleLoadData(&mod.module, image.data()));
        PI_HIP(hipModuleGetFunction(&mod.f_rollout, mod.module, rollout));
        if (query) PI_HIP(hipModuleGetFunction(&mod.f_query, mod.module, query));
    }
    if (table) {
        mod.n_actions = table->n;
        mod.a_min = table->a_min;
        mod.a_max = table->a_max;
    }
    mod.ready = true;
    return 0;
}

extern "C" {

int pi_infer_set_dynamics(pi_infer* h, const char* dynamics_src, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h || !dynamics_src) return fail("null argument");
    std::vector<char> image;
    if (pi::build_infer_module(h, h->grid_defines, dynamics_src, {{"rollout kernel", pi_embedded_rollout}}, log, log_len, image))
        return 1;
    for (pi::InferModule* mod : {&h->hybrid, &h->greedy, &h->stochastic, &h->expect_greedy, &h->hybrid_stochastic, &h->robust})   // they hold the previous plugin
        if (pi::unload(h, *mod)) return 1;
    h->dynamics_src = dynamics_src;
    return pi::install(h, h->rollout, image, nullptr, "pi_rollout_kernel", nullptr);
}

int pi_infer_rollout(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float* d_final,
                     float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj, int traj_every,
                     void* stream) {
    if (!h) return fail("null handle");
    if (h->device < 0) return fail("host-only handle (device = -1) cannot launch kernels");
    if (!h->d_policy) return fail("pi_infer_rollout: pi_infer_set_policy was never called");
    if (!h->rollout.ready || !h->rollout.f_rollout) return fail("pi_infer_rollout: pi_infer_set_dynamics was never called");
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->rollout.f_rollout, {(unsigned)blocks, 1}, 256, (hipStream_t)stream, d_start, (long long)m, n_steps, gamma,
                      h->d_policy, h->d_actions, d_final, d_return, d_length, d_terminated,
                      traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

}  // extern "C"
