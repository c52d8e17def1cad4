// pi_hybrid.cpp — closed-loop rollouts that switch between two inference handles (include/pi_mi355.h, "Inference"
// block): pi_infer_set_partner builds the primary handle's hybrid module — its grid, the partner's grid, pi_math.h,
// the plugin pi_infer_set_dynamics was given, csrc/pi_rollout_kernels.hip (the shared interpolation) and
// csrc/pi_hybrid_kernels.hip in one translation unit — and pi_infer_rollout_hybrid runs whole episodes of a batch of
// start states in one launch.  The same pair in a noisy world: pi_infer_set_partner_stochastic builds the stochastic
// hybrid module — the same unit plus the functions of csrc/pi_stochastic_kernels.hip and
// csrc/pi_hybrid_stochastic_kernels.hip — with the pair's exploration table, and pi_infer_rollout_hybrid_stochastic
// launches it.

#include "pi_internal.h"

#include <cmath>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_hybrid\n"
    "pi_embedded_hybrid:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_hybrid_kernels.hip\"\n"
    ".byte 0\n"
    ".global pi_embedded_hybrid_stochastic\n"
    "pi_embedded_hybrid_stochastic:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_hybrid_stochastic_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_hybrid[];
extern "C" const char pi_embedded_hybrid_stochastic[];

using pi::fail;

namespace {

struct HybridBox {                     // PiHybridBox of pi_hybrid_kernels.hip
    float enter[6], leave[6];
};

// the partner's grid as the SECOND set of defines: PI_D -> PI2_D, PI_LO_INIT -> PI2_LO_INIT, ...
std::string second_defines(const std::string& defines) {
    std::string out;
    const std::string from = "#define PI_", to = "#define PI2_";
    size_t at = 0;
    for (size_t hit; (hit = defines.find(from, at)) != std::string::npos; at = hit + from.size()) {
        out.append(defines, at, hit - at);
        out += to;
    }
    out.append(defines, at, std::string::npos);
    return out;
}

// both grids of a hybrid unit, the primary's first
std::string pair_defines(const pi_infer* h, const pi_infer* partner) {
    return h->grid_defines + "// ---- secondary grid ----\n" + second_defines(partner->grid_defines);
}

// what every entry point refuses about the pair
int check_pair(const char* who, const pi_infer* h, const pi_infer* partner) {
    const std::string w = std::string(who) + ": ";
    if (h->device != partner->device)
        return fail(w + "the handles are on different devices (" + std::to_string(h->device) + " and " +
                    std::to_string(partner->device) + ")");
    if (h->D != partner->D)
        return fail(w + "the handles differ in D (" + std::to_string(h->D) + " and " + std::to_string(partner->D) + ")");
    if (h->corner_bits != partner->corner_bits)
        return fail(w + "the handles differ in their corner_bits tables (the kernel walks one corner order for both grids)");
    return 0;
}

// What both launching entry points refuse before they look at the batch, in three parts (each call orders them so that
// what it can refuse without a device comes first).  The handles: both on a device
int check_on_device(const pi_infer* h, const pi_infer* partner) {
    if (h->device < 0 || partner->device < 0) return fail("host-only handle (device = -1) cannot launch kernels");
    return 0;
}

// ... the policies of both handles and the plugin
int check_policies(const char* who, const pi_infer* h, const pi_infer* partner) {
    const std::string w = std::string(who) + ": ";
    if (!h->d_policy) return fail(w + "pi_infer_set_policy was never called on the primary handle");
    if (!partner->d_policy) return fail(w + "pi_infer_set_policy was never called on the partner");
    if (!h->rollout.ready) return fail(w + "pi_infer_set_dynamics was never called on the primary handle");
    return 0;
}

// ... the module `mod` (built by the call `builder` for the partner grid `built_for`) and the switch box, copied into *box
int check_module_and_box(const char* who, const pi_infer* h, const pi_infer* partner, const pi::InferModule& mod,
                         const std::string& built_for, const char* builder, const float* enter, const float* leave,
                         HybridBox* box) {
    const std::string w = std::string(who) + ": ";
    if (!mod.ready)
        return fail(w + "no hybrid module: call " + builder + " (again after every pi_infer_set_dynamics)");
    if (partner->grid_defines != built_for)
        return fail(w + "the hybrid module was built for another partner grid: call " + builder + " with this partner");
    if (!enter || !leave) return fail("null argument (enter / leave)");
    *box = {};
    for (int d = 0; d < h->D; ++d) {
        if (std::isnan(enter[d]) || std::isnan(leave[d])) return fail(w + "threshold " + std::to_string(d) + " is NaN");
        if (enter[d] > leave[d])
            return fail(w + "enter[" + std::to_string(d) + "] > leave[" + std::to_string(d) +
                        "]: the box to enter must lie inside the box to leave");
        box->enter[d] = enter[d];
        box->leave[d] = leave[d];
    }
    return 0;
}

}  // namespace

extern "C" {

int pi_infer_set_partner(pi_infer* h, pi_infer* partner, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h || !partner) return fail("null handle");
    if (check_pair("pi_infer_set_partner", h, partner)) return 1;
    if (!h->rollout.ready) return fail("pi_infer_set_partner: pi_infer_set_dynamics was never called on the primary handle");
    std::vector<char> image;
    if (pi::build_infer_module(h, "#define PI_HYBRID 1\n" + pair_defines(h, partner), h->dynamics_src,
                               {{"rollout helpers", pi_embedded_rollout}, {"hybrid rollout kernel", pi_embedded_hybrid}},
                               log, log_len, image))
        return 1;
    if (pi::install(h, h->hybrid, image, nullptr, "pi_hybrid_rollout_kernel", nullptr)) return 1;
    h->partner_defines = partner->grid_defines;
    return 0;
}

int pi_infer_rollout_hybrid(pi_infer* h, pi_infer* partner, const float* d_start, int64_t m, int n_steps, float gamma,
                            const float* enter, const float* leave, float* d_final, float* d_return, int32_t* d_length,
                            uint8_t* d_terminated, int32_t* d_secondary_steps, uint8_t* d_last_mode, float* d_traj,
                            int traj_every, void* stream) {
    if (!h || !partner) return fail("null handle");
    const char* who = "pi_infer_rollout_hybrid";
    HybridBox box;
    if (check_on_device(h, partner) || check_pair(who, h, partner) || check_policies(who, h, partner) ||
        check_module_and_box(who, h, partner, h->hybrid, h->partner_defines, "pi_infer_set_partner", enter, leave, &box))
        return 1;
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(h->hybrid.f_rollout, {(unsigned)blocks, 1}, 256, (hipStream_t)stream, d_start, (long long)m, n_steps, gamma,
                      (const int32_t*)h->d_policy, (const float*)h->d_actions, (const int32_t*)partner->d_policy,
                      (const float*)partner->d_actions, box, d_final, d_return, d_length, d_terminated, d_secondary_steps,
                      d_last_mode, traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

int pi_infer_set_partner_stochastic(pi_infer* h, pi_infer* partner, const float* action_space, int n_actions, char* log,
                                    size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h || !partner) return fail("null handle");
    if (check_pair("pi_infer_set_partner_stochastic", h, partner)) return 1;
    pi::ActionTable table;
    if (pi::check_action_table("pi_infer_set_partner_stochastic", true, action_space, n_actions, &table)) return 1;
    if (!h->rollout.ready)
        return fail("pi_infer_set_partner_stochastic: pi_infer_set_dynamics was never called on the primary handle");
    std::vector<char> image;
    if (pi::build_infer_module(h, "#define PI_HYBRID_STOCHASTIC 1\n#define PI_HYBRID 1\n#define PI_STOCHASTIC 1\n" +
                                      pair_defines(h, partner),
                               h->dynamics_src,
                               {{"rollout helpers", pi_embedded_rollout}, {"hybrid functions", pi_embedded_hybrid},
                                {"stochastic functions", pi_embedded_stochastic},
                                {"stochastic hybrid rollout kernel", pi_embedded_hybrid_stochastic}},
                               log, log_len, image))
        return 1;
    if (pi::install(h, h->hybrid_stochastic, image, &table, "pi_hybrid_stochastic_rollout_kernel", nullptr)) return 1;
    h->partner_stochastic_defines = partner->grid_defines;
    return 0;
}

int pi_infer_rollout_hybrid_stochastic(pi_infer* h, pi_infer* partner, const float* d_start, int64_t m, int n_steps,
                                       float gamma, const float* enter, const float* leave, float epsilon,
                                       float action_noise, const float* state_noise, uint64_t seed, uint64_t first_episode,
                                       float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated,
                                       int32_t* d_secondary_steps, uint8_t* d_last_mode, int32_t* d_switches, float* d_traj,
                                       int traj_every, void* stream) {
    const char* who = "pi_infer_rollout_hybrid_stochastic";
    if (!h || !partner) return fail("null handle");
    const pi::InferModule& mod = h->hybrid_stochastic;
    HybridBox box;
    if (check_pair(who, h, partner) ||
        check_module_and_box(who, h, partner, mod, h->partner_stochastic_defines, "pi_infer_set_partner_stochastic", enter,
                             leave, &box))
        return 1;
    pi::StochasticArgs args;
    if (pi::check_stochastic_args(who, h->D, epsilon, action_noise, state_noise, gamma, &args)) return 1;
    // both policies whatever epsilon is: a launch at epsilon = 1 reads neither, but the pair is one controller
    if (check_on_device(h, partner) || check_policies(who, h, partner)) return 1;
    int64_t blocks = 0;
    if (const int rc = pi::check_rollout_args(h->D, d_start, m, n_steps, d_final, d_traj, traj_every, &blocks)) return rc == 2 ? 0 : 1;
    pi::DeviceGuard guard(h->device);
    PI_HIP(pi::launch(mod.f_rollout, {(unsigned)blocks, 1}, 256, (hipStream_t)stream, d_start, (long long)m, n_steps, gamma,
                      (const int32_t*)h->d_policy, (const float*)h->d_actions, (const int32_t*)partner->d_policy,
                      (const float*)partner->d_actions, box, (const float*)mod.d_actions, mod.n_actions, mod.a_min, mod.a_max,
                      args.eps24, action_noise, args.noise, args.any_noise, (unsigned long long)seed,
                      (unsigned long long)first_episode, d_final, d_return, d_length, d_terminated, d_secondary_steps,
                      d_last_mode, d_switches, traj_every > 0 ? d_traj : (float*)nullptr, traj_every));
    return 0;
}

}  // extern "C"
