// pi_hybrid_stochastic_kernels.hip — closed-loop rollouts that switch between TWO policies in a noisy world: the hybrid
// rollout (pi_hybrid_kernels.hip) with the stream of the stochastic rollouts (pi_stochastic_kernels.hip) inside, one launch
// per batch of episodes, for gfx950 (include/pi_mi355.h, pi_infer_rollout_hybrid_stochastic).
//
// A device-code TEMPLATE like the others; pi_hybrid_stochastic.cpp (pi_infer_set_partner_stochastic) builds the
// translation unit
//     <#define PI_HYBRID_STOCHASTIC, PI_HYBRID, PI_STOCHASTIC>
//     <the primary grid PI_* and the secondary grid PI2_*, as in the hybrid module>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*
//     <the primary handle's step_dynamics C string>
//     <pi_rollout_kernels.hip>      the interpolation, the dynamics call, the episode loop
//     <pi_hybrid_kernels.hip>       PiGridPick, PiHybridBox (its kernel stays out: PI_HYBRID_STOCHASTIC)
//     <pi_stochastic_kernels.hip>   pi_stochastic_draw, _noisy_action, _disturb (its kernels likewise)
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).
//
// The episode loop is pi_rollout_episodes; this file adds the mode, its two counters and the stream.  Per step of a
// running episode, in this order:
//   1. the mode, pi_hybrid_rollout_kernel's rule (float32, strict comparisons, mode 0 before step 0) on the state the
//      step starts from — which the step before may have disturbed — on every step taken, exploring or not;
//      secondary_steps += mode; switches += 1 when the mode differs from that of the step taken before (before step 0
//      the mode is 0: an episode that enters at step 0 counts one)
//   2. block 0 of the stream, drawn only when eps24 != 0 or action_noise != 0; the exploration coin as in the
//      stochastic rollouts.  It is drawn AFTER the mode rule, which keeps its words out of the rule's live range
//   3. the action: an exploring step takes table[index] from the module's ONE exploration table (one plant, one
//      actuator); any other step interpolates the mode's policy on its own grid, pi_rollout_action(PiGridPick{mode}) —
//      once for a mixed-mode wave; an exploring lane does not interpolate
//   4. action_noise != 0: a = a + action_noise * sym(x2), a multiply, then an add, then the clamp to the extremes of the
//      exploration table; no clamp when action_noise == 0
//   5. step_dynamics (the primary's plugin); return, discount, length and the freeze are the loop's
//   6. not `done`: the state noise of blocks 1 and 2 as in the stochastic rollouts, neither clamped nor wrapped; it is
//      what is recorded and what the next step's mode rule sees.
// eps24, action_noise and state_noise are kernel arguments: every branch on them is wave-uniform.  The mode, the two
// counters and the state stay in registers for all steps.  With all noise at zero the outputs are
// pi_hybrid_rollout_kernel's; with enter = 0 they are pi_stochastic_rollout_kernel's on the primary.
//
// Resource usage from the code objects (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage;
// tests/test_hybrid_stochastic_host.py asserts the scratch): no scratch in any D.  VGPRs of
// pi_hybrid_stochastic_rollout_kernel: 70 at pendulum 200^2 + 50^2, 102 at cartpole swing-up 50^4 + 30^4 and 256 at
// double cart-pole swing-up 25^6 + double cart-pole 25^6 — against 58 / 82 / 226 of pi_hybrid_rollout_kernel on the same
// pairs.  The 6-D figure is pi_rollout_action's 64 weights and 64 indices, as in the other 6-D rollouts (the
// single-policy stochastic kernel holds 253 to 256 there); 256 is the most two waves per SIMD allow, which is what every
// 6-D rollout of the handle runs at, so the kernel fits that budget exactly and has nothing to spare in it.

#ifndef PI_HYBRID_STOCHASTIC
#error "pi_hybrid_stochastic_kernels.hip is built behind #define PI_HYBRID_STOCHASTIC 1 (pi_hybrid_stochastic.cpp)"
#endif

extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_hybrid_stochastic_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma,
                                    const int* __restrict__ policy0, const float* __restrict__ actions0,
                                    const int* __restrict__ policy1, const float* __restrict__ actions1, PiHybridBox box,
                                    const float* __restrict__ table, int n_actions, float a_min, float a_max,
                                    unsigned int eps24, float action_noise, PiStateNoise state_noise, int any_state_noise,
                                    unsigned long long seed, unsigned long long first_episode,
                                    float* __restrict__ out_final, float* __restrict__ out_return,
                                    int* __restrict__ out_length, unsigned char* __restrict__ out_terminated,
                                    int* __restrict__ out_secondary, unsigned char* __restrict__ out_last_mode,
                                    int* __restrict__ out_switches, float* __restrict__ traj, int traj_every) {
    const bool draw_action = eps24 != 0u || action_noise != 0.0f;
    int secondary = 0, switches = 0;
    bool second = false;                             // the mode; it changes on steps taken only, so it ends as last_mode
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int t, long long k, float (&n)[PI_D], float& r, bool& done) {
                            bool inside = true, outside = false;
#pragma unroll
                            for (int d = 0; d < PI_D; ++d) {
                                const float mag = fabsf(s[d]);
                                inside = inside && mag < box.enter[d];
                                outside = outside || mag > box.leave[d];
                            }
                            const bool now = second ? !outside : inside;
                            switches += now != second ? 1 : 0;
                            second = now;
                            secondary += second ? 1 : 0;
                            const unsigned long long episode = first_episode + (unsigned long long)k;
                            const PiActionDraw draw = pi_stochastic_draw(draw_action, seed, episode, t, eps24, n_actions);
                            float a;
                            if (draw.explore)
                                a = table[draw.index];
                            else
                                a = pi_rollout_action(PiGridPick{second}, s, second ? policy1 : policy0,
                                                      second ? actions1 : actions0);
                            a = pi_stochastic_noisy_action(a, action_noise, draw.noise_word, a_min, a_max);
                            pi_rollout_dynamics(s, a, n, &r, &done);
                            if (any_state_noise && !done) pi_stochastic_disturb(n, state_noise, seed, episode, t);
                        });
    const long long k = pi_rollout_lane();
    if (k >= m) return;
    if (out_secondary != nullptr) out_secondary[k] = secondary;
    if (out_last_mode != nullptr) out_last_mode[k] = second ? 1 : 0;
    if (out_switches != nullptr) out_switches[k] = switches;
}
