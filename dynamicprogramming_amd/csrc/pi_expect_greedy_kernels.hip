// pi_expect_greedy_kernels.hip — expected-value greedy control: the one-step lookahead on the interpolated value function
// with the expectation taken over a disturbance set, at arbitrary continuous states, as a batched query and as the
// controller of a fused closed-loop rollout that draws the stochastic rollouts' noise, for gfx950.
//
// A device-code TEMPLATE like the others; pi_expect_greedy.cpp (pi_infer_set_expect_greedy) builds the translation unit
//     <PI_EXPECT_GREEDY + PI_GREEDY + PI_STOCHASTIC + PI_D + the inference grid: PI_LO_INIT .. PI_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*        (deterministic math, as in the sweeps)
//     <the user's step_dynamics C string>                           (env plugin)
//     <csrc/pi_rollout_kernels.hip>                                 (PI_RG, pi_rollout_dynamics, pi_rollout_episodes)
//     <csrc/pi_greedy_kernels.hip>                                  (pi_greedy_expect; its kernels stay out: PI_EXPECT_GREEDY)
//     <csrc/pi_stochastic_kernels.hip>                              (pi_stochastic_draw, _noisy_action, _disturb; likewise)
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).  The interpolation, Philox, the stochastic step
// and the episode loop are those files'.
//
// Q_K(s, a) is the definition at pi_set_disturbances (include/pi_mi355.h, steps 1-5) evaluated at the point s instead of a
// grid node, per disturbance point in ascending k:
//   1. a_k = a when da_k == 0, otherwise fminf(fmaxf(a + da_k, a_min), a_max), the extremes of this module's action table
//   2. (s', r_k, done_k) = step_dynamics(s, a_k)
//   3. E_k = 0 when done_k; otherwise s'[d] += dx_k[d] for every d with dx_k[d] != 0 (one float32 add, the user's
//      dimension order — the inference grid's) and E_k = pi_greedy_expect(s')
//   4. q_k = r_k + gamma * E_k, a multiply then an add
//   5. Q = p_0 * q_0, then Q = fmaf(p_k, q_k, Q)
// The argmax is pi_greedy_kernel's: strict > from -1.0e30f over ascending action indices, index 0 with Q = -1.0e30f when
// nothing wins, NaN never wins.  With the one-point zero set (da = dx = 0, p = 1) Q is pi_greedy_q bit for bit.
//
// Work layout: one lane per query point / per episode, 256-thread workgroups, the action loop and the point loop serial
// per lane.  The table — K <= 64 rows of {da, dx_0 .. dx_{D-1}, p} — is run-time data in a device buffer of the handle:
// another set is an upload, never a build.  Its rows reach the lanes through loads at wave-uniform addresses (the loop
// counters are kernel-argument bounded) pinned to SGPRs by readfirstlane, so the branches on them — a point with the da
// of the one before it keeps that point's dynamics step (the same function on the same inputs gives the same bits); a
// zero dx is not added — are scalar branches.
// Corner values are NOT held across points: pi_greedy_expect is used as it is, its 2^D loads issued together per point.
// Holding the cell the lane looked at last (the sweeps' `held`) would keep 2^D more registers alive across the action
// loop, the point loop and, in the rollout, the step loop — 64 in 6-D on top of the figures below — and the V tables the
// controllers read sit in L2; the register budget went to occupancy instead.
//
// pi_expect_greedy_rollout_kernel runs on the shared episode loop (pi_rollout_episodes) and calls the stochastic step's
// functions (pi_stochastic_kernels.hip) around the lookahead.  Per step of a running episode, in this order:
//   1. best = argmax_a Q_K(s, a) with lookahead_gamma; a = actions[best]   (skipped by a lane that explores)
//   2. the exploration coin and the random action index of the stochastic kernel's steps 1-2: block j = 0, drawn only
//      when eps24 != 0 or action_noise != 0
//   3. its step 3: action noise, then the clamp to the table's extremes
//   4. step_dynamics(s, a) once more with the action finally taken; ret, disc, length and the freeze are the loop's.
//      With the zero set and no noise these are pi_greedy_rollout_kernel's bits
//   5. its step 5: state noise from blocks 1 and 2, the same words per dimension, not on a `done` step.
//
// Resource usage from the code objects (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage;
// tests/test_expect_greedy_host.py asserts the scratch): no scratch in any D.  VGPRs of pi_expect_greedy_kernel /
// pi_expect_greedy_rollout_kernel: 35 / 51 at 200^2 (pendulum), 59 / 84 at 50^4 (cartpole swing-up), 141 / 178 at 25^6
// (double cart-pole) and 185 / 222 at 25^6 (its swing-up) — the greedy rollout's 136 in 6-D plus the second copy of the
// plugin (the step with the action finally taken) and the stream.  Both 6-D rollouts run two waves per SIMD as the other
// 6-D rollouts do; 64 held corner values more would not fit the 256 architectural registers of that budget.

#ifndef PI_EXPECT_GREEDY
#error "pi_expect_greedy_kernels.hip is built behind #define PI_EXPECT_GREEDY 1 (pi_expect_greedy.cpp)"
#endif

#define PI_EG_BLOCK 256                      // the query kernel's; the rollout kernel runs PI_RO_BLOCK threads
#define PI_EG_ROW (PI_D + 2)                 // da | dx_0 .. dx_{D-1} | p

struct PiExpectSet {
    const float* __restrict__ rows;          // the handle's table, K rows of PI_EG_ROW floats
    int K;
    float a_min, a_max;                      // extremes of the module's action table
};

// A table entry: the address is the same in every lane, and so is the word — it can live in an SGPR.
__device__ __forceinline__ float pi_eg_word(const PiExpectSet& set, int k, int j) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(set.rows[k * PI_EG_ROW + j])));
}

// Q_K(s, a) of the header
__device__ __forceinline__ float pi_expect_greedy_q(const float (&s)[PI_D], float a, const PiExpectSet& set,
                                                    const float* __restrict__ V, float gamma) {
    float n[PI_D], reward = 0.0f, da_prev = 0.0f;
    bool done = false;
#pragma unroll
    for (int d = 0; d < PI_D; ++d) n[d] = 0.0f;
    // -0.0f + p * q is p * q for every value of the product, signed zeros and NaN included: the first point's multiply
    // and the later points' fmaf are one instruction (as in pi_expect_kernels.hip)
    float Q = -0.0f;
    for (int k = 0; k < set.K; ++k) {
        const float da = pi_eg_word(set, k, 0);
        if (k == 0 || da != da_prev) {                                   // wave-uniform
            const float ak = da == 0.0f ? a : fminf(fmaxf(a + da, set.a_min), set.a_max);
            pi_rollout_dynamics(s, ak, n, &reward, &done);
            da_prev = da;
        }
        float e = 0.0f;
        if (!done) {
            float p[PI_D];
#pragma unroll
            for (int d = 0; d < PI_D; ++d) {
                const float dx = pi_eg_word(set, k, 1 + d);
                p[d] = dx != 0.0f ? n[d] + dx : n[d];
            }
            e = pi_greedy_expect(p, V);
        }
        const float future = gamma * e;
        const float q = reward + future;
        Q = fmaf(pi_eg_word(set, k, PI_D + 1), q, Q);
    }
    return Q;
}

// argmax_a Q_K(s, a); q_row (nullable): receives Q_K(s, .)
__device__ __forceinline__ int pi_expect_greedy_argmax(const float (&s)[PI_D], const PiExpectSet& set,
                                                       const float* __restrict__ V, const float* __restrict__ actions,
                                                       int n_actions, float gamma, float* __restrict__ q_row,
                                                       float* best_q_out) {
    float best_q = -1.0e30f;
    int best = 0;
    for (int a = 0; a < n_actions; ++a) {
        const float q = pi_expect_greedy_q(s, pi_rollout_table_entry(actions, a), set, V, gamma);
        if (q_row != nullptr) q_row[a] = q;
        if (q > best_q) {
            best_q = q;
            best = a;
        }
    }
    *best_q_out = best_q;
    return best;
}

// Batched query, the outputs of pi_greedy_kernel: every one may be null: out_best (m) int32, out_action (m) =
// actions[best], out_qbest (m), out_qall (m, n_actions) row-major.
extern "C" __global__ void __launch_bounds__(PI_EG_BLOCK)
pi_expect_greedy_kernel(const float* __restrict__ points, long long m, const float* __restrict__ V,
                        const float* __restrict__ actions, int n_actions, float a_min, float a_max,
                        const float* __restrict__ dist, int K, float gamma, int* __restrict__ out_best,
                        float* __restrict__ out_action, float* __restrict__ out_qbest, float* __restrict__ out_qall) {
    const long long k = (long long)blockIdx.x * PI_EG_BLOCK + threadIdx.x;
    if (k >= m) return;
    float s[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) s[d] = points[k * PI_D + d];
    const PiExpectSet set = {dist, K, a_min, a_max};
    float* q_row = out_qall != nullptr ? out_qall + k * (long long)n_actions : nullptr;
    float best_q;
    const int best = pi_expect_greedy_argmax(s, set, V, actions, n_actions, gamma, q_row, &best_q);
    if (out_best != nullptr) out_best[k] = best;
    if (out_action != nullptr) out_action[k] = actions[best];
    if (out_qbest != nullptr) out_qbest[k] = best_q;
}

extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_expect_greedy_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma,
                                float lookahead_gamma, const float* __restrict__ V, const float* __restrict__ actions,
                                int n_actions, float a_min, float a_max, const float* __restrict__ dist, int K,
                                unsigned int eps24, float action_noise, PiStateNoise state_noise, int any_state_noise,
                                unsigned long long seed, unsigned long long first_episode,
                                float* __restrict__ out_final, float* __restrict__ out_return, int* __restrict__ out_length,
                                unsigned char* __restrict__ out_terminated, float* __restrict__ traj, int traj_every) {
    const PiExpectSet set = {dist, K, a_min, a_max};
    const bool draw_action = eps24 != 0u || action_noise != 0.0f;
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int t, long long k, float (&n)[PI_D], float& r, bool& done) {
                            const unsigned long long episode = first_episode + (unsigned long long)k;
                            const PiActionDraw draw = pi_stochastic_draw(draw_action, seed, episode, t, eps24, n_actions);
                            float a;
                            if (draw.explore) {
                                a = actions[draw.index];
                            } else {
                                float best_q;
                                a = actions[pi_expect_greedy_argmax(s, set, V, actions, n_actions, lookahead_gamma, nullptr,
                                                                    &best_q)];
                            }
                            a = pi_stochastic_noisy_action(a, action_noise, draw.noise_word, a_min, a_max);
                            pi_rollout_dynamics(s, a, n, &r, &done);
                            if (any_state_noise && !done) pi_stochastic_disturb(n, state_noise, seed, episode, t);
                        });
}
