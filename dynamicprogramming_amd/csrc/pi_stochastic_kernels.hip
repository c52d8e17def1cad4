// pi_stochastic_kernels.hip — closed-loop rollouts with a reproducible random stream inside the kernel: the random-policy
// baseline, epsilon-random actions, actuator noise and state disturbances, one launch per batch of episodes, for gfx950.
//
// A device-code TEMPLATE like the others; pi_stochastic.cpp (pi_infer_set_stochastic) builds the translation unit
//     <PI_STOCHASTIC + PI_D + the inference grid: PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*        (deterministic math, as in the sweeps)
//     <the user's step_dynamics C string>                           (env plugin)
//     <csrc/pi_rollout_kernels.hip>                                 (pi_rollout_action, pi_rollout_dynamics, pi_rollout_episodes)
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).
//
// The stream is Philox4x32-10 as published (Salmon et al., SC'11): multipliers 0xD2511F53 and 0xCD9E8D57, Weyl key
// increments 0x9E3779B9 and 0xBB67AE85, ten rounds.  It holds no state in memory: every draw is a function of
//     key     = (low, high 32 bits of the uint64 seed)
//     counter = (low, high 32 bits of e, t, j),  e = first_episode + the episode's row in the batch (uint64), t the step,
//               j the draw block
// so the results do not depend on how a batch is cut into launches, and utils/barycentric.py (philox4x32) reproduces
// them bit for bit.  The four words x0..x3 of a block:
//     j = 0   x0 exploration coin, x1 random action index, x2 action noise, x3 unused
//     j = 1   x0..x3 state noise of dimensions 0..3
//     j = 2   x0, x1 state noise of dimensions 4, 5 (6-D only)
// Two exact conversions, no transcendental anywhere:
//     sym(x)  = (float)((int)(x >> 8) - 8388608) * 2^-23, a value in [-1, 1)
//     explore iff (x0 >> 8) < eps24, eps24 = llrint(epsilon * 2^24) on the host: 0 never explores, 2^24 always does
//     index   = (uint32)(((uint64)x1 * n_actions) >> 32)
//
// pi_stochastic_rollout_kernel runs on the shared episode loop (pi_rollout_episodes, pi_rollout_kernels.hip): one lane
// per episode, the state in registers, the loop exit by vote, the trajectory layout and the outputs are the loop's.  This
// file adds the stream and, per step of a running episode, in this order:
//   1. a = the interpolated action (pi_rollout_action: the bits pi_infer_query returns); skipped without a policy
//   2. explore: a = actions[index], from the module's own action table
//   3. action_noise != 0: a = a + action_noise * sym(x2), a float32 multiply, then an add; then
//      a = fminf(fmaxf(a, a_min), a_max), the table's extremes.  No clamp when action_noise == 0
//   4. step_dynamics; ret, disc, length and the freeze are the loop's
//   5. not `done`: for every d with state_noise[d] != 0, s'[d] = s'[d] + state_noise[d] * sym(word d).  A dimension with
//      zero noise is not touched; the disturbed state is neither clamped nor wrapped; it is what the controller and the
//      plugin see next and what the trajectory records.  A `done` step stores its successor undisturbed.
// epsilon, action_noise and state_noise are kernel arguments: every branch on them is wave-uniform.  Block 0 is drawn
// only when eps24 != 0 or action_noise != 0, blocks 1 and 2 only when some state_noise[d] != 0, so a launch with
// everything at zero does the work of pi_rollout_kernel and returns its bits.
//
// Resource usage from the code objects (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; tests/test_stochastic_host.py
// asserts the scratch): no scratch in any D; pi_random_words_kernel 9 VGPRs; pi_stochastic_rollout_kernel 50 VGPRs at
// 200^2 (pendulum), 81 at 50^4 (cartpole swing-up), 253 at 25^6 (double cart-pole) and 256 at 25^6 (its swing-up) —
// against 46 / 71 / 238 / 250 of pi_rollout_kernel on the same grids.  The 6-D figure is pi_rollout_action's: its fully
// unrolled 64-corner look-up holds 64 weights and 64 indices, and this kernel adds 6 to 15 registers to it.  It is above
// the greedy rollout's 136 (that kernel never calls pi_rollout_action); both 6-D rollouts run two waves per SIMD.

#ifndef PI_STOCHASTIC
#error "pi_stochastic_kernels.hip is built behind #define PI_STOCHASTIC 1 (pi_stochastic.cpp)"
#endif

#define PI_ST_BLOCK 256                      // the words kernel's; the rollout kernel runs PI_RO_BLOCK threads

// state_noise as a kernel argument: six floats whatever D is (the host launches one layout), entries past D are zero
struct PiStateNoise {
    float v[6];
};

struct PiWords {
    unsigned int x[4];
};

__device__ __forceinline__ PiWords pi_philox4x32(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                                 unsigned int k0, unsigned int k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned int hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned int hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// the draw block j of episode e at step t
__device__ __forceinline__ PiWords pi_stochastic_words(unsigned long long seed, unsigned long long e, unsigned int t,
                                                       unsigned int j) {
    return pi_philox4x32((unsigned int)e, (unsigned int)(e >> 32), t, j, (unsigned int)seed, (unsigned int)(seed >> 32));
}

// a word as a float32 in [-1, 1): 24 bits, every value exact
__device__ __forceinline__ float pi_stochastic_sym(unsigned int x) {
    return (float)((int)(x >> 8) - 8388608) * 0x1p-23f;
}

// Block 0 of a step (header): whether the episode explores, the table index it then takes and the action-noise word.
// Drawn only when `draw` (eps24 != 0 or action_noise != 0, wave-uniform); nothing explores otherwise.
struct PiActionDraw {
    bool explore;
    unsigned int index, noise_word;
};
__device__ __forceinline__ PiActionDraw pi_stochastic_draw(bool draw, unsigned long long seed, unsigned long long episode,
                                                           int t, unsigned int eps24, int n_actions) {
    PiWords w0 = {{0u, 0u, 0u, 0u}};
    if (draw) w0 = pi_stochastic_words(seed, episode, (unsigned int)t, 0u);
    return {draw && (w0.x[0] >> 8) < eps24, __umulhi(w0.x[1], (unsigned int)n_actions), w0.x[2]};
}

// step 3 of the header: action noise, a multiply, then an add, then the clamp to the table's extremes; a untouched
// when action_noise == 0
__device__ __forceinline__ float pi_stochastic_noisy_action(float a, float action_noise, unsigned int noise_word,
                                                            float a_min, float a_max) {
    if (action_noise != 0.0f) {
        const float push = action_noise * pi_stochastic_sym(noise_word);
        a = a + push;
        a = fminf(fmaxf(a, a_min), a_max);
    }
    return a;
}

// step 5 of the header: the successor n of a step that is not `done`, disturbed from blocks 1 and 2 in every dimension
// with state_noise[d] != 0
__device__ __forceinline__ void pi_stochastic_disturb(float (&n)[PI_D], const PiStateNoise& state_noise,
                                                      unsigned long long seed, unsigned long long episode, int t) {
    const PiWords w1 = pi_stochastic_words(seed, episode, (unsigned int)t, 1u);
#pragma unroll
    for (int d = 0; d < (PI_D < 4 ? PI_D : 4); ++d)
        if (state_noise.v[d] != 0.0f) {
            const float push = state_noise.v[d] * pi_stochastic_sym(w1.x[d]);
            n[d] = n[d] + push;
        }
#if PI_D == 6
    if (state_noise.v[4] != 0.0f || state_noise.v[5] != 0.0f) {
        const PiWords w2 = pi_stochastic_words(seed, episode, (unsigned int)t, 2u);
#pragma unroll
        for (int d = 4; d < 6; ++d)
            if (state_noise.v[d] != 0.0f) {
                const float push = state_noise.v[d] * pi_stochastic_sym(w2.x[d - 4]);
                n[d] = n[d] + push;
            }
    }
#endif
}

// The expected-greedy module (pi_expect_greedy_kernels.hip) and the stochastic hybrid module
// (pi_hybrid_stochastic_kernels.hip) take the functions above and leave the two kernels out.
#if !defined(PI_EXPECT_GREEDY) && !defined(PI_HYBRID_STOCHASTIC)
// Probe: the four words of (seed, first_episode + row, step, block) for rows 0 .. m, out (m, 4) uint32.
extern "C" __global__ void __launch_bounds__(PI_ST_BLOCK)
pi_random_words_kernel(unsigned long long seed, unsigned long long first_episode, long long m, unsigned int step,
                       unsigned int block, unsigned int* __restrict__ out) {
    const long long k = (long long)blockIdx.x * PI_ST_BLOCK + threadIdx.x;
    if (k >= m) return;
    const PiWords w = pi_stochastic_words(seed, first_episode + (unsigned long long)k, step, block);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[k * 4 + i] = w.x[i];
}

extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_stochastic_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma,
                             const int* __restrict__ policy, const float* __restrict__ policy_actions, int use_policy,
                             const float* __restrict__ actions, int n_actions, float a_min, float a_max,
                             unsigned int eps24, float action_noise, PiStateNoise state_noise, int any_state_noise,
                             unsigned long long seed, unsigned long long first_episode,
                             float* __restrict__ out_final, float* __restrict__ out_return, int* __restrict__ out_length,
                             unsigned char* __restrict__ out_terminated, float* __restrict__ traj, int traj_every) {
    const bool draw_action = eps24 != 0u || action_noise != 0.0f;
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int t, long long k, float (&n)[PI_D], float& r, bool& done) {
                            const unsigned long long episode = first_episode + (unsigned long long)k;
                            const PiActionDraw draw = pi_stochastic_draw(draw_action, seed, episode, t, eps24, n_actions);
                            float a = 0.0f;
                            if (draw.explore)
                                a = actions[draw.index];
                            else if (use_policy)
                                a = pi_rollout_action(PiGridFixed(), s, policy, policy_actions);
                            a = pi_stochastic_noisy_action(a, action_noise, draw.noise_word, a_min, a_max);
                            pi_rollout_dynamics(s, a, n, &r, &done);
                            if (any_state_noise && !done) pi_stochastic_disturb(n, state_noise, seed, episode, t);
                        });
}
#endif  // PI_EXPECT_GREEDY, PI_HYBRID_STOCHASTIC
