// pi_stochastic_kernels.hip — closed-loop rollouts with a reproducible random stream inside the kernel: the random-policy
// baseline, epsilon-random actions, actuator noise and state disturbances, one launch per batch of episodes, for gfx950.
//
// A device-code TEMPLATE like the others; pi_stochastic.cpp (pi_infer_set_stochastic) builds the translation unit
//     <PI_STOCHASTIC + PI_D + the inference grid: PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*        (deterministic math, as in the sweeps)
//     <the user's step_dynamics C string>                           (env plugin)
//     <csrc/pi_rollout_kernels.hip>                                 (pi_rollout_action, pi_rollout_dynamics, pi_rollout_store_state)
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
// pi_stochastic_rollout_kernel is pi_rollout_kernel (pi_rollout_kernels.hip) — one lane per episode, the state in
// registers, the loop exit by vote, the trajectory layout and the vector stores are that kernel's — with, per step of a
// running episode, in this order:
//   1. a = the interpolated action (pi_rollout_action: the bits pi_infer_query returns); skipped without a policy
//   2. explore: a = actions[index], from the module's own action table
//   3. action_noise != 0: a = a + action_noise * sym(x2), a float32 multiply, then an add; then
//      a = fminf(fmaxf(a, a_min), a_max), the table's extremes.  No clamp when action_noise == 0
//   4. step_dynamics; ret, disc, length and the freeze exactly as in pi_rollout_kernel
//   5. not `done`: for every d with state_noise[d] != 0, s'[d] = s'[d] + state_noise[d] * sym(word d).  A dimension with
//      zero noise is not touched; the disturbed state is neither clamped nor wrapped; it is what the controller and the
//      plugin see next and what the trajectory records.  A `done` step stores its successor undisturbed.
// epsilon, action_noise and state_noise are kernel arguments: every branch on them is wave-uniform.  Block 0 is drawn
// only when eps24 != 0 or action_noise != 0, blocks 1 and 2 only when some state_noise[d] != 0, so a launch with
// everything at zero does the work of pi_rollout_kernel and returns its bits.
//
// Resource usage from the code objects (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage; tests/test_stochastic_host.py
// asserts the scratch): no scratch in any D; pi_random_words_kernel 9 VGPRs; pi_stochastic_rollout_kernel 48 VGPRs at
// 200^2 (pendulum), 77 at 50^4 (cartpole swing-up), 250 at 25^6 (double cart-pole) and 256 at 25^6 (its swing-up) —
// against 44 / 70 / 236 / 246 of pi_rollout_kernel on the same grids.  The 6-D figure is pi_rollout_action's: its fully
// unrolled 64-corner look-up holds 64 weights and 64 indices, and this kernel adds 10 to 14 registers to it.  It is above
// the greedy rollout's 136 (that kernel never calls pi_rollout_action); both 6-D rollouts run two waves per SIMD.

#ifndef PI_STOCHASTIC
#error "pi_stochastic_kernels.hip is built behind #define PI_STOCHASTIC 1 (pi_stochastic.cpp)"
#endif

#define PI_ST_BLOCK 256

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

// The expected-greedy module (pi_expect_greedy_kernels.hip) takes the functions above and leaves the two kernels out.
#ifndef PI_EXPECT_GREEDY
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

extern "C" __global__ void __launch_bounds__(PI_ST_BLOCK)
pi_stochastic_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma,
                             const int* __restrict__ policy, const float* __restrict__ policy_actions, int use_policy,
                             const float* __restrict__ actions, int n_actions, float a_min, float a_max,
                             unsigned int eps24, float action_noise, PiStateNoise state_noise, int any_state_noise,
                             unsigned long long seed, unsigned long long first_episode,
                             float* __restrict__ out_final, float* __restrict__ out_return, int* __restrict__ out_length,
                             unsigned char* __restrict__ out_terminated, float* __restrict__ traj, int traj_every) {
    const long long k = (long long)blockIdx.x * PI_ST_BLOCK + threadIdx.x;
    const bool exists = k < m;                       // lanes past the batch are frozen from the start and store nothing
    const unsigned long long episode = first_episode + (unsigned long long)k;
    float s[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) s[d] = exists ? start[k * PI_D + d] : 0.0f;
    const bool record = traj != nullptr && traj_every > 0;
    float* row = traj + k * PI_D;                    // this lane's slot of the next trajectory row (used when exists)
    const long long row_floats = m * PI_D;
    int rows_left = 0, until_row = 0;
    if (record) {
        rows_left = n_steps / traj_every;
        until_row = traj_every;
        if (exists) pi_rollout_store_state(row, s);
        row += row_floats;
    }
    const bool draw_action = eps24 != 0u || action_noise != 0.0f;
    float ret = 0.0f, disc = 1.0f;
    int length = 0;
    bool terminated = false, running = exists;
    for (int t = 0; t < n_steps && __any(running); ++t) {
        if (running) {
            float a = 0.0f;
            bool explore = false;
            PiWords w0 = {{0u, 0u, 0u, 0u}};
            if (draw_action) {
                w0 = pi_stochastic_words(seed, episode, (unsigned int)t, 0u);
                explore = (w0.x[0] >> 8) < eps24;
            }
            if (explore)
                a = actions[__umulhi(w0.x[1], (unsigned int)n_actions)];
            else if (use_policy)
                a = pi_rollout_action(PiGridFixed(), s, policy, policy_actions);
            if (action_noise != 0.0f) {
                const float push = action_noise * pi_stochastic_sym(w0.x[2]);
                a = a + push;
                a = fminf(fmaxf(a, a_min), a_max);
            }
            float n[PI_D], r;
            bool done;
            pi_rollout_dynamics(s, a, n, &r, &done);
            const float gain = disc * r;
            ret = ret + gain;
            disc = disc * gamma;
            if (any_state_noise && !done) {
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
#pragma unroll
            for (int d = 0; d < PI_D; ++d) s[d] = n[d];
            length = t + 1;
            if (done) {
                terminated = true;
                running = false;
            }
        }
        if (record && --until_row == 0) {
            if (exists) pi_rollout_store_state(row, s);
            row += row_floats;
            until_row = traj_every;
            --rows_left;
        }
    }
    // the wave left the loop early: every episode of it is frozen, the remaining rows repeat the last state
    if (record && exists)
        for (; rows_left > 0; --rows_left, row += row_floats) pi_rollout_store_state(row, s);
    if (!exists) return;
    if (out_final != nullptr) pi_rollout_store_state(out_final + k * PI_D, s);
    if (out_return != nullptr) out_return[k] = ret;
    if (out_length != nullptr) out_length[k] = length;
    if (out_terminated != nullptr) out_terminated[k] = terminated ? 1 : 0;
}
#endif  // PI_EXPECT_GREEDY
