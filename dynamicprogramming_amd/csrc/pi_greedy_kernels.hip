// pi_greedy_kernels.hip — value-greedy control: the one-step lookahead on the interpolated value function at
// arbitrary continuous states, as a batched query and as the controller of a fused closed-loop rollout, for gfx950.
//
// A device-code TEMPLATE like the others; pi_greedy.cpp (pi_infer_set_greedy) builds the translation unit
//     <PI_GREEDY + PI_D + the inference grid: PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*        (deterministic math, as in the sweeps)
//     <the user's step_dynamics C string>                           (env plugin)
//     <csrc/pi_rollout_kernels.hip>                                 (PI_RG, pi_rollout_dynamics, pi_rollout_episodes)
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).
//
// Q(s, a) is the backup of the sweeps (oracle/pi_oracle.cpp, backup()) evaluated at the point s
// instead of a grid node, bit for bit — NOT the arithmetic of pi_infer_kernel:
//   1. (s', r, done) = step_dynamics(s, a) with the arity for D
//   2. done: E = 0.  Otherwise per dimension, in the user's order:
//        n = (s' - lo) / (hi - lo) * (float)(g - 1)      float32: an IEEE division, then a multiply
//        n = fmaxf(0, fminf(n, g - 1));  i = min((int)n, g - 2);  frac = n - (float)i
//   3. corner c takes bit d of c for dimension d; in 2-D dimension 1 toggles fastest (the oracle's corner_bit — the
//      handle's corner_bits table plays no part here)
//   4. weight_c = 1.0f * a_0 * a_1 * ... left to right, a_d = frac_d or 1.0f - frac_d; index_c = sum (i_d + bit) * stride_d
//   5. E = fmaf(weight_c, V[index_c], E) over ASCENDING c from 0.0f;  Q = r + gamma * E, a multiply, then an add.
// The greedy action: strict > from -1.0e30f over ascending action indices — the lowest index wins ties, NaN never
// wins, index 0 with Q = -1.0e30f when nothing wins.
//
// One lane per query point / per episode; the action loop is serial per lane, n_actions is run-time data and the action
// values come through wave-uniform loads of the table.  Inside it the 2^D corner loop is fully unrolled over constant
// offsets from the cell's base index: all V loads of one backup are in flight before the first wait.
// Every index is in bounds whatever the point: n is clamped (a NaN lands on the top border), so 0 <= i_d <= g_d - 2 and
// index_c <= sum (g_d - 1) * stride_d, which pi_infer_create checks against the table's length.

#ifndef PI_GREEDY
#error "pi_greedy_kernels.hip is built behind #define PI_GREEDY 1 (pi_greedy.cpp)"
#endif

#define PI_GR_C (1 << PI_D)
#define PI_GR_BLOCK 256                      // the query kernel's; the rollout kernel runs PI_RO_BLOCK threads

// bit of dimension d in corner c
__device__ constexpr int pi_greedy_bit(int c, int d) {
#if PI_D == 2
    return (c >> (1 - d)) & 1;
#else
    return (c >> d) & 1;
#endif
}

// E[V](n): the multilinear interpolation of V at the successor n, the sweeps' arithmetic
__device__ __forceinline__ float pi_greedy_expect(const float (&n)[PI_D], const float* __restrict__ V) {
    int base = 0;
    float fr[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) {
        const float top = (float)(PI_RG.shape[d] - 1);
        float x = (n[d] - PI_RG.lo[d]) / (PI_RG.hi[d] - PI_RG.lo[d]) * top;
        x = fmaxf(0.0f, fminf(x, top));
        const int i = min((int)x, PI_RG.shape[d] - 2);
        fr[d] = x - (float)i;
        base += i * PI_RG.stride[d];
    }
    float v[PI_GR_C];
#pragma unroll
    for (int c = 0; c < PI_GR_C; ++c) {
        int off = 0;
#pragma unroll
        for (int d = 0; d < PI_D; ++d) off += pi_greedy_bit(c, d) * PI_RG.stride[d];
        v[c] = V[base + off];
    }
    float e = 0.0f;
#pragma unroll
    for (int c = 0; c < PI_GR_C; ++c) {
        float w = 1.0f;
#pragma unroll
        for (int d = 0; d < PI_D; ++d) {
            const float side = pi_greedy_bit(c, d) ? fr[d] : 1.0f - fr[d];
            w = w * side;
        }
        e = fmaf(w, v[c], e);
    }
    return e;
}

// Q(s, a); the step it looked at comes back in n, *reward, *done
__device__ __forceinline__ float pi_greedy_q(const float (&s)[PI_D], float a, const float* __restrict__ V, float gamma,
                                             float (&n)[PI_D], float* reward, bool* done) {
    pi_rollout_dynamics(s, a, n, reward, done);
    float e = 0.0f;
    if (!*done) e = pi_greedy_expect(n, V);
    const float future = gamma * e;
    return *reward + future;
}

// The expected-greedy module (pi_expect_greedy_kernels.hip) and the adversary module (pi_adversary_kernels.hip) take the
// functions above and leave the two kernels out.
#if !defined(PI_EXPECT_GREEDY) && !defined(PI_ADVERSARY)
// Batched query.  Every output may be null: out_best (m) int32, out_action (m) = actions[best], out_qbest (m),
// out_qall (m, n_actions) row-major.
extern "C" __global__ void __launch_bounds__(PI_GR_BLOCK)
pi_greedy_kernel(const float* __restrict__ points, long long m, const float* __restrict__ V,
                 const float* __restrict__ actions, int n_actions, float gamma, int* __restrict__ out_best,
                 float* __restrict__ out_action, float* __restrict__ out_qbest, float* __restrict__ out_qall) {
    const long long k = (long long)blockIdx.x * PI_GR_BLOCK + threadIdx.x;
    if (k >= m) return;
    float s[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) s[d] = points[k * PI_D + d];
    float* q_row = out_qall != nullptr ? out_qall + k * (long long)n_actions : nullptr;
    float best_q = -1.0e30f;
    int best = 0;
    for (int a = 0; a < n_actions; ++a) {
        float n[PI_D], r;
        bool done;
        const float q = pi_greedy_q(s, actions[a], V, gamma, n, &r, &done);
        if (q_row != nullptr) q_row[a] = q;
        if (q > best_q) {
            best_q = q;
            best = a;
        }
    }
    if (out_best != nullptr) out_best[k] = best;
    if (out_action != nullptr) out_action[k] = actions[best];
    if (out_qbest != nullptr) out_qbest[k] = best_q;
}

// The controller of a fused rollout on the shared episode loop (pi_rollout_episodes, pi_rollout_kernels.hip).  The step an
// episode takes is step_dynamics(s, actions[best]): the lookahead has computed it already — the same inlined function on
// the same inputs — so the winner's successor, reward and flag are kept instead of stepping again (action 0's when nothing
// wins).  `gamma` discounts the return, `lookahead_gamma` is the discount inside Q.
extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_greedy_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma, float lookahead_gamma,
                         const float* __restrict__ V, const float* __restrict__ actions, int n_actions,
                         float* __restrict__ out_final, float* __restrict__ out_return, int* __restrict__ out_length,
                         unsigned char* __restrict__ out_terminated, float* __restrict__ traj, int traj_every) {
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int, long long, float (&best_n)[PI_D], float& best_r, bool& best_done) {
                            float best_q = -1.0e30f;
                            best_r = 0.0f;
                            best_done = false;
#pragma unroll
                            for (int d = 0; d < PI_D; ++d) best_n[d] = s[d];
                            for (int a = 0; a < n_actions; ++a) {
                                float n[PI_D], r;
                                bool done;
                                const float q = pi_greedy_q(s, pi_rollout_table_entry(actions, a), V, lookahead_gamma, n, &r, &done);
                                const bool wins = q > best_q;
                                if (wins) best_q = q;
                                if (wins || a == 0) {
#pragma unroll
                                    for (int d = 0; d < PI_D; ++d) best_n[d] = n[d];
                                    best_r = r;
                                    best_done = done;
                                }
                            }
                        });
}
#endif  // PI_EXPECT_GREEDY, PI_ADVERSARY
