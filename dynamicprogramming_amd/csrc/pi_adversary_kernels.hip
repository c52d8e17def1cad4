// pi_adversary_kernels.hip — the robust one-step lookahead and the adversary in the closed loop: the worst-case fold of
// include/pi_mi355.h (pi_robust_eval_sweeps) over a disturbance set at arbitrary continuous states, as a batched query and
// as a fused rollout in which the disturbance is chosen against the controller, for gfx950.
//
// A device-code TEMPLATE like the others; pi_adversary.cpp (pi_infer_set_robust) builds the translation unit
//     <PI_ADVERSARY + PI_GREEDY + PI_D + the inference grid: PI_LO_INIT .. PI_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*        (deterministic math, as in the sweeps)
//     <the user's step_dynamics C string>                           (env plugin)
//     <csrc/pi_rollout_kernels.hip>                                 (PI_RG, pi_rollout_action, pi_rollout_dynamics, pi_rollout_episodes)
//     <csrc/pi_greedy_kernels.hip>                                  (pi_greedy_expect; its kernels stay out: PI_ADVERSARY)
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).
//
// Adversary step at a state s with the action value a the controller has chosen, per point in ascending k:
//   0. a point with p_k == 0 takes no part: it neither starts nor breaks a run of equal da
//   1. a_k = a when da_k == 0, otherwise fminf(fmaxf(a + da_k, a_min), a_max), the extremes of this module's action table
//   2. (s', r_k, done_k) = step_dynamics(s, a_k); a point with the da of the participating point before it keeps that step
//   3. E_k = 0 when done_k; otherwise s'[d] += dx_k[d] for every d with dx_k[d] != 0 and E_k = pi_greedy_expect(s')
//   4. q_k = r_k + gamma * E_k, a multiply then an add
//   5. the first participating point gives Q = q_k and k* = k; a later one replaces both when q_k < Q || q_k != q_k
// and the episode moves to s'_{k*} (with dx unless done), collecting r_{k*} and done_{k*}.
// Robust lookahead: best = argmax_a Q(s, actions[a]), strict > from -1.0e30f over ascending indices; the adversary's answer
// is the k* computed for the winner, -1 when no action won; successor, reward and flag are action 0's until an action wins.
//
// Work layout: one lane per query point / per episode, 256-thread workgroups, the action loop and the point loop serial per
// lane.  The table rows are read the way pi_eg_word reads them: wave-uniform addresses, readfirstlane, so the branches on
// a row (its weight, its da, a zero dx) are scalar; the 2^D value loads of a point are issued together (pi_greedy_expect).
// Controller 1 makes ONE pass over (action, point) and keeps the current action's worst successor and the best action's,
// so nothing is stepped twice.  No random numbers, no waits or polls; every loop is bounded by a kernel argument.
// Every index is in bounds whatever the point: rows k < K <= 64 of a 64-row buffer, V through pi_greedy_expect's clamp, the
// policy through pi_rollout_action's.
//
// Resource usage from the code objects (hipcc --offload-arch=gfx950 -O3, kernel-resource-usage;
// tests/test_adversary_host.py asserts the scratch and prints the counts): no scratch in any D.  VGPRs of
// pi_robust_greedy_kernel / pi_adversary_rollout_kernel: 34 / 50 at 200^2 (pendulum), 60 / 97 at 50^4 (cartpole swing-up),
// 134 / 228 at 25^6 (double cart-pole) and 150 / 249 at 25^6 (its swing-up).  The 6-D rollout keeps three states of D floats
// (the point's successor, the current action's worst, the best action's) beside the episode's, and stays under 256: two
// waves per SIMD, as the other 6-D rollouts run.

#ifndef PI_ADVERSARY
#error "pi_adversary_kernels.hip is built behind #define PI_ADVERSARY 1 (pi_adversary.cpp)"
#endif

#define PI_ADV_BLOCK 256                     // the query kernel's; the rollout kernel runs PI_RO_BLOCK threads
#define PI_ADV_ROW (PI_D + 2)                // da | dx_0 .. dx_{D-1} | p

struct PiAdversarySet {
    const float* __restrict__ rows;          // the handle's table, K rows of PI_ADV_ROW floats
    int K;
    float a_min, a_max;                      // extremes of the module's action table
};

// A table entry: the address is the same in every lane, and so is the word — it can live in an SGPR.
__device__ __forceinline__ float pi_adv_word(const PiAdversarySet& set, int k, int j) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(set.rows[k * PI_ADV_ROW + j])));
}

// The fold of the header at s under the action value a: returns Q; k_star, wn, wr, wdone: the worst point, its successor
// (disturbed unless done), reward and flag.
__device__ __forceinline__ float pi_adversary_worst(const float (&s)[PI_D], float a, const PiAdversarySet& set,
                                                    const float* __restrict__ V, float gamma, int& k_star,
                                                    float (&wn)[PI_D], float& wr, bool& wdone) {
    float n[PI_D], reward = 0.0f, da_prev = 0.0f, Q = 0.0f;
    bool done = false, started = false;      // started: wave-uniform
#pragma unroll
    for (int d = 0; d < PI_D; ++d) {
        n[d] = 0.0f;
        wn[d] = s[d];
    }
    k_star = -1;
    wr = 0.0f;
    wdone = false;
    for (int k = 0; k < set.K; ++k) {
        const float da = pi_adv_word(set, k, 0);
        if (pi_adv_word(set, k, PI_D + 1) == 0.0f) continue;
        if (!started || da != da_prev) {                                     // wave-uniform
            const float ak = da == 0.0f ? a : fminf(fmaxf(a + da, set.a_min), set.a_max);
            pi_rollout_dynamics(s, ak, n, &reward, &done);
            da_prev = da;
        }
        float p[PI_D], e = 0.0f;
#pragma unroll
        for (int d = 0; d < PI_D; ++d) p[d] = n[d];
        if (!done) {
#pragma unroll
            for (int d = 0; d < PI_D; ++d) {
                const float dx = pi_adv_word(set, k, 1 + d);
                p[d] = dx != 0.0f ? n[d] + dx : n[d];
            }
            e = pi_greedy_expect(p, V);
        }
        const float future = gamma * e;
        const float q = reward + future;
        if (!started || q < Q || q != q) {
            Q = q;
            k_star = k;
#pragma unroll
            for (int d = 0; d < PI_D; ++d) wn[d] = p[d];
            wr = reward;
            wdone = done;
        }
        started = true;
    }
    return Q;
}

// Batched query: the nullable outputs of pi_greedy_kernel plus out_worst (m) int32, the k* of the winning action as a row
// index of the installed table, -1 when no action won.
extern "C" __global__ void __launch_bounds__(PI_ADV_BLOCK)
pi_robust_greedy_kernel(const float* __restrict__ points, long long m, const float* __restrict__ V,
                        const float* __restrict__ actions, int n_actions, float a_min, float a_max,
                        const float* __restrict__ dist, int K, float gamma, int* __restrict__ out_best,
                        float* __restrict__ out_action, float* __restrict__ out_qbest, float* __restrict__ out_qall,
                        int* __restrict__ out_worst) {
    const long long i = (long long)blockIdx.x * PI_ADV_BLOCK + threadIdx.x;
    if (i >= m) return;
    float s[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) s[d] = points[i * PI_D + d];
    const PiAdversarySet set = {dist, K, a_min, a_max};
    float* q_row = out_qall != nullptr ? out_qall + i * (long long)n_actions : nullptr;
    float best_q = -1.0e30f;
    int best = 0, best_k = -1;
    for (int a = 0; a < n_actions; ++a) {
        float wn[PI_D], wr;
        bool wdone;
        int k_star;
        const float q = pi_adversary_worst(s, pi_rollout_table_entry(actions, a), set, V, gamma, k_star, wn, wr, wdone);
        if (q_row != nullptr) q_row[a] = q;
        if (q > best_q) {
            best_q = q;
            best = a;
            best_k = k_star;
        }
    }
    if (out_best != nullptr) out_best[i] = best;
    if (out_action != nullptr) out_action[i] = actions[best];
    if (out_qbest != nullptr) out_qbest[i] = best_q;
    if (out_worst != nullptr) out_worst[i] = best_k;
}

// The closed loop against the adversary on the shared episode loop (pi_rollout_episodes).  controller (launch-uniform): 0,
// the action of the interpolated policy table (policy, policy_actions: the handle's), one pass over the points; 1, the robust
// lookahead.  `gamma` discounts the return, `lookahead_gamma` is the discount inside the fold.  The outputs are
// pi_rollout_kernel's.
extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_adversary_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma, float lookahead_gamma,
                            int controller, const int* __restrict__ policy, const float* __restrict__ policy_actions,
                            const float* __restrict__ V, const float* __restrict__ actions, int n_actions, float a_min,
                            float a_max, const float* __restrict__ dist, int K, float* __restrict__ out_final,
                            float* __restrict__ out_return, int* __restrict__ out_length,
                            unsigned char* __restrict__ out_terminated, float* __restrict__ traj, int traj_every) {
    const PiAdversarySet set = {dist, K, a_min, a_max};
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int, long long, float (&best_n)[PI_D], float& best_r, bool& best_done) {
                            int k_star;
                            if (controller == 0) {
                                const float a = pi_rollout_action(PiGridFixed(), s, policy, policy_actions);
                                pi_adversary_worst(s, a, set, V, lookahead_gamma, k_star, best_n, best_r, best_done);
                                return;
                            }
                            float best_q = -1.0e30f;
                            best_r = 0.0f;
                            best_done = false;
#pragma unroll
                            for (int d = 0; d < PI_D; ++d) best_n[d] = s[d];
                            for (int a = 0; a < n_actions; ++a) {
                                float wn[PI_D], wr;
                                bool wdone;
                                const float q = pi_adversary_worst(s, pi_rollout_table_entry(actions, a), set, V,
                                                                   lookahead_gamma, k_star, wn, wr, wdone);
                                const bool wins = q > best_q;
                                if (wins) best_q = q;
                                if (wins || a == 0) {
#pragma unroll
                                    for (int d = 0; d < PI_D; ++d) best_n[d] = wn[d];
                                    best_r = wr;
                                    best_done = wdone;
                                }
                            }
                        });
}
