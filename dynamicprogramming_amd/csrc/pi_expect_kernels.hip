// pi_expect_kernels.hip — the EXPECTED and the WORST-CASE Bellman backup over a disturbance set, for gfx950 (MI355X, CDNA4).
//
// Appended to the sweep translation unit (build_source + this file, ensure_expect_module in pi_compile.cpp) and built as a
// further module of the handle by the first pi_set_disturbances after pi_compile; never compiled on its own.  No reference
// counterpart: the reference backs up the one deterministic successor (src/cuda_policy_iteration.py:212-283).
//
// A disturbance set is K <= 64 points (da_k, dx_k[D], p_k); the backup of state s and action value a is
//     Q(s, a) = sum_k p_k * [ r_k + gamma * E[V](f(s, a (+) da_k) + dx_k) ]
// with, per point in ascending k (include/pi_mi355.h, pi_set_disturbances, is the definition):
//   1. a_k = a when da_k == 0, otherwise fminf(fmaxf(a + da_k, a_min), a_max) — the clamp of the stochastic rollouts;
//   2. (s', r_k, done_k) = step_dynamics(s, a_k), the exact instantiation;
//   3. E_k = 0 when done_k; otherwise s'[d] += dx_k[d] for every d with dx_k[d] != 0 (one float32 add, no wrap: the
//      interpolation clamps) and E_k is the sweeps' interpolation (pi_locate + the fmaf chain of pi_combine_corners);
//   4. q_k = r_k + gamma * E_k, a multiply then an add;
//   5. Q = p_0 * q_0, then Q = fmaf(p_k, q_k, Q).
// With K = 1, da = dx = 0 and p = 1 this is pi_backup bit for bit.
//
// The WORST-CASE backup (pi_robust_*_kernel, include/pi_mi355.h at pi_robust_eval_sweeps) keeps steps 1-4 and folds
//     Q(s, a) = min_k q_k over the points with p_k != 0
// with comparisons: the first participating point gives Q, a later one replaces it when q_k < Q || q_k != q_k (strict: the
// first of equal points stays, -0 does not replace +0; a NaN is taken and only another NaN replaces it).  A point with
// p_k == 0 is skipped as if its row were not in the table — it neither starts nor breaks a run of equal da — and that
// skip is a scalar branch on the row the wave holds in SGPRs.  Both folds are ONE point loop, pi_expect_q<WORST>; the
// pi_expect_* kernels instantiate the expectation, the pi_robust_* kernels the minimum, in the same module.
//
// The table — K rows of {da, dx_0 .. dx_{D-1}, p}, dx in the USER's dimension order — is run-time data in a device buffer
// of the handle: another set is another upload, never another build.  A workgroup stages it in LDS beside the bin table
// and every wave reads a row through readfirstlane, so the row lives in SGPRs and the branches on it (a point with the
// da of the one before it keeps that point's dynamics step; a zero dx is not added) are scalar branches.  The same
// function on the same inputs gives the same bits, so sharing a step changes nothing.
// Corner values: the 2^D loads of a point are issued together (pi_request_corners) and only by lanes whose point left
// the cell the lane holds (`held`, as pi_argmax does across its action loop): small disturbances mostly stay inside it.
// Every array below is indexed by compile-time constants under full unrolling: no scratch in any D.
// One thread owns one state; a 256-thread workgroup takes ONE chunk of 256 consecutive states of [s_begin, s_end), dealt
// to the XCDs in contiguous runs like the sweeps' slab schedule (pi_first_chunk).  Grids of n < 2^30 states only (the
// host refuses the others): V offsets are 32-bit byte offsets.

#define PI_BLOCK_EXPECT 256
#define PI_NOISE_MAX 64                      // points per set, at most (pi_set_disturbances checks)
#define PI_NOISE_ROW (PI_D + 2)              // da | dx_0 .. dx_{D-1} | p
static_assert(PI_OFF32, "the expectation sweeps address V with 32-bit byte offsets: n < 2^30");

struct PiNoise {
    const float* rows;                       // LDS copy of the table
    int K;
    float a_min, a_max;                      // extremes of the handle's action table
};

__device__ __forceinline__ void pi_stage_noise(const float* __restrict__ dist, int K, float* lds_rows) {
    for (int i = threadIdx.x; i < K * PI_NOISE_ROW; i += PI_BLOCK_EXPECT) lds_rows[i] = dist[i];
}
// A table entry: the same word in every lane, so it can live in an SGPR.
__device__ __forceinline__ float pi_noise_word(const PiNoise& nz, int k, int j) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(nz.rows[k * PI_NOISE_ROW + j])));
}

// Q(s, a) of the header, WORST: the minimum over the points of weight != 0 instead of the expectation.  vp / held: the
// corner values of the cell the lane looked at last, kept by the caller across points (and across its action loop).
template <bool WORST>
__device__ __forceinline__ float pi_expect_q(const float (&x)[PI_D], float a, const PiNoise& nz,
                                             const float* __restrict__ V, float gamma, PiPair (&vp)[PI_NPAIR],
                                             unsigned int& held) {
    float ns[PI_D], reward = 0.0f, da_prev = 0.0f;
    bool done = false;
#pragma unroll
    for (int d = 0; d < PI_D; ++d) ns[d] = 0.0f;
    // -0.0f + p * q is p * q for every value of the product, signed zeros and NaN included: the first point's multiply
    // and the later points' fmaf are one instruction
    float Q = -0.0f;
    bool started = false;                                                // WORST: a point took part (wave-uniform)
    for (int k = 0; k < nz.K; ++k) {
        // WORST: da is read with the weight, before the branch on it, so that a point opens with one LDS round trip, not two
        const float da = pi_noise_word(nz, k, 0);
        if (WORST && pi_noise_word(nz, k, PI_D + 1) == 0.0f) continue;   // no part in the minimum, nor in the runs of da
        if ((WORST ? !started : k == 0) || da != da_prev) {              // wave-uniform
            const float ak = da == 0.0f ? a : fminf(fmaxf(a + da, nz.a_min), nz.a_max);
            pi_dynamics(x, ak, ns, &reward, &done);
            da_prev = da;
        }
        float e = 0.0f;
        if (!done) {
            float p[PI_D];
#pragma unroll
            for (int d = 0; d < PI_D; ++d) {
                const float dx = pi_noise_word(nz, k, 1 + d);            // user dimension d
                p[PI_MEM_OF[d]] = dx != 0.0f ? ns[PI_MEM_OF[d]] + dx : ns[PI_MEM_OF[d]];
            }
            unsigned int base;
            float fr[PI_D];
            pi_locate(p, base, fr);                                      // clamps: any point names a cell of the grid
            if (base != held) {
                pi_request_corners(V, base, vp);
                held = base;
            }
            __builtin_amdgcn_s_setprio(1);
            e = pi_combine_corners(vp, fr);
            __builtin_amdgcn_s_setprio(0);
        }
        const float q = reward + gamma * e;
        if (WORST) {
            if (!started || q < Q || q != q) Q = q;
            started = true;
        } else {
            Q = fmaf(pi_noise_word(nz, k, PI_D + 1), q, Q);
        }
    }
    return Q;
}

// The chunk of this workgroup: first state and the lane's offset in it; lanes past s_end (tail of the last chunk) shadow the
// last valid state and store nothing.  False: the workgroup has no chunk.
__device__ __forceinline__ bool pi_expect_chunk(long long s_begin, long long s_end, long long& sb, unsigned int& lane) {
    long long chunk0, n_chunks;
    if (!pi_first_chunk<PI_BLOCK_EXPECT>(s_end - s_begin, 1, chunk0, n_chunks)) return false;
    sb = s_begin + chunk0 * PI_BLOCK_EXPECT;
    const unsigned int tid = threadIdx.x;
    lane = min(tid, (unsigned int)(min(s_end - sb, (long long)PI_BLOCK_EXPECT) - 1));
    return true;
}

// ---- evaluation: Vn[s] = Q(s, actions[policy[s]]) for s in [s_begin, s_end); terminal states copy V[s] ---------------
// delta_bits (nullable): the handle's slots, receiving the atomic max of the bit pattern of |Vn - V| (pi_finalize_kernel).
// The body stays in the kernel (a macro, not a function the two kernels inline): the expectation kernel then compiles to the
// instructions and registers it had before the fold became a template argument.
#define PI_EXPECT_EVAL_KERNEL(name, WORST)                                                                               \
    extern "C" __global__ void __launch_bounds__(PI_BLOCK_EXPECT)                                                        \
    name(const float* __restrict__ V, float* __restrict__ Vn, const int* __restrict__ policy,                            \
         const unsigned char* __restrict__ term, const float* __restrict__ tab, const float* __restrict__ dist, int K,   \
         float a_min, float a_max, long long s_begin, long long s_end, float gamma,                                      \
         unsigned int* __restrict__ delta_bits) {                                                                        \
        __shared__ float lds_tab[PI_GRID.tab_len];                                                                       \
        __shared__ float lds_noise[PI_NOISE_MAX * PI_NOISE_ROW];                                                         \
        long long sb;                                                                                                    \
        unsigned int lane;                                                                                               \
        if (!pi_expect_chunk(s_begin, s_end, sb, lane)) return;                                                          \
        /* the residual, the terminal copy (launch-uniform) */                                                           \
        const bool need_old = delta_bits != nullptr || term != nullptr;                                                  \
        const PiStateIn in = pi_load_state(V, policy, term, sb, lane, need_old);                                         \
        pi_stage_table<PI_BLOCK_EXPECT>(tab, lds_tab);                                                                   \
        pi_stage_noise(dist, K, lds_noise);                                                                              \
        __syncthreads();                                                                                                 \
        const PiNoise nz = {lds_noise, K, a_min, a_max};                                                                 \
                                                                                                                         \
        float nv = in.v_old;                                                                                             \
        if (!in.term) {                                                                                                  \
            const unsigned int s = (unsigned int)sb + lane;                                                              \
            float x[PI_D];                                                                                               \
            pi_state_coords(s, lds_tab, x);                                                                              \
            PiPair vp[PI_NPAIR];                                                                                         \
            _Pragma("unroll") for (int p = 0; p < PI_NPAIR; ++p) vp[p] = PiPair{0.0f, 0.0f};                             \
            unsigned int held = 0xffffffffu;                                                                             \
            nv = pi_expect_q<WORST>(x, lds_tab[PI_TAB_ACT + pi_checked_action(in.action, s)], nz, V, gamma, vp, held);   \
        }                                                                                                                \
        float dmax = 0.0f;                                                                                               \
        if (threadIdx.x == lane) {                                                                                       \
            pi_store_lane(Vn + sb, lane, nv);                                                                            \
            const float dlt = fabsf(nv - in.v_old);                                                                      \
            dmax = dlt > dmax ? dlt : dmax;                                                                              \
        }                                                                                                                \
        if (delta_bits != nullptr) pi_wave_max_to<PI_BLOCK_EXPECT>(dmax, delta_bits);                                    \
    }
PI_EXPECT_EVAL_KERNEL(pi_expect_eval_kernel, false)
PI_EXPECT_EVAL_KERNEL(pi_robust_eval_kernel, true)

// ---- improvement and value sweep: policy[s] = argmax_a Q(s, a), strict '>' from -1.0e30f over ascending actions -------
// Terminal states keep their entry.  WRITE_V: also Vn[s] = max_a Q(s, a) (terminal: copy) and the residual.
template <bool WRITE_V, bool WORST>
__device__ __forceinline__ void pi_expect_improve_body(const float* __restrict__ V, float* __restrict__ Vn,
                                                       int* __restrict__ policy, const unsigned char* __restrict__ term,
                                                       const float* __restrict__ tab, const float* __restrict__ dist, int K,
                                                       float a_min, float a_max, long long s_begin, long long s_end,
                                                       float gamma, unsigned int* __restrict__ delta_bits,
                                                       unsigned int* __restrict__ changed) {
    __shared__ float lds_tab[PI_GRID.tab_len];
    __shared__ float lds_noise[PI_NOISE_MAX * PI_NOISE_ROW];
    long long sb;
    unsigned int lane;
    if (!pi_expect_chunk(s_begin, s_end, sb, lane)) return;
    // the old value is only needed by the value sweep (residual, terminal copy)
    const bool need_old = WRITE_V && (delta_bits != nullptr || term != nullptr);
    const PiStateIn in = pi_load_state(V, policy, term, sb, lane, need_old);
    pi_stage_table<PI_BLOCK_EXPECT>(tab, lds_tab);
    pi_stage_noise(dist, K, lds_noise);
    __syncthreads();
    const PiNoise nz = {lds_noise, K, a_min, a_max};

    const bool live = threadIdx.x == lane;
    unsigned int n_changed = 0;
    float dmax = 0.0f;
    if (!in.term) {
        float x[PI_D];
        pi_state_coords((unsigned int)sb + lane, lds_tab, x);
        PiPair vp[PI_NPAIR];
#pragma unroll
        for (int p = 0; p < PI_NPAIR; ++p) vp[p] = PiPair{0.0f, 0.0f};
        unsigned int held = 0xffffffffu;
        float best_q = -1.0e30f;
        int best = 0;
        for (int a = 0; a < PI_NA; ++a) {
            const float q = pi_expect_q<WORST>(x, lds_tab[PI_TAB_ACT + a], nz, V, gamma, vp, held);
            if (q > best_q) { best_q = q; best = a; }
        }
        if (live) {
            pi_store_lane(policy + sb, lane, best);
            n_changed = (in.action != best) ? 1u : 0u;
            if (WRITE_V) {
                pi_store_lane(Vn + sb, lane, best_q);
                const float dlt = fabsf(best_q - in.v_old);
                dmax = dlt > dmax ? dlt : dmax;
            }
        }
    } else if (WRITE_V && live) {
        pi_store_lane(Vn + sb, lane, in.v_old);
    }
    if (changed != nullptr) pi_wave_sum_to<PI_BLOCK_EXPECT>(n_changed, changed);
    if (WRITE_V && delta_bits != nullptr) pi_wave_max_to<PI_BLOCK_EXPECT>(dmax, delta_bits);
}

extern "C" __global__ void __launch_bounds__(PI_BLOCK_EXPECT)
pi_expect_improve_kernel(const float* __restrict__ V, int* __restrict__ policy, const unsigned char* __restrict__ term,
                         const float* __restrict__ tab, const float* __restrict__ dist, int K, float a_min, float a_max,
                         long long s_begin, long long s_end, float gamma, unsigned int* __restrict__ changed) {
    pi_expect_improve_body<false, false>(V, nullptr, policy, term, tab, dist, K, a_min, a_max, s_begin, s_end, gamma, nullptr,
                                         changed);
}

extern "C" __global__ void __launch_bounds__(PI_BLOCK_EXPECT)
pi_expect_value_kernel(const float* __restrict__ V, float* __restrict__ Vn, int* __restrict__ policy,
                       const unsigned char* __restrict__ term, const float* __restrict__ tab,
                       const float* __restrict__ dist, int K, float a_min, float a_max, long long s_begin, long long s_end,
                       float gamma, unsigned int* __restrict__ delta_bits, unsigned int* __restrict__ changed) {
    pi_expect_improve_body<true, false>(V, Vn, policy, term, tab, dist, K, a_min, a_max, s_begin, s_end, gamma, delta_bits,
                                        changed);
}

// The same two with the worst-case fold.
extern "C" __global__ void __launch_bounds__(PI_BLOCK_EXPECT)
pi_robust_improve_kernel(const float* __restrict__ V, int* __restrict__ policy, const unsigned char* __restrict__ term,
                         const float* __restrict__ tab, const float* __restrict__ dist, int K, float a_min, float a_max,
                         long long s_begin, long long s_end, float gamma, unsigned int* __restrict__ changed) {
    pi_expect_improve_body<false, true>(V, nullptr, policy, term, tab, dist, K, a_min, a_max, s_begin, s_end, gamma, nullptr,
                                        changed);
}

extern "C" __global__ void __launch_bounds__(PI_BLOCK_EXPECT)
pi_robust_value_kernel(const float* __restrict__ V, float* __restrict__ Vn, int* __restrict__ policy,
                       const unsigned char* __restrict__ term, const float* __restrict__ tab,
                       const float* __restrict__ dist, int K, float a_min, float a_max, long long s_begin, long long s_end,
                       float gamma, unsigned int* __restrict__ delta_bits, unsigned int* __restrict__ changed) {
    pi_expect_improve_body<true, true>(V, Vn, policy, term, tab, dist, K, a_min, a_max, s_begin, s_end, gamma, delta_bits,
                                       changed);
}
