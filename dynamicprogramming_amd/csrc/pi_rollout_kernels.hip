// pi_rollout_kernels.hip — closed-loop rollouts of a trained policy on the env's own dynamics, one
// launch per batch of episodes, for gfx950.
//
// A device-code TEMPLATE like the others; pi_rollout.cpp (pi_infer_set_dynamics) builds the translation unit
//     <PI_D + the inference grid: PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*        (deterministic math, as in the sweeps)
//     <the user's step_dynamics C string>                           (env plugin)
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).  The grid is the caller's (archive)
// description, dimensions in the order of step_dynamics' arguments: no memory-order permutation here.
//
// One lane per episode; the state stays in registers for all steps.  The episode loop (pi_rollout_episodes, below) is
// shared by every fused rollout of the handle: a controller supplies step 1 and 2, the loop does the rest.  Per step
//   1. the interpolated action, the arithmetic of pi_infer_kernel (pi_infer_kernels.hip) restated type for type:
//      point clamped to the bounds by the reference's comparisons (a NaN coordinate — step_dynamics is free to return
//      one — lands on lo, +-inf on the bounds, a zero at a zero lower bound takes the bound's sign), float64 cell
//      widths, float64 weight products rounded once to float32, corners in the order of the caller's corner_bits,
//      the action a float32 sum over ASCENDING corners, multiply then add.  The corner loop is fully unrolled: the 2^D policy look-ups of a step are in flight together and the
//      action values follow as a second independent batch (profiles/r03/inference.txt);
//   2. step_dynamics with the arity for D;
//   3. ret = ret + disc * r;  disc = disc * gamma      float32, separate multiply and add (gamma = 1: the plain sum);
//   4. s = s', length = t + 1; a `done` step freezes the episode: no further loads, no further dynamics, the
//      state stays.
// The step loop of a wave ends as soon as all its lanes are frozen (one vote per step) or after n_steps.
// So a fused rollout equals, bit for bit, the loop "pi_infer_query, pi_probe_step, freeze ended episodes on the
// host" that it replaces (tests/test_gpu_rollout.py).
//
// Trajectory (traj_every > 0): row j of traj — (n_steps / traj_every + 1, m, D) — holds every episode's state
// after j * traj_every steps; row 0 is the start, a frozen episode repeats its last state.  A wave writes
// 64 * D contiguous floats per row, each lane one float2 (2-D), one float4 (4-D) or three float2 (6-D: 24 bytes
// per lane keep 8-byte alignment only).

#define PI_RO_C (1 << PI_D)
#define PI_RO_BLOCK 256                              // threads per workgroup of every fused rollout kernel

struct PiRolloutGrid {
    float lo[PI_D], hi[PI_D];
    int shape[PI_D], stride[PI_D];
    int bits[PI_RO_C][PI_D];
};
__device__ constexpr PiRolloutGrid PI_RG = {PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT};

// The grid an interpolation runs on, as the operands of its arithmetic.  PiGridFixed is the module's own grid: every
// operand a compile-time constant.  (pi_hybrid_kernels.hip adds a second kind, whose operands a lane picks from two
// grids.)  step(d) is the float64 cell width, (double)(hi - lo) / (double)(shape - 1).
struct PiGridFixed {
    __device__ __forceinline__ float lo(int d) const { return PI_RG.lo[d]; }
    __device__ __forceinline__ float hi(int d) const { return PI_RG.hi[d]; }
    __device__ __forceinline__ int shape(int d) const { return PI_RG.shape[d]; }
    __device__ __forceinline__ int stride(int d) const { return PI_RG.stride[d]; }
    __device__ __forceinline__ double step(int d) const {
        return (double)(PI_RG.hi[d] - PI_RG.lo[d]) / (double)(PI_RG.shape[d] - 1);
    }
};

// the action of pi_infer_kernel at the point s on the grid g (corners in the order of PI_RG.bits)
template <typename G>
__device__ __forceinline__ float pi_rollout_action(const G& g, const float (&s)[PI_D], const int* __restrict__ policy,
                                                   const float* __restrict__ actions) {
    int base[PI_D];
    double t[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) {
        const float l = g.lo(d), h = g.hi(d);
        const double step = g.step(d);
        const float mn = (h < s[d]) ? h : s[d];         // the reference's min / max as two selects: NaN -> lo, +-inf ->
        const float q = (mn > l) ? mn : l;              // the bounds, opposite-sign zeros as in pi_infer_kernels.hip,
        const float p = (q == l) ? l : q;               // whose third select this is
        const double cell = (double)(p - l) / step;
        int i = (int)cell;
        if (i >= g.shape(d) - 1) i = g.shape(d) - 2;
        base[d] = i;
        t[d] = (double)(float)(((double)p - ((double)l + (double)i * step)) / step);
    }
    float wf[PI_RO_C];
    int a_idx[PI_RO_C];
#pragma unroll
    for (int c = 0; c < PI_RO_C; ++c) {
        double w = 1.0;
        int f = 0;
#pragma unroll
        for (int d = 0; d < PI_D; ++d) {
            w *= PI_RG.bits[c][d] ? t[d] : (1.0 - t[d]);
            f += (base[d] + PI_RG.bits[c][d]) * g.stride(d);
        }
        wf[c] = (float)w;
        a_idx[c] = f;
    }
#pragma unroll
    for (int c = 0; c < PI_RO_C; ++c) a_idx[c] = policy[a_idx[c]];
    float av[PI_RO_C];
#pragma unroll
    for (int c = 0; c < PI_RO_C; ++c) av[c] = actions[a_idx[c]];
    float act = 0.0f;
#pragma unroll
    for (int c = 0; c < PI_RO_C; ++c) {
        const float prod = wf[c] * av[c];
        act = act + prod;
    }
    return act;
}

// step_dynamics with the arity the plugin contract gives each D, in the user's argument order
__device__ __forceinline__ void pi_rollout_dynamics(const float (&s)[PI_D], float a, float (&n)[PI_D], float* reward,
                                                    bool* done) {
#if PI_D == 2
    step_dynamics(s[0], s[1], a, &n[0], &n[1], reward, done);
#elif PI_D == 4
    step_dynamics(s[0], s[1], s[2], s[3], a, &n[0], &n[1], &n[2], &n[3], reward, done);
#elif PI_D == 6
    step_dynamics(s[0], s[1], s[2], s[3], s[4], s[5], a, &n[0], &n[1], &n[2], &n[3], &n[4], &n[5], reward, done);
#else
#error "PI_D must be 2, 4 or 6"
#endif
}

// row[0 .. D) = s as vector stores; `row` is 8-byte (2-D, 6-D) or 16-byte (4-D) aligned (checked by the host)
__device__ __forceinline__ void pi_rollout_store_state(float* __restrict__ row, const float (&s)[PI_D]) {
#if PI_D == 4
    *reinterpret_cast<float4*>(row) = make_float4(s[0], s[1], s[2], s[3]);
#else
#pragma unroll
    for (int d = 0; d < PI_D; d += 2) *reinterpret_cast<float2*>(row + d) = make_float2(s[d], s[d + 1]);
#endif
}

// An entry of a table the launch only reads, at a wave-uniform address.  Read through the constant address space the load
// stays on the scalar unit whether or not the compiler can prove that the trajectory stores of the loop below leave the
// table alone: the lookahead controllers wait on this load once per action, and as a vector load it cost the greedy
// rollout up to a fifth of its time on small batches.
__device__ __forceinline__ float pi_rollout_table_entry(const float* __restrict__ table, int i) {
    return *(const __attribute__((address_space(4))) float*)(table + i);
}

// The episode loop of every fused rollout (this file's kernel and those of pi_hybrid_kernels.hip, pi_greedy_kernels.hip,
// pi_stochastic_kernels.hip, pi_expect_greedy_kernels.hip and pi_hybrid_stochastic_kernels.hip): lane k of the launch is
// episode k of the batch.
__device__ __forceinline__ long long pi_rollout_lane() { return (long long)blockIdx.x * PI_RO_BLOCK + threadIdx.x; }

// Everything of a rollout but the controller: the start-state load, the trajectory rows, the loop exit by vote, return,
// discount, length, the freeze on `done` and the four nullable outputs.  step(s, t, k, n, r, done) is called for a running
// episode k at step t in the state s and fills the successor n, the reward r and the flag done.
template <typename Step>
__device__ __forceinline__ void pi_rollout_episodes(const float* __restrict__ start, long long m, int n_steps, float gamma,
                                                    float* __restrict__ out_final, float* __restrict__ out_return,
                                                    int* __restrict__ out_length, unsigned char* __restrict__ out_terminated,
                                                    float* __restrict__ traj, int traj_every, Step&& step) {
    const long long k = pi_rollout_lane();
    const bool exists = k < m;                       // lanes past the batch are frozen from the start and store nothing
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
    float ret = 0.0f, disc = 1.0f;
    int length = 0;
    bool terminated = false, running = exists;
    for (int t = 0; t < n_steps && __any(running); ++t) {
        if (running) {
            float n[PI_D], r;
            bool done;
            step(s, t, k, n, r, done);
            const float gain = disc * r;
            ret = ret + gain;
            disc = disc * gamma;
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

// the hybrid module holds pi_hybrid_rollout_kernel instead, the greedy module (pi_greedy_kernels.hip) and the stochastic
// module (pi_stochastic_kernels.hip) their own two each
#if !defined(PI_HYBRID) && !defined(PI_GREEDY) && !defined(PI_STOCHASTIC)
extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma,
                  const int* __restrict__ policy, const float* __restrict__ actions,
                  float* __restrict__ out_final, float* __restrict__ out_return, int* __restrict__ out_length,
                  unsigned char* __restrict__ out_terminated, float* __restrict__ traj, int traj_every) {
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int, long long, float (&n)[PI_D], float& r, bool& done) {
                            const float a = pi_rollout_action(PiGridFixed(), s, policy, actions);
                            pi_rollout_dynamics(s, a, n, &r, &done);
                        });
}
#endif  // PI_HYBRID, PI_GREEDY, PI_STOCHASTIC
