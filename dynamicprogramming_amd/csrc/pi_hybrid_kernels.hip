// pi_hybrid_kernels.hip — closed-loop rollouts that switch between TWO policies on two grids of the same D, one
// launch per batch of episodes, for gfx950 (include/pi_mi355.h, pi_infer_rollout_hybrid; the reference's
// runners/hybrid_double_cartpole.py:62-69, :112-125 as one kernel).
//
// A device-code TEMPLATE; pi_hybrid.cpp (pi_infer_set_partner) builds the translation unit
//     <#define PI_HYBRID>
//     <the primary grid:   PI_D,  PI_LO_INIT,  PI_HI_INIT,  PI_SHAPE_INIT,  PI_STRIDES_INIT,  PI_BITS_INIT>
//     <the secondary grid: PI2_D, PI2_LO_INIT, PI2_HI_INIT, PI2_SHAPE_INIT, PI2_STRIDES_INIT, PI2_BITS_INIT>
//     <include/pi_math.h>  + #define sinf/cosf/fmodf -> pi_*
//     <the primary handle's step_dynamics C string>
//     <pi_rollout_kernels.hip>      its helpers: the interpolation, the dynamics call, the episode loop
//     <this file>
// and hipRTC compiles it with the sweeps' flags.
//
// The episode loop is pi_rollout_episodes (pi_rollout_kernels.hip); this file adds the mode and its counter, which stay in
// registers for all steps beside the loop's own state.  Per step of a running episode
//   1. the mode (0 primary, 1 secondary): a box with hysteresis, float32, strict comparisons —
//      mode 1 stays unless fabsf(s[d]) > leave[d] for some d; mode 0 becomes 1 iff fabsf(s[d]) < enter[d] for every d;
//   2. the interpolated action of the mode's policy on ITS grid, the arithmetic of pi_rollout_action;
//   3. secondary_steps += mode;
//   4. step_dynamics; return, length and the freeze are the loop's.
// Lanes of one wave are in different modes, and a branch on the mode would run the 2^D-corner interpolation twice for
// a mixed wave.  The interpolation is the same expression on both grids, so a lane SELECTS its operands — bounds,
// shape, strides, the float64 cell widths (compile-time constants of either grid), the policy and action tables —
// and the interpolation runs once: the same operations on the selected operands give the same bits.  Both grids
// share the corner table (checked by the host and below).

#if PI2_D != PI_D
#error "both grids of a hybrid rollout need the same D"
#endif

__device__ constexpr PiRolloutGrid PI_RG2 = {PI2_LO_INIT, PI2_HI_INIT, PI2_SHAPE_INIT, PI2_STRIDES_INIT, PI2_BITS_INIT};

__device__ constexpr bool pi_hybrid_same_corners() {
    for (int c = 0; c < PI_RO_C; ++c)
        for (int d = 0; d < PI_D; ++d)
            if (PI_RG.bits[c][d] != PI_RG2.bits[c][d]) return false;
    return true;
}
static_assert(pi_hybrid_same_corners(), "both grids of a hybrid rollout need the same corner_bits table");

// this lane's grid: PI_RG2 when `second`, PI_RG otherwise
struct PiGridPick {
    bool second;
    __device__ __forceinline__ float lo(int d) const { return second ? PI_RG2.lo[d] : PI_RG.lo[d]; }
    __device__ __forceinline__ float hi(int d) const { return second ? PI_RG2.hi[d] : PI_RG.hi[d]; }
    __device__ __forceinline__ int shape(int d) const { return second ? PI_RG2.shape[d] : PI_RG.shape[d]; }
    __device__ __forceinline__ int stride(int d) const { return second ? PI_RG2.stride[d] : PI_RG.stride[d]; }
    __device__ __forceinline__ double step(int d) const {
        const double a = (double)(PI_RG.hi[d] - PI_RG.lo[d]) / (double)(PI_RG.shape[d] - 1);
        const double b = (double)(PI_RG2.hi[d] - PI_RG2.lo[d]) / (double)(PI_RG2.shape[d] - 1);
        return second ? b : a;
    }
};

// the switch box, D thresholds each (same layout in pi_hybrid.cpp)
struct PiHybridBox {
    float enter[6], leave[6];
};

// The stochastic hybrid module (pi_hybrid_stochastic_kernels.hip) takes what stands above and leaves the kernel out.
#ifndef PI_HYBRID_STOCHASTIC
extern "C" __global__ void __launch_bounds__(PI_RO_BLOCK)
pi_hybrid_rollout_kernel(const float* __restrict__ start, long long m, int n_steps, float gamma,
                         const int* __restrict__ policy0, const float* __restrict__ actions0,
                         const int* __restrict__ policy1, const float* __restrict__ actions1, PiHybridBox box,
                         float* __restrict__ out_final, float* __restrict__ out_return, int* __restrict__ out_length,
                         unsigned char* __restrict__ out_terminated, int* __restrict__ out_secondary,
                         unsigned char* __restrict__ out_last_mode, float* __restrict__ traj, int traj_every) {
    int secondary = 0;
    bool second = false;                             // the mode; it changes on steps taken only, so it ends as last_mode
    pi_rollout_episodes(start, m, n_steps, gamma, out_final, out_return, out_length, out_terminated, traj, traj_every,
                        [&](const float (&s)[PI_D], int, long long, float (&n)[PI_D], float& r, bool& done) {
                            bool inside = true, outside = false;
#pragma unroll
                            for (int d = 0; d < PI_D; ++d) {
                                const float mag = fabsf(s[d]);
                                inside = inside && mag < box.enter[d];
                                outside = outside || mag > box.leave[d];
                            }
                            second = second ? !outside : inside;
                            const float a = pi_rollout_action(PiGridPick{second}, s, second ? policy1 : policy0,
                                                              second ? actions1 : actions0);
                            secondary += second ? 1 : 0;
                            pi_rollout_dynamics(s, a, n, &r, &done);
                        });
    const long long k = pi_rollout_lane();
    if (k >= m) return;
    if (out_secondary != nullptr) out_secondary[k] = secondary;
    if (out_last_mode != nullptr) out_last_mode[k] = second ? 1 : 0;
}
#endif  // PI_HYBRID_STOCHASTIC
