// pi_resample_kernels.hip — a solution on one grid interpolated onto the nodes of another, for gfx950
// (grid continuation: a solver on a fine grid starts from the converged solution of a coarse one).
//
// A device-code TEMPLATE like the others; pi_resample.cpp (pi_infer_set_values) builds the translation unit
//     <PI_D + the inference grid: PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT>
//     <this file>
// and hipRTC compiles it with the sweeps' flags (-O3 -ffp-contract=off).  The handle's grid is the SOURCE: its bounds,
// shape, strides and corner table are compile-time constants.  The DESTINATION is run-time data — per-dimension
// float32 bin tables, any bounds, any shape, any memory order of the dimensions — so one module serves every
// destination.  Device twin of utils.barycentric.resample (numpy).
//
// One thread per destination MEMORY position p (64-bit): V and the policy leave as contiguous stores.  Per node
//   1. i_d = (p / stride_d) mod shape_d for every user dimension d, x_d = bins_d[i_d] from the tables every workgroup
//      stages into LDS.  The 64-bit divisions are done once per workgroup, on its first position (wave-uniform); a
//      thread adds its own 0 .. 255 with 32-bit arithmetic;
//   2. weights and flat indices at the point x on the source grid: the arithmetic of pi_infer_kernel
//      (pi_infer_kernels.hip) restated type for type — the point clamped to the source bounds by the reference's
//      comparisons (a NaN node lands on lo, +-inf on the bounds, a zero at a zero lower bound takes the bound's sign),
//      float64 cell widths,
//      float64 weight products rounded once to float32, corners in the order of the caller's corner_bits;
//   3. V = V + w[c] * Vsrc[flat[c]] in float32 from 0.0f over ASCENDING corners, multiply then add.  The corner loop is
//      fully unrolled over the constant table: the 2^D source-value loads are in flight together;
//   4. policy = map[policy_src[flat[c*]]], c* the corner of largest weight (strict >, from corner 0: the first
//      maximum wins) — ONE policy load, after c* is known; map == null is the identity;
//   5. a node whose terminal-mask byte is non-zero is not written.
// Two entry points, one body: pi_resample_kernel keeps room for 2 048 table floats in LDS (8 KiB: every 4-D and 6-D
// grid the sweep kernels accept and 2-D grids of up to 1 024 bins a side), pi_resample_wide_kernel for the 15 360
// (60 KiB) pi_create admits.

#define PI_RS_C (1 << PI_D)
#define PI_RS_BLOCK 256
#define PI_RS_TABLE 2048
#define PI_RS_TABLE_WIDE 15360

struct PiResampleGrid {
    float lo[PI_D], hi[PI_D];
    int shape[PI_D], stride[PI_D];
    int bits[PI_RS_C][PI_D];
};
__device__ constexpr PiResampleGrid PI_SG = {PI_LO_INIT, PI_HI_INIT, PI_SHAPE_INIT, PI_STRIDES_INIT, PI_BITS_INIT};

// The destination grid in the user's dimension order (PiResampleDst of pi_resample.cpp, same layout; six entries
// whatever D): element stride in memory, bins, where the dimension's table starts in the concatenated tables.
struct PiResampleDst {
    long long stride[6];
    int shape[6];
    int offset[6];
};

template <int TABLE>
__device__ __forceinline__ void pi_resample_body(const float* __restrict__ Vsrc, const int* __restrict__ policy_src,
                                                 const int* __restrict__ action_map, const float* __restrict__ bins,
                                                 int table_floats, const PiResampleDst& dst, long long n,
                                                 const unsigned char* __restrict__ term, float* __restrict__ out_V,
                                                 int* __restrict__ out_policy) {
    __shared__ float lds_bins[TABLE];
    const unsigned int tid = threadIdx.x;
    for (int i = (int)tid; i < table_floats; i += PI_RS_BLOCK) lds_bins[i] = bins[i];
    __syncthreads();
    const long long p0 = (long long)blockIdx.x * PI_RS_BLOCK;
    const long long p = p0 + tid;
    if (p >= n) return;
    int base[PI_D];
    double t[PI_D];
#pragma unroll
    for (int d = 0; d < PI_D; ++d) {
        // (p0 + tid) / stride = p0 / stride + (p0 mod stride + tid) / stride; the second term is 0 or 1 for a stride of at
        // least the workgroup's 256 positions and a 32-bit quotient below 512 otherwise
        const long long stride = dst.stride[d];
        const unsigned int shape = (unsigned int)dst.shape[d];
        const long long q0 = p0 / stride, r0 = p0 - q0 * stride;
        const unsigned int i0 = (unsigned int)(q0 % shape);
        const unsigned int up = stride >= PI_RS_BLOCK ? (unsigned int)(r0 + tid >= stride)
                                                      : ((unsigned int)r0 + tid) / (unsigned int)stride;
        const unsigned int i_dst = (i0 + up) % shape;
        const float x = lds_bins[dst.offset[d] + (int)i_dst];
        const float l = PI_SG.lo[d], h = PI_SG.hi[d];
        const double step = (double)(h - l) / (double)(PI_SG.shape[d] - 1);
        const float mn = (h < x) ? h : x;               // the reference's min / max as two selects: NaN -> lo, +-inf ->
        const float q = (mn > l) ? mn : l;              // the bounds, opposite-sign zeros as in pi_infer_kernels.hip,
        const float pt = (q == l) ? l : q;              // whose third select this is
        const double cell = (double)(pt - l) / step;
        int i = (int)cell;
        if (i >= PI_SG.shape[d] - 1) i = PI_SG.shape[d] - 2;
        base[d] = i;
        t[d] = (double)(float)(((double)pt - ((double)l + (double)i * step)) / step);
    }
    if (term != nullptr && term[p] != 0) return;
    float wf[PI_RS_C];
    int flat[PI_RS_C];
#pragma unroll
    for (int c = 0; c < PI_RS_C; ++c) {
        double w = 1.0;
        int f = 0;
#pragma unroll
        for (int d = 0; d < PI_D; ++d) {
            w *= PI_SG.bits[c][d] ? t[d] : (1.0 - t[d]);
            f += (base[d] + PI_SG.bits[c][d]) * PI_SG.stride[d];
        }
        wf[c] = (float)w;
        flat[c] = f;
    }
    if (out_V != nullptr) {
        float vs[PI_RS_C];
#pragma unroll
        for (int c = 0; c < PI_RS_C; ++c) vs[c] = Vsrc[flat[c]];
        float v = 0.0f;
#pragma unroll
        for (int c = 0; c < PI_RS_C; ++c) {
            const float prod = wf[c] * vs[c];
            v = v + prod;
        }
        out_V[p] = v;
    }
    if (out_policy != nullptr) {
        float best = wf[0];
        int at = flat[0];
#pragma unroll
        for (int c = 1; c < PI_RS_C; ++c)
            if (wf[c] > best) { best = wf[c]; at = flat[c]; }
        int a = policy_src[at];
        if (action_map != nullptr) a = action_map[a];
        out_policy[p] = a;
    }
}

extern "C" __global__ void __launch_bounds__(PI_RS_BLOCK)
pi_resample_kernel(const float* __restrict__ Vsrc, const int* __restrict__ policy_src, const int* __restrict__ action_map,
                   const float* __restrict__ bins, int table_floats, PiResampleDst dst, long long n,
                   const unsigned char* __restrict__ term, float* __restrict__ out_V, int* __restrict__ out_policy) {
    pi_resample_body<PI_RS_TABLE>(Vsrc, policy_src, action_map, bins, table_floats, dst, n, term, out_V, out_policy);
}

extern "C" __global__ void __launch_bounds__(PI_RS_BLOCK)
pi_resample_wide_kernel(const float* __restrict__ Vsrc, const int* __restrict__ policy_src,
                        const int* __restrict__ action_map, const float* __restrict__ bins, int table_floats,
                        PiResampleDst dst, long long n, const unsigned char* __restrict__ term, float* __restrict__ out_V,
                        int* __restrict__ out_policy) {
    pi_resample_body<PI_RS_TABLE_WIDE>(Vsrc, policy_src, action_map, bins, table_floats, dst, n, term, out_V, out_policy);
}
