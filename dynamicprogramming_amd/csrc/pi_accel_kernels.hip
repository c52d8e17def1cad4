// pi_accel_kernels.hip — Anderson-accelerated policy evaluation: the two streaming kernels behind pi_accel_update and
// pi_accel_combine, and the fold of the tile partials.  The arithmetic, the ownership of elements by threads and the
// reduction tree are DEFINED in include/pi_mi355.h at pi_accel_update; dynamicprogramming_amd/accel.py is the numpy twin
// that reproduces them bit for bit.  Nothing here depends on the grid or the env: one code object serves every handle.
//
// Shape of the work: a tile is PI_ACCEL_TILE = 4 096 consecutive elements, one 256-thread workgroup per tile; thread t owns
// the four consecutive elements 4t .. 4t + 3 of each of the tile's four 1 024-element chunks, so a thread's elements are
// one 16-byte access per array and chunk.  PI_VEC instantiations take those accesses as float4 (every base 16-byte
// aligned and n a multiple of 4, so every column of the (m, n) arrays is aligned as well); the others read and write the
// same elements one float at a time — the element -> thread map and the order of the additions are the same, so the results
// are too.  Element offsets are 64-bit: column j starts j * n elements into its array.
// Up to 17 float64 accumulators per thread, all with compile-time indices (the loops over the window are unrolled to
// PI_ACCEL_MAXK and predicated on the uniform k_used): no private memory.  Products are (double)a * (double)b, then one add;
// the unit is built with -ffp-contract=off like the sweeps.  No floating-point atomics anywhere.

#define PI_ACCEL_TILE 4096
#define PI_ACCEL_BLOCK 256
#define PI_ACCEL_MAXK 8
#define PI_ACCEL_MAXDOTS (2 * PI_ACCEL_MAXK + 1)

struct PiAccelCoeffs {
    double c[PI_ACCEL_MAXK];
};

// Lanes 0 .. o - 1 add lanes o .. 2o - 1 for o = 32, 16, .. 1: lane 0 ends with the wave's sum in that fixed association.
__device__ __forceinline__ double pi_accel_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
    return v;
}

// Does a workgroup of a window of k columns carry accumulator q?  q = j: dF_j . f, q = 8 + j: dF_j . dF_slot (j < k), q = 16: f . f.
__device__ __forceinline__ bool pi_accel_used(int q, int k) {
    return q < PI_ACCEL_MAXK ? q < k : (q < 2 * PI_ACCEL_MAXK ? q - PI_ACCEL_MAXK < k : true);
}

// The workgroup's sums of the per-thread accumulators in use: wave sums by shuffles, then (w0 + w2) + (w1 + w3) through
// LDS.  Thread q < N returns with sum q (0.0 for one that is not in use).
template <int N>
__device__ __forceinline__ double pi_accel_block_sums(double (&acc)[N], int k, double (*part)[PI_ACCEL_MAXDOTS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        if (N == 1 || pi_accel_used(q, k)) {
            const double s = pi_accel_wave_sum(acc[q]);
            if (lane == 0) part[wave][q] = s;
        }
    }
    __syncthreads();
    double r = 0.0;
    const int q = threadIdx.x;
    if (q < N && (N == 1 || pi_accel_used(q, k))) r = (part[0][q] + part[2][q]) + (part[1][q] + part[3][q]);
    return r;
}

template <bool VEC>
__device__ __forceinline__ void pi_accel_load4(const float* p, long long e, int cnt, float (&v)[4]) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(p + e);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < cnt ? p[e + i] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void pi_accel_store4(float* p, long long e, int cnt, const float (&v)[4]) {
    if (VEC) {
        *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) p[e + i] = v[i];
    }
}

// One pass over a full batch's iterates: f = g - x, the new column (dF, dG)[slot] = (f - f_prev, g - g_prev) unless
// `first`, (f_prev, g_prev) <- (f, g), and per tile the partial sums of dF_j . f (q = j), dF_j . dF_slot (q = 8 + j) for
// the columns j < k and of f . f (q = 16) into partials[q * tiles + tile].
template <bool VEC>
__device__ __forceinline__ void pi_accel_update_body(const float* __restrict__ x, const float* __restrict__ g,
                                                     float* __restrict__ f_prev, float* __restrict__ g_prev,
                                                     float* __restrict__ dF, float* __restrict__ dG, int slot, int k,
                                                     int first, long long n, double* __restrict__ partials) {
    __shared__ double part[PI_ACCEL_BLOCK / 64][PI_ACCEL_MAXDOTS];
    double acc[PI_ACCEL_MAXDOTS];
#pragma unroll
    for (int q = 0; q < PI_ACCEL_MAXDOTS; ++q) acc[q] = 0.0;
    const long long tile = blockIdx.x;
    const long long slot_off = (long long)slot * n;
#pragma unroll 1
    for (int c = 0; c < PI_ACCEL_TILE / (4 * PI_ACCEL_BLOCK); ++c) {
        const long long e = tile * PI_ACCEL_TILE + (long long)c * (4 * PI_ACCEL_BLOCK) + 4 * (long long)threadIdx.x;
        if (e >= n) break;
        const int cnt = n - e < 4 ? (int)(n - e) : 4;
        float xs[4], gs[4], f[4], dfn[4], dgn[4];
        pi_accel_load4<VEC>(x, e, cnt, xs);
        pi_accel_load4<VEC>(g, e, cnt, gs);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = gs[i] - xs[i];
        if (!first) {
            float fp[4], gp[4];
            pi_accel_load4<VEC>(f_prev, e, cnt, fp);
            pi_accel_load4<VEC>(g_prev, e, cnt, gp);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dfn[i] = f[i] - fp[i];
                dgn[i] = gs[i] - gp[i];
            }
            pi_accel_store4<VEC>(dF + slot_off, e, cnt, dfn);
            pi_accel_store4<VEC>(dG + slot_off, e, cnt, dgn);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) dfn[i] = dgn[i] = 0.0f;
        }
        pi_accel_store4<VEC>(f_prev, e, cnt, f);
        pi_accel_store4<VEC>(g_prev, e, cnt, gs);
#pragma unroll
        for (int j = 0; j < PI_ACCEL_MAXK; ++j) {
            if (j < k) {
                float col[4];
                if (j == slot) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) col[i] = dfn[i];
                } else {
                    pi_accel_load4<VEC>(dF + (long long)j * n, e, cnt, col);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < cnt) {
                        acc[j] = acc[j] + (double)col[i] * (double)f[i];
                        acc[PI_ACCEL_MAXK + j] = acc[PI_ACCEL_MAXK + j] + (double)col[i] * (double)dfn[i];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < cnt) acc[2 * PI_ACCEL_MAXK] = acc[2 * PI_ACCEL_MAXK] + (double)f[i] * (double)f[i];
    }
    const double r = pi_accel_block_sums(acc, k, part);
    const int q = threadIdx.x;
    if (q < PI_ACCEL_MAXDOTS && pi_accel_used(q, k)) partials[(long long)q * gridDim.x + tile] = r;
}

extern "C" __global__ void __launch_bounds__(PI_ACCEL_BLOCK)
pi_accel_update_vec_kernel(const float* x, const float* g, float* f_prev, float* g_prev, float* dF, float* dG, int slot, int k,
                           int first, long long n, double* partials) {
    pi_accel_update_body<true>(x, g, f_prev, g_prev, dF, dG, slot, k, first, n, partials);
}

extern "C" __global__ void __launch_bounds__(PI_ACCEL_BLOCK)
pi_accel_update_kernel(const float* x, const float* g, float* f_prev, float* g_prev, float* dF, float* dG, int slot, int k,
                       int first, long long n, double* partials) {
    pi_accel_update_body<false>(x, g, f_prev, g_prev, dF, dG, slot, k, first, n, partials);
}

// Workgroup o folds the `tiles` partials of output o of a window of k columns — {dF_j . f | dF_j . dF_slot | f . f}, 2k + 1
// values: thread t adds partials t, t + 256, .. in ascending order from 0.0, then the same workgroup tree.
extern "C" __global__ void __launch_bounds__(PI_ACCEL_BLOCK)
pi_accel_fold_kernel(const double* __restrict__ partials, long long tiles, int k, double* __restrict__ dots) {
    __shared__ double part[PI_ACCEL_BLOCK / 64][PI_ACCEL_MAXDOTS];
    const int o = blockIdx.x;
    const int q = o < k ? o : (o < 2 * k ? PI_ACCEL_MAXK + o - k : 2 * PI_ACCEL_MAXK);
    const double* p = partials + (long long)q * tiles;
    double acc[1] = {0.0};
    for (long long i = threadIdx.x; i < tiles; i += PI_ACCEL_BLOCK) acc[0] = acc[0] + p[i];
    const double r = pi_accel_block_sums(acc, 0, part);
    if (threadIdx.x == 0) dots[o] = r;
}

// out[s] = (float)((double)g[s] - sum), sum = 0.0 + c_0 * dG_0[s] + c_1 * dG_1[s] + .. in ascending ring position.  `out`
// may be `g`: every element is read and written by the one thread that owns it.
template <bool VEC>
__device__ __forceinline__ void pi_accel_combine_body(const float* g, const float* __restrict__ dG, PiAccelCoeffs coeffs, int k,
                                                      long long n, float* out) {
    const long long tile = blockIdx.x;
#pragma unroll 1
    for (int c = 0; c < PI_ACCEL_TILE / (4 * PI_ACCEL_BLOCK); ++c) {
        const long long e = tile * PI_ACCEL_TILE + (long long)c * (4 * PI_ACCEL_BLOCK) + 4 * (long long)threadIdx.x;
        if (e >= n) break;
        const int cnt = n - e < 4 ? (int)(n - e) : 4;
        float gs[4], res[4];
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        pi_accel_load4<VEC>(g, e, cnt, gs);
#pragma unroll
        for (int j = 0; j < PI_ACCEL_MAXK; ++j) {
            if (j < k) {
                float col[4];
                pi_accel_load4<VEC>(dG + (long long)j * n, e, cnt, col);
#pragma unroll
                for (int i = 0; i < 4; ++i) sum[i] = sum[i] + coeffs.c[j] * (double)col[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) res[i] = (float)((double)gs[i] - sum[i]);
        pi_accel_store4<VEC>(out, e, cnt, res);
    }
}

extern "C" __global__ void __launch_bounds__(PI_ACCEL_BLOCK)
pi_accel_combine_vec_kernel(const float* g, const float* dG, PiAccelCoeffs coeffs, int k, long long n, float* out) {
    pi_accel_combine_body<true>(g, dG, coeffs, k, n, out);
}

extern "C" __global__ void __launch_bounds__(PI_ACCEL_BLOCK)
pi_accel_combine_kernel(const float* g, const float* dG, PiAccelCoeffs coeffs, int k, long long n, float* out) {
    pi_accel_combine_body<false>(g, dG, coeffs, k, n, out);
}
