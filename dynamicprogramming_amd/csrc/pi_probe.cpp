// pi_probe.cpp — the entry points that look at a grid without sweeping it: the reach of a state range under all
// actions (pi_reach_planes, pi_reach_units, reach_pairs: what a sharded run's exchange planner asks) and the probes
// of single stages of a sweep (pi_probe_step, pi_probe_interp, pi_probe_coords: what the tests compare with the oracle).

#include "pi_internal.h"

using namespace pi;

namespace {

// pi_reach_planes_kernel, pi_reach_units_kernel, pi_reach_pairs_kernel: (term, tab, range, bitmap[, which], cpw = 4)
template <typename... Which>
int launch_reach(pi_handle* h, hipFunction_t f, const uint8_t* term, int64_t s_begin, int64_t s_end, uint32_t* d_bitmap,
                 hipStream_t st, Which... which) {
    if (s_end <= s_begin) return 0;
    const int cpw = 4;
    PI_HIP(launch(f, {launch_blocks(kProbeBlock, s_end - s_begin, cpw), 1}, kProbeBlock, st, term, (const float*)h->d_tab,
                  (long long)s_begin, (long long)s_end, d_bitmap, which..., cpw));
    return 0;
}

}  // namespace

bool pi::pairs_possible(const pi_handle* h) {
    return h->D >= 3 && h->mem_of_user[0] == 0 && (int64_t)h->shape[0] * h->shape[h->mem_of_user[1]] <= (int64_t(1) << 17);
}

int pi::reach_pairs(pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end, uint32_t* d_bitmap, hipStream_t st) {
    if (!pairs_possible(h)) return fail("reach_pairs: needs 3 or more dimensions, dimension 0 slowest and g_0 * g_v <= 2^17");
    if (ensure_push_module(h)) return 1;
    return launch_reach(h, h->f_reach_pairs, term, s_begin, s_end, d_bitmap, st);
}

extern "C" {

int pi_reach_planes(pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end, int dim,
                    uint32_t* d_bitmap, void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (!d_bitmap) return fail("null device pointer");
    if (dim < 0 || dim >= h->D) return fail("dim outside [0, D)");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t words = (size_t)(h->shape[dim] + 31) / 32;
    PI_HIP(hipMemsetAsync(d_bitmap, 0, words * sizeof(uint32_t), st));
    return launch_reach(h, h->f_reach_planes, term, s_begin, s_end, d_bitmap, st, dim);
}

// Units of the leading `depth` dimensions (depth 1: planes of dimension 0; depth 2: rows (i0, i1)).
static int64_t reach_unit_count(const pi_handle* h, int depth) {
    int64_t u = 1;
    for (int d = 0; d < depth; ++d) u *= h->shape[d];
    return u;
}

int pi_reach_depth_max(pi_handle* h) {
    if (!h) return -1;
    return (h->D >= 3 && (int64_t)h->shape[0] * h->shape[1] <= (int64_t(1) << 17)) ? PI_REACH_ROWS : PI_REACH_PLANES;
}

int pi_reach_units(pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end, int depth,
                   uint32_t* d_bitmap, void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (!d_bitmap) return fail("null device pointer");
    if (depth < 1 || depth > pi_reach_depth_max(h)) return fail("depth outside [1, pi_reach_depth_max]");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t words = (size_t)(reach_unit_count(h, depth) + 31) / 32;
    PI_HIP(hipMemsetAsync(d_bitmap, 0, words * sizeof(uint32_t), st));
    return launch_reach(h, h->f_reach_units, term, s_begin, s_end, d_bitmap, st, depth);
}

int pi_probe_step(pi_handle* h, const float* states, const float* acts, float* next,
                  float* reward, uint8_t* done, int64_t m, void* stream) {
    if (check_ready(h)) return 1;
    if (m <= 0) return 0;
    pi::DeviceGuard guard(h->device);
    PI_HIP(launch(h->f_probe_step, {(unsigned)((m + kProbeBlock - 1) / kProbeBlock), 1}, kProbeBlock, (hipStream_t)stream, states,
                  acts, next, reward, done, (long long)m));
    return 0;
}

int pi_probe_interp(pi_handle* h, const float* pts, int32_t* idxs, float* wgts, int64_t m,
                    void* stream) {
    if (check_ready(h)) return 1;
    if (m <= 0) return 0;
    pi::DeviceGuard guard(h->device);
    PI_HIP(launch(h->f_probe_interp, {(unsigned)((m + kProbeBlock - 1) / kProbeBlock), 1}, kProbeBlock, (hipStream_t)stream, pts,
                  idxs, wgts, (long long)m));
    return 0;
}

int pi_probe_coords(pi_handle* h, int64_t s_begin, int64_t s_end, float* out, int chunks_per_workgroup,
                    void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (!out) return fail("null device pointer");
    if (chunks_per_workgroup < 1) return fail("chunks_per_workgroup < 1");
    if (s_end == s_begin) return 0;
    pi::DeviceGuard guard(h->device);
    Sched sc;                    // the sweeps' own schedule (strips included): the probe shows every state is visited once
    const pi::Grid2 blocks = plan_launch(h, kProbeBlock, s_begin, s_end - s_begin, h->n_states, chunks_per_workgroup, &sc);
    PI_HIP(launch(h->f_probe_coords, blocks, kProbeBlock, (hipStream_t)stream, (const float*)h->d_tab, (long long)s_begin,
                  (long long)s_end, out, sc));
    return 0;
}

}  // extern "C"
