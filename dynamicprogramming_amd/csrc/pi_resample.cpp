// pi_resample.cpp — grid continuation on the inference handle (include/pi_mi355.h, "Inference" block): the handle's
// solution — value function and policy on its grid — interpolated onto the nodes of another grid of the same D.
// pi_infer_set_values uploads the value function and builds the handle's resample module (its grid +
// csrc/pi_resample_kernels.hip); pi_infer_resample fills a destination's V and policy arrays in one launch.

#include "pi_internal.h"

#include <algorithm>
#include <cstring>

#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_resample\n"
    "pi_embedded_resample:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_resample_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");
extern "C" const char pi_embedded_resample[];

using pi::fail;

namespace {

constexpr int kBlock = 256;               // PI_RS_BLOCK
constexpr int64_t kTable = 2048;          // PI_RS_TABLE: floats of bin tables pi_resample_kernel stages
constexpr int64_t kTableWide = 15360;     // PI_RS_TABLE_WIDE: 60 KiB, what pi_create admits

struct PiResampleDst {                    // kernel argument, layout of csrc/pi_resample_kernels.hip
    long long stride[6];
    int shape[6];
    int offset[6];
};

// The handle's resample module: its grid + csrc/pi_resample_kernels.hip, built (hipRTC, the handle's cache) once; a compile
// check on host-only handles.
int ensure_module(pi_infer* h, char* log, size_t log_len) {
    if (h->f_resample) return 0;
    std::vector<char> image;
    const std::string src = h->grid_defines + "// ---- resample kernel ----\n" + pi_embedded_resample + "\n";
    if (pi::compile_image(src, h->has_cache_dir ? h->cache_dir.c_str() : nullptr, log, log_len, image, nullptr)) return 1;
    if (h->device < 0) return 0;
    pi::DeviceGuard guard(h->device);
    PI_HIP(hipModuleLoadData(&h->module_resample, image.data()));
    PI_HIP(hipModuleGetFunction(&h->f_resample_wide, h->module_resample, "pi_resample_wide_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_resample, h->module_resample, "pi_resample_kernel"));
    return 0;
}

}  // namespace

extern "C" {

int pi_infer_set_values(pi_infer* h, const float* values, int64_t n_states, char* log, size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h || !values) return fail("null argument");
    if (n_states != h->n_states) return fail("value function length " + std::to_string(n_states) + " != grid size " + std::to_string(h->n_states));
    if (ensure_module(h, log, log_len)) return 1;
    if (h->device < 0) {                            // host-only handle: compile check
        h->has_values = true;
        return 0;
    }
    pi::DeviceGuard guard(h->device);
    if (!h->d_values) PI_HIP(hipMalloc((void**)&h->d_values, (size_t)n_states * sizeof(float)));
    else PI_HIP(hipDeviceSynchronize());            // replaced: launches already enqueued read the old values
    PI_HIP(hipMemcpy(h->d_values, values, (size_t)n_states * sizeof(float), hipMemcpyHostToDevice));
    h->has_values = true;
    return 0;
}

int pi_infer_resample(pi_infer* h, const int32_t* dst_shape, const int64_t* dst_strides, const float* dst_bins,
                      const int32_t* action_map, int dst_n_actions, const uint8_t* d_dst_term, float* d_dst_V,
                      int32_t* d_dst_policy, void* stream) {
    if (!h) return fail("null handle");
    if (!dst_shape || !dst_strides || !dst_bins) return fail("null argument");
    if (!d_dst_V && !d_dst_policy) return fail("pi_infer_resample: both outputs are null");
    const int D = h->D;
    PiResampleDst dst = {};
    int64_t n = 1, table = 0;
    for (int d = 0; d < D; ++d) {
        if (dst_shape[d] < 2) return fail("every dimension of the destination needs at least 2 bins");
        if (__builtin_mul_overflow(n, (int64_t)dst_shape[d], &n)) return fail("the destination's size does not fit 63 bits");
        dst.shape[d] = dst_shape[d];
        dst.stride[d] = dst_strides[d];
        dst.offset[d] = (int)std::min<int64_t>(table, INT32_MAX);
        table += dst_shape[d];
    }
    if (table > kTableWide)
        return fail("the destination's bin tables (" + std::to_string(table * 4) + " bytes) exceed the 60 KiB LDS budget");
    // dense layout in some order of the dimensions: by falling stride, each stride is the product of the shapes behind it
    int by_stride[6];
    for (int d = 0; d < D; ++d) by_stride[d] = d;
    std::sort(by_stride, by_stride + D, [&](int a, int b) { return dst_strides[a] > dst_strides[b]; });
    int64_t expect = 1;
    for (int k = D - 1; k >= 0; --k) {
        if (dst_strides[by_stride[k]] != expect)
            return fail("dst_strides are not the element strides of a dense array of dst_shape in any order of the dimensions");
        expect *= dst_shape[by_stride[k]];
    }
    if ((n + kBlock - 1) / kBlock > INT32_MAX) return fail("the destination is too large for one launch");
    if (d_dst_V && !h->has_values) return fail("pi_infer_resample: values requested but pi_infer_set_values was never called");
    int map_entries = 0;
    if (d_dst_policy) {
        if (!h->d_policy) return fail("pi_infer_resample: a policy requested but pi_infer_set_policy was never called");
        if (dst_n_actions < 1) return fail("the destination needs at least one action");
        if (!action_map) {
            if (dst_n_actions < h->n_actions)
                return fail("a null action_map is the identity: the destination needs at least the source's " +
                            std::to_string(h->n_actions) + " actions");
        } else {
            map_entries = h->n_actions;
            for (int a = 0; a < map_entries; ++a)
                if (action_map[a] < 0 || action_map[a] >= dst_n_actions)
                    return fail("action_map[" + std::to_string(a) + "] = " + std::to_string(action_map[a]) +
                                " is not an index into the destination's " + std::to_string(dst_n_actions) + " actions");
        }
    }
    if (h->device < 0) return fail("host-only handle (device = -1) cannot launch kernels");
    if (ensure_module(h, nullptr, 0)) return 1;      // a policy-only caller never went through pi_infer_set_values
    pi::DeviceGuard guard(h->device);
    // bin tables | action map: uploaded when they differ from the last call's
    std::vector<uint32_t> tab((size_t)table + (size_t)map_entries);
    std::memcpy(tab.data(), dst_bins, (size_t)table * sizeof(float));
    if (map_entries) std::memcpy(tab.data() + table, action_map, (size_t)map_entries * sizeof(int32_t));
    if (tab != h->resample_tab || !h->d_resample_tab) {
        if (h->d_resample_tab) PI_HIP(hipDeviceSynchronize());       // launches already enqueued read the old tables
        h->resample_tab.clear();
        if (h->resample_tab_capacity < tab.size()) {
            if (h->d_resample_tab) { (void)hipFree(h->d_resample_tab); h->d_resample_tab = nullptr; }
            h->resample_tab_capacity = 0;
            PI_HIP(hipMalloc((void**)&h->d_resample_tab, tab.size() * sizeof(uint32_t)));
            h->resample_tab_capacity = tab.size();
        }
        PI_HIP(hipMemcpy(h->d_resample_tab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        h->resample_tab = std::move(tab);
    }
    const float* d_bins = reinterpret_cast<const float*>(h->d_resample_tab);
    const int32_t* d_map = map_entries ? reinterpret_cast<const int32_t*>(h->d_resample_tab + table) : nullptr;
    PI_HIP(pi::launch(table <= kTable ? h->f_resample : h->f_resample_wide, {(unsigned)((n + kBlock - 1) / kBlock), 1}, kBlock,
                      (hipStream_t)stream, (const float*)h->d_values, (const int32_t*)h->d_policy, d_map, d_bins, (int)table,
                      dst, (long long)n, d_dst_term, d_dst_V, d_dst_policy));
    return 0;
}

}  // extern "C"
