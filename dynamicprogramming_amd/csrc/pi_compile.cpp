// pi_compile.cpp — from a handle to loaded kernels: the embedded device sources, the exhaustive check of the reciprocal
// division, the generated translation unit (build_source), hipRTC with the on-disk code-object cache, and the modules
// of a handle (symbol lookups, residency checks of the one-launch kernels, the push and expectation modules built on demand).

#include "pi_internal.h"

#include <hip/hiprtc.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <sys/stat.h>
#include <unistd.h>

// The device-code template and the deterministic math header are embedded verbatim.
#ifndef PI_CSRC_DIR
#error "build with -DPI_CSRC_DIR=\"...\" and -DPI_INCLUDE_DIR=\"...\""
#endif
asm(".section .rodata\n"
    ".global pi_embedded_kernels\n"
    "pi_embedded_kernels:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_sweep_kernels.hip\"\n"
    ".byte 0\n"
    ".global pi_embedded_onelaunch\n"
    "pi_embedded_onelaunch:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_onelaunch_kernels.hip\"\n"
    ".byte 0\n"
    ".global pi_embedded_math\n"
    "pi_embedded_math:\n"
    ".incbin \"" PI_INCLUDE_DIR "/pi_math.h\"\n"
    ".byte 0\n"
    ".global pi_embedded_push\n"
    "pi_embedded_push:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_push_kernels.hip\"\n"
    ".byte 0\n"
    ".global pi_embedded_expect\n"
    "pi_embedded_expect:\n"
    ".incbin \"" PI_CSRC_DIR "/pi_expect_kernels.hip\"\n"
    ".byte 0\n"
    ".text\n");

using pi::fail;
using pi::kXcds;

namespace {

const char* const kCompileFlags[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off",
                                     "-std=c++17"};

uint64_t fnv1a(const std::string& s, uint64_t h) {
    for (unsigned char c : s) {
        h ^= c;
        h *= 1099511628211ull;
    }
    return h;
}

float bits_to_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
uint32_t float_to_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// ---- exact division by a constant through its reciprocal --------------------------------
// The interpolation computes (s - lo) / span with span fixed per dimension.  The kernels replace
// the IEEE division by  t = a * y;  r = fma(-t, span, a);  q = fma(r, y, t)  with y = RN(1/span).
// That is the IEEE quotient for "almost all" operands (Markstein), but not provably for all, so
// it is enabled per divisor only after this exhaustive check: every one of the 2^23 float32
// significands of the dividend (the sequence is invariant under scaling the dividend by a power
// of two as long as nothing leaves the normal range, which the kernel guards, and under its sign).
__attribute__((target("fma"))) bool divisor_exact_fma(float span, float y) {
    for (uint32_t m = 0; m < (1u << 23); ++m) {
        const float a = bits_to_float(0x3F800000u | m);
        const float t = a * y;
        const float r = __builtin_fmaf(-t, span, a);
        const float q = __builtin_fmaf(r, y, t);
        if (q != a / span) return false;
    }
    return true;
}
bool divisor_exact_libm(float span, float y) {
    for (uint32_t m = 0; m < (1u << 23); ++m) {
        const float a = bits_to_float(0x3F800000u | m);
        const float t = a * y;
        const float r = std::fmaf(-t, span, a);
        const float q = std::fmaf(r, y, t);
        if (q != a / span) return false;
    }
    return true;
}

}  // namespace

bool pi::validate_fast_division(float span) {
    if (!(span >= 0x1p-30f && span <= 0x1p30f)) return false;
    static std::mutex mu;
    static std::map<uint32_t, bool> memo;
    std::lock_guard<std::mutex> lock(mu);
    auto it = memo.find(float_to_bits(span));
    if (it != memo.end()) return it->second;
    const float y = 1.0f / span;
    const bool ok = __builtin_cpu_supports("fma") ? divisor_exact_fma(span, y) : divisor_exact_libm(span, y);
    memo[float_to_bits(span)] = ok;
    return ok;
}

std::string pi::hex_float(float v) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%af", (double)v);
    return buf;
}

namespace {

// `fast_first`: the plugin text is instantiated a second time, as the member functions of PiCommonEnv, against the
// common-path-only math of include/pi_math.h (csrc/pi_sweep_kernels.hip, "common paths first").  Inside the struct the
// three names resolve to members that pass the struct's rare flag along, so step_dynamics and its helper functions
// share it through `this`.  The two inclusions are byte-identical copies of the caller's string.
// Not on 6-D grids: there the exact pass, which has to hold a cell's 64 corner values like the hot one, raises the
// kernels' register allocation past an occupancy step (25^6 evaluation: 112 -> 136 VGPRs, four waves -> three).
// Nor for a plugin whose text holds a word that means something else inside a struct than at file scope (`__constant__`
// data would silently become a per-instance member): such a plugin is built exactly as before.
bool fits_struct(const char* dynamics_src) {
    for (const char* word : {"__constant__", "__shared__", "__managed__", "static", "extern", "namespace", "template", "#include"})
        if (std::strstr(dynamics_src, word)) return false;
    return true;
}

std::string build_source(const pi_handle* h, const char* dynamics_src, bool fast_first) {
    std::ostringstream o;
    fast_first = fast_first && h->D <= 4 && fits_struct(dynamics_src);
    auto dec = [](int x) { return std::to_string(x); };
    auto list = [](const auto& v, auto fmt) { return pi::brace_list(v.data(), v.size(), fmt); };
    o << "// generated by libpi_mi355 for " << pi::kArch << "\n";
    o << "#define PI_BLOCK_EVAL " << h->block_eval << "\n";
    o << "#define PI_BLOCK_IMPROVE " << h->block_improve << "\n";
    o << "#define PI_RESIDENT_K " << h->resident_k << "\n";
    o << "#define PI_RESIDENT_BLOCK " << h->resident_block << "\n";
    if (h->flow) o << "#define PI_FLOW 1\n#define PI_FLOW_BLOCK " << h->flow_block << "\n";
    if (h->xcd) o << "#define PI_XCD 1\n#define PI_XCD_S " << h->xcd_states << "\n#define PI_XCD_RING " << pi::kXcdRing
                  << "\n#define PI_XCD_HOST_CTL_WORDS " << pi::kXcdCtlWords << "\n";
    if (h->debug_bounds) o << "#define PI_DEBUG_BOUNDS 1\n";
    o << "#define PI_D " << h->D << "\n";
    o << "#define PI_NA " << h->n_actions << "\n";
    o << "#define PI_GRID_INIT " << list(h->shape, dec) << "\n";
    o << "#define PI_LO_INIT " << list(h->lo, pi::hex_float) << "\n";
    o << "#define PI_SPAN_INIT " << list(h->span, pi::hex_float) << "\n";
    o << "#define PI_RCP_INIT " << list(h->rcp, pi::hex_float) << "\n";
    o << "#define PI_FASTDIV_INIT " << list(h->fastdiv, dec) << "\n";
    o << "#define PI_MEM_OF_INIT " << list(h->mem_of_user, dec) << "\n";
    // the pack kernel and the improvement kernels that read the pair table (PI_OPTION_PAIR_TABLE): what pi_compile decided
    // once it has run, what it would decide now before
    if (h->compiled ? h->pair_built : pi::pair_table_wanted(h)) o << "#define PI_PAIR_TABLE 1\n";
    if (fast_first) o << "#define PI_FAST_FIRST 1\n";
    o << pi_embedded_math << "\n";
    o << "#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n";
    o << "// ---- env plugin (user string) ----\n";
    o << dynamics_src << "\n";
    if (fast_first) {
        o << "// ---- env plugin again: common math paths only, rare arguments flagged ----\n";
        o << "#undef sinf\n#undef cosf\n#undef fmodf\n";
        o << "#define sinf pi_common_sinf\n#define cosf pi_common_cosf\n#define fmodf pi_common_fmodf\n";
        o << "struct PiCommonEnv {\n";
        o << "unsigned int pi_rare;\n";
        o << "__device__ __forceinline__ float pi_common_sinf(float x) { return pi_sinf_common(x, &pi_rare); }\n";
        o << "__device__ __forceinline__ float pi_common_cosf(float x) { return pi_cosf_common(x, &pi_rare); }\n";
        o << "__device__ __forceinline__ float pi_common_fmodf(float x, float y) { return pi_fmodf_common(x, y, &pi_rare); }\n";
        o << dynamics_src << "\n";
        o << "};\n";
        o << "#undef sinf\n#undef cosf\n#undef fmodf\n";
        o << "#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n";
    }
    o << "// ---- sweep kernels ----\n";
    o << pi_embedded_kernels << "\n";
    // the one-launch kernels of launch-bound grids (csrc/pi_onelaunch_kernels.hip): only where the grid qualifies, so
    // the translation units of the big grids stay ~1 000 lines shorter
    if (h->resident_k > 0 || h->flow || h->xcd) {
        o << "// ---- one-launch kernels ----\n";
        o << pi_embedded_onelaunch << "\n";
    }
    return o.str();
}

int load_module(pi_handle* h, const std::vector<char>& image) {
    h->dist_k = 0;                 // a new unit: the expectation module and the disturbance set go with the old one
    h->expect_built = false;
    if (h->device < 0) return 0;   // host-only handle: compile check only
    pi::DeviceGuard guard(h->device);
    pi::drop_graphs(h);
    if (h->module) {
        PI_HIP(hipModuleUnload(h->module));
        h->module = nullptr;
    }
    if (h->module_push) {
        PI_HIP(hipModuleUnload(h->module_push));
        h->module_push = nullptr;
        h->f_eval_push = nullptr;
        h->f_reach_pairs = nullptr;
    }
    if (h->module_expect) {
        PI_HIP(hipModuleUnload(h->module_expect));
        h->module_expect = nullptr;
        h->f_expect_eval = h->f_expect_improve = h->f_expect_value = nullptr;
        h->f_robust_eval = h->f_robust_improve = h->f_robust_value = nullptr;
    }
    PI_HIP(hipModuleLoadData(&h->module, image.data()));
    PI_HIP(hipModuleGetFunction(&h->f_eval, h->module, "pi_eval_sweep_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_eval_live, h->module, "pi_eval_live_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_policy_list, h->module, "pi_policy_list_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_scan_slots, h->module, "pi_scan_slots_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_mask_list, h->module, "pi_mask_list_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_improve, h->module, "pi_improve_sweep_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_improve_live, h->module, "pi_improve_live_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_value, h->module, "pi_value_sweep_kernel"));
    h->f_pack_pairs = h->f_improve_pairs = h->f_improve_live_pairs = nullptr;
    if (h->pair_built) {
        PI_HIP(hipModuleGetFunction(&h->f_pack_pairs, h->module, "pi_pack_pairs_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_improve_pairs, h->module, "pi_improve_sweep_pairs_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_improve_live_pairs, h->module, "pi_improve_live_pairs_kernel"));
    }
    PI_HIP(hipModuleGetFunction(&h->f_finalize, h->module, "pi_finalize_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_reach_planes, h->module, "pi_reach_planes_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_reach_units, h->module, "pi_reach_units_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_probe_step, h->module, "pi_probe_step_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_probe_interp, h->module, "pi_probe_interp_kernel"));
    PI_HIP(hipModuleGetFunction(&h->f_probe_coords, h->module, "pi_probe_coords_kernel"));
    h->f_run_resident = nullptr;
    if (h->resident_k > 0) {
        PI_HIP(hipModuleGetFunction(&h->f_resident, h->module, "pi_eval_resident_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_run_resident, h->module, "pi_run_resident_kernel"));
    }
    h->f_flow = h->f_flow_finish = nullptr;
    if (h->flow) {
        PI_HIP(hipModuleGetFunction(&h->f_flow, h->module, "pi_eval_flow_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_flow_finish, h->module, "pi_flow_finish_kernel"));
        // the kernel's workgroups wait for each other: all of them have to be resident at once.  The occupancy API may
        // answer 1-2 more per CU than the hardware admits (SGPR granules: MI355X_MICROARCH.md, "Residency"): margin.
        int per_cu = 0;
        const int64_t wgs = (h->n_states + h->flow_block - 1) / h->flow_block;
        if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, h->f_flow, h->flow_block, 0) != hipSuccess ||
            (int64_t)(per_cu * 3 / 4) * h->num_cu < wgs) {
            (void)hipGetLastError();
            h->f_flow = nullptr;
        }
    }
    h->f_xcd = h->f_xcd_finish = nullptr;
    if (h->xcd && h->f_flow) {
        PI_HIP(hipModuleGetFunction(&h->f_xcd, h->module, "pi_xcd_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_xcd_finish, h->module, "pi_xcd_finish_kernel"));
        // one workgroup per CU of one XCD, all resident at once: the kernel's LDS padding keeps a second one off a CU
        int regs = 0, lds = 0;
        const int64_t wgs = (h->n_states + h->xcd_states - 1) / h->xcd_states, cus = h->num_cu / kXcds;
        const bool ok = hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, h->f_xcd) == hipSuccess &&
                        hipFuncGetAttribute(&lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, h->f_xcd) == hipSuccess &&
                        wgs <= cus && lds > 80 * 1024 && lds <= 160 * 1024 && regs <= 128;
        if (!ok) {
            (void)hipGetLastError();
            h->f_xcd = nullptr;
        }
    }
    int v = 0;
    if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_NUM_REGS, h->f_eval) == hipSuccess) h->vgpr_eval = v;
    if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_NUM_REGS, h->f_improve) == hipSuccess)
        h->vgpr_improve = v;
    return 0;
}

}  // namespace

namespace pi {

// The handle's second module: the same translation unit + csrc/pi_push_kernels.hip, built (hipRTC, same cache) the
// first time an exchange plan wants the fused swept-first kernel.  Nothing else ever pays for it.
int ensure_push_module(pi_handle* h) {
    if (h->f_eval_push) return 0;
    if (!h->compiled || h->dynamics_src.empty()) return fail("ensure_push_module: pi_compile has not run on this handle");
    std::vector<char> image;
    const std::string src = build_source(h, h->dynamics_src.c_str(), h->fast_first) + "// ---- fused swept-first kernel ----\n" + pi_embedded_push + "\n";
    if (compile_image(src, h->has_cache_dir ? h->cache_dir.c_str() : nullptr, nullptr, 0, image, nullptr)) return 1;
    if (h->device < 0) return 0;            // host-only handle: compile check only
    DeviceGuard guard(h->device);
    PI_HIP(hipModuleLoadData(&h->module_push, image.data()));
    PI_HIP(hipModuleGetFunction(&h->f_eval_push, h->module_push, "pi_eval_push_kernel"));
    if (h->D >= 3) PI_HIP(hipModuleGetFunction(&h->f_reach_pairs, h->module_push, "pi_reach_pairs_kernel"));
    return 0;
}

// The handle's third module: the same translation unit + csrc/pi_expect_kernels.hip, built (hipRTC, same flags, same
// cache) by the first pi_set_disturbances after pi_compile.  A handle that never plans for noise never pays for it.
int ensure_expect_module(pi_handle* h) {
    if (h->expect_built) return 0;
    if (!h->compiled || h->dynamics_src.empty()) return fail("ensure_expect_module: pi_compile has not run on this handle");
    std::vector<char> image;
    const std::string src = build_source(h, h->dynamics_src.c_str(), h->fast_first) + "// ---- expected backup over a disturbance set ----\n" + pi_embedded_expect + "\n";
    if (compile_image(src, h->has_cache_dir ? h->cache_dir.c_str() : nullptr, nullptr, 0, image, nullptr)) return 1;
    if (h->device >= 0) {                  // host-only handle: compile check only
        DeviceGuard guard(h->device);
        PI_HIP(hipModuleLoadData(&h->module_expect, image.data()));
        PI_HIP(hipModuleGetFunction(&h->f_expect_eval, h->module_expect, "pi_expect_eval_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_expect_improve, h->module_expect, "pi_expect_improve_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_expect_value, h->module_expect, "pi_expect_value_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_robust_eval, h->module_expect, "pi_robust_eval_kernel"));       // the worst-case fold
        PI_HIP(hipModuleGetFunction(&h->f_robust_improve, h->module_expect, "pi_robust_improve_kernel"));
        PI_HIP(hipModuleGetFunction(&h->f_robust_value, h->module_expect, "pi_robust_value_kernel"));
    }
    h->expect_built = true;
    return 0;
}

// hipRTC (or the on-disk cache) -> code object image for one translation unit.
int compile_image(const std::string& src, const char* cache_dir, char* log, size_t log_len,
                  std::vector<char>& image, bool* cache_hit) {
    std::string flags;
    for (const char* f : kCompileFlags) { flags += f; flags += ' '; }
    int rtc_major = 0, rtc_minor = 0;                     // a new compiler invalidates the cache
    (void)hiprtcVersion(&rtc_major, &rtc_minor);
    flags += "hiprtc-" + std::to_string(rtc_major) + "." + std::to_string(rtc_minor);
    char name[64];
    std::snprintf(name, sizeof name, "pi_%016llx%016llx.hsaco",
                  (unsigned long long)fnv1a(src + flags, 14695981039346656037ull),
                  (unsigned long long)fnv1a(flags + src, 0x9e3779b97f4a7c15ull));
    std::string path;
    if (cache_hit) *cache_hit = false;
    if (cache_dir && cache_dir[0]) {
        path = std::string(cache_dir) + "/" + name;
        std::ifstream f(path, std::ios::binary);
        if (f) {
            image.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            if (!image.empty()) {
                if (cache_hit) *cache_hit = true;
                return 0;
            }
        }
    }
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "pi_sweep_kernels.hip", 0, nullptr, nullptr) !=
        HIPRTC_SUCCESS)
        return fail("hiprtcCreateProgram failed");
    const int n_flags = (int)(sizeof kCompileFlags / sizeof kCompileFlags[0]);
    hiprtcResult rc = hiprtcCompileProgram(prog, n_flags, const_cast<const char**>(kCompileFlags));
    size_t ls = 0;
    std::string clog;
    if (hiprtcGetProgramLogSize(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        clog.resize(ls);
        (void)hiprtcGetProgramLog(prog, &clog[0]);
    }
    if (log && log_len) std::snprintf(log, log_len, "%s", clog.c_str());
    if (rc != HIPRTC_SUCCESS) {
        (void)hiprtcDestroyProgram(&prog);
        return fail(std::string("hipRTC compile failed: ") + hiprtcGetErrorString(rc) + "\n" + clog);
    }
    size_t cs = 0;
    if (hiprtcGetCodeSize(prog, &cs) != HIPRTC_SUCCESS || cs == 0) {
        (void)hiprtcDestroyProgram(&prog);
        return fail("hiprtcGetCodeSize failed");
    }
    image.resize(cs);
    hiprtcResult rg = hiprtcGetCode(prog, image.data());
    (void)hiprtcDestroyProgram(&prog);
    if (rg != HIPRTC_SUCCESS) return fail("hiprtcGetCode failed");
    if (!path.empty()) {
        (void)mkdir(cache_dir, 0777);
        std::string tmp = path + ".tmp" + std::to_string((long long)getpid());
        std::ofstream f(tmp, std::ios::binary);
        if (f) {
            f.write(image.data(), (std::streamsize)image.size());
            f.close();
            if (std::rename(tmp.c_str(), path.c_str()) != 0) (void)std::remove(tmp.c_str());
        }
    }
    return 0;
}

}  // namespace pi

extern "C" {

int pi_compile(pi_handle* h, const char* dynamics_src, const char* cache_dir, char* log,
               size_t log_len) {
    pi::fail("");
    if (log && log_len) log[0] = 0;
    if (!h || !dynamics_src) return fail("null argument");
    std::vector<char> image;
    h->pair_built = pi::pair_table_wanted(h);      // fixed for this unit: an option set later does not change what was built
    // Common paths first: the plugin is instantiated twice (build_source).  A plugin that is legal at file scope but not
    // as the body of a struct (file-scope __constant__ data, static helpers, ...) is built exactly as before instead,
    // and the log says so; a plugin that does not compile either way fails with the diagnostics of the plain form.
    h->fast_first = fits_struct(dynamics_src);
    if (!h->fast_first || pi::compile_image(build_source(h, dynamics_src, true), cache_dir, log, log_len, image, &h->cache_hit)) {
        h->fast_first = false;
        image.clear();
        if (pi::compile_image(build_source(h, dynamics_src, false), cache_dir, log, log_len, image, &h->cache_hit)) return 1;
        pi::fail("");
        if (log && log_len && h->D <= 4) {
            const std::string rest = log;
            std::snprintf(log, log_len, "note: this plugin cannot be instantiated as member functions; its sweep kernels are built "
                          "without the common-path-first instantiation\n%s", rest.c_str());
        }
    }
    h->compiled = true;
    pi::resolve_strip(h);               // the memory order is final now
    h->dynamics_src = dynamics_src;
    h->has_cache_dir = cache_dir != nullptr;
    h->cache_dir = cache_dir ? cache_dir : "";
    return load_module(h, image);
}

size_t pi_kernel_source(pi_handle* h, const char* dynamics_src, char* buf, size_t buf_len) {
    if (!h || !dynamics_src) return 0;
    std::string s = build_source(h, dynamics_src, h->fast_first);
    if (buf && buf_len) {
        size_t k = std::min(buf_len - 1, s.size());
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size();
}

}  // extern "C"
