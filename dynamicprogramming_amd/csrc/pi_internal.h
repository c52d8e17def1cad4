// pi_internal.h — shared between the host sources of libpi_mi355.so.  Not part of the C ABI.  What lives where:
//   pi_knobs.cpp      the PI_MI355_* environment knobs: one table, the only readers of the environment (pi_knobs.h)
//   pi_api.cpp        error state, pi_create / pi_destroy and the dispatch policy, the sweep launchers and the graph cache,
//                     the sweep entry points, pi_set_option, pi_info
//   pi_probe.cpp      the reach and probe entry points
//   pi_compile.cpp    embedded device sources, reciprocal-division check, build_source, hipRTC + code-object cache, modules
//   pi_onelaunch.cpp  the one-launch families (dataflow, XCD-local, LDS-resident runs) and their scratch blocks
//   pi_live.cpp       the live-state list of pi_prepare_mask and the per-evaluation list of pi_eval_begin
//   pi_comm.cpp       multi-GPU transports and the sharded sweep driver;  pi_p2p.cpp  the peer-to-peer transport
//   pi_infer.cpp, pi_rollout.cpp   the inference handle and its rollouts;  pi_hybrid.cpp  rollouts that switch between two handles,
//                     deterministic and with the stochastic rollouts' stream inside
//   pi_resample.cpp   the inference handle's solution interpolated onto another grid (grid continuation)
//   pi_greedy.cpp     value-greedy control on the inference handle: one-step lookahead on V, queries and rollouts
//   pi_stochastic.cpp stochastic rollouts on the inference handle: random baseline, epsilon-random actions, noise (Philox)
//   pi_expect.cpp     the expected and the worst-case backup over a disturbance set: pi_set_disturbances, the pi_expect_*
//                     and the pi_robust_* sweeps (one host function per pair, parametrised on the kernel)
//   pi_expect_greedy.cpp  expected-value greedy control on the inference handle: the lookahead over a disturbance set
//   pi_adversary.cpp  the robust lookahead and the adversary rollout on the inference handle: the worst case over that set
//   pi_accel.cpp      Anderson-accelerated policy evaluation: the acceleration module, pi_accel_update and pi_accel_combine
#pragma once

#include "pi_knobs.h"
#include "pi_mi355.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

namespace pi {

int fail(const std::string& msg);                 // records the thread-local error, returns 1
const std::string& last_error();

#define PI_HIP(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return ::pi::fail(std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

constexpr int kProbeBlock = 256; // threads per workgroup of the probe kernels' host launches
constexpr int kXcds = 8;         // PI_NXCD
constexpr int kSlots = 256;      // PI_NSLOT
constexpr int kXcdCtlWords = 128 + 256;   // control block of the XCD-local kernel: PI_XCD_CTL_FLAGS + 2 banks x 64 flag granules
constexpr int kXcdRing = 64;              // granule versions of V the XCD-local kernel keeps (PI_XCD_RING)
constexpr const char* kArch = "gfx950";

// Where a kernel launch goes: onto a stream, or into a graph under construction as the node behind *prev.
struct LaunchTo {
    hipStream_t st = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphNode_t* prev = nullptr;
    LaunchTo(hipStream_t s) : st(s) {}
    LaunchTo(hipGraph_t g, hipGraphNode_t* p) : graph(g), prev(p) {}
};
struct Grid2 { unsigned x, y; };
// One kernel launch.  The arguments are taken BY VALUE and passed by address: the deduced type of every one of them must
// be the kernel's parameter type (an int64_t where the kernel takes an int is read wrong, silently).
template <typename... A>
hipError_t launch(hipFunction_t f, Grid2 grid, unsigned block, LaunchTo to, A... a) {
    void* args[] = {(void*)&a...};
    if (!to.graph) return hipModuleLaunchKernel(f, grid.x, grid.y, 1, block, 1, 1, 0, to.st, args, nullptr);
    hipKernelNodeParams p = {};
    p.func = (void*)f;
    p.gridDim = dim3(grid.x, grid.y, 1);
    p.blockDim = dim3(block, 1, 1);
    p.kernelParams = args;
    hipGraphNode_t node;
    const hipError_t e = hipGraphAddKernelNode(&node, to.graph, *to.prev ? to.prev : nullptr, *to.prev ? 1 : 0, &p);
    if (e == hipSuccess) *to.prev = node;
    return e;
}

// PI_*_INIT lists of the generated translation units: "{a,b,c}", floats as hexadecimal literals (%af)
std::string hex_float(float v);
template <typename T, typename F>
std::string brace_list(const T* v, size_t count, F fmt) {
    std::string r = "{";
    for (size_t i = 0; i < count; ++i) r += (i ? "," : "") + fmt(v[i]);
    return r + "}";
}

// Makes `device` current for the lifetime of the guard and restores the caller's device after.
struct DeviceGuard {
    int saved = -1;
    bool active = false;
    explicit DeviceGuard(int device) {
        if (device < 0) return;
        if (hipGetDevice(&saved) != hipSuccess) saved = -1;
        if (saved != device) active = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (active && saved >= 0) (void)hipSetDevice(saved);
    }
};

// Transport of a multi-rank run (pi_comm.cpp: RCCL and the in-process test transport; pi_p2p.cpp: peer-to-peer stores
// into IPC-mapped buffers).  send / recv between group_begin and group_end have the stream semantics of an RCCL group:
// everything enqueued on `st` before group_end is visible to the transfer, everything enqueued after it sees the result.
struct Comm {
    int rank = 0, world = 1;
    virtual ~Comm() {}
    virtual int transport() const = 0;                    // PI_TRANSPORT_* (pi_comm_info)
    virtual int group_begin() = 0;
    virtual int send(const void* p, size_t bytes, int peer, hipStream_t st) = 0;
    virtual int recv(void* p, size_t bytes, int peer, hipStream_t st) = 0;
    virtual int group_end(hipStream_t st) = 0;
    // every rank contributes `bytes` at full + rank * bytes; afterwards all ranks hold all
    virtual int allgather(void* full, size_t bytes, hipStream_t st) = 0;
    virtual int allreduce_max_f32(float* d, hipStream_t st) = 0;
    virtual int allreduce_sum_u32(uint32_t* d, hipStream_t st) = 0;
    // a sharded batch failed on this rank: stop peers of the same process from waiting (in-process transport)
    virtual void give_up() {}
    // Fused exchange (peer-to-peer transport only): the swept-first kernel stores its rows into the peers' buffers
    // itself (pi_eval_push_kernel), everything on the ONE stream the sweeps run on.  Per sweep:
    //   push_begin   "my receives are posted" to `senders`, wait for the same from `receivers` (one wave); returns the
    //                device table of the receivers' addresses of `local_dst` (the full V' buffer being written)
    //   <the caller launches the push kernel with that table>
    //   push_signal  raise the receivers' data counters — the kernel boundary in front of it is the release
    //   <the caller launches the interior>
    //   push_wait    wait for the senders' data counters (push_wait_deferred: leave it to the next sweep's push_begin, which
    //                then waits for both in its one launch)
    // Same message numbers as send / recv groups, so fused and unfused exchanges may alternate (all ranks alike).
    virtual bool can_push() const { return false; }
    virtual int push_begin(const std::vector<int>&, const std::vector<int>&, float*, float* const**, hipStream_t) { return 1; }
    virtual int push_signal(hipStream_t) { return 1; }
    virtual int push_wait(hipStream_t) { return 1; }
    // instead of push_wait when the very next call on the stream is the push_begin of another fused sweep
    virtual int push_wait_deferred(hipStream_t st) { return push_wait(st); }
};
struct ShardPlan;
struct P2pPending;   // pi_p2p.cpp: what pi_p2p_describe allocated for a pi_comm_init_p2p that has not happened yet

struct GraphEntry {               // one captured batch of evaluation sweeps
    const void *Va = nullptr, *Vb = nullptr, *policy = nullptr, *term = nullptr, *d_delta = nullptr;
    int64_t s_begin = 0, s_end = 0;
    float gamma = 0.0f;
    int n_sweeps = 0;
    hipGraphExec_t exec = nullptr;
    uint64_t stamp = 0;
};

}  // namespace pi

// The device sources and the math header, embedded verbatim (pi_compile.cpp)
extern "C" const char pi_embedded_kernels[];
extern "C" const char pi_embedded_onelaunch[];
extern "C" const char pi_embedded_math[];
extern "C" const char pi_embedded_push[];
extern "C" const char pi_embedded_expect[];
extern "C" const char pi_embedded_rollout[];      // pi_rollout.cpp
extern "C" const char pi_embedded_greedy[];       // pi_greedy.cpp
extern "C" const char pi_embedded_stochastic[];   // pi_stochastic.cpp

struct pi_handle {
    int device = -1;
    int D = 0;
    int n_actions = 0;
    int64_t n_states = 0;
    std::vector<int32_t> shape;
    std::vector<float> lo, span, rcp;
    std::vector<int> fastdiv;
    // Memory order of the dimensions (PI_OPTION_MEMORY_ORDER): memory dimension k (0 = slowest) is user dimension user_of_mem[k];
    // user dimension d lives in memory dimension mem_of_user[d].  shape / lo / span / rcp / fastdiv / the bin tables
    // are kept in MEMORY order; every flat state index of the C ABI is an index in that order.  Identity by default.
    std::vector<int> mem_of_user, user_of_mem;
    bool compiled = false;               // pi_compile has run: the memory order can no longer change
    std::vector<float> tab;              // actions | bins_0 | bins_1 | ...
    float* d_tab = nullptr;
    unsigned int* d_slots = nullptr;     // 2 x kSlots accumulator words: residual bits | changed
    hipModule_t module = nullptr;
    // second module, built on demand from the same translation unit + csrc/pi_push_kernels.hip (ensure_push_module)
    hipModule_t module_push = nullptr;
    hipFunction_t f_eval_push = nullptr, f_reach_pairs = nullptr;
    std::string dynamics_src, cache_dir; // what pi_compile was given (for the second module)
    // third module, built by the first pi_set_disturbances after pi_compile from the same translation unit +
    // csrc/pi_expect_kernels.hip (ensure_expect_module); expect_built: that build went through (host-only handles: it
    // compiled).  The disturbance set in use (pi_expect.cpp): dist_k points (0: none), d_dist their table, 64 rows of
    // {da, dx_0 .. dx_{D-1}, p} (owned, allocated once), dist_a_min / _a_max the extremes of the action table
    hipModule_t module_expect = nullptr;
    hipFunction_t f_expect_eval = nullptr, f_expect_improve = nullptr, f_expect_value = nullptr;
    hipFunction_t f_robust_eval = nullptr, f_robust_improve = nullptr, f_robust_value = nullptr;   // same module: min over the set
    bool expect_built = false;
    int dist_k = 0;
    float* d_dist = nullptr;
    float dist_a_min = 0.0f, dist_a_max = 0.0f;
    // fourth module, built by the first pi_accel_update / pi_accel_combine from csrc/pi_accel_kernels.hip alone (pi_accel.cpp:
    // it depends on neither the grid nor the env, so a later pi_compile keeps it); accel_built: that build went through
    // (host-only handles: it compiled).  d_accel_part: 17 rows of accel_tiles float64 tile partials (owned, grown on demand)
    hipModule_t module_accel = nullptr;
    hipFunction_t f_accel_update = nullptr, f_accel_update_vec = nullptr, f_accel_fold = nullptr, f_accel_combine = nullptr,
                  f_accel_combine_vec = nullptr;
    bool accel_built = false;
    double* d_accel_part = nullptr;
    int64_t accel_tiles = 0;
    bool has_cache_dir = false;
    bool fast_first = true;              // the unit holds the plugin's common-path instantiation too (pi_compile clears it for a plugin that cannot take that form)
    hipFunction_t f_eval = nullptr, f_eval_live = nullptr, f_policy_list = nullptr, f_scan_slots = nullptr, f_mask_list = nullptr, f_improve = nullptr, f_improve_live = nullptr, f_value = nullptr, f_finalize = nullptr,
                  f_reach_planes = nullptr, f_reach_units = nullptr, f_probe_step = nullptr, f_probe_interp = nullptr,
                  f_probe_coords = nullptr, f_resident = nullptr, f_run_resident = nullptr;
    int num_cu = 0;
    int block_eval = 256, block_improve = 256;   // threads per workgroup = states per chunk
    int cpw_eval = 1, cpw_improve = 1;           // chunks a workgroup sweeps
    // Strip schedule of the sweeps (PI_OPTION_STRIP_STATES, PI_MI355_STRIP): states per period — a plane of a slow memory
    // dimension; every XCD takes its eighth of every period.  0 = the slab schedule (an XCD walks one contiguous run).
    int64_t strip_states = 0;
    int64_t strip_mode = -1;             // -1 the library's choice (resolve_strip), 0 off, > 0 states per period as given
    int vgpr_eval = -1, vgpr_improve = -1;
    // Pair table of the improvement sweeps (PI_OPTION_PAIR_TABLE; csrc/pi_sweep_kernels.hip, PI_PAIR_TABLE).  pair_mode: -1 the
    // library's choice (pi::pair_table_wanted), 0 off, 1 on where the grid admits it.  pair_built: the unit pi_compile built
    // holds the pack kernel and the two table kernels.  d_pairs: the 8 n-byte table (owned), allocated by the first sweep
    // that takes the path; pair_alloc_failed: that allocation failed once — the plain path from then on, logged once.
    // pair_last: the last improvement sweep read the table (PI_INFO_PAIR_TABLE).
    int pair_mode = -1;
    bool pair_built = false, pair_alloc_failed = false, pair_last = false;
    hipFunction_t f_pack_pairs = nullptr, f_improve_pairs = nullptr, f_improve_live_pairs = nullptr;
    float* d_pairs = nullptr;
    bool cache_hit = false;
    bool debug_bounds = false;           // PI_MI355_DEBUG=1 at pi_create: checked kernels (pi_debug_report)
    bool use_graphs = true;
    // LDS-resident evaluation batches (grids of up to ~12 k states): states per thread of the one
    // workgroup (resident_block threads), 0 = this grid is too big; the switch is PI_OPTION_RESIDENT
    int resident_k = 0, resident_block = 1024;
    bool use_resident = true;
    // Dataflow evaluation (pi_eval_flow_kernel): launch-bound grids that do not fit one CU's LDS run a whole policy
    // evaluation in one launch, the iterates travelling between workgroups as tagged granules.  flow: this grid
    // qualifies; f_flow is null when the occupancy query does not admit all workgroups at once.  d_flow: ring of 16
    // granule versions | progress words + status | check slots (owned; flow_bytes).
    bool flow = false;
    int flow_block = 256;
    hipFunction_t f_flow = nullptr, f_flow_finish = nullptr;
    void* d_flow = nullptr;
    size_t flow_bytes = 0;
    // XCD-local evaluation / whole run (pi_xcd_kernel, csrc/pi_onelaunch_kernels.hip): one 1 024-thread workgroup per CU of
    // ONE XCD, the iterates as tagged granules through that XCD's L2, flag granules as the barrier every 32nd sweep.
    // xcd: this grid qualifies; xcd_off: switched off after repeated failures (pi_policy_evaluation counts its own; a failed
    // whole run is reported back through PI_OPTION_XCD_RUN_FAILED).  d_xcd: ring of kXcdRing versions | scratch policy | control
    // words (owned).  Counters for PI_INFO_XCD_ENABLED - PI_INFO_WHOLE_RUNS.
    bool xcd = false, xcd_off = false;
    int xcd_states = 1024;                               // states per workgroup (PI_XCD_S)
    hipFunction_t f_xcd = nullptr, f_xcd_finish = nullptr;
    void* d_xcd = nullptr;
    size_t xcd_bytes = 0;
    int64_t xcd_used = 0, xcd_failed = 0, whole_runs = 0;
    std::vector<pi::GraphEntry> graphs;
    uint64_t graph_clock = 0;
    // pi_prepare_mask: the non-terminal states of the mask at live_term, ascending (device, owned); in use only
    // when visiting them instead of all states saves enough idle lanes (live_count > 0)
    const uint8_t* live_term = nullptr;
    int32_t* d_live = nullptr;
    int64_t live_count = 0;
    bool live_force = false;             // PI_OPTION_KEEP_LIVE_LIST: keep the list whatever the share of idle lanes
    int64_t live_lo = 0, live_hi = 0;    // the state range the list covers (pi_prepare_mask_range; the whole grid otherwise)
    // pi_eval_begin .. pi_eval_end: the live states that bootstrap under the policy at eval_policy (device list,
    // capacity live_count); eval_count < 0: none.  eval_holds: buffers every live state of which has been written
    // by a full sweep since pi_eval_begin — a sweep may use the shorter list only between two such buffers.
    int32_t* d_eval_list = nullptr;
    unsigned long long* d_eval_cursor = nullptr;     // per-block survivor counts -> offsets (+ total)
    int64_t eval_count = -1;
    const int32_t* eval_policy = nullptr;
    std::vector<const float*> eval_holds;
    std::vector<uint64_t> live_bits;     // host: bit s of word s / 64 = state s is live (30 MB for 25^6)
    std::vector<int64_t> live_before;    // host: live states before each 64-state block -> list position of any state
    pi::Comm* comm = nullptr;            // multi-GPU transport (owned; pi_comm.cpp), null = single rank
    pi::ShardPlan* plan = nullptr;       // exchange plan (owned; pi_comm.cpp)
    pi::P2pPending* p2p_pending = nullptr;   // pi_p2p_describe without its pi_comm_init_p2p yet (owned; pi_p2p.cpp)
};

namespace pi {
// One rollout module of an inference handle: a code object built on demand by a pi_infer_set_* call, and the action table
// that call brought, where it brings one.
struct InferModule {
    hipModule_t module = nullptr;
    hipFunction_t f_rollout = nullptr, f_query = nullptr;   // its rollout kernel; its batched-query kernel, if it has one
    bool ready = false;                  // the pi_infer_set_* call went through (host-only handles: the unit compiled)
    float* d_actions = nullptr;          // the action table of that call (owned: a handle without a policy has no other)
    int n_actions = 0;
    float a_min = 0.0f, a_max = 0.0f;    // the table's extremes
};
}  // namespace pi

// One inference handle (pi_infer.cpp; the rollout entry points on it: pi_rollout.cpp).
struct pi_infer {
    int device = -1;
    int D = 0;
    int64_t n_corners = 0, n_states = 0;
    int n_actions = 0;
    hipModule_t module = nullptr;
    hipFunction_t f = nullptr;
    float* d_actions = nullptr;
    int32_t* d_policy = nullptr;
    // what pi_infer_create was given, for the modules built later: the grid as the generated
    // defines of the translation unit (PI_D, PI_LO_INIT, ... PI_BITS_INIT) and the code-object cache
    std::string grid_defines, cache_dir;
    bool has_cache_dir = false;
    std::string dynamics_src;            // the plugin of the last pi_infer_set_dynamics, for the modules built after it
    std::vector<int32_t> corner_bits;    // what pi_infer_create was given: both handles of a hybrid rollout share it
    // The rollout modules (pi::InferModule, above; pi::build_infer_module assembles their translation units).  Every one
    // is this grid + pi_math.h + the env plugin + csrc/pi_rollout_kernels.hip, and then
    //   rollout        (pi_infer_set_dynamics, pi_rollout.cpp)             nothing more: pi_rollout_kernel
    //   hybrid         (pi_infer_set_partner, pi_hybrid.cpp)               a partner's grid + csrc/pi_hybrid_kernels.hip;
    //                  partner_defines: the partner grid it was built for
    //   greedy         (pi_infer_set_greedy, pi_greedy.cpp)                csrc/pi_greedy_kernels.hip; its launches read d_values
    //   stochastic     (pi_infer_set_stochastic, pi_stochastic.cpp)        csrc/pi_stochastic_kernels.hip; f_query is
    //                  pi_random_words_kernel; the table is what exploring steps draw from, its extremes clamp a noisy action
    //   expect_greedy  (pi_infer_set_expect_greedy, pi_expect_greedy.cpp)  the functions of the greedy and the stochastic
    //                  file + csrc/pi_expect_greedy_kernels.hip; the extremes clamp a + da_k and a noisy action
    //   hybrid_stochastic  (pi_infer_set_partner_stochastic, pi_hybrid.cpp)  a partner's grid + the functions of the hybrid
    //                  and the stochastic file + csrc/pi_hybrid_stochastic_kernels.hip; the table is the pair's exploration
    //                  table; partner_stochastic_defines: the partner grid it was built for
    //   robust         (pi_infer_set_robust, pi_adversary.cpp)             the functions of the greedy file +
    //                  csrc/pi_adversary_kernels.hip: the robust lookahead (f_query) and the adversary rollout over the set
    //                  of pi_infer_set_disturbances; the extremes clamp a + da_k
    // A new plugin unloads the six that were built on the one before it.
    pi::InferModule rollout, hybrid, greedy, stochastic, expect_greedy, hybrid_stochastic, robust;
    std::string partner_defines, partner_stochastic_defines;
    // the resample module (pi_infer_set_values, pi_resample.cpp): this grid + csrc/pi_resample_kernels.hip, and the value
    // function of the solution.  d_resample_tab: the destination's bin tables | action map of the last pi_infer_resample
    // (owned; resample_tab: the same words on the host — a call that brings the same destination uploads nothing)
    hipModule_t module_resample = nullptr;
    hipFunction_t f_resample = nullptr, f_resample_wide = nullptr;
    bool has_values = false;             // pi_infer_set_values went through (host-only handles: the module compiled)
    float* d_values = nullptr;
    uint32_t* d_resample_tab = nullptr;
    size_t resample_tab_capacity = 0;    // words allocated at d_resample_tab
    std::vector<uint32_t> resample_tab;
    // the disturbance set of that controller (pi_infer_set_disturbances): K rows of {da, dx_0 .. dx_{D-1}, p} at d_dist,
    // a buffer of 64 rows allocated by the first call; dist_k == 0: no set.  Independent of the module
    float* d_dist = nullptr;
    int dist_k = 0;
};

namespace pi {

int check_ready(const pi_handle* h);
int check_range(const pi_handle* h, int64_t s_begin, int64_t s_end);
// One evaluation sweep over [s_begin, s_end) WITHOUT the finalize step: the residual stays in the
// accumulator slots (want_delta) until finalize_delta is called, so several sub-range launches of
// one logical sweep can share it.
// keep_terminals: Vnew already holds the terminal states' values (every sweep of a ping-pong batch but the
// first), so the sweep neither copies them nor streams old values for them.
int launch_eval(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, const uint8_t* term,
                int64_t s_begin, int64_t s_end, float gamma, bool want_delta, LaunchTo to,
                bool keep_terminals = false);
int finalize(pi_handle* h, float* d_delta, uint32_t* d_changed, LaunchTo to);
int zero_outputs(float* d_delta, uint32_t* d_changed, hipStream_t st);   // a sweep over an empty range: zero the outputs given
// The live-state list of pi_prepare_mask.  live_usable: a list is in use, `term` is the mask it was built from and
// [s_begin, s_end) lies inside the range it covers.
// live_span: the run of list entries whose states lie in [s_begin, s_end).  launch_eval_live: one evaluation sweep
// over `count` list entries from position `first` — for sweeps that need not copy terminal values.
bool live_usable(const pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end);
void live_span(const pi_handle* h, int64_t s_begin, int64_t s_end, int64_t* first, int64_t* count);
void live_states(const pi_handle* h, int64_t s_begin, int64_t s_end, std::vector<int32_t>& out);   // appends, ascending
// list_total (lists the caller passes): what the list would count over the whole grid, for the strip schedule; 0 = slab
int launch_eval_live(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, int64_t first, int64_t count,
                     float gamma, bool want_delta, hipStream_t st, const int32_t* list = nullptr, int64_t list_total = 0);
int64_t live_list_total(const pi_handle* h, int64_t entries);
// PiSched of pi_sweep_kernels.hip (same layout) and the planner that fills it: the launch grid (x, y)
struct Sched {
    int cpw;
    unsigned int period, phase;
};
Grid2 plan_launch(const pi_handle* h, int block, int64_t first, int64_t count, int64_t total, int cpw, Sched* sc);
// pi_eval_push_kernel over `count` entries of `list` with their destination masks: V'(s) goes to Vnew[s] and to
// peers[j][s] for every bit j of dest[k] (ensure_push_module builds the kernel the first time)
int ensure_push_module(pi_handle* h);                                      // pi_compile.cpp
int ensure_expect_module(pi_handle* h);                                    // pi_compile.cpp: the module of pi_set_disturbances
unsigned launch_blocks(int block, int64_t count, int cpw);                 // slab schedule: workgroups for `count` units
int launch_eval_push(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, const int32_t* list,
                     const uint8_t* dest, float* const* d_peers, int n_peers, int64_t count, float gamma, bool want_delta,
                     hipStream_t st);
// Reach of [s_begin, s_end) under all actions in pairs (i_0, i_v), v = the memory dimension of the user's dimension 1:
// bit i_0 * g_v + i_v of d_bitmap (zeroed by the caller; g_0 * g_v bits).  Second module; 3-D and up, g_0 * g_v <= 2^17.
bool pairs_possible(const pi_handle* h);
int reach_pairs(pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end, uint32_t* d_bitmap, hipStream_t st);
void drop_eval_list(pi_handle* h);     // the policy may have changed: forget the per-evaluation list
void release_comm(pi_handle* h);      // pi_comm.cpp: tears down the transport and the exchange plan
void drop_p2p_pending(pi_handle* h);  // pi_p2p.cpp
void drop_graphs(pi_handle* h);       // the cached graphs hold launch geometry and kernel handles: forget them
bool pair_table_wanted(const pi_handle* h);   // pi_api.cpp: does this handle's unit get the pair-table kernels?
void resolve_strip(pi_handle* h);     // strip_mode -> strip_states (the library's choice needs the final memory order)
bool validate_fast_division(float span);   // pi_compile.cpp: is the reciprocal division exact for this divisor?
// hipRTC (gfx950, -O3 -ffp-contract=off) or the on-disk code-object cache -> image of one translation unit
int compile_image(const std::string& src, const char* cache_dir, char* log, size_t log_len,
                  std::vector<char>& image, bool* cache_hit);
// pi_rollout.cpp: the argument rules pi_infer_rollout and pi_infer_rollout_hybrid share (m, n_steps, traj_every, the
// 63-bit size, d_start, alignment).  0: launch `*blocks` workgroups; 1: refused (pi::fail was called); 2: m == 0, nothing to do
int check_rollout_args(int D, const float* d_start, int64_t m, int n_steps, const float* d_final, const float* d_traj,
                       int traj_every, int64_t* blocks);
// pi_rollout.cpp: what the six rollout modules share.  build_infer_module assembles a translation unit — `leading` (the
// module's defines and the grid(s)), pi_math.h, the sinf / cosf / fmodf defines, `plugin`, then every part behind its
// "// ---- <section> ----" line — and compiles it with the handle's code-object cache.
struct UnitPart {
    const char *section, *text;
};
int build_infer_module(const pi_infer* h, const std::string& leading, const std::string& plugin,
                       std::initializer_list<UnitPart> parts, char* log, size_t log_len, std::vector<char>& image);
// the rules of an action table: not null, at least one entry and, where `finite`, every entry finite (`who` names the caller
// in that message); fills values, n and the extremes
struct ActionTable {
    const float* values = nullptr;
    int n = 0;
    float a_min = 0.0f, a_max = 0.0f;
};
int check_action_table(const char* who, bool finite, const float* action_space, int n_actions, ActionTable* table);
int unload(pi_infer* h, InferModule& mod);      // waits for the device, unloads the module, clears `ready`
// replaces `mod` by `image`: unload, then (on a device) the upload of `table` if there is one, the load and the two kernels
// by name (`query` may be null); sets `ready`
int install(pi_infer* h, InferModule& mod, const std::vector<char>& image, const ActionTable* table, const char* rollout,
            const char* query);
// pi_stochastic.cpp: the rules of epsilon, action_noise, state_noise and gamma that both stochastic rollouts share
struct StateNoise {                     // PiStateNoise of pi_stochastic_kernels.hip
    float v[6];
};
struct StochasticArgs {
    StateNoise noise = {};
    int any_noise = 0;
    unsigned int eps24 = 0;
};
int check_stochastic_args(const char* who, int D, float epsilon, float action_noise, const float* state_noise, float gamma,
                          StochasticArgs* out);
// pi_expect.cpp: the rules of a disturbance set, shared by pi_set_disturbances and pi_infer_set_disturbances (`who`).
// 0: `table` holds K rows of {da, dx_0 .. dx_{D-1}, p}, null offsets as zeros (K == 0: empty); 1: refused (pi::fail was called)
constexpr int kMaxDisturbances = 64;    // PI_NOISE_MAX
int build_disturbance_table(const char* who, int D, int K, const float* action_offsets, const float* state_offsets,
                            const float* weights, std::vector<float>& table);

}  // namespace pi
