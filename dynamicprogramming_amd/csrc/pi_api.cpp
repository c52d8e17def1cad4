// pi_api.cpp — host side of libpi_mi355.so: error state, handle management (pi_create's dispatch policy), the sweep
// launchers and the graph cache, the sweep entry points, options and info.
// The C ABI is declared (with reference citations) in include/pi_mi355.h; pi_internal.h says which file holds the rest.

#include "pi_internal.h"

#include <algorithm>
#include <cstdio>

namespace pi {

static thread_local std::string g_error;

int fail(const std::string& msg) {
    g_error = msg;
    return 1;
}
const std::string& last_error() { return g_error; }

// The strip period the sweeps of this handle use (PiSched): strip_mode > 0 as given, 0 none, -1 the library's choice,
// from measurements on MI355X (profiles/r06/strip_schedule.txt):
//  * 6-D grids of >= 2^24 states: ~2^21 states, a whole number of (i0, i1) sub-planes (25^6: five of them, 1 953 125
//    states): evaluation -4 to -5 %, improvement -1 to -7 %.  Not an L2 effect — L2 <-> fabric traffic goes UP by a third —
//    but an Infinity-Cache one: V (977 MB) does not fit it, and with all eight XCDs inside the same few sub-planes what
//    they re-read from the neighbouring planes was fetched by SOME XCD a moment ago; under the slab schedule eight
//    separate 122 MB regions stream through the 256 MB cache at once and the re-reads go to HBM.
//  * 4-D grids: off.  On 80^4 a period of one theta_1 plane cuts the traffic past L2 from 1.64x to 1.17x of the compulsory
//    bytes (V fetched 1.5x instead of 2.9x per sweep), and the evaluation sweep gets 3 % SLOWER (0.357 -> 0.369 ms,
//    improvement unchanged) at every launch geometry: that sweep does not wait for L2 misses (V fits the Infinity Cache).
void resolve_strip(pi_handle* h) {
    if (h->strip_mode >= 0) { h->strip_states = h->strip_mode; return; }
    h->strip_states = 0;
    if (h->D == 6 && h->n_states >= (int64_t(1) << 24)) {
        const int64_t sub = h->n_states / ((int64_t)h->shape[0] * h->shape[1]);
        h->strip_states = sub * std::max<int64_t>(1, ((int64_t(1) << 21) + sub / 2) / sub);
    }
}

// Pair table of the improvement sweeps (csrc/pi_sweep_kernels.hip, PI_PAIR_TABLE): which units get its kernels.  The grid
// has to admit it — 4-D (in 6-D the doubled footprint loses, profiles/r03/negative_results.txt (18); 2-D has one pair load
// per backup as it is) and 8 n < 2^32, so that the table's byte offsets stay 32-bit —, and the caller or the library has to
// want it: PI_OPTION_PAIR_TABLE 1, or -1 (the default) on grids of at least kPairTableMinStates states, the class of grids
// on which it was measured to pay (profiles/r11/pair_table_ab.txt).
constexpr int64_t kPairTableMinStates = int64_t(1) << 24;
bool pair_table_wanted(const pi_handle* h) {
    if (h->D != 4 || h->n_states * 8 >= (int64_t(1) << 32)) return false;
    return h->pair_mode == 1 || (h->pair_mode < 0 && h->n_states >= kPairTableMinStates);
}

void drop_graphs(pi_handle* h) {
    for (auto& g : h->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    h->graphs.clear();
}

// Workgroups for a range: one per group of `cpw` chunks, rounded up so that every XCD gets the
// same number (the kernels' chunk schedule deals groups to XCDs in contiguous runs).
unsigned launch_blocks(int block, int64_t count, int cpw) {
    const int64_t chunks = (count + block - 1) / block;
    const int64_t groups = (chunks + cpw - 1) / cpw;
    const int64_t span = (groups + kXcds - 1) / kXcds;
    return (unsigned)std::max<int64_t>(span * kXcds, kXcds);
}

// The schedule of one sweep launch over `count` units (states of a range, or entries of a state list) starting at unit
// `first` of `total` units that stand for the handle's whole grid (a list of live states: its length; a state range: n).
// Strip schedule (PiSched in pi_sweep_kernels.hip; a two-dimensional launch: y = period, x = 8 r + XCD) when the handle
// has a strip period and it comes to at least 16 groups of this launch's size; the slab schedule otherwise.  Periods are planes of a slow memory dimension, counted in states;
// for a list the same share of the list (exact where every plane lists the same number of states — a terminal set that
// depends on the fast dimensions only —, approximate otherwise: placement only, every group is still taken exactly once).
Grid2 plan_launch(const pi_handle* h, int block, int64_t first, int64_t count, int64_t total, int cpw, Sched* sc) {
    sc->cpw = cpw;
    sc->period = sc->phase = 0u;
    const int64_t group = (int64_t)block * cpw;
    const int64_t groups = ((count + block - 1) / block + cpw - 1) / cpw;
    if (h->strip_states > 0 && total > 0) {
        const double units = (double)h->strip_states * ((double)total / (double)h->n_states);
        const int64_t T = (int64_t)(units / (double)group + 0.5);
        if (T >= 16 && T < (int64_t(1) << 24) && groups > T) {
            const int64_t seg = (T + kXcds - 1) / kXcds;
            const int64_t phase = (first / group) % T;
            const int64_t periods = (groups + phase + T - 1) / T;
            if (periods <= 65535 && periods * T < (int64_t(1) << 31)) {      // gridDim.y; the kernel's 32-bit group number
                sc->period = (unsigned)T;
                sc->phase = (unsigned)phase;
                return Grid2{(unsigned)(seg * kXcds), (unsigned)periods};
            }
        }
    }
    return Grid2{launch_blocks(block, count, cpw), 1u};
}

}  // namespace pi

using namespace pi;

namespace {

unsigned int* delta_slots(pi_handle* h) { return h->d_slots; }
unsigned int* changed_slots(pi_handle* h) { return h->d_slots + kSlots; }

// Everything the handle owns on its device (pi_destroy, and pi_create when an allocation fails)
void free_device_state(pi_handle* h) {
    drop_graphs(h);
    if (h->module) (void)hipModuleUnload(h->module);
    if (h->module_push) (void)hipModuleUnload(h->module_push);
    if (h->module_expect) (void)hipModuleUnload(h->module_expect);
    if (h->module_accel) (void)hipModuleUnload(h->module_accel);
    for (void* p : {(void*)h->d_tab, (void*)h->d_slots, (void*)h->d_live, (void*)h->d_eval_list, (void*)h->d_eval_cursor,
                    h->d_flow, h->d_xcd, (void*)h->d_pairs, (void*)h->d_dist, (void*)h->d_accel_part})
        if (p) (void)hipFree(p);
}

// pi_create, step 3: the tables and the accumulator slots on the device, the number of CUs
int allocate_device_state(pi_handle* h) {
    h->num_cu = 256;
    if (h->device < 0) return 0;
    pi::DeviceGuard guard(h->device);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, h->device);
    if (e == hipSuccess && std::string(prop.gcnArchName).rfind(pi::kArch, 0) != 0)
        return fail(std::string("pi_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_tab, h->tab.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, h->tab.data(), h->tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_slots, 2 * kSlots * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(h->d_slots, 0, 2 * kSlots * sizeof(unsigned int));
    if (e != hipSuccess) {
        free_device_state(h);
        return fail(std::string("pi_create: ") + hipGetErrorString(e));
    }
    h->num_cu = prop.multiProcessorCount;
    return 0;
}

// pi_create, step 2: every launch-geometry and one-launch decision for this grid, with every knob that bears on one.
// tests/test_edge_dispatch.py pins the outcome (helpers.DISPATCH_TABLE).
void choose_dispatch(pi_handle* h) {
    const int D = h->D;
    const int64_t n = h->n_states;
    // Launch geometry (profiles/r02/block_cpw_sweep.txt): big 4-D grids sweep best with 1024-thread
    // workgroups taking two chunks each (evaluation: the 16 waves' corner rows overlap in one L1)
    // and 512-thread ones taking one (improvement); 6-D grids (64 corners, register-heavy) and
    // smaller grids keep 256-thread workgroups, two chunks each once there are enough chunks
    // (big 6-D grids: four and three, below).
    const bool big = D <= 4 && n >= (int64_t(1) << 24);
    h->block_eval = knob_int(Knob::EVAL_BLOCK, big ? 1024 : 256);          // any whole number of waves, 256..1024 threads
    h->block_improve = knob_int(Knob::IMPROVE_BLOCK, big ? 512 : 256);
    // 6-D grids of >= 2^24 states: four chunks per evaluation workgroup and three per improvement workgroup
    // (profiles/r03/block_cpw_sweep_6d.txt: 4.19 -> 4.11 ms and 9.05 -> 8.52 ms at 25^6).  Re-run under the strip schedule in
    // round 6 (profiles/r06/cpw_sweep_6d.txt): 6 or 8 evaluation chunks measure 1-2 % faster on one box (2.726 / 2.702 /
    // 2.668 ms on the double cartpole, 4.516 / 4.474 / 4.510 on its swing-up variant) but the workgroups' wider window costs
    // L2 hits — the swing-up sweep fetches 18.2 GB past L2 instead of 11.7 GB for the same 4.52 ms under the profiler
    // (cpw_sweep_6d.txt, second table) — so four stay
    const bool big6 = D == 6 && n >= (int64_t(1) << 24);
    h->cpw_eval = knob_int(Knob::EVAL_CPW, big6 ? 4 : n >= (int64_t(1) << 20) ? 2 : 1);
    h->cpw_improve = knob_int(Knob::IMPROVE_CPW, big6 ? 3 : 1);
    h->use_graphs = knob_int(Knob::GRAPHS) != 0;
    h->strip_mode = knob_count(Knob::STRIP, n);                   // states per period | 0 (slab schedule) | -1: auto
    h->debug_bounds = knob_int(Knob::DEBUG) != 0;
    // Small grids: the whole value table in LDS, one 1024-thread workgroup runs a batch of sweeps
    // (pi_eval_resident_kernel).  The limits keep table + per-state registers inside one CU.
    const int64_t resident_max = D == 2 ? 12288 : D == 4 ? 4096 : 1024;
    h->resident_block = D == 2 ? 1024 : 512;
    h->resident_k = (n <= resident_max && knob_int(Knob::RESIDENT))
                        ? (int)((n + h->resident_block - 1) / h->resident_block) : 0;
    // Launch-bound grids beyond that (BASELINE config C2, pendulum 200 x 200): the dataflow kernel, one launch per policy
    // evaluation across ceil(n / 256) workgroups (pi_eval_flow_kernel).  Per sweep it moves 2^D granules of 8 bytes per
    // state past L2, so it only pays while a sweep is launch-bound: up to 2^17 states in 2-D and 4-D.
    // 2-D grids of up to 2^16 states among those run on the CUs of ONE XCD instead (pi_xcd_kernel: hand-off through that
    // XCD's L2, the whole run in one launch), with the dataflow kernel behind it — and so do the bigger ones of the grids
    // one CU holds: beyond ~4 000 states 32 CUs are faster than one (pendulum 80 x 80: 0.9 against 1.3 us per sweep,
    // 110 x 110: 1.2 against 2.9), the LDS-resident kernel stays their fallback and serves their sweep batches.
    const bool one_launch = knob_int(Knob::RESIDENT) != 0;
    const bool xcd_wanted = one_launch && D == 2 && n <= (int64_t(1) << 16) && knob_int(Knob::XCD) != 0;
    const int64_t flow_min = xcd_wanted ? std::min<int64_t>(resident_max, 4096) : resident_max;
    const int64_t flow_max = D <= 4 ? (int64_t(1) << 17) : 0;
    h->flow = one_launch && n > flow_min && n <= flow_max;    // PI_MI355_RESIDENT=0 switches all one-launch kernels off
    h->xcd = h->flow && xcd_wanted;
    h->xcd_states = (int)(((n + 31) / 32 + 31) / 32 * 32);  // states per workgroup: n over 32 CUs, whole 128-byte lines
}

// A batch of evaluation sweeps as one hipGraph (kernel nodes built explicitly, so it also works
// when the caller's stream is the legacy default stream, where stream capture is not allowed).
// Small grids are launch-bound: an eager hipModuleLaunchKernel costs the host 3-5 us, a replayed
// graph node ~1.5 us (MI355X_MICROARCH.md, rows "boundary" and "graph-replay-floor").
int build_eval_graph(pi_handle* h, float* Va, float* Vb, const int32_t* policy, const uint8_t* term,
                     int64_t s_begin, int64_t s_end, float gamma, int n_sweeps, float* d_delta,
                     hipGraphExec_t* out) {
    hipGraph_t graph;
    PI_HIP(hipGraphCreate(&graph, 0));
    hipGraphNode_t prev = nullptr;
    int rc = 0;
    // sweep 0 copies the terminal values from Va into Vb; from then on both hold them
    for (int i = 0; i < n_sweeps && !rc; ++i)
        rc = pi::launch_eval(h, (i & 1) ? Vb : Va, (i & 1) ? Va : Vb, policy, term, s_begin, s_end, gamma,
                             i == n_sweeps - 1 && d_delta, pi::LaunchTo(graph, &prev), i >= 1);
    if (!rc) rc = pi::finalize(h, d_delta, nullptr, pi::LaunchTo(graph, &prev));
    if (!rc && hipGraphInstantiate(out, graph, nullptr, nullptr, 0) != hipSuccess) rc = 1;
    (void)hipGraphDestroy(graph);
    if (rc) {
        (void)hipGetLastError();
        return fail("could not build the evaluation-sweep graph");
    }
    return 0;
}

// The pair table of `V` for a whole-grid improvement sweep on `st`, in *out: packed on EVERY call — callers write V
// behind the library's back, so nothing is remembered from one call to the next.  *out stays null where the sweep takes
// the plain kernels: the unit has no table kernels, the option says no, or the 8 n-byte buffer could not be had (said
// once on stderr, never tried again).  A pack that cannot be launched is an error like any other launch.
int pack_pair_table(pi_handle* h, const float* V, hipStream_t st, const float** out) {
    *out = nullptr;
    if (!h->pair_built || !pair_table_wanted(h) || h->pair_alloc_failed) return 0;
    if (!h->d_pairs && hipMalloc((void**)&h->d_pairs, (size_t)h->n_states * 8) != hipSuccess) {
        (void)hipGetLastError();
        h->d_pairs = nullptr;
        h->pair_alloc_failed = true;
        std::fprintf(stderr, "libpi_mi355: no memory for the %lld-byte pair table of the improvement sweeps; they read V\n",
                     (long long)h->n_states * 8);
        return 0;
    }
    const unsigned blocks = (unsigned)((h->n_states + kProbeBlock - 1) / kProbeBlock);
    PI_HIP(launch(h->f_pack_pairs, {blocks, 1}, kProbeBlock, st, V, h->d_pairs));
    *out = h->d_pairs;
    return 0;
}

}  // namespace

// empty range: zero whichever of the outputs were given, nothing to launch
int pi::zero_outputs(float* d_delta, uint32_t* d_changed, hipStream_t st) {
    if (d_delta) PI_HIP(hipMemsetAsync(d_delta, 0, sizeof(float), st));
    if (d_changed) PI_HIP(hipMemsetAsync(d_changed, 0, sizeof(uint32_t), st));
    return 0;
}

int pi::check_ready(const pi_handle* h) {
    if (!h) return fail("null handle");
    if (h->device < 0) return fail("host-only handle (device = -1) cannot launch kernels");
    if (!h->module) return fail("pi_compile has not been called on this handle");
    return 0;
}

int pi::check_range(const pi_handle* h, int64_t s_begin, int64_t s_end) {
    if (s_begin < 0 || s_end < s_begin || s_end > h->n_states)
        return fail("state range [" + std::to_string(s_begin) + ", " + std::to_string(s_end) +
                    ") outside [0, " + std::to_string(h->n_states) + ")");
    return 0;
}

// The one place pi_finalize_kernel's arguments are written out (eager, or the last node of an evaluation graph).
int pi::finalize(pi_handle* h, float* d_delta, uint32_t* d_changed, LaunchTo to) {
    if (!d_delta && !d_changed) return 0;
    PI_HIP(launch(h->f_finalize, {1, 1}, 64, to, d_delta ? delta_slots(h) : (unsigned int*)nullptr, d_delta,
                  d_changed ? changed_slots(h) : (unsigned int*)nullptr, d_changed));
    return 0;
}

// The one place pi_eval_sweep_kernel's arguments are written out (eager, or a node of an evaluation graph).
int pi::launch_eval(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, const uint8_t* term,
                int64_t s_begin, int64_t s_end, float gamma, bool want_delta, LaunchTo to, bool keep_terminals) {
    if (s_end == s_begin) return 0;
    Sched sc;
    const Grid2 blocks = plan_launch(h, h->block_eval, s_begin, s_end - s_begin, h->n_states, h->cpw_eval, &sc);
    PI_HIP(launch(h->f_eval, blocks, h->block_eval, to, V, Vnew, policy, term, (const float*)h->d_tab, (long long)s_begin,
                  (long long)s_end, gamma, want_delta ? delta_slots(h) : (unsigned int*)nullptr, sc, keep_terminals ? 1 : 0));
    return 0;
}

// One evaluation sweep over `count` entries of the list of live states from position `first` (pi_prepare_mask): a
// sweep that need not copy terminal values.
int pi::launch_eval_live(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, int64_t first, int64_t count,
                     float gamma, bool want_delta, hipStream_t st, const int32_t* list, int64_t list_total) {
    if (count <= 0) return 0;
    const int32_t* live = (list ? list : h->d_live) + first;
    if (!list) list_total = live_list_total(h, h->live_count);
    // a list the caller passes (the per-evaluation list, the lists of an exchange plan) is some subset of the live
    // states in ascending order: its periods are the same share of ITS length only when it covers the listed range
    Sched sc;
    const pi::Grid2 blocks = plan_launch(h, h->block_eval, first, count, list_total, h->cpw_eval, &sc);
    PI_HIP(launch(h->f_eval_live, blocks, h->block_eval, st, V, Vnew, policy, live, (const float*)h->d_tab, (long long)count, gamma,
                  want_delta ? delta_slots(h) : (unsigned int*)nullptr, sc));
    return 0;
}

int pi::launch_eval_push(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, const int32_t* list,
                     const uint8_t* dest, float* const* d_peers, int n_peers, int64_t count, float gamma, bool want_delta,
                     hipStream_t st) {
    if (count <= 0) return 0;
    if (ensure_push_module(h)) return 1;
    const int cpw = h->cpw_eval;
    PI_HIP(launch(h->f_eval_push, {launch_blocks(h->block_eval, count, cpw), 1}, h->block_eval, st, V, Vnew, policy, list, dest,
                  d_peers, n_peers, (const float*)h->d_tab, (long long)count, gamma,
                  want_delta ? delta_slots(h) : (unsigned int*)nullptr, cpw));
    return 0;
}

extern "C" {

int pi_abi_version(void) { return PI_MI355_ABI_VERSION; }

const char* pi_last_error(void) { return pi::last_error().c_str(); }

pi_handle* pi_create(int device, int D, const int32_t* grid_shape, const float* lo,
                     const float* hi, const float* const* bins, const float* actions,
                     int n_actions) {
    pi::fail("");
    // step 1: validation and the tables; step 2: choose_dispatch; step 3: allocate_device_state
    if (D != 2 && D != 4 && D != 6) { fail("D must be 2, 4 or 6"); return nullptr; }
    if (n_actions < 1) { fail("need at least one action"); return nullptr; }
    if (!grid_shape || !lo || !hi || !bins || !actions) { fail("null argument"); return nullptr; }
    std::unique_ptr<pi_handle> h(new pi_handle);
    h->device = device;
    h->D = D;
    h->n_actions = n_actions;
    h->shape.assign(grid_shape, grid_shape + D);
    for (int d = 0; d < D; ++d) { h->mem_of_user.push_back(d); h->user_of_mem.push_back(d); }
    int64_t n = 1;
    for (int d = 0; d < D; ++d) {
        if (grid_shape[d] < 2) { fail("every dimension needs at least 2 bins"); return nullptr; }
        n *= grid_shape[d];
        if (n >= (int64_t(1) << 31)) { fail("n_states must be < 2^31"); return nullptr; }
    }
    h->n_states = n;
    for (int d = 0; d < D; ++d) {
        const float span = hi[d] - lo[d];            // float32 subtraction, as the reference's kernels
        h->lo.push_back(lo[d]);
        h->span.push_back(span);
        h->rcp.push_back(1.0f / span);
        h->fastdiv.push_back(pi::validate_fast_division(span) ? 1 : 0);
    }
    if (pi::knob_flag(pi::Knob::IEEE_DIV)) std::fill(h->fastdiv.begin(), h->fastdiv.end(), 0);
    h->tab.insert(h->tab.end(), actions, actions + n_actions);
    for (int d = 0; d < D; ++d) h->tab.insert(h->tab.end(), bins[d], bins[d] + grid_shape[d]);
    if (h->tab.size() * sizeof(float) > 60 * 1024) {
        fail("bin tables + actions exceed the 60 KiB LDS budget of the sweep kernels");
        return nullptr;
    }
    choose_dispatch(h.get());
    if (allocate_device_state(h.get())) return nullptr;
    return h.release();
}

void pi_destroy(pi_handle* h) {
    if (!h) return;
    if (h->device >= 0) {
        pi::DeviceGuard guard(h->device);
        pi::release_comm(h);
        free_device_state(h);
    }
    delete h;
}

int pi_eval_sweep(pi_handle* h, const float* V, float* Vnew, const int32_t* policy,
                  const uint8_t* term, int64_t s_begin, int64_t s_end, float gamma,
                  float* d_delta, void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (!V || !Vnew || !policy) return fail("null device pointer");
    if (V == Vnew) return fail("V and Vnew must be different buffers (Jacobi sweep)");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(d_delta, nullptr, st);   // empty shard: residual 0, nothing to launch
    if (pi::launch_eval(h, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta != nullptr, st)) return 1;
    return pi::finalize(h, d_delta, nullptr, st);
}

int pi_eval_sweeps(pi_handle* h, float* Va, float* Vb, const int32_t* policy,
                   const uint8_t* term, int64_t s_begin, int64_t s_end, float gamma,
                   int n_sweeps, float* d_delta, void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (n_sweeps < 0) return fail("n_sweeps < 0");
    if (!Va || !Vb || !policy) return fail("null device pointer");
    if (Va == Vb) return fail("Va and Vb must be different buffers (Jacobi sweep)");
    if (n_sweeps == 0) return 0;
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(d_delta, nullptr, st);
    // Small grids, whole-grid batches: one workgroup keeps V in LDS and runs all the sweeps.
    if (h->f_resident && h->use_resident && n_sweeps >= 2 && s_begin == 0 && s_end == h->n_states) {
        PI_HIP(launch(h->f_resident, {1, 1}, h->resident_block, st, Va, Vb, policy, term, (const float*)h->d_tab, gamma, n_sweeps,
                      d_delta, /*theta*/ 0.0, /*check_interval*/ 1, /*sweeps_out*/ (int*)nullptr, /*residual_log*/ (float*)nullptr));
        return 0;
    }
    // Launch-bound sizes: replay the whole batch as one graph.
    if (h->use_graphs && n_sweeps >= 4 && s_end - s_begin <= (int64_t(1) << 20)) {
        pi::GraphEntry* hit = nullptr;
        for (auto& g : h->graphs)
            if (g.Va == Va && g.Vb == Vb && g.policy == policy && g.term == term &&
                g.d_delta == d_delta && g.s_begin == s_begin && g.s_end == s_end &&
                g.gamma == gamma && g.n_sweeps == n_sweeps)
                hit = &g;
        if (!hit) {
            hipGraphExec_t exec = nullptr;
            if (build_eval_graph(h, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta, &exec)) {
                h->use_graphs = false;           // fall back to eager launches from here on
            } else {
                if (h->graphs.size() >= 16) {    // evict the least recently used entry
                    auto lru = std::min_element(h->graphs.begin(), h->graphs.end(),
                                                [](const GraphEntry& a, const GraphEntry& b) { return a.stamp < b.stamp; });
                    (void)hipGraphExecDestroy(lru->exec);
                    h->graphs.erase(lru);
                }
                h->graphs.push_back({Va, Vb, policy, term, d_delta, s_begin, s_end, gamma, n_sweeps, exec, 0});
                hit = &h->graphs.back();
            }
        }
        if (hit) {
            hit->stamp = ++h->graph_clock;
            PI_HIP(hipGraphLaunch(hit->exec, st));
            return 0;
        }
    }
    // later sweeps of a batch visit only the live states of the range when pi_prepare_mask found that worthwhile
    const bool live = pi::live_usable(h, term, s_begin, s_end);
    int64_t first = 0, count = 0;
    if (live) pi::live_span(h, s_begin, s_end, &first, &count);
    // ... and between pi_eval_begin and pi_eval_end only those that bootstrap under this policy, once both buffers
    // of a sweep have been written in full since pi_eval_begin (whole-grid batches)
    const bool shorter = live && h->eval_count >= 0 && policy == h->eval_policy && s_begin == 0 && s_end == h->n_states;
    auto holds = [&](const float* buf) {
        return std::find(h->eval_holds.begin(), h->eval_holds.end(), buf) != h->eval_holds.end();
    };
    for (int i = 0; i < n_sweeps; ++i) {
        const float* src = (i & 1) ? Vb : Va;
        float* dst = (i & 1) ? Va : Vb;
        const bool want = i == n_sweeps - 1 && d_delta != nullptr;
        // sweep 0 copies the terminal states' values from Va into Vb; from then on both buffers hold them
        int rc;
        if (i >= 1 && shorter && holds(src) && holds(dst)) {
            rc = pi::launch_eval_live(h, src, dst, policy, 0, h->eval_count, gamma, want, st, h->d_eval_list,
                                      pi::live_list_total(h, h->eval_count));
        } else {
            rc = i >= 1 && live ? pi::launch_eval_live(h, src, dst, policy, first, count, gamma, want, st)
                                : pi::launch_eval(h, src, dst, policy, term, s_begin, s_end, gamma, want, st, i >= 1);
            if (shorter && !holds(dst)) h->eval_holds.push_back(dst);      // a full sweep wrote every live state of dst
        }
        if (rc) return 1;
    }
    return pi::finalize(h, d_delta, nullptr, st);
}

int pi_improve_sweep(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term,
                     int64_t s_begin, int64_t s_end, float gamma, uint32_t* d_changed,
                     void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (!V || !policy) return fail("null device pointer");
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(nullptr, d_changed, st);
    pi::drop_eval_list(h);                                   // the policy is about to change
    const float* tab = h->d_tab;
    unsigned int* cslots = d_changed ? changed_slots(h) : nullptr;
    Sched sc;
    // whole-grid sweeps gather from the pair table of V where the unit has the kernels; a sub-range (the shard of a rank,
    // pi_comm.cpp) reads V: packing all of V for a shard's worth of work cannot pay
    const float* pairs = nullptr;
    if (s_begin == 0 && s_end == h->n_states && pack_pair_table(h, V, st, &pairs)) return 1;
    h->pair_last = pairs != nullptr;
    if (pi::live_usable(h, term, s_begin, s_end)) {
        // the improvement sweep never touches terminal states: visit the listed live ones only (pi_prepare_mask)
        int64_t first = 0, cnt = 0;
        pi::live_span(h, s_begin, s_end, &first, &cnt);
        if (cnt > 0) {
            const pi::Grid2 blocks = plan_launch(h, h->block_improve, first, cnt, pi::live_list_total(h, h->live_count),
                                                h->cpw_improve, &sc);
            if (pairs)
                PI_HIP(launch(h->f_improve_live_pairs, blocks, h->block_improve, st, V, pairs, policy,
                              (const int32_t*)(h->d_live + first), tab, (long long)cnt, gamma, cslots, sc));
            else
                PI_HIP(launch(h->f_improve_live, blocks, h->block_improve, st, V, policy, (const int32_t*)(h->d_live + first), tab,
                              (long long)cnt, gamma, cslots, sc));
        }
        return pi::finalize(h, nullptr, d_changed, st);
    }
    const pi::Grid2 blocks = plan_launch(h, h->block_improve, s_begin, s_end - s_begin, h->n_states, h->cpw_improve, &sc);
    if (pairs)
        PI_HIP(launch(h->f_improve_pairs, blocks, h->block_improve, st, V, pairs, policy, term, tab, (long long)s_begin,
                      (long long)s_end, gamma, cslots, sc));
    else
        PI_HIP(launch(h->f_improve, blocks, h->block_improve, st, V, policy, term, tab, (long long)s_begin, (long long)s_end, gamma,
                      cslots, sc));
    return pi::finalize(h, nullptr, d_changed, st);
}

int pi_value_sweep(pi_handle* h, const float* V, float* Vnew, int32_t* policy, const uint8_t* term,
                   int64_t s_begin, int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed,
                   void* stream) {
    if (check_ready(h) || check_range(h, s_begin, s_end)) return 1;
    if (!V || !Vnew || !policy) return fail("null device pointer");
    if (V == Vnew) return fail("V and Vnew must be different buffers (Jacobi sweep)");
    pi::drop_eval_list(h);                                   // the policy is about to change
    pi::DeviceGuard guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (s_end == s_begin) return zero_outputs(d_delta, d_changed, st);
    Sched sc;
    const pi::Grid2 blocks = plan_launch(h, h->block_improve, s_begin, s_end - s_begin, h->n_states, h->cpw_improve, &sc);
    PI_HIP(launch(h->f_value, blocks, h->block_improve, st, V, Vnew, policy, term, (const float*)h->d_tab, (long long)s_begin,
                  (long long)s_end, gamma, d_delta ? delta_slots(h) : (unsigned int*)nullptr,
                  d_changed ? changed_slots(h) : (unsigned int*)nullptr, sc));
    return pi::finalize(h, d_delta, d_changed, st);
}

int pi_plan_schedule(pi_handle* h, int block, int64_t first, int64_t count, int64_t total, int chunks_per_workgroup,
                     uint64_t* out6) {
    if (!h || !out6) return fail("null argument");
    // block: any whole number of waves, like the sizes the knobs accept for the sweeps
    if (block < 64 || block > 1024 || block % 64 != 0 || chunks_per_workgroup < 1 || chunks_per_workgroup > 64 ||
        first < 0 || count < 1 || total < 0)
        return fail("pi_plan_schedule: bad launch shape");
    Sched sc;
    const pi::Grid2 grid = plan_launch(h, block, first, count, total, chunks_per_workgroup, &sc);
    out6[0] = grid.x; out6[1] = grid.y; out6[2] = sc.period; out6[3] = sc.phase; out6[4] = (uint64_t)sc.cpw; out6[5] = 0;
    return 0;
}

int pi_set_option(pi_handle* h, int what, int64_t value) {
    if (!h) return fail("null handle");
    switch (what) {
        case PI_OPTION_EVAL_CPW:
            if (value < 1 || value > 64) return fail("chunks per workgroup must be in [1, 64]");
            h->cpw_eval = (int)value;
            drop_graphs(h);
            return 0;
        case PI_OPTION_IMPROVE_CPW:
            if (value < 1 || value > 64) return fail("chunks per workgroup must be in [1, 64]");
            h->cpw_improve = (int)value;
            return 0;
        case PI_OPTION_GRAPHS:
            h->use_graphs = value != 0;
            return 0;
        case PI_OPTION_RESIDENT:
            h->use_resident = value != 0;
            return 0;
        case PI_OPTION_MEMORY_ORDER: {
            // Memory order of the dimensions: digit k (base 8) of `value` = the user dimension stored as memory
            // dimension k, 0 = slowest.  Which dimensions are slow decides how far apart in memory the corners of a
            // successor cell lie and how long a value stays useful in an XCD's L2: measured on MI355X (tools/
            // dim_order_sweep.py) the best order beats the user's by 7-11 % on the evaluation sweeps of the big
            // BASELINE grids.  The arithmetic (weights as products in USER order, the fmaf chain in USER corner order,
            // step_dynamics' arguments) does not depend on it; only where a state lives does.
            if (h->compiled) return fail("the memory order must be set before pi_compile");
            for (int d = 0; d < h->D; ++d)
                if (h->user_of_mem[d] != d) return fail("the memory order of this handle has already been set");
            std::vector<int> perm(h->D), seen(h->D, 0);
            int64_t v = value;
            for (int k = 0; k < h->D; ++k) {
                perm[k] = (int)(v & 7);
                v >>= 3;
                if (perm[k] >= h->D || seen[perm[k]]++) return fail("memory order: not a permutation of the dimensions");
            }
            if (v != 0) return fail("memory order: too many digits");
            std::vector<int32_t> shape(h->D);
            std::vector<float> lo(h->D), span(h->D), rcp(h->D), tab(h->tab.begin(), h->tab.begin() + h->n_actions);
            std::vector<int> fastdiv(h->D);
            std::vector<size_t> off(h->D);
            size_t at = (size_t)h->n_actions;
            for (int d = 0; d < h->D; ++d) { off[d] = at; at += (size_t)h->shape[d]; }
            for (int k = 0; k < h->D; ++k) {
                const int d = perm[k];
                shape[k] = h->shape[d]; lo[k] = h->lo[d]; span[k] = h->span[d]; rcp[k] = h->rcp[d]; fastdiv[k] = h->fastdiv[d];
                tab.insert(tab.end(), h->tab.begin() + off[d], h->tab.begin() + off[d] + h->shape[d]);
                h->mem_of_user[d] = k;
            }
            h->user_of_mem = perm;
            h->shape = shape; h->lo = lo; h->span = span; h->rcp = rcp; h->fastdiv = fastdiv; h->tab = tab;
            if (h->device >= 0) {
                pi::DeviceGuard guard(h->device);
                PI_HIP(hipMemcpy(h->d_tab, h->tab.data(), h->tab.size() * sizeof(float), hipMemcpyHostToDevice));
            }
            return 0;
        }
        case PI_OPTION_BUILD_PUSH:
            // build the fused swept-first kernel of the peer-to-peer exchange now (pi_exchange_plan does it on demand);
            // on a host-only handle this is a compile check that fills the code-object cache
            if (value == 0) return 0;
            return pi::ensure_push_module(h);
        case PI_OPTION_KEEP_LIVE_LIST:
            // keep the live-state list of pi_prepare_mask even when it saves no idle lanes: the fused exchange of a
            // sharded run on a grid with terminal states delivers from the list sweeps (csrc/pi_comm.cpp)
            h->live_force = value != 0;
            return 0;
        case PI_OPTION_STRIP_STATES:
            // strip schedule of the sweeps: states per period (a plane of a slow memory dimension; every XCD takes its
            // eighth of every period); 0 = slab schedule, -1 = the library's choice for this grid.  Placement only.
            if (value < -1 || value > h->n_states) return fail("strip period must be -1 (auto), 0 (off) or a number of states <= n");
            h->strip_mode = value;
            resolve_strip(h);
            drop_graphs(h);
            return 0;
        case PI_OPTION_XCD_RUN_FAILED:
            // the caller reports that the last whole run launched on the XCD-local kernel (pi_policy_iteration) did not go
            // through (d_result[0] < 0): the call is asynchronous and cannot count that itself.
            // PI_XCD_FAILURE_COUNT counts it (two failures switch the kernel off for this handle, as in pi_policy_evaluation),
            // PI_XCD_FAILURE_SWITCH_OFF also switches it off now (the caller is about to run the LDS-resident whole-run
            // kernel instead, which cannot fail).
            if (value != PI_XCD_FAILURE_COUNT && value != PI_XCD_FAILURE_SWITCH_OFF)
                return fail("option 8 takes 1 (count a failed whole run) or 2 (and switch the XCD-local kernel off)");
            if (++h->xcd_failed >= 2 || value == PI_XCD_FAILURE_SWITCH_OFF) h->xcd_off = true;
            return 0;
        case PI_OPTION_PAIR_TABLE:
            // the improvement sweeps' pair table: -1 = the library's choice for the grid, 0 = off, 1 = on where the grid
            // admits it (4-D, 8 n < 2^32).  Which kernels a unit holds is settled when pi_compile builds it, so a handle
            // whose unit was built without them cannot be switched on afterwards; switching off always works.
            if (value < -1 || value > 1) return fail("the pair table option takes -1 (auto), 0 (off) or 1 (on)");
            {
                const int before = h->pair_mode;
                h->pair_mode = (int)value;
                if (h->compiled && !h->pair_built && pair_table_wanted(h)) {
                    h->pair_mode = before;
                    return fail("the pair table must be switched on before pi_compile: this handle's kernels were built without it");
                }
            }
            return 0;
        default:
            return fail("unknown option");
    }
}

int pi_debug_report(pi_handle* h, uint32_t* out4) {
    if (pi::check_ready(h)) return 1;
    if (!out4) return fail("null argument");
    if (!h->debug_bounds) return fail("this handle's kernels were built without the checks: set PI_MI355_DEBUG=1 before pi_create");
    pi::DeviceGuard guard(h->device);
    PI_HIP(hipDeviceSynchronize());                       // every sweep launched so far has reported
    // Every code object built from the sweep unit has its own copy of pi_debug_words: the sweeps' module, the push
    // module of an exchange plan and the expectation module, the last two loaded on demand.
    const hipModule_t modules[3] = {h->module, h->module_push, h->module_expect};
    uint32_t total[4] = {0u, 0u, 0u, 0u};
    for (hipModule_t m : modules) {
        if (!m) continue;
        hipDeviceptr_t words = nullptr;
        size_t bytes = 0;
        uint32_t got[4];
        PI_HIP(hipModuleGetGlobal(&words, &bytes, m, "pi_debug_words"));
        if (bytes != sizeof(got)) return fail("pi_debug_words has an unexpected size");
        PI_HIP(hipMemcpy(got, words, bytes, hipMemcpyDeviceToHost));
        PI_HIP(hipMemset(words, 0, bytes));
        if (got[0] != 0u && total[0] == 0u)               // the first module, in that order, that recorded one
            for (int i = 1; i < 4; ++i) total[i] = got[i];
        total[0] += got[0];
    }
    for (int i = 0; i < 4; ++i) out4[i] = total[i];
    return 0;
}

int64_t pi_info(pi_handle* h, int what) {
    if (!h) return -1;
    switch (what) {
        case PI_INFO_N_STATES: return h->n_states;
        case PI_INFO_N_ACTIONS: return h->n_actions;
        case PI_INFO_DIMS: return h->D;
        case PI_INFO_EVAL_CPW: return h->cpw_eval;
        case PI_INFO_EVAL_VGPRS: return h->vgpr_eval;
        case PI_INFO_IMPROVE_VGPRS: return h->vgpr_improve;
        case PI_INFO_COMPUTE_UNITS: return h->num_cu;
        case PI_INFO_CACHE_HIT: return h->cache_hit ? 1 : 0;
        case PI_INFO_IMPROVE_CPW: return h->cpw_improve;
        case PI_INFO_CACHED_GRAPHS: return (int64_t)h->graphs.size();
        case PI_INFO_GRAPHS_ENABLED: return h->use_graphs ? 1 : 0;
        case PI_INFO_EVAL_BLOCK: return h->block_eval;
        case PI_INFO_IMPROVE_BLOCK: return h->block_improve;
        case PI_INFO_RESIDENT_STATES_PER_THREAD: return h->resident_k;
        case PI_INFO_RESIDENT_ENABLED: return h->use_resident ? 1 : 0;
        case PI_INFO_DEBUG_CHECKS: return h->debug_bounds ? 1 : 0;
        case PI_INFO_LIVE_STATES: return h->live_count;
        case PI_INFO_EVAL_LIST_ENTRIES: return h->eval_count < 0 ? 0 : h->eval_count;
        case PI_INFO_MEMORY_ORDER: {
            int64_t code = 0;
            for (int k = h->D - 1; k >= 0; --k) code = (code << 3) | h->user_of_mem[k];
            return code;
        }
        case PI_INFO_FLOW_WORKGROUPS:
            return h->f_flow ? (h->n_states + h->flow_block - 1) / h->flow_block : (h->flow && h->device < 0 ? 1 : 0);
        case PI_INFO_XCD_ENABLED: return h->f_xcd && !h->xcd_off ? 1 : 0;
        case PI_INFO_XCD_EVALUATIONS: return h->xcd_used;
        case PI_INFO_XCD_FALLBACKS: return h->xcd_failed;
        case PI_INFO_WHOLE_RUNS: return h->whole_runs;
        case PI_INFO_WHOLE_RUN_AVAILABLE: return (h->f_run_resident && h->use_resident) || (h->f_xcd && !h->xcd_off) ? 1 : 0;
        case PI_INFO_STRIP_STATES: return h->strip_states;
        case PI_INFO_PAIR_TABLE: return h->pair_last ? 1 : 0;
        case PI_INFO_DISTURBANCES: return h->dist_k;
        default:
            if (what >= PI_INFO_RECIPROCAL_DIV && what < PI_INFO_RECIPROCAL_DIV + h->D)
                return h->fastdiv[what - PI_INFO_RECIPROCAL_DIV];
            return -1;
    }
}

}  // extern "C"

