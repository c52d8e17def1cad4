/*
 * pi_mi355.h — C ABI of libpi_mi355.so, the MI355X (gfx950) Bellman-backup engine.
 *
 * This is the drop-in boundary for the reference's device path: every entry point
 * replaces one piece of /root/reference/src/cuda_policy_iteration.py that the
 * reference reaches through cupy (citations are to that file unless noted).  The
 * reference has no FFI of its own — its "binding" is cupy.RawModule/ReductionKernel —
 * so the ABI below is what a ctypes stub in that file would bind instead
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C types only; device buffers are raw device pointers borrowed from the
 *     caller (the Python host uses torch-ROCm tensors' data_ptr()); `stream` is a
 *     hipStream_t passed as void* (NULL = the legacy default stream).
 *   - every int-returning call returns 0 on success, non-zero on failure;
 *     pi_last_error() then describes the failure (thread-local string).
 *   - one handle per (device, grid, action set); a handle is not thread-safe.
 *   - sweep calls never allocate, never synchronise, never copy to the host: they
 *     only enqueue kernels (and one memset for a counter) on `stream`.
 *   - flat state indices and V offsets are int32 on the device like the reference's
 *     (`int s_idx`, `int idxs[]`): n_states must be < 2^31.
 */
#ifndef PI_MI355_H_
#define PI_MI355_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pi_handle pi_handle;

/* ABI version of this header (bumped on any signature change). */
#define PI_MI355_ABI_VERSION 12
int pi_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* pi_last_error(void);

/*
 * Create an engine for one grid + action set.
 * Replaces the device-array uploads of _allocate_tensors_and_compile (:145-150,
 * :545-550, :969-974): bounds, grid shape, strides and actions.  The (n, D) `d_states`
 * array is NOT uploaded — `bins[d]` (grid_shape[d] floats each; states_space[:, d]
 * takes exactly these values) replaces it.
 *   device      HIP device ordinal, or -1 for a host-only handle that can compile
 *               (pi_compile) but not launch — used by the CPU-side build check.
 *   D           2, 4 or 6          (CudaPolicyIteration2D/4D/6D)
 *   lo, hi      bounds_low/high, D floats (:96-97)
 *   actions     action_space, n_actions floats (:78)
 */
pi_handle* pi_create(int device, int D, const int32_t* grid_shape, const float* lo,
                     const float* hi, const float* const* bins, const float* actions,
                     int n_actions);
void pi_destroy(pi_handle* h);

/*
 * Compile the sweep kernels with the user's `step_dynamics` inlined.
 * Replaces _compile_cuda_module (:177-296, :576-704, :1000-1136): `source = user
 * string + generic kernels` -> NVRTC there, -> hipRTC for gfx950 here.  The string is
 * the reference plugin format unchanged (`__device__ void step_dynamics(...)` with
 * the arity for D; helper __device__ functions and #defines allowed).
 *   cache_dir   directory for compiled code objects (NULL = no cache).  A hit skips
 *               hipRTC entirely.
 *   log/log_len receives the compiler log (may be NULL/0).
 * On a host-only handle the code object is produced (and cached) but not loaded.
 */
int pi_compile(pi_handle* h, const char* dynamics_src, const char* cache_dir, char* log,
               size_t log_len);

/* The full translation unit pi_compile would build (for inspection / AOT builds).
 * Returns the length needed (excluding NUL); copies at most buf_len-1 bytes. */
size_t pi_kernel_source(pi_handle* h, const char* dynamics_src, char* buf, size_t buf_len);

/*
 * One Jacobi policy-evaluation sweep over states [s_begin, s_end):
 *   Vnew[s] = r(s, pi(s)) + gamma * sum_c w_c V[idx_c],  terminal states copy V[s].
 * Replaces the eval_kernel launch (:306-316, :714-724, :1146-1156) AND the
 * max_abs_diff reduction launched after it (:318-320): when d_delta != NULL it is
 * zeroed on `stream` and receives max|Vnew - V| over the range (float, device).
 * V is read over the whole grid; Vnew/policy/term only over the range.
 * term == NULL means "this grid has no terminal states" (the caller's promise; every sweep, reach and
 * sharded entry point accepts it): the kernels then stream no mask, and a sweep that is not asked for a
 * residual does not read the states' old values either — 4 B per state instead of 9 besides the gather.
 */
int pi_eval_sweep(pi_handle* h, const float* V, float* Vnew, const int32_t* policy,
                  const uint8_t* term, int64_t s_begin, int64_t s_end, float gamma,
                  float* d_delta, void* stream);

/*
 * n_sweeps evaluation sweeps ping-ponging between Va and Vb (sweep 0 reads Va and
 * writes Vb, sweep 1 reads Vb, ...) — the body of policy_evaluation's loop between
 * two host checks (:305-331, SYNC_INTERVAL = 25).  d_delta (nullable) receives the
 * residual of the LAST sweep only, which is the only one the reference looks at.
 * The newest iterate is in Vb when n_sweeps is odd, in Va when even.
 * Terminal states keep their value: sweep 0 copies it from Va into Vb, after which both buffers hold it
 * and the later sweeps of the batch neither store it again nor stream the old values for it (without a
 * residual request they read 5 B per state besides the gather instead of 9, and write only non-terminal
 * states) — same values in both buffers as a copy on every sweep gives.
 * Ranges of up to 2^20 states are launch-bound (a few microseconds per sweep): there the whole
 * batch, including the residual fold, is replayed as ONE hipGraph (built on first use per
 * argument set, cached in the handle) instead of n_sweeps host launches.  Grids of up to 12 288
 * states (4 096 in 4-D, 1 024 in 6-D) swept whole go further: ONE workgroup keeps the value table in LDS and
 * each state's successor cell, weights and reward in registers and runs the entire batch in one
 * launch (pi_eval_resident_kernel); the two newest iterates land in Va / Vb as above.
 */
int pi_eval_sweeps(pi_handle* h, float* Va, float* Vb, const int32_t* policy,
                   const uint8_t* term, int64_t s_begin, int64_t s_end, float gamma,
                   int n_sweeps, float* d_delta, void* stream);

/*
 * Optional, once per terminal mask (the reference computes its mask once, at allocation: :150-160): lets the
 * later sweeps of pi_eval_sweeps / pi_eval_sweeps_sharded batches and pi_improve_sweep(_sharded) launches (an
 * improvement sweep never touches terminal states, :253) visit only the NON-terminal states of their range — for the
 * sharded driver: of every launch range of the rank — through a list of
 * their indices the library builds here (one device-to-host copy of the mask, one upload of the list; blocks
 * on `stream`).  Worth it where terminal regions cut through many waves — double cartpole 25^6: 35 % of the
 * states are terminal and 16 % of the waves are partly idle — and skipped where it is not: the list is kept
 * only when at least 3 % of the grid's lane slots would be idle otherwise and the grid has 2^20 states or more
 * (PI_INFO_LIVE_STATES = length of the list in use, 0 = none).  Results are identical with and without it.
 * Contract: the bytes behind d_term must not change while the list is in use; call again after changing
 * them, or with d_term == NULL to drop the list.  Calls given another mask pointer, or a state range that is not
 * inside the listed one, ignore the list.  pi_prepare_mask lists the whole grid (4 B per live state on the device,
 * n / 8 + n / 8 bytes of index on the host); pi_prepare_mask_range lists [s_begin, s_end) only — what a rank of a
 * sharded run needs (its launches never leave its shard): 1 / world of the list, of the index and of the host pass.
 */
int pi_prepare_mask(pi_handle* h, const uint8_t* d_term, void* stream);
int pi_prepare_mask_range(pi_handle* h, const uint8_t* d_term, int64_t s_begin, int64_t s_end, void* stream);
/* The list pi_prepare_mask built (ascending flat indices of the non-terminal states of the listed range), copied into
 * d_out (device, `capacity` entries) on `stream`; returns its length (0: no list is in use; d_out == NULL: length only;
 * -1: error).  For inspection and tests: the sweeps use the list inside the library. */
int64_t pi_live_list(pi_handle* h, int32_t* d_out, int64_t capacity, void* stream);

/*
 * Optional bracket around one policy_evaluation (:300-336), for handles with a live-state list: under a FIXED
 * policy a live state whose successor is terminal has V'(s) = reward + gamma * 0 in every sweep, so once both
 * Jacobi buffers hold that value it need not be visited again.  pi_eval_begin filters the live list down to the
 * states that bootstrap under `policy` (one launch, one 8-byte read-back; blocks on `stream`; the shorter list is
 * kept when it saves at least 3 %), and until pi_eval_end whole-grid pi_eval_sweeps batches with this policy
 * pointer use it for every sweep whose source AND destination buffer have been written by a full sweep since
 * pi_eval_begin (the library tracks the buffers; with the reference's ping-pong that is every sweep after the
 * evaluation's second).  Results are identical with and without the bracket.  PI_INFO_EVAL_LIST_ENTRIES = entries in use.
 * Contract: between begin and end neither the policy array nor the value buffers are written by anyone but
 * the evaluation sweeps; pi_improve_sweep / pi_value_sweep end the bracket by themselves.
 */
int pi_eval_begin(pi_handle* h, const int32_t* policy, const uint8_t* term, void* stream);
int pi_eval_end(pi_handle* h);

/*
 * The whole policy_evaluation loop (:300-336) in ONE launch, for grids the LDS-resident kernel
 * holds (PI_INFO_RESIDENT_STATES_PER_THREAD > 0: up to 12 288 states in 2-D, 4 096 in 4-D, 1 024 in 6-D) and, beyond those, for
 * launch-bound grids of up to 2^17 states in 2-D / 4-D (PI_INFO_FLOW_WORKGROUPS > 0 = workgroups of the dataflow kernel:
 * the iterates travel between workgroups as tagged 8-byte granules, no grid barrier between sweeps; BASELINE
 * config C2, pendulum 200 x 200, is one); fails on every other grid: up to max_sweeps Jacobi sweeps of the whole grid under
 * `policy`, the residual looked at on sweeps 0, check_interval, 2 check_interval, ... (the
 * reference's SYNC_INTERVAL = 25) and on the last one, stopping at the first residual below theta.
 * V is updated in place (the newest iterate); *d_sweeps receives the number of sweeps done,
 * *d_delta (nullable) the last residual looked at, d_residual_log[k] every residual looked at
 * (k-th look; at least max_sweeps / check_interval + 2 floats).  Same arithmetic, same sweep
 * count and same V as the same loop driven from the host through pi_eval_sweeps.
 * On 2-D grids of ~4 000 to 2^16 states among those (PI_INFO_XCD_ENABLED) the evaluation first runs on the CUs of ONE XCD, with
 * the hand-off through that XCD's L2 (pi_xcd_kernel; placement checked at run time; the call then synchronises `stream`
 * once); when that launch cannot go through V is untouched and the LDS-resident or the dataflow kernel runs the evaluation.
 * Dataflow kernel: every device-side wait is bounded (PI_MI355_FLOW_TIMEOUT seconds, default 2; the kernel needs all its
 * workgroups resident at once, which another stream or process holding CUs can prevent); when a workgroup gives up,
 * *d_sweeps = -1 and V holds what it held before the call (a finish kernel is the only writer of V) — the caller runs the
 * same evaluation through pi_eval_sweeps.
 */
int pi_policy_evaluation(pi_handle* h, float* V, const int32_t* policy, const uint8_t* term, float gamma,
                         double theta, int max_sweeps, int check_interval, int32_t* d_sweeps, float* d_delta,
                         float* d_residual_log, void* stream);

/*
 * The reference's whole run() (:357-370) — policy_evaluation (:300-336), policy_improvement (:338-355), until no entry
 * of the policy changes or max_pi_iter rounds are done — in ONE launch (PI_INFO_WHOLE_RUN_AVAILABLE), for grids the
 * LDS-resident kernel holds (PI_INFO_RESIDENT_STATES_PER_THREAD > 0; BASELINE config C1, pendulum 50 x 50, is one: V and
 * the policy stay in one CU's LDS) and for 2-D grids of ~4 000 to 2^16 states (PI_INFO_XCD_ENABLED; BASELINE config C2, pendulum 200 x 200, is one: the
 * kernel runs on the CUs of one XCD, the iterates travel through that XCD's L2 as tagged granules, a thread keeps the
 * actions of its states in registers).  V and policy are updated in place (the last iterate, the last policy); each
 * evaluation does up to max_eval_sweeps sweeps with the residual looked at every check_interval sweeps exactly as
 * pi_policy_evaluation does.
 * d_result[0] = rounds done (>= 1), d_result[1] = 1 when the policy is stable; d_iter_log[4 r ..] = {sweeps of round r's
 * evaluation, bits of its last residual, policy entries changed by its improvement, 0} (4 * max_pi_iter words).
 * Same arithmetic, sweep counts, V and policy as the same loop driven through pi_policy_evaluation / pi_improve_sweep.
 * XCD-local kernel: every device-side wait is bounded and workgroup placement is checked, not assumed: when the launch
 * could not go through, d_result[0] < 0 and V and policy hold what they held before the call — the caller runs the loop
 * itself.  Asynchronous on `stream`.  PI_INFO_WHOLE_RUNS = whole runs launched.
 */
int pi_policy_iteration(pi_handle* h, float* V, int32_t* policy, const uint8_t* term, float gamma, double theta,
                        int max_eval_sweeps, int check_interval, int max_pi_iter, int32_t* d_result, uint32_t* d_iter_log,
                        void* stream);

/*
 * Greedy improvement over [s_begin, s_end): policy[s] = argmax_a Q(s, a), first
 * maximum wins, terminal states untouched.  Replaces the improve_kernel launch
 * (:342-352, :750-760, :1182-1192) AND `old = policy.copy(); all(policy == old)`
 * (:340, :354): when d_changed != NULL it is zeroed on `stream` and receives the
 * number of entries that changed (uint32, device); stable <=> 0.
 */
int pi_improve_sweep(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term,
                     int64_t s_begin, int64_t s_end, float gamma, uint32_t* d_changed,
                     void* stream);

/*
 * Value-iteration sweep over [s_begin, s_end): Vnew[s] = max_a Q(s, a) and policy[s] = argmax
 * in one pass (terminal states copy V and keep their policy entry).  This is the fused form the
 * reference's README sketches (README.md:790-799, "V_new <- best_Q") but does not implement —
 * its code alternates policy_eval_kernel / policy_improve_kernel.  d_delta (nullable, zeroed
 * here) receives max|Vnew - V|, d_changed (nullable, zeroed here) the number of policy entries
 * that changed.
 */
int pi_value_sweep(pi_handle* h, const float* V, float* Vnew, int32_t* policy, const uint8_t* term,
                   int64_t s_begin, int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed,
                   void* stream);

/*
 * Noise-aware solving: the EXPECTED backup over a disturbance set (csrc/pi_expect_kernels.hip, csrc/pi_expect.cpp).  No
 * reference counterpart: the reference backs up the one deterministic successor, Q(s, a) = r + gamma * E[V](f(s, a))
 * (:212-283).  With a set installed the pi_expect_* sweeps compute
 *     Q(s, a) = sum_k p_k * [ r_k + gamma * E[V](f(s, a (+) da_k) + dx_k) ]
 * over K points, 1 <= K <= 64, each an action offset da_k, D state offsets dx_k[d] in the order of step_dynamics'
 * arguments, and a weight p_k — the noise model of pi_infer_rollout_stochastic as a quadrature.  For a grid node s
 * (coordinates from the bin tables, as the sweeps compute them) and an action value a, per point in ascending k:
 *   1. a_k = a when da_k == 0.0f; otherwise a_k = fminf(fmaxf(a + da_k, a_min), a_max), a_min / a_max the extremes of the
 *      handle's action table (the clamp of the stochastic rollouts);
 *   2. (s', r_k, done_k) = step_dynamics(s, a_k), the exact instantiation with the functions of pi_math.h;
 *   3. E_k = 0.0f when done_k.  Otherwise s'[d] = s'[d] + dx_k[d] for every d with dx_k[d] != 0 (one float32 add; the
 *      disturbed successor is not wrapped, the interpolation clamps it) and E_k is the sweeps' interpolation at s';
 *   4. q_k = r_k + gamma * E_k, a multiply then an add;
 *   5. Q = p_0 * q_0 (a multiply), then Q = fmaf(p_k, q_k, Q) for k = 1 .. K - 1.
 * With K = 1, da = dx = 0 and p = 1 this is the backup of pi_eval_sweep / pi_improve_sweep bit for bit, -0 and NaN
 * included.  Points with equal da_k next to each other share one dynamics step (same function, same inputs, same bits).
 *   pi_set_disturbances   HOST arrays: action_offsets (K floats) and state_offsets (K x D, row-major) may each be NULL =
 *                       zeros; weights (K floats).  Every value finite, p_k >= 0, |sum p_k - 1| <= 1e-4 (summed in
 *                       float64: the backup stays a gamma-contraction).  K = 0 drops the set.  Needs pi_compile; the first
 *                       call after it builds the handle's expectation module — the same translation unit +
 *                       csrc/pi_expect_kernels.hip, same flags and cache (a compile check on device = -1 handles) —,
 *                       every call uploads the table (after a device synchronisation): K is run-time data, another set
 *                       never builds anything.  A later pi_compile drops the module and the set.  Grids of 2^30 states or
 *                       more are refused.  Every refusal is an error code and pi_last_error, never a launch.
 *                       PI_INFO_DISTURBANCES = K in use.
 *   pi_expect_eval_sweeps, pi_expect_improve_sweep, pi_expect_value_sweep
 *                       pi_eval_sweeps, pi_improve_sweep and pi_value_sweep with Q as above: same arguments, same
 *                       Va / Vb ping-pong, nullable d_delta / d_changed, term == NULL, terminal states, residual and
 *                       changed count; strict > argmax from -1.0e30f over ascending action indices.  Asynchronous on
 *                       `stream`.  Without a set they fail, naming pi_set_disturbances.  Every call launches the
 *                       state-order kernels: they end a pi_eval_begin bracket and use neither the live-state list, graphs,
 *                       the pair table nor the one-launch kernels.
 */
int pi_set_disturbances(pi_handle* h, int K, const float* action_offsets, const float* state_offsets, const float* weights);
int pi_expect_eval_sweeps(pi_handle* h, float* Va, float* Vb, const int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, int n_sweeps, float* d_delta, void* stream);
int pi_expect_improve_sweep(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term, int64_t s_begin,
                            int64_t s_end, float gamma, uint32_t* d_changed, void* stream);
int pi_expect_value_sweep(pi_handle* h, const float* V, float* Vnew, int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed, void* stream);

/*
 * Worst-case solving over the same set: the max-min backup, Q(s, a) = min_k q_k over the points that take part, for a
 * bounded disturbance chosen against the controller (same files; no reference counterpart).
 * Worst-case fold.  Steps 1-4 of the definition at pi_set_disturbances stay as they are: a_k, step_dynamics, dx_k added
 * where it is not zero, q_k = r_k + gamma * E_k.  Step 5 becomes, over the points in ascending k:
 *   - a point with p_k == 0.0f takes no part, as if its row were not in the table: it neither starts nor breaks a run of
 *     equal da that shares one dynamics step;
 *   - the first participating point gives Q = q_k and k* = k;
 *   - every later participating point replaces both when q_k < Q || q_k != q_k.  The comparison is strict, so the first of
 *     equal points stays, and -0.0f does not replace +0.0f;
 *   - a NaN point is taken, and nothing replaces a NaN afterwards except another NaN: a NaN in any participating point
 *     gives Q = NaN, which never wins the strict > argmax — as the expectation's fmaf chain behaves;
 *   - comparisons, not fminf: the sign of a zero and the NaN rule are the same on the device, in C++ and in numpy.
 * Weights are otherwise ignored; the validation of pi_set_disturbances (finite, >= 0, sum 1 within 1e-4) stays, so at
 * least one point participates.  With the one-point zero set this is the backup of pi_eval_sweep / pi_improve_sweep bit
 * for bit.  max_a min_k is a gamma-contraction; the evaluation sweeps of a fixed policy, V'(s) = min_k q_k(s, pi(s)), are
 * the adversary's value iteration against that policy.
 *   pi_robust_eval_sweeps, pi_robust_improve_sweep, pi_robust_value_sweep
 *                       pi_expect_eval_sweeps, pi_expect_improve_sweep and pi_expect_value_sweep with that fold: the same
 *                       arguments, refusals (no set, no pi_compile, range, null pointers, Va == Vb), pi_eval_begin
 *                       handling and limits.  The kernels (pi_robust_*_kernel) are further instantiations in the handle's
 *                       expectation module: nothing more is built, and no mode is kept on the handle — the caller says
 *                       which backup it wants by the call it makes, and may alternate the two on one set.
 */
int pi_robust_eval_sweeps(pi_handle* h, float* Va, float* Vb, const int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, int n_sweeps, float* d_delta, void* stream);
int pi_robust_improve_sweep(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term, int64_t s_begin,
                            int64_t s_end, float gamma, uint32_t* d_changed, void* stream);
int pi_robust_value_sweep(pi_handle* h, const float* V, float* Vnew, int32_t* policy, const uint8_t* term, int64_t s_begin,
                          int64_t s_end, float gamma, float* d_delta, uint32_t* d_changed, void* stream);

/*
 * Anderson-accelerated policy evaluation (csrc/pi_accel_kernels.hip, csrc/pi_accel.cpp; no reference counterpart).
 * Evaluating a fixed policy is a linear fixed-point iteration; once per full batch of sweeps the solver extrapolates over
 * a ring of up to 8 past batches (dynamicprogramming_amd/accel.py holds the loop, the small solve and the numpy twin of
 * everything below).  Per full batch: x the iterate before it, g the iterate after it, f = g - x.  The ring holds columns
 * dF_j = f - f_prev, dG_j = g - g_prev of earlier batches at ring positions j; (m, n) float32 arrays, column j at element
 * offset j * n (64-bit).  The arithmetic, so that the device and numpy agree bit for bit:
 *   - f, dF and dG are float32, each ONE float32 subtraction;
 *   - a dot product accumulates float64 products (double)a * (double)b, a multiply then an add, never contracted;
 *   - its reduction tree is fixed and independent of the launch: the flat index (memory order) is cut into tiles of
 *     4 096 consecutive elements, each of 4 chunks of 1 024; thread t of 256 owns elements 4t .. 4t + 3 of every chunk
 *     and adds their products to 0.0 in ascending index; the 256 thread sums are added wave by wave (4 waves of 64
 *     lanes), in each wave lanes 0 .. o - 1 adding lanes o .. 2o - 1 for o = 32, 16, 8, 4, 2, 1, and the four wave sums as
 *     (w0 + w2) + (w1 + w3); elements past n take no part.  The tile sums are folded the same way: thread t of 256 adds
 *     tile sums t, t + 256, .. to 0.0 in ascending order, then the same tree over the 256 threads.  No atomics;
 *   - the combine is out[s] = (float)((double)g[s] - S), S = 0.0 + c_0 * (double)dG_0[s] + c_1 * (double)dG_1[s] + ..
 *     in ascending ring position, each term a multiply then an add, then one subtraction and one rounding.  Where every
 *     column is zero at s — terminal states, states whose successor is terminal — S is +0.0 and out[s] has g[s]'s bits,
 *     -0.0 included.
 *   pi_accel_update     one streaming pass after a full batch.  first != 0 (k_used = 0): (f_prev, g_prev) <- (f, g), no
 *                       column is written, d_dots[0] = f . f.  Otherwise (1 <= k_used <= m, slot < k_used): column `slot`
 *                       of dF and dG is overwritten by (f - f_prev, g - g_prev), then (f_prev, g_prev) <- (f, g), and
 *                       d_dots (device, 2 k_used + 1 float64) receives dF_j . f for j < k_used, then dF_j . dF_slot for
 *                       j < k_used — the new column's row of the Gram matrix; the caller keeps the older entries —, then
 *                       f . f.  The columns in use are ring positions 0 .. k_used - 1.  Asynchronous on `stream`.
 *   pi_accel_combine    out <- g - dG c over the k_used columns at ring positions 0 .. k_used - 1; `coeffs`: k_used HOST
 *                       float64, passed to the kernel by value.  `out` may be `g`.  Asynchronous on `stream`.
 * 16-byte accesses when n is a multiple of 4 and every base is 16-byte aligned, float by float otherwise: same results.
 * Refusals, an error code and pi_last_error, never a launch, in this order: null handle; null pointers; n <= 0; m outside
 * [1, 8]; k_used outside [0, min(m, 8)]; slot outside [0, m); first with k_used != 0, or a later push with k_used = 0 or
 * slot >= k_used; coefficients that are not finite; arrays that overlap, `out == g` excepted.  The first call builds the
 * handle's acceleration module (hipRTC, the sweeps' flags, the code-object cache of pi_compile if it has run): it depends
 * on neither the grid nor the env, so it is the same code object for every handle and survives a later pi_compile; on
 * device = -1 handles a call is those checks and that build.
 */
int pi_accel_update(pi_handle* h, const float* x, const float* g, float* f_prev, float* g_prev, float* dF, float* dG, int m,
                    int slot, int k_used, int first, int64_t n, double* d_dots, void* stream);
int pi_accel_combine(pi_handle* h, const float* g, const float* dG, const double* coeffs, int k_used, int64_t n, float* out,
                     void* stream);

/*
 * Which planes of V can the states of [s_begin, s_end) read, under ANY action?  Along dimension
 * `dim`: d_bitmap (device, ceil(grid_shape[dim] / 32) uint32 words, zeroed here) receives one bit
 * per index: that of every successor cell and the one above it.  No counterpart in the reference
 * (it has no multi-GPU path); the multi-GPU plan uses dim = 0 to exchange only reachable planes
 * between ranks instead of all-gathering V after every sweep; the other
 * dimensions tell how wide a halo a shard along them would need.
 */
int pi_reach_planes(pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end, int dim,
                    uint32_t* d_bitmap, void* stream);

/*
 * The same question at a finer grain.  "Units" are the leading `depth` dimensions flattened: depth 1
 * = the planes of dimension 0, depth 2 = the rows (i0, i1), each a contiguous run of
 * n_states / (grid_shape[0] * grid_shape[1]) states.  d_bitmap (device, ceil(units / 32) words,
 * zeroed here) receives one bit per unit some state of [s_begin, s_end) can read under ANY action.
 * Every env moves a position by dt * velocity, so the rows a shard reaches in a neighbouring plane
 * are the ones with the right sign and size of velocity: 2-4x fewer values than whole planes.
 * pi_reach_depth_max: 2 for grids of three or more dimensions with up to 2^17 such rows, else 1.
 */
int pi_reach_depth_max(pi_handle* h);
int pi_reach_units(pi_handle* h, const uint8_t* term, int64_t s_begin, int64_t s_end, int depth,
                   uint32_t* d_bitmap, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU, RCCL over xGMI).  SURVEY.md section 8b/8e: the reference is a
 * single-device loop (:300-336), so these entry points have no line to replace — they are what a
 * maintainer binds to run the same loop over several GPUs.  Partition: rank r owns the contiguous
 * state range [r * per, min((r + 1) * per, n)), per = ceil(n / world); every rank keeps full-size
 * V buffers of per * world floats.
 * ------------------------------------------------------------------------------------------- */

/* 128-byte RCCL id: created once (any rank), handed to every rank out of band. */
int pi_comm_unique_id(void* id128);
/* Join the RCCL communicator on the handle's device (collective: every rank calls it). */
int pi_comm_init(pi_handle* h, int rank, int world, const void* id128);
/* In-process transport for tests: `world` handles of ONE process, one host thread each, exchange
 * through device-to-device copies ordered by HIP events — same stream semantics as RCCL. */
int pi_comm_init_local(pi_handle* h, int rank, int world, const char* group_name);
/*
 * Peer-to-peer transport (csrc/pi_p2p.cpp): no RCCL on the data path.  The sending GPU STORES its halo rows straight
 * into the receiving rank's buffer (mapped with hipIpcOpenMemHandle; the stores travel over xGMI) and the two sides
 * hand-shake through counters in a small uncached flag page per rank — the rendezvous of an ncclSend / ncclRecv pair
 * without the ~30 us group latency, which at C4 @ 8 is of the order of a rank's whole sweep; the scalar reductions go
 * through the same pages.  One process per rank.  Everything above the transport (pi_exchange_plan,
 * pi_eval_sweeps_sharded, the collectives below) is unchanged.  No reference counterpart
 * (src/cuda_policy_iteration.py:300-336 is a single-device loop).
 *   pi_p2p_describe   registers up to 4 device buffers of this rank — the ones sends and receives will name: both V
 *                     buffers and the policy; same sizes on every rank, addresses are symmetric (offset o of buffer b
 *                     goes to offset o of the peer's buffer b) — allocates the rank's flag page and fills a 512-byte
 *                     descriptor (process id, device, IPC handles).  The caller all-gathers the descriptors of all ranks
 *                     out of band, as it hands the RCCL id around (MPI, files, a socket: 512 bytes per rank);
 *   pi_comm_init_p2p  descs = world x 512 bytes ordered by rank: maps the peers' buffers and pages, builds the transport's
 *                     kernels (hipRTC, cache_dir as pi_compile) and installs it on the handle.  Collective in the sense
 *                     that every rank must call it before any rank exchanges.
 * Every device-side wait is bounded by PI_MI355_COMM_TIMEOUT seconds (default 120); a peer that never arrives is
 * reported by the next reduction or all-gather (which therefore block on their stream), never a hung wave.
 * pi_p2p_compile_check: the transport's device code builds for gfx950 (needs no GPU).
 */
int pi_p2p_describe(pi_handle* h, int rank, int world, const void* const* bufs, const int64_t* bytes, int n_bufs,
                    void* desc512);
int pi_comm_init_p2p(pi_handle* h, int rank, int world, const void* descs, const char* cache_dir);
int pi_p2p_compile_check(const char* cache_dir);
int pi_comm_destroy(pi_handle* h);
/* Fused exchange: when the plan is row-exact (PI_COMM_INFO_ROW_EXACT) and the transport is the peer-to-peer one, the
 * swept-first launch of every sharded evaluation sweep is pi_eval_push_kernel (csrc/pi_push_kernels.hip): the lane that
 * stores V'(s) stores it into the peers that read the row as well, one-wave kernels hand-shake in front of it and behind
 * it, everything on the caller's stream — no copy kernel, no second stream (PI_COMM_INFO_FUSED;
 * PI_MI355_P2P_FUSED=0 keeps the copy kernel); on grids with terminal states whose shard keeps a live-state list
 * (pi_prepare_mask_range) the later sweeps of every batch are fused the same way.  The kernel lives in a second module of the handle that is built on
 * demand from the same translation unit (PI_OPTION_BUILD_PUSH builds it ahead of time). */
/* The `what` of pi_comm_info.  Every other code, and every code on a handle without a communicator, returns -1. */
enum pi_comm_info_code {
    PI_COMM_INFO_RANK = 0,              /* this rank */
    PI_COMM_INFO_WORLD = 1,             /* number of ranks */
    PI_COMM_INFO_TRANSPORT = 2,         /* enum pi_transport */
    PI_COMM_INFO_PLAN = 3,              /* enum pi_plan */
    PI_COMM_INFO_REACH_UNITS = 4,       /* granularity of the plan's reach probe: enum pi_reach_unit (0: no plan) */
    PI_COMM_INFO_ROW_EXACT = 5,         /* row-exact plan (0 | 1) */
    PI_COMM_INFO_FUSED = 6,             /* fused exchange (0 | 1) */
    PI_COMM_INFO_PAIR_EXACT = 7,        /* destination masks cut down to the pairs (i_0, i_v) each peer reads (0 | 1; any
                                           memory order with dimension 0 slowest) */
    PI_COMM_INFO_FUSED_VALUES = 8,      /* values one fused sweep delivers, counted per receiver (-1: not a fused plan) */
    PI_COMM_INFO_FIRST_ENTRIES = 9,     /* entries of the swept-first state list of a row-exact or state-exact plan (-1:
                                           the plan sweeps ranges) */
    PI_COMM_INFO_INTERIOR_ENTRIES = 10  /* entries of the interior state list of such a plan (-1: the plan sweeps ranges) */
};
/* PI_COMM_INFO_TRANSPORT */
enum pi_transport {
    PI_TRANSPORT_RCCL = 1,              /* RCCL (pi_comm_init) */
    PI_TRANSPORT_IN_PROCESS = 2,        /* in-process test transport (pi_comm_init_local) */
    PI_TRANSPORT_P2P = 3                /* peer-to-peer stores (pi_comm_init_p2p) */
};
/* PI_COMM_INFO_PLAN; also the `mode` of pi_exchange_plan and the mode it reports in info[0] */
enum pi_plan {
    PI_PLAN_NONE = 0,                   /* no plan; as the `mode` of pi_exchange_plan: let the library choose */
    PI_PLAN_ALLGATHER = 1,              /* all-gather V after every sweep */
    PI_PLAN_HALO = 2                    /* send only the values peers read */
};
/* PI_COMM_INFO_REACH_UNITS; also the `depth` of pi_reach_units and what pi_reach_depth_max returns */
enum pi_reach_unit {
    PI_REACH_PLANES = 1,                /* planes of dimension 0 */
    PI_REACH_ROWS = 2                   /* rows (i0, i1) */
};
int pi_comm_info(pi_handle* h, int what);

/* In-place collectives on the caller's stream: shard r of the buffer lives at r * shard_elems. */
int pi_allgather_V(pi_handle* h, float* V_full, int64_t shard_elems, void* stream);
int pi_allgather_policy(pi_handle* h, int32_t* policy_full, int64_t shard_elems, void* stream);
int pi_allreduce_max_f32(pi_handle* h, float* d_value, void* stream);
int pi_allreduce_sum_u32(pi_handle* h, uint32_t* d_value, void* stream);

/*
 * Pure host logic (needs no GPU and no communicator): which pieces of V' travel after a sweep.
 *   reach[r * g0 + p] != 0  <=>  rank r's shard can read unit p, the g0 units being consecutive
 *   runs of stride0 states (planes of dimension 0, or rows (i0, i1): pi_reach_units)
 * Writes up to `cap` segments {src, dst, a, b} ("src sends V'[a, b) to dst") and returns how many
 * there are (-1 on bad arguments).  Every rank derives the same list from the same bitmaps.
 */
int64_t pi_plan_segments(int world, int64_t g0, int64_t stride0, int64_t n_states, int64_t per,
                         const uint8_t* reach, int64_t* segs, int64_t cap);

/*
 * Collective: measure this shard's reach (pi_reach_units at pi_reach_depth_max), all-gather the
 * bitmaps, derive the segments and choose the exchange.  mode (enum pi_plan): PI_PLAN_NONE = choose (halo unless some
 * rank would receive more than 60 % of an all-gather), PI_PLAN_ALLGATHER, PI_PLAN_HALO; overlap != 0 sweeps the planes peers
 * wait for first and sends them on a second stream while the interior is swept.
 * info (nullable, 5 values): mode chosen (PI_PLAN_ALLGATHER | PI_PLAN_HALO), elements received / sent per sweep by this rank,
 * number of send ranges, number of interior ranges.  Blocks on `stream` (one-off).
 */
int pi_exchange_plan(pi_handle* h, const uint8_t* term, int64_t per, int mode, int overlap,
                     int64_t* info, void* stream);
/* The launch ranges of the current plan: up to cap triples {kind, begin, end}, kind 0 = swept first
 * (peers wait for rows inside it), 1 = interior (swept while the halo travels).  Returns how many
 * there are (-1 without a plan).  A plan without overlap reports the shard as one kind-0 range; a plan whose swept-first
 * set is a list of single states (PI_COMM_INFO_PAIR_EXACT: the fused exchange in a memory order whose rows are all reachable)
 * reports the coarse row ranges it was cut from. */
int64_t pi_plan_ranges(pi_handle* h, int64_t* ranges, int64_t cap);
/*
 * One part of a sharded evaluation sweep WITHOUT the exchange, launched exactly as pi_eval_sweeps_sharded launches it:
 * part 0 = what the peers wait for (swept first), part 1 = the interior; both together are one sweep of the shard.
 * On grids without terminal states the plan may be ROW-EXACT (PI_COMM_INFO_ROW_EXACT; PI_MI355_ROW_EXACT=0 / 1
 * forces it): part 0 is then the list of exactly the rows that travel, swept in one launch of the list kernel, and
 * part 1 the list of all other states of the shard, instead of a few contiguous ranges that also hold rows nobody
 * waits for.  No reference counterpart (src/cuda_policy_iteration.py:300-336 is a single-device loop); for measurements
 * and tests.
 */
int pi_eval_sweep_part(pi_handle* h, const float* V, float* Vnew, const int32_t* policy, const uint8_t* term, int part,
                       float gamma, void* stream);
/* Make this rank's freshly written shard of V_full visible where the other ranks read it. */
int pi_exchange_V(pi_handle* h, float* V_full, void* stream);
/*
 * pi_eval_sweeps over this rank's shard with the exchange after every sweep — the 25-sweep batch
 * between two host checks (:305-331) without returning to the host.  d_delta (nullable) receives
 * the residual of the last sweep, already MAX-reduced over all ranks.
 */
int pi_eval_sweeps_sharded(pi_handle* h, float* Va, float* Vb, const int32_t* policy,
                           const uint8_t* term, float gamma, int n_sweeps, float* d_delta,
                           void* stream);
/* pi_improve_sweep over this rank's shard; d_changed (nullable) is SUM-reduced over all ranks. */
int pi_improve_sweep_sharded(pi_handle* h, const float* V, int32_t* policy, const uint8_t* term,
                             float gamma, uint32_t* d_changed, void* stream);

/*
 * Probes used by the parity tests (not on the hot path): run the compiled plugin /
 * interpolation on m arbitrary points.  All pointers are device pointers.
 *   pi_probe_step   : states (m,D), acts (m) -> next (m,D), reward (m), done (m)
 *   pi_probe_interp : pts (m,D) -> idxs (m,2^D) int32, wgts (m,2^D) float
 *                     (get_barycentric_{2,4,6}d, reference corner order)
 *   pi_probe_coords : out[(s - s_begin) * D + d] = coordinate d of grid node s, computed the way
 *                     the sweeps compute it (flat index -> per-dimension indices -> LDS bin tables), with
 *                     `chunks_per_workgroup` chunks per workgroup — states_space[s] of :84-87
 */
int pi_probe_step(pi_handle* h, const float* states, const float* acts, float* next,
                  float* reward, uint8_t* done, int64_t m, void* stream);
int pi_probe_interp(pi_handle* h, const float* pts, int32_t* idxs, float* wgts, int64_t m,
                    void* stream);
int pi_probe_coords(pi_handle* h, int64_t s_begin, int64_t s_end, float* out, int chunks_per_workgroup,
                    void* stream);
/*
 * The workgroup -> chunk schedule a sweep launch would use (host only, no launch; tests and tools): a launch of
 * `block`-thread workgroups taking `chunks_per_workgroup` chunks each over `count` units (states, or entries of a state
 * list) from unit `first`, where `total` units stand for the whole grid (n_states for a state range).
 * out6 = {grid x, grid y, period, phase, chunks per workgroup, 0}: period == 0 is the slab schedule (grid y = 1; XCD x =
 * workgroup index mod 8 walks the x-th contiguous eighth of the groups); otherwise the STRIP schedule (PI_OPTION_STRIP_STATES,
 * PI_MI355_STRIP, PI_INFO_STRIP_STATES): the groups are cut into periods of `period` groups — a plane of a slow memory
 * dimension —, the launch is two-dimensional (y = period p, x = 8 r + XCD) and XCD x takes groups
 * [floor((x period + rot) / 8), floor(((x + 1) period + rot) / 8)), rot = 3 p mod 8, of EVERY period p, so that what an
 * XCD's L2 sees between the two sweeps that read a line of V is an eighth of a plane instead of a whole one.  Placement only: results do not depend on it.  No reference counterpart
 * (the reference launches one thread per state in index order, src/cuda_policy_iteration.py:305-318).
 */
int pi_plan_schedule(pi_handle* h, int block, int64_t first, int64_t count, int64_t total, int chunks_per_workgroup,
                     uint64_t* out6);

/* ---------------------------------------------------------------------------------------------
 * Inference: the reference's CPU helper utils/barycentric.py as one batched
 * device kernel — get_barycentric_weights_and_indices (:15-77) and get_optimal_action (:80-112)
 * for m states per launch, same arithmetic type for type (float64 cell widths, the POINT clamped
 * to the bounds, weights = float64 products rounded once to float32, corners in the order of the
 * caller's corner_bits table — itertools.product, MSB first, in the reference :233).  Independent of
 * pi_handle: needs no env plugin.
 * The clamp is the reference's max(lo, min(x, hi)) with Python's comparisons, m = (hi < x) ? hi : x; p = (m > lo) ? m : lo
 * (from the reference's text run under CPython; numba is read, not run, to lower min / max the same way): a NaN
 * coordinate lands on lo — cell 0, t = +0, finite weights —, +inf on hi, -inf on lo, and when x and lo are zeros of
 * opposite sign p is lo's zero (at hi the sign of the point does not reach t).  Every other input gives the value of
 * fmaxf(lo, fminf(x, hi)).  The query, the policy-table rollouts (pi_infer_rollout, _hybrid, _stochastic,
 * _hybrid_stochastic) and pi_infer_resample share this clamp; the lookaheads (pi_infer_greedy, pi_infer_expect_greedy
 * and their rollouts) interpolate as the sweeps do, where a NaN lands on the top border.
 *   pi_infer_create     host arrays; corner_bits is (n_corners = 2^D, D) int32 of 0/1; device = -1
 *                       builds the kernel only (compile check without a GPU); cache_dir as pi_compile.
 *                       The grid and the corner table are compiled INTO the kernel (hipRTC, one code
 *                       object per grid, cached on disk like the sweep kernels)
 *   pi_infer_set_policy host arrays: the greedy policy (n_states int32) and the action values; copied
 *                       to the device once, validated (every entry an index into action_space)
 *   pi_infer_query      d_points (m, D) float32 on the device; any of the three outputs may be null:
 *                       d_actions_out (m) float32 = sum_c w[c] * action_space[policy[idx[c]]] (ascending c),
 *                       d_weights_out (m, 2^D) float32, d_indices_out (m, 2^D) int32.  Asynchronous.
 * Closed-loop rollouts on the same handle (the reference's per-runner evaluate(), e.g. pendulum_cuda.py:135-189:
 * get_optimal_action + one env step per time step on the CPU) as ONE launch for m episodes:
 *   pi_infer_set_dynamics  the env plugin (the step_dynamics string pi_compile takes), compiled with the handle's grid
 *                       and csrc/pi_rollout_kernels.hip into a second module (same flags and cache as pi_compile;
 *                       compiler output in `log`, errors in `log` and pi_last_error).  device = -1: compile check.
 *                       Calling it again replaces the module (after a device synchronisation)
 *   pi_infer_rollout    d_start (m, D) float32 on the device, dimensions in the order of step_dynamics' arguments.
 *                       Every episode runs n_steps steps of: action = what pi_infer_query returns for the state
 *                       (same bits); step_dynamics; ret = ret + disc * r, disc = disc * gamma (float32, separate
 *                       multiply and add); state = successor, length = t + 1; a `done` step ends the episode,
 *                       which keeps its state from then on.  Outputs, any of which may be null: d_final (m, D)
 *                       float32, d_return (m) float32, d_length (m) int32, d_terminated (m) uint8 (1: ended by
 *                       `done`).  traj_every > 0: row j of d_traj, (n_steps / traj_every + 1, m, D) float32, is every
 *                       episode's state after j * traj_every steps (row 0 the start; an ended episode repeats its
 *                       last state).  d_final and d_traj must be 8-byte aligned (4-D: 16-byte).  Needs
 *                       pi_infer_set_policy and pi_infer_set_dynamics; m == 0 is a no-op, n_steps == 0 copies the
 *                       start (length 0, return 0); traj_every > n_steps (n_steps > 0) is an error.  Asynchronous.
 * Rollouts that switch between TWO policies (the reference's runners/hybrid_double_cartpole.py: _use_balance :62-69
 * and the body of evaluate's loop :112-125, two get_optimal_action tables and one _step_python per step on the CPU)
 * as ONE launch for m episodes.  Two handles of the same D, device and corner_bits table: the PRIMARY h (mode 0) and
 * the SECONDARY `partner` (mode 1), each with its own bounds, shape, strides, policy and ACTION table; the env plugin
 * is h's.  The switch is a box with hysteresis, two float32 vectors of D thresholds, `enter` and `leave`.  Every
 * episode starts in mode 0; per step t of an episode still running, in this order:
 *   1. mode: if it is 1 it stays 1 unless fabsf(s[d]) > leave[d] for some d; if it is 0 it becomes 1 iff
 *      fabsf(s[d]) < enter[d] for every d.  float32, strict comparisons; +inf in both vectors = the dimension takes
 *      no part.  Applied before the first step too: an episode that starts inside the box acts on the secondary policy
 *   2. action: the interpolated action of the mode's policy on ITS grid, the bits pi_infer_query returns on that
 *      handle for the state (the point clamped to that grid's bounds, as in the reference)
 *   3. secondary_steps += 1 when the mode is 1
 *   4. step_dynamics, ret = ret + disc * r, disc = disc * gamma, state = successor, length = t + 1, `done` freezes
 *      the episode: exactly as in pi_infer_rollout.
 * The reference's rule is enter = (inf, inf, 0.32, 4.0, 0.32, 4.0), leave = (inf, inf, 0.38, 5.0, 0.38, 5.0), its
 * balance_steps = secondary_steps.
 *   pi_infer_set_partner   builds h's THIRD module: h's grid + partner's grid + the plugin last given to
 *                       pi_infer_set_dynamics(h) + csrc/pi_hybrid_kernels.hip.  Same cache, flags and log convention
 *                       as pi_infer_set_dynamics; device = -1 handles: compile check.  pi_infer_set_dynamics on h
 *                       drops the module again (the next hybrid rollout then fails, naming pi_infer_set_partner)
 *   pi_infer_rollout_hybrid  arguments and outputs of pi_infer_rollout, plus: enter, leave HOST arrays of D floats
 *                       (no NaN, enter[d] <= leave[d]); d_secondary_steps (m) int32; d_last_mode (m) uint8, the mode of
 *                       the last step taken (0 when length is 0); either may be null.  Policy and action tables of
 *                       both handles are read at launch: a later pi_infer_set_policy on either is picked up.  The
 *                       partner must have the grid the module was built for.  m == 0 is a no-op, n_steps == 0 copies
 *                       the start (lengths, returns, secondary_steps, last_mode 0).  Asynchronous.
 * Grid continuation on the same handle (no reference counterpart: the reference starts every run from V = 0): the
 * handle's solution — value function and policy on ITS grid, the SOURCE — interpolated onto the nodes of a DESTINATION
 * grid of the same D with its own per-dimension bin tables, any bounds, any shape, any memory order of the dimensions
 * and its own action table, as ONE launch.  For the destination node s with coordinates x_d = bins_d[i_d]:
 *   1. (w, idx) = the weights and indices pi_infer_query returns for the point x (same bits: the point clamped to the
 *      source's bounds, corners in the order of the source's corner_bits)
 *   2. V[s] = float32 sum from 0.0f over ASCENDING corners c of w[c] * V_source[idx[c]], multiply then add
 *   3. policy[s] = map[policy_source[idx[c*]]], c* the corner of largest w (strict >, from c = 0: the first maximum)
 *   4. a node whose terminal-mask byte is non-zero is not written.
 *   pi_infer_set_values    host array: the source's value function (n_states float32, the user's order), copied to the
 *                       device; builds the handle's FOURTH module, its grid + csrc/pi_resample_kernels.hip (same cache,
 *                       flags and log convention as pi_infer_set_dynamics).  device = -1: compile check
 *   pi_infer_resample   dst_shape, dst_strides HOST arrays of D entries in the user's dimension order; dst_strides are
 *                       the element strides of a dense array of that shape in SOME order of the dimensions (validated),
 *                       every flat position of the outputs and of the mask is sum_d i_d * dst_strides[d].  dst_bins: the
 *                       HOST concatenation of the D bin tables (sum_d dst_shape[d] float32; at most 60 KiB, the table
 *                       pi_create admits).  action_map: HOST, one entry per source action, each in [0, dst_n_actions);
 *                       null = the identity, which needs dst_n_actions >= the source's action count.  d_dst_term
 *                       (n uint8 on the device) may be null: every node is written.  d_dst_V (n float32) needs
 *                       pi_infer_set_values, d_dst_policy (n int32) needs pi_infer_set_policy; one of them may be null.
 *                       Every refusal is an error code and pi_last_error, never a launch.  The launch is asynchronous on
 *                       `stream`; a call whose tables or map differ from the previous call's first waits for the device
 *                       and uploads them.
 * Value-greedy control on the same handle (no reference counterpart: the reference acts on the policy table only): the
 * one-step lookahead on the interpolated value function, a*(s) = argmax_a Q(s, a), at ANY continuous state s.
 * Q(s, a) is the backup of the sweeps evaluated at s instead of a grid node, bit for bit (NOT the arithmetic of
 * pi_infer_query): (s', r, done) = step_dynamics(s, a); E = 0 when done, otherwise per dimension
 * n = (s' - lo) / (hi - lo) * (float)(g - 1) in float32 (IEEE division, then multiply), n = fmaxf(0, fminf(n, g - 1)),
 * i = min((int)n, g - 2), frac = n - (float)i; corner c takes bit d of c for dimension d (2-D: dimension 1 toggles
 * fastest; the handle's corner_bits play no part), its weight is the left-to-right float32 product from 1.0f, its index
 * sum_d (i_d + bit) * strides[d]; E one fmaf chain over ascending corners from 0.0f; Q = r + gamma * E, multiply then add.
 * The argmax is strict > from -1.0e30f over ascending action indices: the lowest index wins ties, NaN never wins, index 0
 * with Q = -1.0e30f when nothing wins.  At a non-terminal node of a converged run it returns that node's policy entry.
 *   pi_infer_set_greedy  host array: the action table (n_actions >= 1 float32), copied to the device — the handle's own
 *                       copy, a handle without a policy will do; builds the handle's FIFTH module: its grid + the plugin
 *                       last given to pi_infer_set_dynamics + csrc/pi_greedy_kernels.hip.  Needs pi_infer_set_values and
 *                       pi_infer_set_dynamics.  Same cache, flags and log convention as pi_infer_set_dynamics; device = -1
 *                       handles: compile check.  pi_infer_set_dynamics drops the module again (the next greedy call then
 *                       fails, naming pi_infer_set_greedy); pi_infer_set_values only replaces the values the launches read
 *   pi_infer_greedy     m query points (m, D) float32 on the device, `gamma` the discount inside Q (not NaN).  Outputs on
 *                       the device, each may be null but not all: d_best (m) int32 the greedy index, d_action (m) float32
 *                       its action VALUE, d_q_best (m) float32 its Q, d_q_all (m, n_actions) float32 row-major all of
 *                       Q(s, .).  m == 0 is a no-op.  Asynchronous.
 *   pi_infer_rollout_greedy  pi_infer_rollout with the action of every step chosen by the lookahead with the discount
 *                       `lookahead_gamma`, a property of the solution; `gamma` discounts the return as in pi_infer_rollout
 *                       (neither may be NaN).  The step taken is step_dynamics(s, actions[best]).  Outputs, trajectory
 *                       layout, alignment and argument rules are pi_infer_rollout's.  Needs no policy.  Asynchronous.
 * Stochastic rollouts on the same handle (the reference's evaluate_random() behind --random, e.g. pendulum_cuda.py, as ONE
 * launch for m episodes; epsilon-random actions and noise have no reference counterpart): pi_infer_rollout with a random
 * stream inside the kernel.  The stream is Philox4x32-10 as published (multipliers 0xD2511F53, 0xCD9E8D57; Weyl key
 * increments 0x9E3779B9, 0xBB67AE85; ten rounds), key = (low, high 32 bits of `seed`), counter = (low, high 32 bits of e,
 * t, j) with e = first_episode + the episode's row in the batch (uint64), t the step, j the draw block: no state in
 * memory, results independent of how a batch is cut into launches, reproduced bit for bit by utils/barycentric.py
 * (philox4x32).  Of a block's words x0..x3, block 0 gives x0 the exploration coin, x1 the random action index, x2 the
 * action noise; block 1 the state noise of dimensions 0..3; block 2 (6-D) that of dimensions 4, 5 in x0, x1.
 * sym(x) = (float)((int)(x >> 8) - 8388608) * 2^-23, a value in [-1, 1).  Per step of a running episode, in this order:
 *   1. a = the bits pi_infer_query returns for the state (skipped on a handle without a policy)
 *   2. explore iff (x0 >> 8) < eps24, eps24 = (uint32) llrint((double)epsilon * 16777216.0): epsilon = 0 never explores,
 *      epsilon = 1 always; then a = action_space[(uint32)(((uint64)x1 * n_actions) >> 32)], the table of
 *      pi_infer_set_stochastic
 *   3. action_noise != 0: a = a + action_noise * sym(x2), a float32 multiply, then an add; then
 *      a = fminf(fmaxf(a, a_min), a_max), the extremes of that table.  No clamp when action_noise == 0
 *   4. step_dynamics; ret, disc, length and the freeze exactly as in pi_infer_rollout
 *   5. not `done`: for every d with state_noise[d] != 0, s'[d] = s'[d] + state_noise[d] * sym(word d); a dimension with
 *      zero noise is not touched, the disturbed state is neither clamped nor wrapped, it is what the controller and the
 *      plugin see next and what the trajectory records; a `done` step stores its successor undisturbed.
 * With epsilon, action_noise and state_noise all zero the outputs are pi_infer_rollout's, bit for bit.
 *   pi_infer_set_stochastic  host array: the action table (n_actions >= 1 finite float32), copied to the device — the
 *                       handle's own copy; builds the handle's SIXTH module: its grid + the plugin last given to
 *                       pi_infer_set_dynamics + csrc/pi_stochastic_kernels.hip.  Needs pi_infer_set_dynamics, neither a
 *                       policy nor values.  Same cache, flags and log convention as pi_infer_set_dynamics; device = -1
 *                       handles: compile check.  pi_infer_set_dynamics drops the module again (the next stochastic call
 *                       then fails, naming pi_infer_set_stochastic)
 *   pi_infer_rollout_stochastic  arguments and outputs of pi_infer_rollout (alignment, m == 0, n_steps == 0 and traj_every
 *                       as there), plus: epsilon in [0, 1]; action_noise >= 0, finite; state_noise a HOST array of D
 *                       floats >= 0, finite, or null = none; seed, first_episode as above; gamma not NaN.  A handle
 *                       without a policy is served only when epsilon == 1 (the random-policy baseline); otherwise the
 *                       call fails, naming pi_infer_set_policy.  Every refusal is an error code and pi_last_error, never
 *                       a launch.  Asynchronous.
 *   pi_infer_random_words  probe of the stream: for rows 0 .. m the four words of (seed, first_episode + row, step, block)
 *                       into d_words, (m, 4) uint32 on the device.  m == 0 is a no-op.  Asynchronous.
 * Expected-value greedy control on the same handle (no reference counterpart): the greedy lookahead with the expectation
 * of noise-aware solving inside it, a*(s) = argmax_a Q_K(s, a), and closed-loop rollouts under it that draw the
 * stochastic rollouts' noise.  Q_K(s, a) is the definition at pi_set_disturbances, steps 1-5, evaluated at the point s
 * instead of a grid node, with the interpolation of pi_infer_greedy: per point of the set in ascending k, a_k = a when
 * da_k == 0, else fminf(fmaxf(a + da_k, a_min), a_max) with the extremes of the table of pi_infer_set_expect_greedy;
 * (s', r_k, done_k) = step_dynamics(s, a_k) (consecutive points with equal da share the step); E_k = 0 when done_k, else
 * every non-zero dx_k[d] is added to s'[d] with one float32 add (d in the handle's dimension order) and E_k is the
 * interpolation there; q_k = r_k + gamma * E_k, a multiply then an add; Q = p_0 * q_0, then Q = fmaf(p_k, q_k, Q).  The
 * argmax is pi_infer_greedy's.  With the one-point zero set (da = dx = 0, p = 1) every output is pi_infer_greedy's and
 * pi_infer_rollout_greedy's, bit for bit; at a non-terminal node, with the set and the value function of a solver handle,
 * the index is what pi_expect_improve_sweep writes there.
 *   pi_infer_set_expect_greedy  host array: the action table (n_actions >= 1 finite float32), copied to the device — the
 *                       handle's own copy; builds the handle's SEVENTH module: its grid + the plugin last given to
 *                       pi_infer_set_dynamics + the functions of csrc/pi_greedy_kernels.hip and
 *                       csrc/pi_stochastic_kernels.hip + csrc/pi_expect_greedy_kernels.hip.  Needs pi_infer_set_values
 *                       and pi_infer_set_dynamics.  Same cache, flags and log convention as pi_infer_set_dynamics;
 *                       device = -1 handles: compile check.  pi_infer_set_dynamics drops the module again (the next call
 *                       then fails, naming pi_infer_set_expect_greedy)
 *   pi_infer_set_disturbances  the set of that controller: arguments, validation and NULL-means-zeros rules of
 *                       pi_set_disturbances (K <= 64, finite values, weights >= 0 summing to 1 within 1e-4; state_offsets
 *                       (K, D) in the handle's dimension order); K = 0 drops the set.  Run-time data: an upload, never a
 *                       build, and independent of the module (before or after it, kept across pi_infer_set_dynamics).
 *                       Synchronises the device before it overwrites the table
 *   pi_infer_expect_greedy  pi_infer_greedy with Q_K in place of Q: the same arguments, outputs and rules.  Refused
 *                       without the module or without a set, naming the call that is missing.  Asynchronous.
 *   pi_infer_rollout_expect_greedy  pi_infer_rollout_stochastic with the lookahead in place of the interpolated action.
 *                       Per step of a running episode: best = argmax_a Q_K(s, a) with `lookahead_gamma`, a =
 *                       action_space[best]; then steps 2-5 of the stochastic rollouts above with the same draws from the
 *                       same counters (an exploring step takes its random action instead, from this module's table),
 *                       step_dynamics running once more on the action finally taken.  epsilon, action_noise,
 *                       state_noise, seed, first_episode, gamma and the outputs as in pi_infer_rollout_stochastic;
 *                       neither gamma may be NaN.  Needs no policy.  Refused without the module or without a set; every
 *                       refusal is an error code and pi_last_error, never a launch.  m == 0 is a no-op.  Asynchronous.
 * Stochastic hybrid rollouts (no reference counterpart: the reference's hybrid demo runs in a noiseless world, where the
 * hysteresis of its switch is never tested): pi_infer_rollout_hybrid with the stream of pi_infer_rollout_stochastic
 * inside, as ONE launch for m episodes.  The counters, the conversions and the words of blocks 0, 1 and 2 are exactly
 * those of the stochastic rollouts, so the pair and a single policy are compared under common random numbers.  Per step
 * of a running episode, in this order:
 *   1. mode: the rule of pi_infer_rollout_hybrid (float32, strict comparisons, mode 0 at the start of every episode)
 *      applied to the state the step starts from, which the step before may have disturbed; on every step taken,
 *      exploring or not.  secondary_steps += mode; switches += 1 when the mode differs from that of the previous step
 *      taken — before step 0 the mode is 0, so an episode that enters at step 0 counts one
 *   2. block 0, drawn only when eps24 != 0 or action_noise != 0; explore iff (x0 >> 8) < eps24, as in the stochastic
 *      rollouts
 *   3. action: an exploring step takes action_space[(uint32)(((uint64)x1 * n_actions) >> 32)] from the module's own
 *      exploration table — ONE table for the pair: one plant, one actuator; any other step takes the interpolated action
 *      of the mode's policy on its own grid, the bits pi_infer_query returns on that handle
 *   4. action_noise != 0: a = a + action_noise * sym(x2), a float32 multiply, then an add; then
 *      a = fminf(fmaxf(a, a_min), a_max), the extremes of the exploration table.  No clamp when action_noise == 0
 *   5. step_dynamics with the primary handle's plugin; ret, disc, length and the freeze exactly as in pi_infer_rollout
 *   6. not `done`: the state noise of block 1 (and block 2 in 6-D) as in the stochastic rollouts, step 5 there: neither
 *      clamped nor wrapped, it is what the trajectory records and what the next step's mode rule, controller and plugin see.
 * With epsilon, action_noise and state_noise all zero the outputs are pi_infer_rollout_hybrid's, bit for bit; with
 * enter = 0 they are pi_infer_rollout_stochastic's on the primary handle with the same table.
 *   pi_infer_set_partner_stochastic  host array: the exploration table (n_actions >= 1 finite float32), copied to the
 *                       device — the module's own copy; builds h's EIGHTH module: h's grid + partner's grid + the plugin
 *                       last given to pi_infer_set_dynamics(h) + the functions of csrc/pi_hybrid_kernels.hip and
 *                       csrc/pi_stochastic_kernels.hip + csrc/pi_hybrid_stochastic_kernels.hip.  The pair must pass the
 *                       checks of pi_infer_set_partner.  Same cache, flags and log convention as pi_infer_set_dynamics;
 *                       device = -1 handles: compile check.  pi_infer_set_dynamics on h drops the module again (the next
 *                       call then fails, naming pi_infer_set_partner_stochastic).  Independent of pi_infer_set_partner
 *                       and pi_infer_set_stochastic: neither is needed
 *   pi_infer_rollout_hybrid_stochastic  arguments, outputs and refusals of pi_infer_rollout_hybrid (the pair, a policy on
 *                       BOTH handles whatever epsilon is, the module missing or built for another partner grid, NaN
 *                       thresholds, enter[d] > leave[d]), plus epsilon, action_noise, state_noise, seed, first_episode
 *                       with the rules of pi_infer_rollout_stochastic, and d_switches (m) int32, which may be null like
 *                       every other output.  Every refusal is an error code and pi_last_error, never a launch.
 *                       m == 0 is a no-op, n_steps == 0 copies the start (lengths, returns, secondary_steps, last_mode,
 *                       switches 0).  Asynchronous.
 * ------------------------------------------------------------------------------------------- */
typedef struct pi_infer pi_infer;
pi_infer* pi_infer_create(int device, int D, const float* lo, const float* hi, const int32_t* grid_shape,
                          const int32_t* strides, const int32_t* corner_bits, int64_t n_corners,
                          const char* cache_dir);
void pi_infer_destroy(pi_infer* h);
int pi_infer_set_policy(pi_infer* h, const int32_t* policy, int64_t n_states, const float* action_space,
                        int n_actions);
int pi_infer_query(pi_infer* h, const float* d_points, int64_t m, float* d_actions_out, float* d_weights_out,
                   int32_t* d_indices_out, void* stream);
int pi_infer_set_dynamics(pi_infer* h, const char* dynamics_src, char* log, size_t log_len);
int pi_infer_rollout(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float* d_final,
                     float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj, int traj_every,
                     void* stream);
int pi_infer_set_partner(pi_infer* h, pi_infer* partner, char* log, size_t log_len);
int pi_infer_rollout_hybrid(pi_infer* h, pi_infer* partner, const float* d_start, int64_t m, int n_steps, float gamma,
                            const float* enter, const float* leave, float* d_final, float* d_return, int32_t* d_length,
                            uint8_t* d_terminated, int32_t* d_secondary_steps, uint8_t* d_last_mode, float* d_traj,
                            int traj_every, void* stream);
int pi_infer_set_values(pi_infer* h, const float* values, int64_t n_states, char* log, size_t log_len);
int pi_infer_resample(pi_infer* h, const int32_t* dst_shape, const int64_t* dst_strides, const float* dst_bins,
                      const int32_t* action_map, int dst_n_actions, const uint8_t* d_dst_term, float* d_dst_V,
                      int32_t* d_dst_policy, void* stream);
int pi_infer_set_greedy(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len);
int pi_infer_greedy(pi_infer* h, const float* d_points, int64_t m, float gamma, int32_t* d_best, float* d_action,
                    float* d_q_best, float* d_q_all, void* stream);
int pi_infer_rollout_greedy(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float lookahead_gamma,
                            float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj,
                            int traj_every, void* stream);
int pi_infer_set_stochastic(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len);
int pi_infer_rollout_stochastic(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float epsilon,
                                float action_noise, const float* state_noise, uint64_t seed, uint64_t first_episode,
                                float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated, float* d_traj,
                                int traj_every, void* stream);
int pi_infer_random_words(pi_infer* h, uint64_t seed, uint64_t first_episode, int64_t m, uint32_t step, uint32_t block,
                          uint32_t* d_words, void* stream);
int pi_infer_set_expect_greedy(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len);
int pi_infer_set_disturbances(pi_infer* h, int K, const float* action_offsets, const float* state_offsets,
                              const float* weights);
int pi_infer_expect_greedy(pi_infer* h, const float* d_points, int64_t m, float gamma, int32_t* d_best, float* d_action,
                           float* d_q_best, float* d_q_all, void* stream);
int pi_infer_rollout_expect_greedy(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma,
                                   float lookahead_gamma, float epsilon, float action_noise, const float* state_noise,
                                   uint64_t seed, uint64_t first_episode, float* d_final, float* d_return,
                                   int32_t* d_length, uint8_t* d_terminated, float* d_traj, int traj_every, void* stream);
/*
 * The robust lookahead and the adversary in the closed loop (csrc/pi_adversary_kernels.hip, csrc/pi_adversary.cpp; no
 * reference counterpart): the worst-case fold at pi_robust_eval_sweeps over the set of pi_infer_set_disturbances, at
 * arbitrary continuous states.
 * Adversary step.  At a state s with an action value a the controller has chosen: k* is that fold with
 * E_k = pi_greedy_expect(s'_k) (the sweeps' arithmetic, as the lookaheads use it), the discount lookahead_gamma and the
 * clamp of a + da_k to the extremes of the table of pi_infer_set_robust.  The episode moves to s'_{k*}, which is
 * f(s, a (+) da_{k*}) + dx_{k*} with no dx on a `done` step, and collects r_{k*} and done_{k*}.
 * Robust lookahead.  best = argmax_a Q_worst(s, actions[a]), strict > from -1.0e30f over ascending indices.  The
 * adversary's answer to the winner is the k* computed for it.  The successor, reward and flag that are kept are action 0's
 * until an action wins.
 *   pi_infer_set_robust   host array: the action table (n_actions >= 1 finite float32), copied to the device; builds the
 *                       handle's adversary module (a further code object, cached like the others).  Needs
 *                       pi_infer_set_values and pi_infer_set_dynamics; a later pi_infer_set_dynamics drops the module.
 *   pi_infer_robust     the batched query: the arguments, nullable outputs and rules of pi_infer_greedy plus d_worst (m)
 *                       int32, the k* of the winning action as a row index of the installed table, -1 when no action won.
 *   pi_infer_rollout_adversary  m episodes of n_steps steps, one launch, no random numbers; the outputs of
 *                       pi_infer_rollout.  controller 0: the action of the interpolated policy table (needs
 *                       pi_infer_set_policy), then the adversary step; controller 1: the robust lookahead and the
 *                       adversary's answer to it, nothing stepped twice.
 * Refusals, by return code, in this order: a missing module, then a missing set; NaN discounts; a controller other than
 * 0 or 1; controller 0 on a handle without a policy; then what the other rollouts refuse.
 */
int pi_infer_set_robust(pi_infer* h, const float* action_space, int n_actions, char* log, size_t log_len);
int pi_infer_robust(pi_infer* h, const float* d_points, int64_t m, float gamma, int32_t* d_best, float* d_action,
                    float* d_q_best, float* d_q_all, int32_t* d_worst, void* stream);
int pi_infer_rollout_adversary(pi_infer* h, const float* d_start, int64_t m, int n_steps, float gamma, float lookahead_gamma,
                               int controller, float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated,
                               float* d_traj, int traj_every, void* stream);
int pi_infer_set_partner_stochastic(pi_infer* h, pi_infer* partner, const float* action_space, int n_actions, char* log,
                                    size_t log_len);
int pi_infer_rollout_hybrid_stochastic(pi_infer* h, pi_infer* partner, const float* d_start, int64_t m, int n_steps,
                                       float gamma, const float* enter, const float* leave, float epsilon,
                                       float action_noise, const float* state_noise, uint64_t seed, uint64_t first_episode,
                                       float* d_final, float* d_return, int32_t* d_length, uint8_t* d_terminated,
                                       int32_t* d_secondary_steps, uint8_t* d_last_mode, int32_t* d_switches, float* d_traj,
                                       int traj_every, void* stream);

/* Tuning: the `what` of pi_set_option. */
enum pi_option_code {
    PI_OPTION_EVAL_CPW = 0,          /* chunks per workgroup of the evaluation sweeps (1..64) */
    PI_OPTION_IMPROVE_CPW = 1,       /* chunks per workgroup of the improvement / value sweeps (1..64) */
    PI_OPTION_GRAPHS = 2,            /* replay small evaluation batches as hipGraphs (0 | 1) */
    PI_OPTION_RESIDENT = 3,          /* run whole-grid batches of small grids in the LDS-resident kernel (0 | 1) */
    PI_OPTION_MEMORY_ORDER = 4,      /* MEMORY ORDER of the dimensions (before pi_compile, once; see below) */
    PI_OPTION_BUILD_PUSH = 5,        /* value != 0: build the fused swept-first kernel of the peer-to-peer exchange now
                                        (after pi_compile; a compile check on host-only handles) */
    PI_OPTION_KEEP_LIVE_LIST = 6,    /* keep the live-state list of pi_prepare_mask even when it fills no idle lanes
                                        (0 | 1; the fused exchange of a sharded run delivers from the list sweeps) */
    PI_OPTION_STRIP_STATES = 7,      /* STRIP SCHEDULE of the sweeps: states per period (see pi_plan_schedule; -1 = the
                                        library's choice for the grid, the default; 0 = slab schedule; PI_MI355_STRIP in
                                        the environment at pi_create sets the same) */
    PI_OPTION_XCD_RUN_FAILED = 8,    /* the last pi_policy_iteration launch on the XCD-local kernel did not go through
                                        (value: enum pi_xcd_failure) */
    PI_OPTION_PAIR_TABLE = 9         /* PAIR TABLE of the improvement sweeps: whole-grid pi_improve_sweep calls on 4-D grids
                                        with 8 n < 2^32 pack V into {V[s], V[s + row]} pairs (an 8 n-byte buffer of the
                                        handle, packed on every call) and gather from those with half as many loads.
                                        -1 = the library's choice for the grid, the default; 0 = off; 1 = on where the
                                        grid admits it.  Switching it ON takes effect at pi_compile, which builds the
                                        kernels; results do not depend on it */
};
/* The values PI_OPTION_XCD_RUN_FAILED takes. */
enum pi_xcd_failure {
    PI_XCD_FAILURE_COUNT = 1,        /* count it: two failures switch that kernel off for the handle */
    PI_XCD_FAILURE_SWITCH_OFF = 2    /* count it and switch that kernel off now */
};
/* PI_OPTION_MEMORY_ORDER: digit k (base 8) of the value is the dimension — numbered as in pi_create and in
 * step_dynamics' arguments — that is stored as memory dimension k, 0 = slowest; e.g. 03120 (octal) = order (0, 2, 1, 3).
 * From then on EVERY flat state index of this ABI (s_begin / s_end, the entries of V, policy and the mask, the indices the
 * interpolation probe returns) refers to that order: index = sum_k i_{order[k]} * stride_k with row-major
 * strides over the permuted shape.  The reference has one order, the meshgrid's (:84-87); which dimensions
 * are slow decides how far apart in memory the 2^D corners of a successor cell lie and how long a value
 * stays useful in an XCD's L2 — the best order beats the user's by 7-11 % on the evaluation sweeps of the
 * big BASELINE grids (tools/dim_order_sweep.py).  The order-sensitive arithmetic (corner weights as products
 * over the dimensions, the fmaf chain over the corners, :580-614, :616-649) stays in the caller's dimension
 * order, so results do not depend on the memory order, bit for bit; neither do they depend on PI_OPTION_EVAL_CPW,
 * PI_OPTION_IMPROVE_CPW, PI_OPTION_GRAPHS, PI_OPTION_RESIDENT and PI_OPTION_STRIP_STATES. */
int pi_set_option(pi_handle* h, int what, int64_t value);

/* Introspection: the `what` of pi_info.  Every other code returns -1. */
enum pi_info_code {
    PI_INFO_N_STATES = 0,                     /* states of the grid */
    PI_INFO_N_ACTIONS = 1,                    /* actions */
    PI_INFO_DIMS = 2,                         /* D */
    PI_INFO_EVAL_CPW = 3,                     /* chunks per workgroup of the evaluation sweeps */
    PI_INFO_EVAL_VGPRS = 4,                   /* VGPRs of the evaluation kernel (-1 until a device loads it) */
    PI_INFO_IMPROVE_VGPRS = 5,                /* VGPRs of the improvement kernel (-1 until a device loads it) */
    PI_INFO_COMPUTE_UNITS = 6,                /* compute units of the device */
    PI_INFO_CACHE_HIT = 7,                    /* 1 if the last pi_compile was served from the cache */
    PI_INFO_IMPROVE_CPW = 8,                  /* chunks per workgroup of the improvement sweeps */
    PI_INFO_CACHED_GRAPHS = 9,                /* hipGraphs cached by the handle */
    PI_INFO_GRAPHS_ENABLED = 10,              /* 1 if PI_OPTION_GRAPHS is on */
    PI_INFO_EVAL_BLOCK = 11,                  /* threads per workgroup of the evaluation sweeps */
    PI_INFO_IMPROVE_BLOCK = 12,               /* threads per workgroup of the improvement sweeps */
    PI_INFO_RESIDENT_STATES_PER_THREAD = 13,  /* states per thread of the LDS-resident batch kernel (0: grid too big) */
    PI_INFO_RESIDENT_ENABLED = 14,            /* 1 if that kernel is enabled (PI_OPTION_RESIDENT) */
    PI_INFO_DEBUG_CHECKS = 15,                /* 1 if the handle's kernels are checked (pi_debug_report) */
    PI_INFO_LIVE_STATES = 16,                 /* live states listed by pi_prepare_mask (0: no list in use) */
    PI_INFO_EVAL_LIST_ENTRIES = 17,           /* entries of the per-evaluation list of pi_eval_begin (0: none) */
    PI_INFO_MEMORY_ORDER = 18,                /* the memory order as set with PI_OPTION_MEMORY_ORDER (octal digits,
                                                 identity by default) */
    PI_INFO_FLOW_WORKGROUPS = 19,             /* workgroups of the dataflow evaluation kernel (0: not for this grid; 1 on
                                                 a host-only handle whose grid it serves) */
    PI_INFO_RECIPROCAL_DIV = 20,              /* base: code + d (d < D) = 1 if dimension d's interpolation division
                                                 runs through the proven reciprocal path */
    PI_INFO_XCD_ENABLED = 30,                 /* 1 if the XCD-local evaluation kernel is in use */
    PI_INFO_XCD_EVALUATIONS = 31,             /* evaluations attempted in it */
    PI_INFO_XCD_FALLBACKS = 32,               /* ... run again after a placement failure or a time-out */
    PI_INFO_WHOLE_RUNS = 33,                  /* whole runs launched (pi_policy_iteration) */
    PI_INFO_WHOLE_RUN_AVAILABLE = 34,         /* 1 if pi_policy_iteration serves this grid */
    PI_INFO_STRIP_STATES = 35,                /* states per period of the strip schedule in use (0: slab schedule) */
    PI_INFO_PAIR_TABLE = 37,                  /* 1 if the last pi_improve_sweep gathered from the pair table
                                                 (PI_OPTION_PAIR_TABLE); 36 stays unassigned */
    PI_INFO_DISTURBANCES = 38                 /* points of the disturbance set in use (pi_set_disturbances; 0: none) */
};
int64_t pi_info(pi_handle* h, int what);

/*
 * Checked build (sanitizer row: the reference has none; GPU address sanitizers are not
 * available on this platform).  With PI_MI355_DEBUG=1 in the environment when pi_create runs, the handle's
 * kernels check every index they derive from DATA before using it — the action a policy entry names
 * (kind 1: where = flat state, value = the entry) and the cell a successor falls in (kind 2: where = the
 * cell's flat index) — count violations, remember the first and carry on with index 0 instead of reading
 * out of bounds.  pi_debug_report synchronises the device, copies {violations, kind, where, value} of the
 * sweeps launched since the last report to out4 (host) and clears them; it fails on a handle built
 * without the checks.  Results of a run without violations are those of the unchecked kernels.
 * Every code object of the handle that is built from the sweep unit keeps a tally of its own: the sweeps'
 * module, the push module of an exchange plan and the expectation module of pi_set_disturbances, as far as
 * they are loaded.  The report covers all of them: violations is their sum, and kind / where / value are
 * those of the first module in that order that recorded a violation; all of them are cleared.
 */
int pi_debug_report(pi_handle* h, uint32_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* PI_MI355_H_ */
