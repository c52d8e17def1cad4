"""
GPU end-to-end checks that close the parity loop ON the device ("next round" item 3):

* the HIP path against the reference-HELD fixtures themselves (tests/golden/reference_results.npz =
  the two archives the reference commits under runners/results/): full run() through the solver,
  and the "reference policy is greedy to 4 ulp" check with Q computed by pi_eval_sweep on the GPU;
* pi_sinf / pi_cosf / pi_fmodf evaluated on the GPU over 2^24 seeded arguments (dense around the
  angle range, huge, special values), bit for bit against the g++ build of include/pi_math.h;
* host features that until now only ran on the CPU checker: the crane's goal-value seeding
  (boolean-mask writes on torch-ROCm tensors), save_checkpoint -> load_checkpoint -> run(), and the
  value_iteration() loop.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info, Option
from tests import helpers as H

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _oracle_grid(name, shape):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    term, tval = H.terminal_mask(name, states)
    return bins, (lo, hi, gshape, strides), states, term, tval


@pytest.mark.parametrize("name", ["mountain_car", "continuous_mountain_car"])
def test_gpu_run_against_reference_committed_results(name, cuda_device):
    """The only reference-PRODUCED end-to-end numbers (runners/results/*.npz, RTX 3090 + libdevice)
    against the HIP path directly: (a) full run() on the GPU — policy agreement >= 99.5 %,
    |dV| <= 2e-4 on >= 99.5 % of the states; (b) with Q(s, a) computed by pi_eval_sweep ON THE GPU
    from the reference's own committed V, the reference's committed policy is greedy to within
    4 ulp everywhere, and wherever the GPU run ends with another action the two are a tie."""
    torch = _torch()
    ref = np.load(H.GOLDEN / "reference_results.npz")
    cls = envs.ENVS[name]
    shape = tuple(int(x) for x in ref[f"{name}_grid_shape"])
    solver = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cls.CONFIG), device=cuda_device)
    assert np.array_equal(solver.bounds_low, ref[f"{name}_bounds_low"])
    assert np.array_equal(solver.bounds_high, ref[f"{name}_bounds_high"])
    assert np.array_equal(solver.action_space, ref[f"{name}_action_space"])
    n, nA = solver.n_states, solver.n_actions
    V_ref = ref[f"{name}_value_function"].astype(np.float32)
    P_ref = ref[f"{name}_policy"].astype(np.int32)

    # (b) first, while the solver still owns its device arrays: Q on the device from the reference's V
    eng = solver._backend.engine
    gamma = float(np.float32(solver.config.gamma))
    d_V = torch.from_numpy(V_ref).to(cuda_device)
    d_Q = torch.empty((nA, n), dtype=torch.float32, device=cuda_device)
    for a in range(nA):
        d_pol = torch.full((n,), a, dtype=torch.int32, device=cuda_device)
        eng.eval_sweep(d_V.data_ptr(), d_Q[a].data_ptr(), d_pol.data_ptr(), solver.d_terminal_mask.data_ptr(),
                       0, n, gamma, 0)
    torch.cuda.synchronize()
    Q = d_Q.cpu().numpy().T.astype(np.float64)
    live = ~solver.d_terminal_mask[:n].cpu().numpy().astype(bool)

    # (a) the full run
    solver.run()
    assert solver.stats["stable"]
    agree = float(np.mean(solver.policy == P_ref))
    dv = np.abs(solver.value_function - V_ref)
    assert agree >= 0.995, agree                                   # measured: 0.9971 / 0.9995
    assert float(np.mean(dv <= 2e-4)) >= 0.995, float(np.mean(dv <= 2e-4))

    idx = np.arange(n)
    q_ref, q_mine, q_max = Q[idx, P_ref], Q[idx, solver.policy], Q.max(axis=1)
    ulps = 5e-7 * np.maximum(1.0, np.abs(q_max))                    # ~4 ulp of a float32 of that size
    assert np.all((q_max - q_ref)[live] <= ulps[live]), float(np.max((q_max - q_ref)[live]))
    differ = live & (solver.policy != P_ref)
    assert differ.sum() <= 0.005 * live.sum()
    gap = np.abs(q_mine - q_ref)[differ]
    assert np.mean(gap <= ulps[differ]) >= 0.98 and np.all(gap <= 1e-2), (int(differ.sum()), float(gap.max()))


# A 2-D "env" whose successor IS the math under test: next = (sin s0, cos s0), reward = fmod(s0, s1).
MATH_PROBE_SRC = r'''
__device__ void step_dynamics(float x, float y, float a, float* nx, float* ny, float* rew, bool* done) {
    *nx = sinf(x);
    *ny = cosf(x);
    *rew = fmodf(x, y);
    (void)a;
    *done = false;
}
'''


def test_pi_math_on_gpu_dense(cuda_device):
    """include/pi_math.h on the GPU itself: 2^24 seeded arguments — dense in [-4 pi, 4 pi], every
    multiple of pi/2 up to 1e5 and its float neighbours, large and huge magnitudes, denormals, zeros,
    infinities and NaN — through the product's hipRTC path (pi_probe_step with the plugin above),
    bit for bit against the same header compiled by g++ (the oracle in the product's arithmetic mode).
    The kernels and the oracle share this header, so this is the direct check that the two
    compilers produce the same bits from it (NaN results compared as NaN)."""
    torch = _torch()
    m = 1 << 24
    rng = np.random.default_rng(2024)
    x = np.empty(m, dtype=np.float32)
    y = np.empty(m, dtype=np.float32)
    k = m // 8
    x[:4 * k] = rng.uniform(-4 * np.pi, 4 * np.pi, 4 * k)                       # the angle range, dense
    x[4 * k:5 * k] = rng.uniform(-1, 1, k) * 1.0e3
    x[5 * k:6 * k] = rng.uniform(-1, 1, k) * 1.0e6                               # beyond the fast-path cut (1e5)
    x[6 * k:7 * k] = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32).view(np.float32)   # any bits
    q = (np.arange(-100_000, 100_000) * (np.pi / 2)).astype(np.float32)
    edge = np.concatenate([q, np.nextafter(q, np.float32(np.inf)), np.nextafter(q, np.float32(-np.inf)),
                           np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.17549435e-38, 3.4e38,
                                     -3.4e38, 1e-30, 1e5, 100000.01, -1e5], dtype=np.float32)])
    x[7 * k:7 * k + len(edge)] = edge
    x[7 * k + len(edge):] = rng.uniform(-10, 10, m - 7 * k - len(edge))
    # divisors: the angle wrap's 2 pi, random magnitudes, any bits, special values against special values
    y[:4 * k] = np.float32(2 * np.float32(np.pi))
    y[4 * k:6 * k] = (rng.uniform(-1, 1, 2 * k) * 10.0).astype(np.float32)
    y[6 * k:7 * k] = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32).view(np.float32)
    y[7 * k:] = np.resize(np.array([1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38, 6.2831855, 0.5],
                                   dtype=np.float32), m - 7 * k)
    states = np.stack([x, y], axis=1)

    bins = [np.linspace(-1, 1, 4, dtype=np.float32)] * 2
    eng = _native.Engine(2, [4, 4], [-1.0, -1.0], [1.0, 1.0], bins, np.zeros(1, np.float32),
                         device=cuda_device.index or 0)
    eng.compile(MATH_PROBE_SRC)
    d_st = torch.from_numpy(states).to(cuda_device)
    d_act = torch.zeros(m, dtype=torch.float32, device=cuda_device)
    d_next = torch.empty((m, 2), dtype=torch.float32, device=cuda_device)
    d_rew = torch.empty(m, dtype=torch.float32, device=cuda_device)
    d_done = torch.empty(m, dtype=torch.uint8, device=cuda_device)
    eng.probe_step(d_st.data_ptr(), d_act.data_ptr(), d_next.data_ptr(), d_rew.data_ptr(), d_done.data_ptr(), m)
    torch.cuda.synchronize()
    g_next, g_rew = d_next.cpu().numpy(), d_rew.cpu().numpy()
    eng.close()

    chk = oracle.build(2, MATH_PROBE_SRC)
    assert not chk.libm
    o_next, o_rew, _ = chk.step(states, np.zeros(m, np.float32))
    for what, got, want in (("sin", g_next[:, 0], o_next[:, 0]), ("cos", g_next[:, 1], o_next[:, 1]),
                            ("fmod", g_rew, o_rew)):
        both_nan = np.isnan(got) & np.isnan(want)
        same = (got.view(np.uint32) == want.view(np.uint32)) | both_nan
        bad = np.flatnonzero(~same)
        assert bad.size == 0, (what, bad.size, x[bad[:5]], y[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the probe really exercised the functions (not a constant-folded stub)
    assert np.nanmax(np.abs(g_next[:4 * k, 0])) > 0.999 and abs(float(g_next[7 * k + len(q) // 2, 1]) - 1.0) < 1e-6


def test_crane_goal_seeding_end_to_end(cuda_device):
    """OverheadCrane through the solver on the GPU (reference runners/overhead_crane_cuda.py:193-206):
    goal cells start at 1 / (1 - gamma) in BOTH Jacobi buffers (boolean-mask writes on device
    tensors), are terminal, keep that value through run(), and the whole run equals the oracle's
    run from the same seeded V bit for bit."""
    name, shape = "overhead_crane", (13, 9, 13, 9)
    cls = envs.ENVS[name]
    cfg = envs.CudaPIConfig(**{**cls.CONFIG, "max_eval_iter": 400, "max_pi_iter": 6})
    s = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device, target_x=0.0)
    n = s.n_states
    goal = s._goal_mask
    seed = np.float32(1.0 / (1.0 - cfg.gamma))
    assert goal.any() and s.d_value_function.is_cuda
    v0 = s.d_value_function[:n].cpu().numpy()
    assert np.all(v0[goal] == seed) and np.all(v0[~goal] == 0.0)
    assert np.array_equal(s.d_new_value_function[:n].cpu().numpy(), v0)
    assert np.all(s.d_terminal_mask[:n].cpu().numpy().astype(bool)[goal])
    s.run()
    assert np.all(s.value_function[goal] == seed)                     # terminal: copied by every sweep
    bins, (lo, hi, gshape, strides), states, term, tval = _oracle_grid(name, shape)
    V0 = np.zeros(n, np.float32)
    V0[goal] = seed
    ref = H.oracle_for(name).run(states, cls.ACTIONS, term, lo, hi, gshape, strides, gamma=cfg.gamma,
                                 theta=cfg.theta, max_eval_iter=cfg.max_eval_iter, max_pi_iter=cfg.max_pi_iter,
                                 terminal_value=tval, V0=V0)
    assert s.stats["sweeps_per_iter"] == list(ref["sweeps_per_iter"])
    assert np.array_equal(s.policy, ref["policy"])
    H.assert_bits_equal(s.value_function, ref["value_function"], "crane V")
    # the generic hook on its own: any mask, both buffers
    s2 = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device, target_x=0.5)
    mask = np.zeros(n, bool)
    mask[::7] = True
    s2._seed_values(mask, 3.25)
    for buf in (s2.d_value_function, s2.d_new_value_function):
        h = buf[:n].cpu().numpy()
        assert np.all(h[mask] == np.float32(3.25))
    s2._backend.close()


@pytest.mark.parametrize("name,shape", [("mountain_car", (64, 48)), ("cartpole", (11, 9, 13, 7))])
def test_checkpoint_resume_on_gpu(name, shape, cuda_device, tmp_path):
    """save_checkpoint after one outer iteration, load_checkpoint into a fresh solver, run():
    identical (bit for bit) to the uninterrupted run — device-tensor copies, counters and all."""
    cls = envs.ENVS[name]
    cfg = envs.CudaPIConfig(**{**cls.CONFIG, "max_eval_iter": 300, "max_pi_iter": 8})

    def fresh():
        return cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device)

    whole = fresh()
    whole.run()
    a = fresh()
    a.policy_evaluation()
    a.stats["pi_iterations"] = 1
    a.policy_improvement()
    a.save_checkpoint(tmp_path / "ck")
    snap = np.load(tmp_path / "ck.npz")
    n = a.n_states
    H.assert_bits_equal(snap["value_function"], a.d_value_function[:n].cpu().numpy(), "checkpoint V")
    assert np.array_equal(snap["policy"], a.d_policy[:n].cpu().numpy())
    b = fresh()
    b.load_checkpoint(tmp_path / "ck")
    assert b.d_value_function.is_cuda and b.stats["eval_sweeps"] == a.stats["eval_sweeps"]
    H.assert_bits_equal(b.d_new_value_function[:n].cpu().numpy(), snap["value_function"], "second Jacobi buffer")
    a._backend.close()
    # continue: the remaining outer iterations of the uninterrupted run
    b.config.max_pi_iter = cfg.max_pi_iter - 1
    b.run()
    assert np.array_equal(b.policy, whole.policy)
    H.assert_bits_equal(b.value_function, whole.value_function, "resumed run")
    assert b.stats["eval_sweeps"] == whole.stats["eval_sweeps"]
    with pytest.raises(ValueError, match="different grid"):
        other = cls(H.env_bins_space(name, tuple(g + 1 for g in shape)), cls.ACTIONS, cfg, device=cuda_device)
        try:
            other.load_checkpoint(tmp_path / "ck")
        finally:
            other._backend.close()


@pytest.mark.parametrize("name,shape,max_iter", [("mountain_car", (30, 20), 2000), ("cartpole_swingup", (9, 7, 11, 7), 120),
                                                 ("double_cartpole", (4, 3, 4, 3, 4, 3), 60)])
def test_value_iteration_loop_on_gpu(name, shape, max_iter, cuda_device):
    """value_iteration() (the fused form the reference's README sketches at :790-799) on the GPU
    against the oracle's value_sweep driven by the same loop (residual looked at on sweeps 0, 25, ...
    and the last): same number of sweeps, V, policy and last residual, bit for bit."""
    cls = envs.ENVS[name]
    cfg = envs.CudaPIConfig(**{**cls.CONFIG, "gamma": 0.95, "theta": 1e-5, "max_eval_iter": max_iter})
    s = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device)
    delta = s.value_iteration()
    n = s.n_states
    bins, (lo, hi, gshape, strides), states, term, tval = _oracle_grid(name, shape)
    chk = H.oracle_for(name)
    V = np.zeros(n, np.float32)
    V[term] = np.float32(tval)
    pol = np.zeros(n, np.int32)
    gamma = np.float32(cfg.gamma)
    sweeps, o_delta = 0, float("inf")
    for i in range(max_iter):
        V, pol, d, _ = chk.value_sweep(states, cls.ACTIONS, pol, V, term, lo, hi, gshape, strides, gamma)
        sweeps += 1
        if i % 25 == 0 or i == max_iter - 1:
            o_delta = d
            if d < cfg.theta:
                break
    assert s.stats["value_sweeps"] == sweeps
    assert np.float32(delta) == np.float32(o_delta)
    H.assert_bits_equal(s.d_value_function[:n].cpu().numpy(), V, "value iteration V")
    assert np.array_equal(s.d_policy[:n].cpu().numpy(), pol)
    s._backend.close()


def test_64_bit_addressing_path_at_2_pow_30_states(cuda_device):
    """Grids of n >= 2^30 states no longer fit 32-bit BYTE offsets (4 n >= 2^32): the kernels switch
    to 64-bit element addressing (PI_OFF32 == false in pi_sweep_kernels.hip) — the "buy VRAM" axis
    where 288 GB matter (the reference's own limits: src/cuda_policy_iteration.py:932, :1051-1060).
    double_cartpole 32^6 = 2^30 states, ~14 GB of buffers: one evaluation sweep checked by the
    residual (== an independent torch reduction), terminal copies, shard invariance, and oracle
    windows at the start, in the middle and at the very end of the table; windowed improvement
    sweeps against the oracle as well."""
    torch = _torch()
    name, shape = "double_cartpole", (32,) * 6
    cls = envs.ENVS[name]
    n = 32 ** 6
    assert n == 1 << 30 and 4 * n >= 1 << 32
    bins = H.env_bins(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    eng = _native.Engine(6, [32] * 6, [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                         device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    assert "PI_OFF32" in eng.kernel_source(envs.dynamics_source(name))
    gamma = float(np.float32(0.999))
    gen = torch.Generator(device=cuda_device).manual_seed(3)
    d_V = torch.randn(n, generator=gen, dtype=torch.float32, device=cuda_device)
    d_pol = torch.randint(0, len(acts), (n,), generator=gen, dtype=torch.int32, device=cuda_device)
    lim = envs.DoubleCartPoleCuda._TH_FAIL
    bad = [np.abs(bins[0]) > 2.4, np.zeros(32, bool), np.abs(bins[2]) > lim, np.zeros(32, bool),
           np.abs(bins[4]) > lim, np.zeros(32, bool)]
    term = torch.zeros(shape, dtype=torch.bool, device=cuda_device)
    for d, b in enumerate(bad):
        view = [1] * 6
        view[d] = 32
        term |= torch.from_numpy(b).to(cuda_device).view(view)
    d_term = term.reshape(-1).to(torch.uint8)
    del term
    d_Vn = torch.empty_like(d_V)
    d_delta = torch.zeros(1, dtype=torch.float32, device=cuda_device)
    eng.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), 0, n, gamma,
                   d_delta.data_ptr())
    torch.cuda.synchronize()
    assert float(d_delta.item()) == float((d_Vn - d_V).abs().max().item())
    tmask = d_term.bool()
    assert int(tmask.sum()) > 0 and torch.equal(d_Vn[tmask], d_V[tmask])
    assert not torch.equal(d_Vn[-4096:], d_V[-4096:]) or bool(tmask[-4096:].all())     # the far end was swept
    del tmask
    # the same sweep in three ragged pieces (what a sharded run launches) gives the same table
    d_Vs = torch.empty_like(d_V)
    cuts = [0, n // 3 + 17, n - (1 << 28) - 5, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        eng.eval_sweep(d_V.data_ptr(), d_Vs.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), a, b, gamma, 0)
    torch.cuda.synchronize()
    assert torch.equal(d_Vs, d_Vn)
    del d_Vs
    chk = H.oracle_for(name)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    Vh, polh, termh = d_V.cpu().numpy(), d_pol.cpu().numpy(), d_term.cpu().numpy()
    d_changed = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    for a, b in [(0, 1536), (n // 2 - 1000, n // 2 + 1000), (n - (1 << 29) - 700, n - (1 << 29) + 700), (n - 1536, n)]:
        sub = np.arange(a, b)
        idx = np.stack(np.unravel_index(sub, shape), axis=1)
        pad_states = np.zeros((b, 6), dtype=np.float32)          # calloc: only rows [a, b) are ever touched
        pad_states[a:b] = np.stack([bins[d][idx[:, d]] for d in range(6)], axis=1)
        o_Vn = np.zeros(b, dtype=np.float32)
        chk.eval_sweep(pad_states, acts, polh[:b], Vh, termh[:b], lo, hi, gshape, strides, gamma, a, b, out=o_Vn)
        H.assert_bits_equal(d_Vn[a:b].cpu().numpy(), o_Vn[a:b], f"2^30 eval window [{a},{b})")
        eng.improve_sweep(d_V.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), a, b, gamma, d_changed.data_ptr())
        o_pol, o_changed = chk.improve_sweep(pad_states, acts, polh[:b], Vh, termh[:b], lo, hi, gshape, strides,
                                             gamma, a, b)
        assert np.array_equal(d_pol[a:b].cpu().numpy(), o_pol[a:b])
        assert int(d_changed.item()) == o_changed
        del pad_states, o_Vn
    eng.close()


def test_device_inference_matches_the_reference_function(cuda_device):
    """SURVEY row f2, device half: the batched HIP kernel behind utils.barycentric (DevicePolicy /
    ``device=``) against tests/golden/barycentric_utils.npz — vectors produced in the build container
    by the reference's OWN utils/barycentric.py (numba typing).  Indices equal and weights bit-equal
    on 2 000 seeded points per dimension count (out-of-range, exact-node and last-cell points
    included); the interpolated action within 4 ulp-sized steps of the reference's (its `@` leaves the
    summation order to BLAS; the kernel sums in ascending corner order); and the device path equals
    this package's numpy twin exactly on a larger batch."""
    from itertools import product
    from utils.barycentric import DevicePolicy, get_barycentric_weights_and_indices, get_optimal_action
    gold = np.load(H.GOLDEN / "barycentric_utils.npz")
    for D in (2, 4, 6):
        name, shape = str(gold[f"d{D}_env"]), tuple(int(x) for x in gold[f"d{D}_shape"])
        bins = H.env_bins(name, shape)
        lo, hi, gshape, strides = oracle.grid_metadata(bins)
        bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
        pts = gold[f"d{D}_points"]
        policy, actions = gold[f"d{D}_policy"], gold[f"d{D}_actions"]
        dp = DevicePolicy(policy, actions, lo, hi, gshape, strides, bits, device=cuda_device)
        w, idx = dp.weights_and_indices(pts)
        assert w.dtype == np.float32 and idx.dtype == np.int32 and w.shape == (len(pts), 1 << D)
        assert np.array_equal(idx, gold[f"d{D}_indices"])
        H.assert_bits_equal(w, gold[f"d{D}_weights_numba"], f"D={D} device weights")
        act = dp(pts[:300])
        want = gold[f"d{D}_optimal_action"]
        tol = 4 * np.spacing(np.float32(np.abs(actions).max())) * (1 << D) / 4
        assert act.dtype == np.float32 and np.max(np.abs(act.astype(np.float64) - want)) <= tol
        # the module-level functions with device=: a batch, and a single state like the reference's call
        w2, idx2 = get_barycentric_weights_and_indices(pts[:64], lo, hi, gshape, strides, bits, device=cuda_device)
        assert np.array_equal(idx2, idx[:64]) and np.array_equal(w2.view(np.uint32), w[:64].view(np.uint32))
        one = get_optimal_action(pts[7], policy, actions, lo, hi, gshape, strides, bits, device=cuda_device)
        assert np.ndim(one) == 0 and np.float32(one) == act[7]
        # against the numpy twin on a bigger batch, incl. points far outside the grid
        rng = np.random.default_rng(D)
        big = H.sample_states(rng, bins, 50_000)
        big[::97] *= 40.0
        wn, idxn = get_barycentric_weights_and_indices(big, lo, hi, gshape, strides, bits)
        wd, idxd = dp.weights_and_indices(big)
        assert np.array_equal(idxd, idxn)
        H.assert_bits_equal(wd, wn, f"D={D} device vs numpy weights")
        seq = np.zeros(len(big), np.float32)
        for c in range(1 << D):                                    # ascending corners, multiply then add
            seq = seq + wn[:, c] * actions[policy[idxn[:, c]]]
        H.assert_bits_equal(dp(big), seq, f"D={D} device action")
        # states already on the device: a device tensor comes back, same bits, no host round trip
        d_big = _torch().from_numpy(big).to(cuda_device)
        d_act = dp(d_big)
        assert _torch().is_tensor(d_act) and d_act.device == d_big.device
        H.assert_bits_equal(d_act.cpu().numpy(), seq, f"D={D} device action from a device tensor")
        with pytest.raises(ValueError, match="float32"):
            dp(d_big.double())
        # a permuted corner table is honoured (the reference takes corner_bits as an argument)
        perm = rng.permutation(1 << D)
        dq = DevicePolicy(policy, actions, lo, hi, gshape, strides, bits[perm], device=cuda_device)
        wq, idxq = dq.weights_and_indices(pts[:128])
        assert np.array_equal(idxq, idx[:128][:, perm]) and np.array_equal(wq.view(np.uint32), w[:128][:, perm].view(np.uint32))
        dq.close()
        dp.close()
    with pytest.raises(_native.NativeError, match="not an index"):
        bits = np.array(list(product([0, 1], repeat=2)), dtype=np.int32)
        DevicePolicy(np.full(6, 9, np.int32), np.zeros(3, np.float32), [0, 0], [1, 1], [2, 3], [3, 1], bits,
                     device=cuda_device)




def test_plan_ranges_tile_the_shard_and_a_missing_peer_is_an_error_not_a_hang(cuda_device, monkeypatch):
    """The sharded driver's launch ranges (pi_plan_ranges) of every logical rank are disjoint, cover
    exactly its shard and put every row a peer waits for into a swept-first range; and the in-process
    transport bounds its host waits: a rank whose peer never arrives gets an error after
    PI_MI355_COMM_TIMEOUT seconds (failure -> abort with a message, never a hang),
    after which the handle refuses sharded sweeps until a new plan is made."""
    import threading
    import time
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    monkeypatch.setenv("PI_MI355_EXCHANGE", "halo")
    name, shape, world = "cartpole_swingup", (18, 7, 9, 8), 4
    cls = envs.ENVS[name]
    cfg = envs.CudaPIConfig(**cls.CONFIG)
    group = f"ranges-{uuid.uuid4().hex}"
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=cuda_device)):
                s = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device,
                        transport=T.NativeTransport.local(r, world, group))
                out[r] = (s._s_begin, s._s_end, s._backend.engine.plan_ranges(), dict(s._comm.info))
                s._backend.close()
        except Exception as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors and all(o is not None for o in out), errors
    for a, b, ranges, info in out:
        assert info["mode"] == "halo" and ranges
        assert {k for k, _, _ in ranges} <= {0, 1}
        spans = sorted((lo, hi) for _, lo, hi in ranges)
        assert spans[0][0] == a and spans[-1][1] == b
        assert all(x[1] == y[0] for x, y in zip(spans, spans[1:]))           # disjoint, no holes
        assert sum(1 for k, _, _ in ranges if k == 0) == info["send_ranges"]
        assert sum(1 for k, _, _ in ranges if k == 1) == info["interior_ranges"]

    # a peer that never shows up: bounded wait, then an error
    monkeypatch.setenv("PI_MI355_COMM_TIMEOUT", "2")
    lonely = f"lonely-{uuid.uuid4().hex}"
    t0 = time.perf_counter()
    with pytest.raises(_native.NativeError, match="gave up waiting"):
        cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device,
            transport=T.NativeTransport.local(0, 2, lonely))             # the plan's all-gather needs rank 1
    assert 1.5 < time.perf_counter() - t0 < 60.0


@pytest.mark.parametrize("name,shape", [("pendulum", (64, 48)), ("pendulum", (200, 200)),
                                         ("double_pendulum_swingup", (12, 9, 11, 17)), ("double_cartpole", (4, 3, 5, 3, 4, 6))])
def test_null_mask_means_no_terminal_states(name, shape, cuda_device):
    """term == NULL (what the solver passes for envs without terminal states: no mask stream, and no
    old-value stream on sweeps without a residual) gives exactly what an all-zero mask gives: single
    sweeps with and without a residual, batches (eager, graph and LDS-resident paths), improvement and
    value sweeps, and the reach probe; and the solver really passes NULL for such envs and the tensor
    for envs with terminal states."""
    torch = _torch()
    cls = envs.ENVS[name]
    bins = H.env_bins(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    D = len(shape)
    eng = _native.Engine(D, list(shape), [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                         device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    n = int(np.prod(shape))
    rng = np.random.default_rng(9)
    V = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(cuda_device)
    pol = torch.from_numpy(rng.integers(0, len(acts), n).astype(np.int32)).to(cuda_device)
    zero = torch.zeros(n, dtype=torch.uint8, device=cuda_device)
    gamma = float(np.float32(0.97))

    def run(mask_ptr):
        out = {}
        Vn = torch.full_like(V, float("nan"))
        d = torch.zeros(1, dtype=torch.float32, device=cuda_device)
        eng.eval_sweep(V.data_ptr(), Vn.data_ptr(), pol.data_ptr(), mask_ptr, 3, n - 2, gamma, d.data_ptr())
        out["eval+res"] = (Vn.clone(), d.clone())
        Vn2 = torch.full_like(V, float("nan"))
        eng.eval_sweep(V.data_ptr(), Vn2.data_ptr(), pol.data_ptr(), mask_ptr, 0, n, gamma, 0)
        out["eval"] = (Vn2,)
        for sweeps in (3, 26):                                  # eager / resident and graph paths
            a, b = V.clone(), torch.zeros_like(V)
            eng.eval_sweeps(a.data_ptr(), b.data_ptr(), pol.data_ptr(), mask_ptr, 0, n, gamma, sweeps, d.data_ptr())
            out[f"batch{sweeps}"] = (a, b, d.clone())
        p2 = pol.clone()
        c = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        eng.improve_sweep(V.data_ptr(), p2.data_ptr(), mask_ptr, 0, n, gamma, c.data_ptr())
        out["improve"] = (p2, c.clone())
        p3, Vv = pol.clone(), torch.zeros_like(V)
        eng.value_sweep(V.data_ptr(), Vv.data_ptr(), p3.data_ptr(), mask_ptr, 0, n, gamma, d.data_ptr(), c.data_ptr())
        out["value"] = (Vv, p3, d.clone(), c.clone())
        p4, Vw = pol.clone(), torch.zeros_like(V)
        eng.value_sweep(V.data_ptr(), Vw.data_ptr(), p4.data_ptr(), mask_ptr, 0, n, gamma, 0, 0)
        out["value-noresidual"] = (Vw, p4)
        bm = torch.zeros((shape[0] + 31) // 32, dtype=torch.int32, device=cuda_device)
        eng.reach_planes(mask_ptr, 0, n // 2, bm.data_ptr(), dim=0)
        out["reach"] = (bm,)
        torch.cuda.synchronize()
        return out

    with_mask, without = run(zero.data_ptr()), run(0)
    for key in with_mask:
        for x, y in zip(with_mask[key], without[key]):
            xa, ya = x.cpu().numpy(), y.cpu().numpy()
            same = (xa.view(np.uint32 if xa.dtype.itemsize == 4 else np.uint8) == ya.view(np.uint32 if ya.dtype.itemsize == 4 else np.uint8))
            assert same.all(), (key, int((~same).sum()))
    eng.close()
    s = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cls.CONFIG), device=cuda_device)
    has_terminals = bool(s.d_terminal_mask.any().item())
    assert (s._mask_arg() is None) == (not has_terminals)
    s._backend.close()


@pytest.mark.parametrize("name,shape", [("pendulum", (64, 48)), ("pendulum", (200, 200)), ("cartpole", (9, 8, 11, 7)),
                                         ("double_pendulum_swingup", (12, 9, 11, 17)), ("double_cartpole", (4, 3, 5, 3, 4, 6))])
def test_checked_build_reports_bad_indices_and_changes_nothing_else(name, shape, cuda_device, monkeypatch, tmp_path):
    """PI_MI355_DEBUG=1 (the sanitizer row of SURVEY section 5: checked kernels instead of an address sanitizer):
    clean sweeps of every kind report no violation and give the unchecked kernels' bits; a policy array with
    entries that are no action indices is REPORTED (count, first state, its value) and contained (the sweep
    carries on with action 0 there instead of reading wild)."""
    torch = _torch()
    cls = envs.ENVS[name]
    bins = H.env_bins(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    D = len(shape)
    n = int(np.prod(shape))
    rng = np.random.default_rng(21)
    V = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(cuda_device)
    pol = torch.from_numpy(rng.integers(0, len(acts), n).astype(np.int32)).to(cuda_device)
    gamma = float(np.float32(0.97))

    def engine():
        e = _native.Engine(D, list(shape), [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                           device=cuda_device.index or 0)
        e.compile(envs.dynamics_source(name), cache_dir=tmp_path)
        return e

    def sweeps(e, policy):
        a, b = V.clone(), torch.full_like(V, float("nan"))
        d = torch.zeros(1, dtype=torch.float32, device=cuda_device)
        c = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        e.eval_sweeps(a.data_ptr(), b.data_ptr(), policy.data_ptr(), 0, 0, n, gamma, 4, d.data_ptr())   # resident / graph / eager
        single = torch.full_like(V, float("nan"))
        e.eval_sweep(V.data_ptr(), single.data_ptr(), policy.data_ptr(), 0, 0, n, gamma, 0)
        p2 = policy.clone()
        e.improve_sweep(V.data_ptr(), p2.data_ptr(), 0, 0, n, gamma, c.data_ptr())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (a, b, d, single, p2, c)]

    plain = engine()
    assert plain.info(Info.DEBUG_CHECKS) == 0
    with pytest.raises(_native.NativeError, match="PI_MI355_DEBUG"):
        plain.debug_report()
    want = sweeps(plain, pol)
    plain.close()
    monkeypatch.setenv("PI_MI355_DEBUG", "1")
    chk = engine()
    assert chk.info(Info.DEBUG_CHECKS) == 1 and "#define PI_DEBUG_BOUNDS 1" in chk.kernel_source(envs.dynamics_source(name))
    got = sweeps(chk, pol)
    assert chk.debug_report() == {"violations": 0, "kind": 0, "where": 0, "value": 0}
    for x, y in zip(want, got):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    # corrupt three policy entries: an index one past the end, a negative one, a huge one
    bad = pol.clone()
    where = [5, n // 2, n - 3]
    for s_, v_ in zip(where, (len(acts), -1, 1 << 30)):
        bad[s_] = v_
    single = torch.full_like(V, float("nan"))
    chk.eval_sweep(V.data_ptr(), single.data_ptr(), bad.data_ptr(), 0, 0, n, gamma, 0)
    rep = chk.debug_report()
    assert rep["violations"] == 3 and rep["kind"] == 1 and rep["where"] in where
    fixed = pol.clone()
    for s_ in where:
        fixed[s_] = 0                                           # what the checked kernel substitutes
    ref = torch.full_like(V, float("nan"))
    chk.eval_sweep(V.data_ptr(), ref.data_ptr(), fixed.data_ptr(), 0, 0, n, gamma, 0)
    torch.cuda.synchronize()
    assert np.array_equal(single.cpu().numpy().view(np.uint32), ref.cpu().numpy().view(np.uint32))
    assert chk.debug_report()["violations"] == 0                # cleared by the report before
    chk.close()
    if name == "cartpole":                                      # and through the solver API, on a real env run
        solver = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**{**cls.CONFIG, "max_pi_iter": 2,
                                                                                       "max_eval_iter": 60}), device=cuda_device)
        solver.policy_evaluation()
        solver.policy_improvement()
        assert solver.debug_report()["violations"] == 0
        solver._backend.close()


@pytest.mark.parametrize("mode", ["halo", "allgather"])
@pytest.mark.parametrize("world,name,shape", [(2, "cartpole", (9, 8, 11, 7)), (4, "double_pendulum_swingup", (16, 6, 8, 6))])
def test_sharded_value_iteration_and_checkpoint_on_the_native_transport(world, name, shape, mode, cuda_device,
                                                                        monkeypatch, tmp_path):
    """Rows f4 + e together through the C++ transport (in-process form, `world` logical ranks on one GPU): fused
    value-iteration sweeps with pi_exchange_V after every sweep, a collective checkpoint written by rank 0, every
    rank resuming from it — bit-identical to one rank doing 31 + 7 sweeps (tests/test_distributed_gloo.py runs
    the same scenario over gloo with the CPU checker)."""
    import threading
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    monkeypatch.setenv("PI_MI355_EXCHANGE", mode)
    cls = envs.ENVS[name]
    cfg = dict(cls.CONFIG, theta=1e-30)
    make = lambda **kw: cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg), device=cuda_device, **kw)
    single = make()
    d1 = single.value_iteration(max_iter=31)
    d2 = single.value_iteration(max_iter=7)
    single._pull_tensors_from_gpu()
    groups = [f"vi-{uuid.uuid4().hex}", f"vi-{uuid.uuid4().hex}"]
    barrier = threading.Barrier(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            stream = torch.cuda.Stream(device=cuda_device)
            with torch.cuda.stream(stream):
                s = make(transport=T.NativeTransport.local(r, world, groups[0]))
                a = s.value_iteration(max_iter=31)
                s.save_checkpoint(tmp_path / "ckpt")
                stream.synchronize()
                barrier.wait(timeout=120)
                t = make(transport=T.NativeTransport.local(r, world, groups[1]))
                t.load_checkpoint(tmp_path / "ckpt")
                b = t.value_iteration(max_iter=7)
                t._pull_tensors_from_gpu()
            out[r] = (t.value_function, t.policy, a, b)
        except Exception as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))
            barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert all(o is not None for o in out), "a rank did not finish"
    for r in range(world):
        V, pol, a, b = out[r]
        H.assert_bits_equal(V, single.value_function, f"rank {r} V")
        assert np.array_equal(pol, single.policy)
        assert (a, b) == (d1, d2)


@pytest.mark.parametrize("name,shape", [("cartpole", (11, 9, 13, 8)), ("double_cartpole", (6, 5, 7, 5, 6, 7)),
                                         ("overhead_crane", (12, 7, 9, 8))])
def test_live_state_list_changes_speed_not_results(name, shape, cuda_device, monkeypatch):
    """pi_prepare_mask: later sweeps of a whole-grid batch visit only the non-terminal states through a list.
    On small grids (the size threshold lowered, graphs and the LDS-resident kernel off so that the eager batch path
    runs) batches with the list equal batches without it bit for bit in BOTH buffers, with and without a residual;
    sub-ranges use the part of the list that lies in them; another mask pointer and a single sweep ignore the
    list; preparing NULL drops it."""
    torch = _torch()
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")
    monkeypatch.setenv("PI_MI355_GRAPHS", "0")
    monkeypatch.setenv("PI_MI355_RESIDENT", "0")
    cls = envs.ENVS[name]
    bins, (lo, hi, gshape, strides), states, term, tval = _oracle_grid(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    D, n = len(shape), int(np.prod(shape))
    assert 0.05 < term.mean() < 0.95
    eng = _native.Engine(D, list(shape), [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                         device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    rng = np.random.default_rng(17)
    V0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(cuda_device)
    pol = torch.from_numpy(rng.integers(0, len(acts), n).astype(np.int32)).to(cuda_device)
    d_term = torch.from_numpy(term.astype(np.uint8)).to(cuda_device)
    other = d_term.clone()                                     # same bytes behind another pointer
    gamma = float(np.float32(0.97))

    def batch(mask, sweeps, residual, s_begin=0, s_end=n):
        a, b = V0.clone(), torch.full_like(V0, float("nan"))
        d = torch.full((1,), -1.0, dtype=torch.float32, device=cuda_device)
        eng.eval_sweeps(a.data_ptr(), b.data_ptr(), pol.data_ptr(), mask.data_ptr(), s_begin, s_end, gamma, sweeps,
                        d.data_ptr() if residual else 0)
        torch.cuda.synchronize()
        return a.cpu().numpy(), b.cpu().numpy(), d.item()

    def improve(mask, s_begin=0, s_end=n):
        p2 = pol.clone()
        c = torch.full((1,), 77, dtype=torch.int32, device=cuda_device)
        eng.improve_sweep(V0.data_ptr(), p2.data_ptr(), mask.data_ptr(), s_begin, s_end, gamma, c.data_ptr())
        torch.cuda.synchronize()
        return p2.cpu().numpy(), int(c.item())

    plain = {(k, r): batch(d_term, k, r) for k in (1, 2, 5, 6) for r in (False, True)}
    part = batch(d_term, 5, True, 7, n - 9)
    plain_improve, part_improve = improve(d_term), improve(d_term, 7, n - 9)
    listed = eng.prepare_mask(d_term.data_ptr())
    pad = np.concatenate([term, np.ones(-n % 64, bool)]).reshape(-1, 64)
    idle = ((~pad).any(axis=1).sum() * 64 - (~term).sum()) / n          # lane slots idle in partly live waves
    if idle < 0.03:                                            # the crane: terminal states come in whole planes
        assert listed == 0 and eng.info(Info.LIVE_STATES) == 0
        eng.close()
        return
    assert listed == int((~term).sum()) and eng.info(Info.LIVE_STATES) == listed
    for (k, r), want in plain.items():
        got = batch(d_term, k, r)
        for x, y in zip(want[:2], got[:2]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (k, r)
        assert want[2] == got[2]
    for got, want in ((improve(d_term), plain_improve), (improve(other), plain_improve),
                      (improve(d_term, 7, n - 9), part_improve)):
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    o_pol, o_changed = H.oracle_for(name).improve_sweep(states, acts, pol.cpu().numpy(), V0.cpu().numpy(), term, lo, hi,
                                                        gshape, strides, gamma)
    assert np.array_equal(plain_improve[0], o_pol) and plain_improve[1] == o_changed
    got = batch(other, 5, True)                                # another pointer: list ignored, same result anyway
    assert np.array_equal(got[1].view(np.uint32), plain[(5, True)][1].view(np.uint32))
    got = batch(d_term, 5, True, 7, n - 9)                     # sub-range: the entries of the list inside it
    assert np.array_equal(got[1].view(np.uint32), part[1].view(np.uint32)) and got[2] == part[2]
    # and against the oracle: 5 sweeps with the list
    chk = H.oracle_for(name)
    cur = V0.cpu().numpy()
    for _ in range(5):
        cur, o_delta = chk.eval_sweep(states, acts, pol.cpu().numpy(), cur, term, lo, hi, gshape, strides, gamma)
    got = batch(d_term, 5, True)
    H.assert_bits_equal(got[1], cur, "5 sweeps through the live list vs oracle")
    assert np.float32(got[2]) == np.float32(o_delta)
    assert eng.prepare_mask(0) == 0 and eng.info(Info.LIVE_STATES) == 0
    eng.close()


@pytest.mark.parametrize("mode", ["halo", "allgather"])
@pytest.mark.parametrize("world,name,shape", [(2, "cartpole", (10, 8, 11, 7)), (4, "double_cartpole", (8, 4, 5, 4, 5, 4))])
def test_live_state_list_in_the_sharded_driver(world, name, shape, mode, cuda_device, monkeypatch):
    """Every rank of a sharded run sweeps the part of the live-state list that lies in its launch ranges (swept-first
    and interior ranges alike): `world` logical ranks through the in-process transport, the size threshold lowered
    so that these small grids get a list — run() bit-identical to the single-rank run without a list."""
    import threading
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    cls = envs.ENVS[name]
    cfg_kw = {**cls.CONFIG, "max_pi_iter": 3, "max_eval_iter": 60}
    monkeypatch.setenv("PI_MI355_LIVE", "0")
    single = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg_kw), device=cuda_device)
    assert single._backend.engine.info(Info.LIVE_STATES) == 0
    single.run()
    monkeypatch.setenv("PI_MI355_LIVE", "1")
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")
    monkeypatch.setenv("PI_MI355_GRAPHS", "0")
    monkeypatch.setenv("PI_MI355_RESIDENT", "0")
    monkeypatch.setenv("PI_MI355_EXCHANGE", mode)
    group = f"live-{uuid.uuid4().hex}"
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            stream = torch.cuda.Stream(device=cuda_device)
            with torch.cuda.stream(stream):
                s = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg_kw), device=cuda_device,
                        transport=T.NativeTransport.local(r, world, group))
                listed = s._backend.engine.info(Info.LIVE_STATES)
                s.run()
            out[r] = (s.value_function, s.policy, list(s.stats["sweeps_per_iter"]), listed)
        except Exception as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for r in range(world):
        V, pol, sweeps, listed = out[r]
        assert listed > 0
        H.assert_bits_equal(V, single.value_function, f"rank {r} V")
        assert np.array_equal(pol, single.policy) and sweeps == single.stats["sweeps_per_iter"]


@pytest.mark.parametrize("name,shape", [("cartpole", (11, 9, 13, 8)), ("double_cartpole", (6, 5, 7, 5, 6, 7))])
def test_per_evaluation_list_changes_speed_not_results(name, shape, cuda_device, monkeypatch):
    """pi_eval_begin / pi_eval_end: under a fixed policy the live states whose successor is terminal drop out of the
    sweeps once both buffers hold their (constant) value.  Engine level: the same sequences of batches — the solver's
    1 + 25 + 25 pattern, a caller that never swaps its buffers, single-sweep batches — give the same bits in both
    buffers and the same residuals with and without the bracket; an improvement sweep ends the bracket.  Solver level:
    a full run() equals the run without the bracket (V, policy, sweeps of every evaluation)."""
    torch = _torch()
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")
    monkeypatch.setenv("PI_MI355_GRAPHS", "0")
    monkeypatch.setenv("PI_MI355_RESIDENT", "0")
    cls = envs.ENVS[name]
    bins, (lo, hi, gshape, strides), states, term, tval = _oracle_grid(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    D, n = len(shape), int(np.prod(shape))
    eng = _native.Engine(D, list(shape), [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                         device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    rng = np.random.default_rng(23)
    V0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(cuda_device)
    pol = torch.from_numpy(rng.integers(0, len(acts), n).astype(np.int32)).to(cuda_device)
    d_term = torch.from_numpy(term.astype(np.uint8)).to(cuda_device)
    gamma = float(np.float32(0.97))
    assert eng.prepare_mask(d_term.data_ptr()) > 0

    def sequence(pattern, bracket):
        a, b = V0.clone(), torch.full_like(V0, float("nan"))
        d = torch.zeros(1, dtype=torch.float32, device=cuda_device)
        deltas, listed = [], 0
        if bracket:
            listed = eng.eval_begin(pol.data_ptr(), d_term.data_ptr())
        for k, swap in pattern:
            eng.eval_sweeps(a.data_ptr(), b.data_ptr(), pol.data_ptr(), d_term.data_ptr(), 0, n, gamma, k, d.data_ptr())
            torch.cuda.synchronize()
            deltas.append(d.item())
            if swap and k % 2:
                a, b = b, a
        if bracket:
            eng.eval_end()
        return a.cpu().numpy(), b.cpu().numpy(), deltas, listed

    live = int((~term).sum())
    for pattern in ([(1, True), (25, True), (25, True)],            # the solver's loop
                    [(3, False), (4, False), (5, False)],           # a caller that never swaps
                    [(1, True)] * 6,                                # single-sweep batches
                    [(2, True), (7, True)]):
        want = sequence(pattern, False)
        got = sequence(pattern, True)
        assert 0 < got[3] < live, got[3]
        for x, y in zip(want[:2], got[:2]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), pattern
        assert want[2] == got[2], pattern
    # an improvement sweep ends the bracket by itself (the policy may have changed)
    assert eng.eval_begin(pol.data_ptr(), d_term.data_ptr()) > 0 and eng.info(Info.EVAL_LIST_ENTRIES) > 0
    eng.improve_sweep(V0.data_ptr(), pol.clone().data_ptr(), d_term.data_ptr(), 0, n, gamma, 0)
    assert eng.info(Info.EVAL_LIST_ENTRIES) == 0
    eng.close()
    # solver level
    runs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("PI_MI355_EVAL_LIST", flag)
        s = cls(H.env_bins_space(name, shape), cls.ACTIONS,
                envs.CudaPIConfig(**{**cls.CONFIG, "max_pi_iter": 4, "max_eval_iter": 120}), device=cuda_device)
        s.run()
        runs[flag] = (s.value_function, s.policy, list(s.stats["sweeps_per_iter"]))
    H.assert_bits_equal(runs["1"][0], runs["0"][0], "run() with the per-evaluation list")
    assert np.array_equal(runs["1"][1], runs["0"][1]) and runs["1"][2] == runs["0"][2]


def test_live_state_list_at_full_c5_size(cuda_device):
    """The config the list exists for: double cartpole 25^6 (35 % terminal states, 16 % of the waves partly idle).
    The solver prepares it by itself; three-sweep batches with and without it agree on all 244 M values, and the
    later sweeps get faster (recorded in profiles/r03, asserted loosely)."""
    torch = _torch()
    solver = envs.make("double_cartpole", 25)
    eng = solver._backend.engine
    n = solver.n_states
    assert eng.info(Info.LIVE_STATES) == int((solver.d_terminal_mask[:n] == 0).sum().item()) > 0
    gen = torch.Generator(device="cpu").manual_seed(3)
    solver.d_value_function[:n].copy_(torch.randn(n, generator=gen, dtype=torch.float32))
    solver.d_policy[:n].copy_(torch.randint(0, solver.n_actions, (n,), generator=gen, dtype=torch.int32))
    V0 = solver.d_value_function.clone()
    term, pol = solver._mask_arg(), solver.d_policy
    gamma = float(np.float32(solver.config.gamma))
    d = torch.zeros(1, dtype=torch.float32, device=cuda_device)

    def batch(sweeps):
        a, b = V0.clone(), torch.empty_like(V0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.eval_sweeps(a.data_ptr(), b.data_ptr(), pol.data_ptr(), term.data_ptr(), 0, n, gamma, sweeps, d.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        return a, b, d.item(), e0.elapsed_time(e1)

    def improve():
        p2 = pol.clone()
        c = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.improve_sweep(V0.data_ptr(), p2.data_ptr(), term.data_ptr(), 0, n, gamma, c.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        return p2, int(c.item()), e0.elapsed_time(e1)

    with_list = batch(3)
    t_list = min(batch(11)[3] for _ in range(2))
    imp_list = improve()
    ti_list = min(improve()[2] for _ in range(2))
    eng.prepare_mask(0)
    without = batch(3)
    t_plain = min(batch(11)[3] for _ in range(2))
    imp_plain = improve()
    ti_plain = min(improve()[2] for _ in range(2))
    assert torch.equal(imp_list[0], imp_plain[0]) and imp_list[1] == imp_plain[1]
    print(f"25^6 improvement sweep: {ti_plain:.2f} ms in state order, {ti_list:.2f} ms through the live list")
    assert ti_list < ti_plain * 1.02
    assert torch.equal(with_list[0].view(torch.int32), without[0].view(torch.int32))
    assert torch.equal(with_list[1].view(torch.int32), without[1].view(torch.int32))
    assert with_list[2] == without[2]
    print(f"25^6 11-sweep batch: {t_plain:.2f} ms in state order, {t_list:.2f} ms through the live list")
    assert t_list < t_plain * 1.02
    solver._backend.close()


def _closed_loop(name, bins, start, steps, cuda_device, m=4096):
    """Train `name` on its reference grid with run(), then drive m states in closed loop entirely on the GPU: the
    interpolated action from the batched inference kernel (DevicePolicy on device tensors), the env step from the
    plugin's own step_dynamics (pi_probe_step).  Returns (final states, ever-terminated flags, rewards of the
    last 50 steps)."""
    torch = _torch()
    from utils.barycentric import DevicePolicy
    cls = envs.ENVS[name]
    solver = envs.make(name, bins)
    solver.run()                                               # releases its device arrays and its handle
    assert solver.stats["stable"] or name == "pendulum"        # pendulum 200^2 stops at max_pi_iter, as the reference does
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    eng = _native.Engine(D, [len(t) for t in tabs], [t.min() for t in tabs], [t.max() for t in tabs], tabs,
                         solver.action_space, device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))                    # the env step of the rollout: the plugin itself
    dp = DevicePolicy(solver.policy, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape,
                      solver.strides, solver.corner_bits, device=cuda_device)
    gen = torch.Generator(device="cpu").manual_seed(5)
    states = start(torch.rand((m, D), generator=gen), solver).to(torch.float32).to(cuda_device)
    nxt = torch.empty_like(states)
    rew = torch.empty(m, dtype=torch.float32, device=cuda_device)
    done = torch.empty(m, dtype=torch.uint8, device=cuda_device)
    ended = torch.zeros(m, dtype=torch.bool, device=cuda_device)
    tail = torch.zeros(m, dtype=torch.float32, device=cuda_device)
    st = torch.cuda.current_stream(cuda_device).cuda_stream
    for t in range(steps):
        act = dp(states)
        assert act.device == states.device
        eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
        ended |= done != 0
        states, nxt = nxt, states
        if t >= steps - 50:
            tail += rew
    torch.cuda.synchronize()
    dp.close()
    eng.close()
    return states, ended, tail / 50


def test_trained_policies_solve_their_tasks_in_closed_loop(cuda_device):
    """What the reference uses in place of tests (rollouts of the learned policy on the real env,
    e.g. pendulum_cuda.py:151-177, cartpole_cuda.py:163-191): an end-to-end check that the solver produces policies
    that SOLVE the tasks, not only bits that match the oracle's.
      Pendulum 200^2        4 096 states anywhere on the grid -> upright and still after 400 steps
      CartPole 30^4         gymnasium's start (all coordinates within +-0.05) -> no termination in 500 steps (CartPole-v1's bar)
      CartPole swing-up 50^4  pole hanging DOWN -> swung up, balanced, cart on the track after 1 000 steps"""
    torch = _torch()

    def anywhere(u, solver):
        lo, hi = torch.tensor(solver.bounds_low), torch.tensor(solver.bounds_high)
        return lo + (hi - lo) * u
    states, _, cost = _closed_loop("pendulum", 200, anywhere, 400, cuda_device)
    upright = ((states[:, 0].abs() < 0.1) & (states[:, 1].abs() < 0.5)).float().mean().item()
    assert upright >= 0.97, f"only {upright:.3f} of the pendulums end upright"
    assert cost.mean().item() > -0.05                          # gymnasium's cost: ~0 when balanced

    states, ended, _ = _closed_loop("cartpole", 30, lambda u, s: (u * 2 - 1) * 0.05, 500, cuda_device)
    assert not ended.any().item(), f"{int(ended.sum())} of {len(ended)} cart-poles fell within 500 steps"

    def hanging(u, solver):
        x = (u * 2 - 1) * 0.05
        x[:, 2] += float(np.pi)
        return x
    states, ended, _ = _closed_loop("cartpole_swingup", 50, hanging, 1000, cuda_device)
    theta = torch.atan2(torch.sin(states[:, 2]), torch.cos(states[:, 2])).abs()
    up = ((theta < 0.05) & (states[:, 3].abs() < 0.1) & ~ended).float().mean().item()
    assert up >= 0.99, f"only {up:.3f} of the poles were swung up and held"


def test_handles_give_their_device_memory_back(cuda_device):
    """pi_destroy / pi_infer_destroy / pi_comm_destroy release everything the library allocated itself (bin tables,
    accumulator slots, graphs, code objects, policy tables, in-process transport state): 60 create-use-destroy cycles
    leave the device's free memory where it was."""
    import uuid
    from itertools import product
    torch = _torch()
    name, shape = "cartpole_swingup", (14, 9, 12, 8)
    cls = envs.ENVS[name]
    bins = H.env_bins(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    n = int(np.prod(shape))
    V = torch.zeros(n, dtype=torch.float32, device=cuda_device)
    Vn = torch.zeros_like(V)
    pol = torch.zeros(n, dtype=torch.int32, device=cuda_device)
    d = torch.zeros(1, dtype=torch.float32, device=cuda_device)
    bits = np.array(list(product([0, 1], repeat=4)), dtype=np.int32)
    strides = [int(np.prod(shape[k + 1:])) for k in range(4)]
    policy_host = np.zeros(n, np.int32)

    def cycle():
        eng = _native.Engine(4, list(shape), [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                             device=cuda_device.index or 0)
        eng.compile(envs.dynamics_source(name))
        eng.comm_init_local(0, 1, f"leak-{uuid.uuid4().hex}")
        eng.eval_sweeps(V.data_ptr(), Vn.data_ptr(), pol.data_ptr(), 0, 0, n, 0.99, 26, d.data_ptr())    # a cached graph
        eng.improve_sweep(V.data_ptr(), pol.data_ptr(), 0, 0, n, 0.99, 0)
        torch.cuda.synchronize()
        eng.close()
        inf = _native.InferenceEngine([b.min() for b in bins], [b.max() for b in bins], list(shape), strides, bits,
                                      device=cuda_device.index or 0)
        inf.set_policy(policy_host, acts)
        inf.close()

    for _ in range(3):
        cycle()                                                  # warm the allocator pools and the caches
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(cuda_device)
    for _ in range(60):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(cuda_device)
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) / 2**20:.1f} MiB not returned after 60 handle cycles"


def test_headline_sweep_times_stay_in_range(cuda_device):
    """A coarse guard against performance cliffs on the metric config (double pendulum 80^4 x 11): the
    evaluation sweep measured 0.40-0.43 ms and the improvement sweep 2.3-2.4 ms on MI355X (DESIGN.md section
    5); one VGPR too many on the evaluation kernel alone costs ~20 % (one 1 024-thread workgroup per CU
    instead of two).  Thresholds are a third above the measurements: a noisy box passes, a cliff does not."""
    torch = _torch()
    s = envs.make("double_pendulum_swingup", 80, device=cuda_device)
    n, gamma = s.n_states, float(np.float32(s.config.gamma))
    gen = torch.Generator(device="cpu").manual_seed(0)
    s.d_value_function[:n].copy_(torch.randn(n, generator=gen, dtype=torch.float32))
    s.d_new_value_function.copy_(s.d_value_function)
    s.d_policy[:n].copy_(torch.randint(0, s.n_actions, (n,), generator=gen, dtype=torch.int32))
    s._evaluation_sweeps(10, gamma)
    s._improvement_sweep(gamma)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    s._evaluation_sweeps(40, gamma)
    e[1].record()
    for _ in range(3):
        s._improvement_sweep(gamma)
    e[2].record()
    e[2].synchronize()
    eval_ms, improve_ms = e[0].elapsed_time(e[1]) / 40, e[1].elapsed_time(e[2]) / 3
    s._backend.close()
    assert eval_ms < 0.56, eval_ms
    assert improve_ms < 3.2, improve_ms


@pytest.mark.parametrize("world,name,shape", [(2, "double_pendulum_swingup", (14, 9, 11, 8)), (3, "cartpole_swingup", (18, 7, 9, 8))])
def test_bench_self_check_of_sharded_sweeps(world, name, shape, cuda_device, monkeypatch):
    """bench.py's N-rank self-check (`sharded_equals_unsharded`: 2 evaluation + 1 improvement sweeps through the sharded
    driver against the same sweeps over the whole grid, torch.equal) — run here with logical ranks over the in-process
    transport, since a development box has one GPU: it must pass on the real driver and FAIL when the exchange delivers
    nothing (a halo that is never sent is exactly what a first RCCL run could get wrong)."""
    import importlib.util
    import threading
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    spec = importlib.util.spec_from_file_location("bench_under_test", H.GOLDEN.parents[1] / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setenv("PI_MI355_EXCHANGE", "halo")
    cls = envs.ENVS[name]
    gamma = float(np.float32(cls.CONFIG["gamma"]))
    n = int(np.prod(shape))
    gen = torch.Generator(device="cpu").manual_seed(5)
    V0 = torch.randn(n, generator=gen, dtype=torch.float32)
    P0 = torch.randint(0, len(cls.ACTIONS), (n,), generator=gen, dtype=torch.int32)

    class Dist:                                        # every logical rank reaches its own verdict; MIN over one value
        class ReduceOp:
            MIN = "min"

        @staticmethod
        def all_reduce(t, op=None):
            return None

    def run(broken):
        group = f"bench-check-{uuid.uuid4().hex}"
        out, errors = [None] * world, []

        def rank_main(r):
            try:
                stream = torch.cuda.Stream(device=cuda_device)
                with torch.cuda.stream(stream):
                    s = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cls.CONFIG), device=cuda_device,
                            transport=T.NativeTransport.local(r, world, group))
                    s.d_value_function[:n].copy_(V0)
                    s.d_new_value_function.copy_(s.d_value_function)
                    s.d_policy[:n].copy_(P0)
                    if broken:                         # the exchange "succeeds" but moves nothing
                        real = s._comm.engine.eval_sweeps_sharded

                        def no_exchange(Va, Vb, policy, term, g, k, d_delta=0, st=0):
                            for i in range(k):
                                src, dst = (Vb, Va) if (i & 1) else (Va, Vb)
                                s._backend.engine.eval_sweep(src, dst, policy, term, s._s_begin, s._s_end, g,
                                                             d_delta if i == k - 1 else 0, st)
                        s._comm.engine.eval_sweeps_sharded = no_exchange
                    out[r] = bench.sharded_equals_unsharded(s, s._backend.engine, gamma, torch, Dist)
                    # the solver's state is what it was before the check
                    assert torch.equal(s.d_value_function[:n].cpu(), V0) and torch.equal(s.d_policy[:n].cpu(), P0)
                    torch.cuda.synchronize()
                    s._backend.close()
            except Exception as exc:  # noqa: BLE001
                errors.append((r, repr(exc)))

        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not errors, errors
        return out

    good = run(False)
    assert all(o["ok"] and o["V"] and o["policy"] and o["residual"] and o["changed"] for o in good), good
    bad = run(True)
    assert not any(o["ok"] for o in bad) and not all(o["V"] for o in bad), bad


def test_plain_bench_run_dumps_what_its_last_timed_step_computed(cuda_device, tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` without --full: the line holds the headline and nothing that
    takes runs of its own; the dump is identical from run to run and equal, bit for bit, to V and the policy after the same
    seeded steps through the solver here (the env's own order, at the dump's sampled indices)."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys
    torch = _torch()
    root = H.GOLDEN.parents[1]
    spec = importlib.util.spec_from_file_location("bench_under_test", root / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    lines, dumps = [], []
    for k in range(2):
        out = tmp_path / f"run{k}"
        res = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                              "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env)
        assert res.returncode == 0, res.stderr[-3000:]
        lines.append(json.loads(bench.result_line(res.stdout)))
        dumps.append({p.stem: np.load(p) for p in out.glob("*.npy")})
    line, dump = lines[0], dumps[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["ms_per_step"] > 0
    assert not {"roofline", "kernels", "sweeps_to_converge", "full_runs", "extra_configs", "cpu_baseline"} & set(line)
    assert sorted(dump) == ["changed", "policy", "residual", "state_index", "value_function"]
    assert all(dump[k].dtype in (np.float32, np.float64) and np.array_equal(dump[k], dumps[1][k]) for k in dump)
    assert sum(a.nbytes for a in dump.values()) <= 64 << 20
    assert dump["residual"].tolist() == [line["check"]["last_residual"]]
    assert dump["changed"].tolist() == [line["check"]["last_changed"]]

    cls = envs.ENVS[bench.ENV]
    solver = envs.make(bench.ENV, bench.BINS, config=envs.CudaPIConfig(**cls.CONFIG), device=cuda_device)
    n, nA = solver.n_states, solver.n_actions
    gen = torch.Generator(device="cpu").manual_seed(0)
    solver.d_value_function[:n].copy_(torch.randn(n, generator=gen, dtype=torch.float32))
    solver.d_new_value_function.copy_(solver.d_value_function)
    solver.d_policy[:n].copy_(torch.randint(0, nA, (n,), generator=gen, dtype=torch.int32))
    gamma = float(np.float32(solver.config.gamma))
    for _ in range(3):                                   # the warm-up step and the two timed ones
        solver._evaluation_sweeps(bench.EVAL_PER_STEP, gamma)
        solver._improvement_sweep(gamma)
    idx = dump["state_index"].astype(np.int64)
    V = solver._to_user(solver.d_value_function[:n].cpu().numpy())
    P = solver._to_user(solver.d_policy[:n].cpu().numpy())
    solver._backend.close()
    assert len(idx) == bench.DUMP_SAMPLES < n
    assert np.array_equal(V[idx].view(np.uint32), dump["value_function"].view(np.uint32))
    assert np.array_equal(P[idx], dump["policy"].astype(np.int32))


ROW_EXACT_CASES = [(8, "double_pendulum_swingup", (40, 12, 8, 6)), (4, "double_pendulum_swingup", (24, 9, 7, 5)),
                   (3, "pendulum", (60, 33))]


@pytest.mark.parametrize("world,name,shape", ROW_EXACT_CASES)
def test_row_exact_swept_first_lists(world, name, shape, cuda_device, monkeypatch):
    """Row-exact exchange plans (grids without terminal states, PI_MI355_ROW_EXACT): what is swept first is exactly the
    rows that travel — as a state list swept by the list kernel in one launch — and the interior is the rest of the
    shard.  Checked with logical ranks over the in-process transport: the two parts tile the shard, every state a peer
    receives lies in part 0, part 0 + part 1 through pi_eval_sweep_part equal one plain sweep of the shard bit for bit,
    and whole run()s equal the single-rank run.  The coarse plan of the same grid sweeps MORE states first."""
    import threading
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    monkeypatch.setenv("PI_MI355_EXCHANGE", "halo")
    cls = envs.ENVS[name]
    cfg_kw = {**cls.CONFIG, "max_pi_iter": 2, "max_eval_iter": 40}
    single = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg_kw), device=cuda_device)
    single.run()
    n = single.n_states
    gen = torch.Generator(device="cpu").manual_seed(11)
    V0 = torch.randn(n, generator=gen, dtype=torch.float32)
    P0 = torch.randint(0, len(cls.ACTIONS), (n,), generator=gen, dtype=torch.int32)
    gamma = float(np.float32(cls.CONFIG["gamma"]))

    def run(row_exact):
        monkeypatch.setenv("PI_MI355_ROW_EXACT", "1" if row_exact else "0")
        group = f"rowexact-{uuid.uuid4().hex}"
        out, errors = [None] * world, []

        def rank_main(r):
            try:
                with torch.cuda.stream(torch.cuda.Stream(device=cuda_device)):
                    s = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg_kw), device=cuda_device,
                            transport=T.NativeTransport.local(r, world, group))
                    eng, info, ranges = s._backend.engine, dict(s._comm.info), s._backend.engine.plan_ranges()
                    plan = H.plan_record(eng, info)
                    a, b = s._s_begin, s._s_end
                    # parts of one sweep against the plain range sweep of the shard
                    dV, dP = V0.to(cuda_device), P0.to(cuda_device)
                    whole, parts = torch.zeros_like(dV), torch.zeros_like(dV)
                    st = torch.cuda.current_stream().cuda_stream
                    eng.eval_sweep(dV.data_ptr(), whole.data_ptr(), dP.data_ptr(), 0, a, b, gamma, 0, st)
                    eng.eval_sweep_part(dV.data_ptr(), parts.data_ptr(), dP.data_ptr(), 0, 0, gamma, st)
                    torch.cuda.synchronize()
                    first_only = parts.clone()
                    eng.eval_sweep_part(dV.data_ptr(), parts.data_ptr(), dP.data_ptr(), 0, 1, gamma, st)
                    torch.cuda.synchronize()
                    same = bool(torch.equal(whole, parts))
                    touched_first = int((first_only != 0).sum().item())
                    s.run()
                    out[r] = dict(info=info, ranges=ranges, plan=plan, shard=(a, b), same=same, touched_first=touched_first,
                                  V=s.value_function, P=s.policy, sweeps=list(s.stats["sweeps_per_iter"]))
            except Exception as exc:  # noqa: BLE001
                errors.append((r, repr(exc)))

        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not errors, errors
        return out

    exact, coarse = run(True), run(False)
    for got, row_exact in ((exact, "1"), (coarse, "0")):       # the plans are the recorded ones (tests/golden/shard_plans.json)
        key = H.plan_key("local", world, name, shape, {"PI_MI355_EXCHANGE": "halo", "PI_MI355_ROW_EXACT": row_exact})
        assert [o["plan"] for o in got] == H.golden_plans(key), key
    for r, (e, c) in enumerate(zip(exact, coarse)):
        assert e["info"]["mode"] == "halo" and e["info"]["row_exact"] and not c["info"]["row_exact"]
        a, b = e["shard"]
        spans = sorted((lo, hi) for _, lo, hi in e["ranges"])
        assert spans[0][0] == a and spans[-1][1] == b and all(x[1] == y[0] for x, y in zip(spans, spans[1:]))
        first = sum(hi - lo for k, lo, hi in e["ranges"] if k == 0)
        assert first == e["info"]["send_elems"] or first <= e["info"]["send_elems"]     # rows sent to several peers count once here
        assert 0 < first < b - a
        assert abs(e["touched_first"] - first) <= first * 1e-3 + 2                      # part 0 wrote those states (V' == 0 is rare)
        assert first <= sum(hi - lo for k, lo, hi in c["ranges"] if k == 0)             # never more than the coarse plan
        assert e["same"] and c["same"]
        H.assert_bits_equal(e["V"], single.value_function, f"rank {r} V (row-exact)")
        assert np.array_equal(e["P"], single.policy) and e["sweeps"] == single.stats["sweeps_per_iter"]
    total_exact = sum(sum(hi - lo for k, lo, hi in e["ranges"] if k == 0) for e in exact)
    total_coarse = sum(sum(hi - lo for k, lo, hi in c["ranges"] if k == 0) for c in coarse)
    assert total_exact <= total_coarse
    if cls._D >= 4:                                     # rows (i0, i1): the coarse plan merges across rows nobody waits for
        assert total_exact < total_coarse


def test_recovery_after_an_abandoned_sharded_batch(cuda_device, monkeypatch):
    """The documented recovery path (include/pi_mi355.h): a sharded batch that fails half-way — here
    because the peer never takes part — is abandoned with a message, the handle then refuses sharded sweeps and says
    what to do, and after pi_comm_destroy + a new communicator + a collective pi_exchange_plan on every rank the same
    handles sweep again, bit-identical to a single-rank solver."""
    import threading
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    monkeypatch.setenv("PI_MI355_EXCHANGE", "halo")
    monkeypatch.setenv("PI_MI355_COMM_TIMEOUT", "2")
    name, shape, world = "double_pendulum_swingup", (14, 9, 11, 8), 2
    cls = envs.ENVS[name]
    cfg = envs.CudaPIConfig(**cls.CONFIG)
    gamma = float(np.float32(cfg.gamma))
    n = int(np.prod(shape))
    gen = torch.Generator(device="cpu").manual_seed(3)
    V0 = torch.randn(n, generator=gen, dtype=torch.float32)
    P0 = torch.randint(0, len(cls.ACTIONS), (n,), generator=gen, dtype=torch.int32)
    single = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device, transport=False)
    single.d_value_function[:n].copy_(V0)
    single.d_new_value_function.copy_(single.d_value_function)
    single.d_policy[:n].copy_(P0)
    single._evaluation_sweeps(3, gamma)
    torch.cuda.synchronize()
    V_ref = single.d_value_function[:n].clone()

    first, second = f"doomed-{uuid.uuid4().hex}", f"fresh-{uuid.uuid4().hex}"
    failed, rebuilt = threading.Event(), threading.Barrier(world, timeout=120)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=cuda_device)):
                s = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device,
                        transport=T.NativeTransport.local(r, world, first))
                s.d_value_function[:n].copy_(V0)
                s.d_new_value_function.copy_(s.d_value_function)
                s.d_policy[:n].copy_(P0)
                torch.cuda.synchronize()
                if r == 0:
                    with pytest.raises(_native.NativeError, match="abandoned"):
                        s._evaluation_sweeps(3, gamma)             # rank 1 never posts its rows
                    with pytest.raises(_native.NativeError, match="pi_comm_destroy"):
                        s._evaluation_sweeps(1, gamma)             # refuses, and says how to recover
                    failed.set()
                else:
                    assert failed.wait(timeout=120)
                # recovery, every rank: destroy, new communicator, new plan
                eng = s._backend.engine
                eng.comm_destroy()
                rebuilt.wait()
                eng.comm_init_local(r, world, second)
                s._comm.plan(s)
                s.d_value_function[:n].copy_(V0)
                s.d_new_value_function.copy_(s.d_value_function)
                s._evaluation_sweeps(3, gamma)
                torch.cuda.synchronize()
                out[r] = bool(torch.equal(s.d_value_function[s._s_begin:s._s_end], V_ref[s._s_begin:s._s_end]))
                s._backend.close()
        except BaseException as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))
            failed.set()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert out == [True] * world


@pytest.mark.parametrize("name,shape,rng_lo,rng_hi", [("cartpole", (11, 9, 13, 8), None, None),
                                                      ("double_cartpole", (6, 5, 7, 5, 6, 7), 1003, 70001),
                                                      ("cartpole", (11, 9, 13, 8), 64, 4097),
                                                      ("cartpole", (11, 9, 13, 8), -7, 64)])
def test_live_state_list_is_built_on_the_device(name, shape, rng_lo, rng_hi, cuda_device, monkeypatch):
    """pi_prepare_mask / pi_prepare_mask_range build the list with count -> scan -> ordered-write kernels (no host
    pass over the mask): the list equals the ascending non-terminal states of the range — whole grid, a ragged shard
    whose borders are not multiples of 64, ranges inside one block — and nothing is listed when no lane would idle."""
    torch = _torch()
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")
    cls = envs.ENVS[name]
    bins = H.env_bins(name, shape)
    eng = _native.Engine(cls._D, [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins,
                         np.asarray(cls.ACTIONS, np.float32), device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    eng.set_option(Option.KEEP_LIVE_LIST, 1)                  # keep the list whatever it saves: this test reads it
    states = oracle.states_from_bins(bins)
    term, _ = H.terminal_mask(name, states)
    n = len(states)
    d_term = torch.from_numpy(term.astype(np.uint8)).to(cuda_device)
    if rng_lo is not None and rng_lo < 0:                     # a range inside one or two 64-state blocks in mid-grid
        rng_lo, rng_hi = n // 2 - rng_lo, n // 2 - rng_lo + rng_hi
    a, b = (0, n) if rng_lo is None else (rng_lo, min(rng_hi, n))
    count = eng.prepare_mask(d_term.data_ptr(), 0, a, b) if rng_lo is not None else eng.prepare_mask(d_term.data_ptr())
    want = np.flatnonzero(~term[a:b]).astype(np.int32) + a
    assert count == len(want) > 0
    out = torch.full((count + 3,), -1, dtype=torch.int32, device=cuda_device)
    assert eng.live_list(out.data_ptr(), count + 3) == count
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:count], want) and np.all(got[count:] == -1)
    # the positions the library derives from its bitmap: a sub-range sweep over the list equals the state-order sweep
    V = torch.randn(n, dtype=torch.float32, device=cuda_device)
    V[d_term.bool()] = 0.0
    pol = torch.randint(0, len(cls.ACTIONS), (n,), dtype=torch.int32, device=cuda_device)
    lo2, hi2 = a + (b - a) // 3, b - (b - a) // 5
    with_list = [V.clone(), V.clone()]
    eng.eval_sweeps(with_list[0].data_ptr(), with_list[1].data_ptr(), pol.data_ptr(), d_term.data_ptr(), lo2, hi2, 0.99, 3, 0)
    eng.prepare_mask(0)
    assert eng.live_list() == 0
    plain = [V.clone(), V.clone()]
    eng.eval_sweeps(plain[0].data_ptr(), plain[1].data_ptr(), pol.data_ptr(), d_term.data_ptr(), lo2, hi2, 0.99, 3, 0)
    torch.cuda.synchronize()
    assert torch.equal(with_list[0].view(torch.int32), plain[0].view(torch.int32))
    assert torch.equal(with_list[1].view(torch.int32), plain[1].view(torch.int32))
    # without the "keep it anyway" option a mask that leaves no lane idle is not listed
    eng.set_option(Option.KEEP_LIVE_LIST, 0)
    none = torch.zeros(n, dtype=torch.uint8, device=cuda_device)
    none[: (n // 64) * 32] = 1                                 # whole waves terminal: no partly idle wave
    assert eng.prepare_mask(none.data_ptr()) == 0
    eng.close()


def test_live_state_list_of_the_full_c5_grid_is_the_sorted_set_of_live_states(cuda_device):
    """25^6 = 244 140 625 states, 35 % terminal, in the solver's own memory order: the device-built list is exactly the
    ascending set of non-terminal states (torch.nonzero of the mask), and building the solver no longer materialises
    the (n, 6) grid on the host (the mask comes from the bin tables: _terminal_fn_axes)."""
    import time
    torch = _torch()
    t0 = time.perf_counter()
    solver = envs.make("double_cartpole", 25, device=cuda_device)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"envs.make('double_cartpole', 25): {seconds:.1f} s (round 4: host-built mask and list)")
    assert solver._states_space is None
    eng = solver._backend.engine
    n = solver.n_states
    count = eng.live_list()
    assert count == eng.info(Info.LIVE_STATES) > 0
    out = torch.empty(count, dtype=torch.int32, device=cuda_device)
    assert eng.live_list(out.data_ptr(), count) == count
    want = torch.nonzero(solver.d_terminal_mask[:n] == 0).reshape(-1).to(torch.int32)
    assert want.numel() == count and torch.equal(out, want)
    # the mask itself against the reference's hook, evaluated on the bin tables of a few whole planes
    bins = solver._bins
    lim = envs.DoubleCartPoleCuda._TH_FAIL
    x_bad, t1_bad, t2_bad = np.abs(bins[0]) > 2.4, np.abs(bins[2]) > lim, np.abs(bins[4]) > lim
    user = solver._to_user(solver.d_terminal_mask[:n]).reshape([25] * 6)
    assert int(user.sum().item()) == n - count
    assert bool(user[torch.from_numpy(x_bad)].all()) and bool(user[:, :, torch.from_numpy(t1_bad)].all())
    assert bool(user[:, :, :, :, torch.from_numpy(t2_bad)].all())
    keep = user[torch.from_numpy(~x_bad)][:, :, torch.from_numpy(~t1_bad)][:, :, :, :, torch.from_numpy(~t2_bad)]
    assert not bool(keep.any())
    solver._backend.close()
