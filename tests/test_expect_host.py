"""
Noise-aware solving without a GPU: the numpy twins of the expectation sweeps (dynamicprogramming_amd/noise.py) against
the checker, the quadrature of Disturbances.uniform, pi_set_disturbances' refusals and build on host-only handles, the
register budget of csrc/pi_expect_kernels.hip, and the solver / runner wiring on the CPU backend of
tests/noise_backend.py.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd._native import Info
from dynamicprogramming_amd.noise import Disturbances
from dynamicprogramming_amd.solver import CudaPIConfig
from tests import helpers as H
from tests.noise_backend import NoiseSweepBackend, with_noise_backend

ROOT = Path(__file__).resolve().parents[1]
GOLDEN_GRIDS = ("pendulum", "cartpole", "double_cartpole")
SYMBOLS = ("pi_set_disturbances", "pi_expect_eval_sweeps", "pi_expect_improve_sweep", "pi_expect_value_sweep")


def _case(name, shape, seed=0, scale=30.0):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    term, tval = H.terminal_mask(name, states)
    rng = np.random.default_rng(seed)
    V = (rng.standard_normal(len(states)) * scale).astype(np.float32)
    acts = H.edge_actions(name)
    pol = rng.integers(0, len(acts), size=len(states)).astype(np.int32)
    return dict(bins=bins, grid=(lo, hi, gshape, strides), states=states, term=term, tval=tval, V=V, pol=pol, acts=acts,
                gamma=float(np.float32(envs.ENVS[name].CONFIG["gamma"])), chk=H.oracle_for(name))


# ---- 1. the twin at K = 1 is the checker's backup -------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_GRIDS)
def test_zero_set_twin_is_the_checkers_sweeps(name):
    """On the golden g0 grids with random V: the twins with the one-point zero set give the checker's improvement policy
    on live states and its evaluation values, bit for bit."""
    c = _case(name, tuple(int(g) for g in H.golden(name)["g0_shape"]))
    d = Disturbances.none(len(c["bins"]))
    args = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    o_V, o_delta = c["chk"].eval_sweep(c["states"], c["acts"], c["pol"], c["V"], c["term"], *c["grid"], c["gamma"])
    t_V, t_delta = noise.expected_eval(c["chk"].step, c["states"], c["pol"], c["V"], *args)
    H.assert_bits_equal(t_V, o_V, f"{name} V'")
    assert np.float32(t_delta) == np.float32(o_delta)
    o_pol, o_changed = c["chk"].improve_sweep(c["states"], c["acts"], c["pol"], c["V"], c["term"], *c["grid"], c["gamma"])
    t_pol, t_changed = noise.expected_improve(c["chk"].step, c["states"], c["pol"], c["V"], *args)
    live = ~c["term"]
    assert live.any() and np.array_equal(t_pol[live], o_pol[live]) and np.array_equal(t_pol[~live], c["pol"][~live])
    assert t_changed == o_changed
    v_V, v_pol, v_delta, v_changed = noise.expected_value_sweep(c["chk"].step, c["states"], c["pol"], c["V"], *args)
    w_V, w_pol, w_delta, w_changed = c["chk"].value_sweep(c["states"], c["acts"], c["pol"], c["V"], c["term"], *c["grid"],
                                                          c["gamma"])
    H.assert_bits_equal(v_V, w_V, f"{name} value sweep V'")
    assert np.array_equal(v_pol, w_pol) and np.float32(v_delta) == np.float32(w_delta) and v_changed == w_changed


# ---- 2. quadrature -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("points", [1, 2, 3, 4])
def test_uniform_rule_has_the_moments_of_the_rollout_noise(points):
    """X * u, u uniform on [-1, 1): mean 0, second moment X^2 / 3.  Gauss-Legendre with n nodes is exact to degree
    2 n - 1, so the ONE-point rule (a single node at 0: the deterministic backup) has second moment 0, not X^2 / 3 —
    every rule from two points on reproduces it."""
    X = np.array([0.3, 0.0, 1.7, 0.05])
    d = Disturbances.uniform(4, state_noise=X, action_noise=0.0, points=points)
    assert d.K == points ** 3 and d.D == 4
    p = d.weights.astype(np.float64)
    assert abs(p.sum() - 1.0) <= 1e-6
    for k in range(4):
        delta = d.state_offsets[:, k].astype(np.float64)
        assert abs((p * delta).sum()) <= 1e-6 * max(X[k], 1e-30)
        second = (p * delta ** 2).sum()
        if points == 1 or X[k] == 0:
            assert second == 0.0
        else:
            assert abs(second - X[k] ** 2 / 3) <= 1e-6 * X[k] ** 2 / 3
    a = Disturbances.uniform(2, action_noise=2.0, points=points)
    pa, da = a.weights.astype(np.float64), a.action_offsets.astype(np.float64)
    assert a.K == points and not a.state_offsets.any() and abs(pa.sum() - 1.0) <= 1e-6 and abs((pa * da).sum()) <= 2e-6
    if points >= 2:
        assert abs((pa * da ** 2).sum() - 4.0 / 3) <= 1e-6 * 4.0 / 3


def test_uniform_rule_order_size_and_limit():
    """Action slowest, last noisy dimension fastest, nodes ascending; weights = float32 of the float64 product."""
    d = Disturbances.uniform(4, state_noise=[0.0, 0.2, 0.0, 0.1], action_noise=0.5, points=3)
    assert d.K == 27
    x, w = np.polynomial.legendre.leggauss(3)
    k = 0
    for ia in range(3):
        for i1 in range(3):
            for i3 in range(3):
                assert d.action_offsets[k] == np.float32(0.5 * x[ia])
                assert np.array_equal(d.state_offsets[k], np.array([0, 0.2 * x[i1], 0, 0.1 * x[i3]], np.float32))
                assert d.weights[k] == np.float32(w[ia] / 2 * (w[i1] / 2) * (w[i3] / 2))
                k += 1
    assert np.array_equal(d.action_offsets[:9], np.full(9, d.action_offsets[0]))       # equal da: contiguous
    assert Disturbances.uniform(2, state_noise=0.1, points=8).K == 64
    for kw in (dict(D=6, state_noise=0.1, points=3), dict(D=2, state_noise=0.1, action_noise=1.0, points=5)):
        with pytest.raises(ValueError, match="more than 64"):
            Disturbances.uniform(**kw)
    assert Disturbances.uniform(6, points=3).K == 1                                   # no noise: the zero set
    t = d.table()
    assert t.shape == (27, 6) and t.dtype == np.float32
    back = Disturbances.from_table(t)
    assert all(np.array_equal(getattr(back, f), getattr(d, f)) for f in ("action_offsets", "state_offsets", "weights"))
    for bad in (dict(weights=[0.5, 0.6]), dict(weights=[1.5, -0.5]), dict(weights=[np.nan, 1.0]), dict(weights=[]),
                dict(weights=[0.5, 0.5], action_offsets=[np.inf, 0.0])):
        kw = dict(action_offsets=None, state_offsets=np.zeros((len(bad["weights"]), 2)), **bad) if "action_offsets" not in bad \
            else dict(state_offsets=np.zeros((2, 2)), **bad)
        with pytest.raises(ValueError):
            Disturbances(**kw)


# ---- 3. a symmetric rule leaves an affine V alone ---------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [("pendulum", (16, 16)), ("cartpole_swingup", (9, 7, 11, 5)),
                                         ("double_cartpole_swingup", (5, 4, 6, 4, 5, 4))])
def test_symmetric_disturbances_leave_an_affine_value_function_alone(name, shape):
    """Independent of the twin's structure: multilinear interpolation reproduces an affine V, and a rule with
    sum p dx = 0 then has the expectation of the nominal successor.  V affine in the state; the symmetric 3-point rule
    at 0.4 cell widths in the first min(D, 3) dimensions; states whose nominal successor is more than one cell inside
    every border and not done: |Q_noisy - Q_det| <= 2e-6 * max|V| (float32 rounding of the interpolations and of up to
    27 fmaf steps: measured at most 7.6e-6 at max|V| 32-43, 2.4e-7 relative; the bound is ten times the 2e-7 a prototype
    gave, to cover other seeds)."""
    c = _case(name, shape)
    lo, hi, gshape, strides = c["grid"]
    D = len(shape)
    rng = np.random.default_rng(5)
    coef = rng.standard_normal(D) * 20.0
    unit = (c["states"].astype(np.float64) - lo.astype(np.float64)) / (hi.astype(np.float64) - lo.astype(np.float64))
    V = (10.0 + unit @ coef).astype(np.float32)
    cell = (hi.astype(np.float64) - lo.astype(np.float64)) / (np.asarray(gshape, np.float64) - 1)
    X = np.where(np.arange(D) < min(D, 3), 0.4 * cell, 0.0)
    d = Disturbances.uniform(D, state_noise=X, points=3)
    assert d.K == 3 ** min(D, 3)
    tables = (V, c["acts"], *c["grid"], c["gamma"])
    worst, checked = 0.0, 0
    for u in c["acts"]:
        nxt, _, done = c["chk"].step(c["states"], u)
        pos = (nxt.astype(np.float64) - lo) / cell
        inside = ~done & np.all((pos > 1.0) & (pos < np.asarray(gshape) - 2.0), axis=1)
        if not inside.any():
            continue
        q_det = noise.expected_q(c["chk"].step, c["states"][inside], u, Disturbances.none(D), *tables)
        q_noisy = noise.expected_q(c["chk"].step, c["states"][inside], u, d, *tables)
        worst = max(worst, float(np.abs(q_noisy.astype(np.float64) - q_det).max()))
        checked += int(inside.sum())
    vmax = float(np.abs(V).max())
    print(f"{name} {shape}: {checked} (state, action) pairs, max|V| = {vmax:.1f}, worst |dQ| = {worst:.3g} = {worst / vmax:.3g} relative")
    assert checked > 0
    assert worst <= 2e-6 * vmax


# ---- 4. refusals, on host-only handles ----------------------------------------------------------------------------------
def test_set_disturbances_refusals_and_info_on_a_host_only_handle(tmp_path):
    name, shape = "cartpole_swingup", (9, 7, 11, 5)
    eng = H.host_engine(name, shape)
    assert eng.info(Info.DISTURBANCES) == 0
    with pytest.raises(_native.NativeError, match="pi_compile"):                   # before pi_compile
        eng.set_disturbances(None, None, [1.0])
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)
    assert eng.info(Info.DISTURBANCES) == 0
    lib = _native.lib()
    for fn, args in (("pi_expect_eval_sweeps", (8, 16, 24, None, 0, 10, 0.9, 1, None, None)),
                     ("pi_expect_improve_sweep", (8, 24, None, 0, 10, 0.9, None, None)),
                     ("pi_expect_value_sweep", (8, 16, 24, None, 0, 10, 0.9, None, None, None))):
        assert getattr(lib, fn)(eng._h, *args) != 0                              # no set: refused, by name
        assert "pi_set_disturbances" in _native.last_error(), fn
    zeros4 = np.zeros((2, 4), np.float32)
    for what, (da, dx, p), msg in (
            ("K = 65", (None, None, np.full(65, 1 / 65, np.float32)), r"\[0, 64\]"),
            ("NaN weight", (None, zeros4, [np.nan, 1.0]), "not finite"),
            ("inf action offset", ([np.inf, 0.0], zeros4, [0.5, 0.5]), "not finite"),
            ("NaN state offset", (None, np.array([[0, 0, np.nan, 0], [0, 0, 0, 0]], np.float32), [0.5, 0.5]), "not finite"),
            ("-inf state offset", (None, np.array([[0, 0, 0, 0], [0, -np.inf, 0, 0]], np.float32), [0.5, 0.5]), "not finite"),
            ("negative weight", (None, zeros4, [1.25, -0.25]), "negative"),
            ("sum off by 1e-3", (None, zeros4, [0.5, 0.501]), "sum to")):
        with pytest.raises(_native.NativeError, match=msg):
            eng.set_disturbances(da, dx, p)
        assert eng.info(Info.DISTURBANCES) == 0, what
    assert lib.pi_set_disturbances(eng._h, -1, None, None, None) != 0
    assert lib.pi_set_disturbances(eng._h, 1, None, None, None) != 0 and "weights" in _native.last_error()
    assert eng.set_disturbances(None, None, [1.0]) == 1                            # NULL offsets: zeros
    assert eng.set_disturbances([0.0, 0.5], zeros4, [0.5, 0.50005]) == 2 and eng.info(Info.DISTURBANCES) == 2
    rc = lib.pi_expect_improve_sweep(eng._h, 8, 24, None, 0, 10, 0.9, None, None)   # a set, but no device
    assert rc != 0 and "host-only" in _native.last_error()
    assert eng.set_disturbances(None, None, None) == 0 and eng.info(Info.DISTURBANCES) == 0      # K = 0 drops it
    assert eng.set_disturbances(None, None, np.full(64, 1 / 64, np.float32)) == 64
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)                      # a second pi_compile drops it
    assert eng.info(Info.DISTURBANCES) == 0
    eng.close()


def test_grids_of_2_pow_30_states_are_refused_by_name():
    eng = H.host_engine("double_cartpole", (32,) * 6)
    assert eng.n_states == 1 << 30
    with pytest.raises(_native.NativeError, match="2\\^30"):
        eng.set_disturbances(None, None, [1.0])
    eng.close()


def test_new_symbols_are_declared_commented_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    lib = _native.lib()
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(pi_handle\* h,", header, re.M), sym
        assert header.count(sym) >= 2, f"{sym} has no comment in the header"
        assert hasattr(lib, sym) and sym in _native.SIGNATURES
    for method in ("set_disturbances", "expect_eval_sweeps", "expect_improve_sweep", "expect_value_sweep"):
        assert callable(getattr(_native.Engine, method))
    assert re.search(r"PI_INFO_DISTURBANCES = 38\b", header) and Info.DISTURBANCES == 38
    assert _native.ABI_VERSION == 12 and lib.pi_abi_version() == 12
    makefile = (ROOT / "dynamicprogramming_amd" / "csrc" / "Makefile").read_text()
    assert "pi_expect.cpp" in makefile


# ---- 5. build checks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_expectation_module_builds_for_gfx950_and_is_one_more_cache_object(name, tmp_path):
    shape = {2: (24, 17), 4: (9, 7, 11, 5), 6: (5, 4, 6, 4, 5, 4)}[envs.ENVS[name]._D]
    eng = H.host_engine(name, shape)
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)
    first = sorted(tmp_path.glob("pi_*.hsaco"))
    assert len(first) == 1                                       # pi_compile alone: exactly one object, as before
    D = eng.D
    assert eng.set_disturbances(None, None, [1.0]) == 1          # builds the module (lazily: only now)
    both = sorted(tmp_path.glob("pi_*.hsaco"))
    assert len(both) == 2 and set(first) < set(both)
    new = (set(both) - set(first)).pop()
    assert new.stat().st_size > 4096 and new.read_bytes()[:4] == b"\x7fELF"
    stamp = new.stat().st_mtime_ns
    d = Disturbances.uniform(D, state_noise=0.01, points=2) if D <= 4 else Disturbances.uniform(D, action_noise=0.5, points=5)
    assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K      # another K: nothing is built
    assert sorted(tmp_path.glob("pi_*.hsaco")) == both and new.stat().st_mtime_ns == stamp
    eng.close()


def test_expectation_kernels_do_not_spill(tmp_path):
    """No scratch and at most 512 VGPRs for the three kernels in every D, on the ahead-of-time build of the translation
    unit pi_set_disturbances hands to hipRTC — Engine.kernel_source + csrc/pi_expect_kernels.hip — with the method of
    tests/test_stochastic_host.py.  The register counts are printed: README quotes them."""
    import __graft_entry__ as G
    kernel = (ROOT / "dynamicprogramming_amd" / "csrc" / "pi_expect_kernels.hip").read_text()
    for name, bins in (("pendulum", 200), ("cartpole_swingup", 50), ("double_cartpole", 25), ("double_cartpole_swingup", 25)):
        eng, dyn = G._engine_for(name, bins)
        text = eng.kernel_source(dyn) + "\n" + kernel + "\n"
        n_actions = eng.info(Info.N_ACTIONS)
        eng.close()
        usage = H.kernel_resource_usage(text, tmp_path, name)
        mine = {fn: k for fn, k in usage.items() if fn.startswith("pi_expect_")}
        assert set(mine) == {"pi_expect_eval_kernel", "pi_expect_improve_kernel", "pi_expect_value_kernel"}
        for fn, k in mine.items():
            print(f"{fn} {name} {bins}^{envs.ENVS[name]._D} x {n_actions}: {k}")
            assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, fn, k)


def test_kernel_file_is_embedded_and_the_sweep_unit_is_untouched():
    """pi_compile's unit does not hold the expectation kernels (they are a module of their own), and product code of the
    new module imports nothing from the oracle or the tests."""
    eng = H.host_engine("pendulum", (24, 17))
    assert "pi_expect_eval_kernel" not in eng.kernel_source(envs.dynamics_source("pendulum"))
    eng.close()
    text = (ROOT / "dynamicprogramming_amd" / "noise.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests)\b", text, re.M)


# ---- 6. solver logic on the checker backend -------------------------------------------------------------------------
def _solver(name, shape, cfg, **kw):
    cls = envs.ENVS[name]
    return with_noise_backend(cls)(H.env_bins_space(name, shape), cls.ACTIONS, cfg, **kw)


def test_solver_routes_its_sweeps_through_the_expectation_and_back():
    name, shape = "pendulum", (12, 11)
    # theta = 0: no evaluation ends early, so the books below are fixed numbers
    cfg = CudaPIConfig(**{**envs.ENVS[name].CONFIG, "max_pi_iter": 2, "max_eval_iter": 30, "theta": 0.0})
    d = Disturbances.uniform(2, state_noise=[0.2, 0.3], action_noise=0.5, points=2)
    s = _solver(name, shape, cfg)
    assert isinstance(s._backend, NoiseSweepBackend) and s.disturbances is None and "disturbances" not in s.stats
    s.set_disturbances(d)
    assert s.stats["disturbances"] == 8 and s.disturbances is d and s._backend.disturbances is d
    s._backend.resident = True                                   # a backend that offers the one-launch shortcuts ...
    s._backend.whole_run = True
    s._backend.policy_evaluation = s._backend.policy_iteration = s._backend.eval_begin = None   # ... which must not be called
    s.run()
    calls = s._backend.calls
    assert calls["eval"] == 0 and calls["improve"] == 0 and calls["expect_eval"] == s.stats["eval_sweeps"] > 0
    assert calls["expect_improve"] == s.stats["improve_sweeps"] == 2
    # the same loop spelled out with the twins
    c = _case(name, shape)
    V, pol = np.zeros(len(c["states"]), np.float32), np.zeros(len(c["states"]), np.int32)
    args = (None, d, envs.ENVS[name].ACTIONS, *c["grid"], float(np.float32(cfg.gamma)))
    for _ in range(2):
        for _ in range(30):
            V, _ = noise.expected_eval(c["chk"].step, c["states"], pol, V, *args)
        pol, _ = noise.expected_improve(c["chk"].step, c["states"], pol, V, *args)
    H.assert_bits_equal(s.value_function, V, "V of the noise-aware run")
    assert np.array_equal(s.policy, pol)
    # value iteration, then None restores the deterministic calls
    v = _solver(name, shape, cfg)
    v.set_disturbances(d)
    v.value_iteration(3)
    assert v._backend.calls["expect_value"] == 3 and v._backend.calls["value"] == 0
    v.set_disturbances(None)
    assert v.stats["disturbances"] == 0 and v.disturbances is None
    v.value_iteration(2)
    v.policy_evaluation()
    v.policy_improvement()
    assert v._backend.calls["expect_value"] == 3 and v._backend.calls["value"] == 2
    assert v._backend.calls["eval"] == 30 and v._backend.calls["improve"] == 1 and v._backend.calls["expect_eval"] == 0
    # a deterministic solver equals one that had a set installed and dropped again
    a, b = _solver(name, shape, cfg), _solver(name, shape, cfg)
    b.set_disturbances(d)
    b.set_disturbances(None)
    a.run()
    b.run()
    H.assert_bits_equal(a.value_function, b.value_function, "V after set / unset")
    assert np.array_equal(a.policy, b.policy)


def test_sharded_solver_refuses_a_disturbance_set():
    class TwoRanks:
        world, rank, halo_elems = 2, 0, -1

        def attach(self, solver):
            pass

        def plan(self, solver):
            pass

    cfg = CudaPIConfig(**envs.ENVS["pendulum"].CONFIG)
    s = _solver("pendulum", (12, 11), cfg, transport=TwoRanks())
    with pytest.raises(NotImplementedError, match="single-rank"):
        s.set_disturbances(Disturbances.none(2))
    assert s.disturbances is None


def test_save_and_load_keep_the_set(tmp_path):
    name, shape = "pendulum", (12, 11)
    cfg = CudaPIConfig(**{**envs.ENVS[name].CONFIG, "max_pi_iter": 1, "max_eval_iter": 2})
    d = Disturbances.uniform(2, state_noise=[0.2, 0.0], action_noise=0.5, points=3)
    s = _solver(name, shape, cfg)
    s.set_disturbances(d)
    s.run()
    s.save(tmp_path / "noisy")
    data = np.load(tmp_path / "noisy.npz")
    assert data["disturbances"].shape == (9, 4) and data["disturbances"].dtype == np.float32
    assert np.array_equal(data["disturbances"], d.table())
    back = envs.ENVS[name].load(tmp_path / "noisy")
    assert back.disturbances.K == 9 and np.array_equal(back.disturbances.table(), d.table())
    p = _solver(name, shape, cfg)
    p.run()
    p.save(tmp_path / "plain")
    assert "disturbances" not in np.load(tmp_path / "plain.npz").files          # only when a set is installed
    assert envs.ENVS[name].load(tmp_path / "plain").disturbances is None


def test_runner_flags(tmp_path, capsys):
    from runners import _cli
    args = _cli.build_parser("cartpole", "x.npz").parse_args([])
    assert (args.train_action_noise, args.train_state_noise, args.train_noise_points) == (0.0, None, 3)
    assert _cli.ignored_flags(args) == [] and not _cli.training_noise_requested(args)
    assert _cli.training_disturbances("cartpole") is None
    args = _cli.build_parser("cartpole", "x.npz").parse_args(
        ["--train-action-noise", "2.5", "--train-state-noise", "0.1", "0", "0.02", "0", "--train-noise-points", "2"])
    assert _cli.ignored_flags(args) == [] and _cli.training_noise_requested(args)
    d = _cli.training_disturbances("cartpole", args.train_action_noise, args.train_state_noise, args.train_noise_points)
    assert d.K == 8 and d.D == 4 and not d.state_offsets[:, [1, 3]].any() and d.state_offsets[:, [0, 2]].all()
    one = _cli.training_disturbances("double_cartpole", 0.0, [0.0, 0.0, 0.0, 0.0, 0.0, 0.3], 3)
    assert one.K == 3 and one.D == 6
    assert _cli.training_disturbances("pendulum", 0.0, [0.0], 3) is None
    for runner in sorted((ROOT / "runners").glob("*.py")):                         # every runner that trains goes through _cli
        if runner.name not in ("_cli.py", "__init__.py", "hybrid_double_cartpole.py"):    # (the hybrid one only loads)
            assert "_cli" in runner.read_text(), runner.name
    # a saved policy is loaded instead of trained: the flags had no effect, and the run says so
    cfg = CudaPIConfig(**{**envs.ENVS["pendulum"].CONFIG, "max_pi_iter": 1, "max_eval_iter": 2})
    s = _solver("pendulum", (12, 11), cfg)
    s.run()
    s.save(tmp_path / "saved")
    capsys.readouterr()
    _cli.main("pendulum", str(tmp_path / "saved.npz"), ["--save-path", str(tmp_path / "saved.npz"), "--train-action-noise", "0.5"])
    assert "had no effect" in capsys.readouterr().out
    _cli.main("pendulum", str(tmp_path / "saved.npz"), ["--save-path", str(tmp_path / "saved.npz")])
    assert "had no effect" not in capsys.readouterr().out
