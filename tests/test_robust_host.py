"""
Worst-case solving without a GPU: the numpy twins with risk="worst" (dynamicprogramming_amd/noise.py) against the checker
and against the properties of a minimum over the set, the pi_robust_* entry points on host-only handles, the register
budget of the pi_robust_* kernels of csrc/pi_expect_kernels.hip, and the solver / runner wiring on the CPU backend of
tests/robust_backend.py.
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
from tests.robust_backend import RobustSweepBackend, with_robust_backend
from tests.robust_cases import ZERO_ROWS, zero_weight_sets
from tests.test_gpu_expect import _make_set

ROOT = Path(__file__).resolve().parents[1]
GOLDEN_GRIDS = ("pendulum", "cartpole", "double_cartpole")
RAGGED = (("pendulum", (24, 17)), ("cartpole_swingup", (9, 7, 11, 5)), ("double_cartpole", (5, 4, 6, 4, 5, 4)))
SYMBOLS = ("pi_robust_eval_sweeps", "pi_robust_improve_sweep", "pi_robust_value_sweep")
KERNELS = {"pi_robust_eval_kernel", "pi_robust_improve_kernel", "pi_robust_value_kernel"}


def _case(name, shape, seed=0, scale=30.0):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    term, tval = H.terminal_mask(name, states)
    rng = np.random.default_rng(seed)
    V = (rng.standard_normal(len(states)) * scale).astype(np.float32)
    acts = H.edge_actions(name)
    pol = rng.integers(0, len(acts), size=len(states)).astype(np.int32)
    cell = (hi.astype(np.float64) - lo.astype(np.float64)) / (np.asarray(gshape, np.float64) - 1)
    return dict(bins=bins, grid=(lo, hi, gshape, strides), states=states, term=term, tval=tval, V=V, pol=pol, acts=acts,
                cell=cell, D=len(bins), gamma=float(np.float32(envs.ENVS[name].CONFIG["gamma"])), chk=H.oracle_for(name))


def _sweeps(c, d, risk="worst", V=None):
    """(V' of an evaluation sweep, V' and policy of a value sweep, policy of an improvement sweep) of the twins."""
    V = c["V"] if V is None else V
    args = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    e_V, _ = noise.expected_eval(c["chk"].step, c["states"], c["pol"], V, *args, risk=risk)
    v_V, v_pol, _, _ = noise.expected_value_sweep(c["chk"].step, c["states"], c["pol"], V, *args, risk=risk)
    i_pol, _ = noise.expected_improve(c["chk"].step, c["states"], c["pol"], V, *args, risk=risk)
    return e_V, v_V, v_pol, i_pol


# ---- 1. the twin at K = 1 is the checker's backup -------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_GRIDS)
def test_zero_set_worst_case_twin_is_the_checkers_sweeps(name):
    c = _case(name, tuple(int(g) for g in H.golden(name)["g0_shape"]))
    d = Disturbances.none(c["D"])
    args = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    targs = (c["states"], c["acts"], c["pol"], c["V"], c["term"], *c["grid"], c["gamma"])
    o_V, o_delta = c["chk"].eval_sweep(*targs)
    t_V, t_delta = noise.expected_eval(c["chk"].step, c["states"], c["pol"], c["V"], *args, risk="worst")
    H.assert_bits_equal(t_V, o_V, f"{name} V'")
    assert np.float32(t_delta) == np.float32(o_delta)
    o_pol, o_changed = c["chk"].improve_sweep(*targs)
    t_pol, t_changed = noise.expected_improve(c["chk"].step, c["states"], c["pol"], c["V"], *args, risk="worst")
    live = ~c["term"]
    assert live.any() and np.array_equal(t_pol[live], o_pol[live]) and np.array_equal(t_pol[~live], c["pol"][~live])
    assert t_changed == o_changed
    v_V, v_pol, v_delta, v_changed = noise.expected_value_sweep(c["chk"].step, c["states"], c["pol"], c["V"], *args,
                                                                risk="worst")
    w_V, w_pol, w_delta, w_changed = c["chk"].value_sweep(*targs)
    H.assert_bits_equal(v_V, w_V, f"{name} value sweep V'")
    assert np.array_equal(v_pol, w_pol) and np.float32(v_delta) == np.float32(w_delta) and v_changed == w_changed


def test_risk_keyword_defaults_and_refusals():
    c = _case("pendulum", (12, 11))
    d = _make_set("S2", 2, c["cell"], c["acts"])
    tables = (d, c["V"], c["acts"], *c["grid"], c["gamma"])
    q = noise.expected_q(c["chk"].step, c["states"], c["acts"][0], *tables)
    H.assert_bits_equal(noise.expected_q(c["chk"].step, c["states"], c["acts"][0], *tables, risk="expected"), q, "default")
    for fn in (noise.expected_q, noise.expected_eval, noise.expected_improve, noise.expected_value_sweep):
        with pytest.raises(ValueError, match="risk"):
            fn(c["chk"].step, c["states"], c["pol"], c["V"], None, d, c["acts"], *c["grid"], c["gamma"], risk="cvar") \
                if fn is not noise.expected_q else fn(c["chk"].step, c["states"], c["acts"][0], *tables, risk="cvar")
    with pytest.raises(ValueError, match="worst_point"):
        noise.expected_q(c["chk"].step, c["states"], c["acts"][0], *tables, worst_point=True)


# ---- 2. points of weight zero are not in the set -----------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", RAGGED)
def test_zero_weight_rows_take_no_part(name, shape):
    """S3 (K = 64, da in runs of 8) with 16 rows rewritten to weight 0 and offsets of +-1e30 — row 0, first, inner and
    last rows of runs — gives the bits of the 48-row set without them, and its k* after index mapping.  V is -1e4 at the
    2^D corner nodes of the grid, where offsets of +-1e30 in every dimension clamp to: with a weight those rows would be the
    minimum wherever their step is not done, which the last lines check."""
    c = _case(name, shape)
    lo, hi = c["grid"][0], c["grid"][1]
    c["V"] = c["V"].copy()
    c["V"][np.all((c["states"] == lo) | (c["states"] == hi), axis=1)] = np.float32(-1e4)
    assert (c["V"] == np.float32(-1e4)).sum() == 2 ** c["D"]
    full = _make_set("S3", c["D"], c["cell"], c["acts"])
    with_zeros, without, kept = zero_weight_sets(full)
    assert with_zeros.K == 64 and without.K == 48 and (with_zeros.weights[list(ZERO_ROWS)] == 0).all()
    for got, want, what in zip(_sweeps(c, with_zeros), _sweeps(c, without), ("eval V'", "value V'", "value policy", "policy")):
        if got.dtype == np.float32:
            H.assert_bits_equal(got, want, f"{name} {what}")
        assert np.array_equal(got, want), what
    live = ~c["term"]
    tables = (c["V"], c["acts"], *c["grid"], c["gamma"])
    for u in c["acts"]:
        q64, k64 = noise.expected_q(c["chk"].step, c["states"][live], u, with_zeros, *tables, risk="worst", worst_point=True)
        q48, k48 = noise.expected_q(c["chk"].step, c["states"][live], u, without, *tables, risk="worst", worst_point=True)
        H.assert_bits_equal(q64, q48, f"{name} Q at action {u}")
        assert np.array_equal(k64, kept[k48]) and not np.isin(k64, ZERO_ROWS).any()
    tiny = with_zeros.weights.copy()
    tiny[list(ZERO_ROWS)] = np.float32(1e-7)                         # the same rows, taking part
    taking_part = Disturbances(with_zeros.action_offsets, with_zeros.state_offsets, tiny)
    assert (_sweeps(c, taking_part)[0][live] != _sweeps(c, without)[0][live]).mean() > 0.5


# ---- 3. a minimum does not depend on the order of the points -----------------------------------------------------------
@pytest.mark.parametrize("name,shape", RAGGED)
def test_permuting_the_points_leaves_the_values_equal(name, shape):
    c = _case(name, shape)
    for which in ("S2", "S3"):
        d = _make_set(which, c["D"], c["cell"], c["acts"])
        perm = np.random.default_rng(7).permutation(d.K)
        p = Disturbances(d.action_offsets[perm], d.state_offsets[perm], d.weights[perm])
        a, b = _sweeps(c, d), _sweeps(c, p)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), f"{name} {which}"
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- 4. the minimum is below the mean ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", RAGGED)
def test_worst_case_is_not_above_the_expectation(name, shape):
    """Q_worst <= Q_expected + 2e-4 * max(1, max_k |q_k|) at every live node: Q_expected = sum p_k q_k >= (sum p_k) min_k q_k,
    the weight sum is within 1e-4 of 1, and the at most 64 fmaf roundings of the chain add at most 64 * 2^-24 < 1e-5
    relative to max_k |q_k|.  q_k is the backup of the one-point set {(da_k, dx_k, 1)}: 1.0f * q_k is q_k."""
    c = _case(name, shape)
    live = ~c["term"]
    pts, a = c["states"][live], c["acts"][c["pol"][live]]
    tables = (c["V"], c["acts"], *c["grid"], c["gamma"])
    for which in ("S2", "S3", "S4"):
        d = _make_set(which, c["D"], c["cell"], c["acts"])
        q_max = np.zeros(len(pts))
        q_min = np.full(len(pts), np.inf)
        for k in range(d.K):
            one = Disturbances(d.action_offsets[k:k + 1], d.state_offsets[k:k + 1], [1.0])
            q_k = noise.expected_q(c["chk"].step, pts, a, one, *tables).astype(np.float64)
            q_max, q_min = np.maximum(q_max, np.abs(q_k)), np.minimum(q_min, q_k)
        worst = noise.expected_q(c["chk"].step, pts, a, d, *tables, risk="worst").astype(np.float64)
        mean = noise.expected_q(c["chk"].step, pts, a, d, *tables).astype(np.float64)
        assert (worst == q_min).all(), f"{name} {which}: the fold is the minimum of the points' backups"
        slack = worst - mean - 2e-4 * np.maximum(1.0, q_max)
        print(f"{name} {which}: {len(pts)} live nodes, max (Q_worst - Q_expected - bound) = {slack.max():.3g}, "
              f"Q_worst < Q_expected at {(worst < mean).mean():.1%}")
        assert (slack <= 0).all()


# ---- 5. NaN ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_nan_under_one_point_makes_q_nan(where):
    """Pendulum 24 x 17, three points 4 cells apart along dimension 0, one state whose three successors are inside the
    grid: NaN on the planes of V within 1.5 cells of ONE point's successor (the two planes it interpolates between, and
    none a point 4 cells away reads) makes Q NaN there, whether that point is first, middle or last; with weight 0 on
    that point Q is the minimum of the other two."""
    c = _case("pendulum", (24, 17))
    lo, hi, gshape, strides = c["grid"]
    u = c["acts"][1]
    dx = np.zeros((3, 2), np.float32)
    dx[:, 0] = np.array([-4.0, 0.0, 4.0]) * c["cell"][0]
    d = Disturbances(None, dx, [0.25, 0.5, 0.25])
    nxt, _, done = c["chk"].step(c["states"], u)
    pos0 = (nxt[:, 0].astype(np.float64) - float(lo[0])) / c["cell"][0]
    ok = np.flatnonzero(~done & (pos0 > 7.0) & (pos0 < 15.0))
    assert len(ok)
    s = ok[len(ok) // 2]
    plane = np.rint((c["states"][:, 0].astype(np.float64) - float(lo[0])) / c["cell"][0])
    V = c["V"].copy()
    V[np.abs(plane - (pos0[s] + 4.0 * (where - 1))) < 1.5] = np.nan
    tables = (c["acts"], *c["grid"], c["gamma"])
    clean = noise.expected_q(c["chk"].step, c["states"][s:s + 1], u, d, c["V"], *tables, risk="worst")
    q, k = noise.expected_q(c["chk"].step, c["states"][s:s + 1], u, d, V, *tables, risk="worst", worst_point=True)
    assert np.isfinite(clean).all() and np.isnan(q).all() and k[0] == where
    w = np.array([0.5, 0.5, 0.5], np.float32)
    w[where] = 0.0
    others = Disturbances(None, dx, w)
    q_others = noise.expected_q(c["chk"].step, c["states"][s:s + 1], u, others, V, *tables, risk="worst")
    H.assert_bits_equal(q_others, noise.expected_q(c["chk"].step, c["states"][s:s + 1], u, others, c["V"], *tables,
                                                   risk="worst"), "the NaN is under a point that takes no part")
    assert np.isfinite(q_others).all()
    # a NaN never wins the strict > argmax: the improvement of that state ignores the action
    pol, _ = noise.expected_improve(c["chk"].step, c["states"], c["pol"], np.full_like(V, np.nan), None, d, *tables, risk="worst")
    assert (pol == 0).all()


# ---- 6. solver logic on the checker backend -------------------------------------------------------------------------
def _solver(name, shape, cfg, **kw):
    cls = envs.ENVS[name]
    return with_robust_backend(cls)(H.env_bins_space(name, shape), cls.ACTIONS, cfg, **kw)


NAME, SHAPE = "pendulum", (12, 11)


def _cfg(**kw):
    # theta = 0: no evaluation ends early, so the books below are fixed numbers
    return CudaPIConfig(**{**envs.ENVS[NAME].CONFIG, "max_pi_iter": 2, "max_eval_iter": 30, "theta": 0.0, **kw})


def _set():
    return Disturbances.uniform(2, state_noise=[0.2, 0.3], action_noise=0.5, points=2)


def test_solver_routes_its_sweeps_through_the_worst_case_and_back():
    cfg, d = _cfg(), _set()
    s = _solver(NAME, SHAPE, cfg)
    assert isinstance(s._backend, RobustSweepBackend) and s.risk == "expected" and "risk" not in s.stats
    with pytest.raises(ValueError, match="risk"):
        s.set_disturbances(d, risk="cvar")
    s.set_disturbances(d, risk="worst")
    assert s.risk == "worst" and s.stats["risk"] == "worst" and s.stats["disturbances"] == 8 and s._backend.disturbances is d
    s._backend.resident = True                                   # a backend that offers the one-launch shortcuts ...
    s._backend.whole_run = True
    s._backend.policy_evaluation = s._backend.policy_iteration = s._backend.eval_begin = None   # ... which must not be called
    s.run()
    calls = s._backend.calls
    assert calls["robust_eval"] == s.stats["eval_sweeps"] > 0 and calls["robust_improve"] == s.stats["improve_sweeps"] == 2
    assert not any(calls[k] for k in ("eval", "improve", "value", "expect_eval", "expect_improve", "expect_value", "robust_value"))
    c = _case(NAME, SHAPE)
    V, pol = np.zeros(len(c["states"]), np.float32), np.zeros(len(c["states"]), np.int32)
    args = (None, d, envs.ENVS[NAME].ACTIONS, *c["grid"], float(np.float32(cfg.gamma)))
    for _ in range(2):
        for _ in range(30):
            V, _ = noise.expected_eval(c["chk"].step, c["states"], pol, V, *args, risk="worst")
        pol, _ = noise.expected_improve(c["chk"].step, c["states"], pol, V, *args, risk="worst")
    H.assert_bits_equal(s.value_function, V, "V of the worst-case run")
    assert np.array_equal(s.policy, pol)
    # not the expectation's solution
    e = _solver(NAME, SHAPE, cfg)
    e.set_disturbances(d)
    e.run()
    assert e._backend.calls["expect_eval"] == 60 and e._backend.calls["robust_eval"] == 0
    assert (s.value_function <= e.value_function + 2e-4 * np.maximum(1, np.abs(e.value_function))).all()
    assert (s.value_function < e.value_function).mean() > 0.5


def test_risk_expected_and_none_restore_the_calls_of_before():
    cfg, d = _cfg(), _set()
    v = _solver(NAME, SHAPE, cfg)
    v.set_disturbances(d, risk="worst")
    v.value_iteration(3)
    assert v._backend.calls["robust_value"] == 3 and v._backend.calls["expect_value"] == 0 and v._backend.calls["value"] == 0
    c = _case(NAME, SHAPE)
    V, pol = np.zeros(len(c["states"]), np.float32), np.zeros(len(c["states"]), np.int32)
    for _ in range(3):
        V, pol, _, _ = noise.expected_value_sweep(c["chk"].step, c["states"], pol, V, None, d, envs.ENVS[NAME].ACTIONS,
                                                  *c["grid"], float(np.float32(cfg.gamma)), risk="worst")
    n = len(c["states"])                                             # (the default memory order is the user's)
    H.assert_bits_equal(np.ascontiguousarray(v.d_value_function.numpy()[:n]), V, "V of three worst-case value sweeps")
    assert np.array_equal(v.d_policy.numpy()[:n], pol)
    v.set_disturbances(d, risk="expected")
    assert v.risk == "expected" and "risk" not in v.stats and v.stats["disturbances"] == 8
    v.value_iteration(2)
    v.policy_evaluation()
    v.policy_improvement()
    calls = v._backend.calls
    assert calls["expect_value"] == 2 and calls["expect_eval"] == 30 and calls["expect_improve"] == 1
    assert calls["robust_value"] == 3 and calls["robust_eval"] == 0 and calls["robust_improve"] == 0
    v.set_disturbances(d, risk="worst")
    v.set_disturbances(None)
    assert v.risk == "expected" and "risk" not in v.stats and v.stats["disturbances"] == 0 and v.disturbances is None
    v.value_iteration(2)
    v.policy_evaluation()
    v.policy_improvement()
    assert calls["value"] == 2 and calls["eval"] == 30 and calls["improve"] == 1
    assert calls["robust_value"] == 3 and calls["robust_eval"] == 0 and calls["expect_value"] == 2
    # a deterministic solver equals one that had a worst-case set installed and dropped again
    a, b = _solver(NAME, SHAPE, cfg), _solver(NAME, SHAPE, cfg)
    b.set_disturbances(d, risk="worst")
    b.set_disturbances(None)
    a.run()
    b.run()
    H.assert_bits_equal(a.value_function, b.value_function, "V after set / unset")
    assert np.array_equal(a.policy, b.policy)


def test_sharded_solver_refuses_a_worst_case_set():
    class TwoRanks:
        world, rank, halo_elems = 2, 0, -1

        def attach(self, solver):
            pass

        def plan(self, solver):
            pass

    s = _solver(NAME, SHAPE, CudaPIConfig(**envs.ENVS[NAME].CONFIG), transport=TwoRanks())
    with pytest.raises(NotImplementedError, match="single-rank"):
        s.set_disturbances(Disturbances.none(2), risk="worst")
    assert s.disturbances is None and s.risk == "expected"


def test_save_and_load_keep_the_risk(tmp_path):
    cfg = _cfg(max_pi_iter=1, max_eval_iter=2)
    d = Disturbances.uniform(2, state_noise=[0.2, 0.0], action_noise=0.5, points=3)
    plain_keys = {"value_function", "policy", "bounds_low", "bounds_high", "grid_shape", "strides", "corner_bits",
                  "action_space", "states_space"}
    for risk, keys in (("worst", plain_keys | {"disturbances", "risk"}), ("expected", plain_keys | {"disturbances"}),
                       (None, plain_keys)):
        s = _solver(NAME, SHAPE, cfg)
        if risk is not None:
            s.set_disturbances(d, risk=risk)
        s.run()
        s.save(tmp_path / f"{risk}")
        data = np.load(tmp_path / f"{risk}.npz")                     # no pickle: the entry is a plain string array
        assert set(data.files) == keys, risk
        back = envs.ENVS[NAME].load(tmp_path / f"{risk}")
        assert back.risk == ("worst" if risk == "worst" else "expected")
        assert (back.disturbances is None) == (risk is None)
        if risk == "worst":
            assert str(data["risk"]) == "worst" and np.array_equal(back.disturbances.table(), d.table())


# ---- 7. host-only handles -----------------------------------------------------------------------------------------------
def test_refusals_on_a_host_only_handle_in_order(tmp_path):
    name, shape = "cartpole_swingup", (9, 7, 11, 5)
    eng = H.host_engine(name, shape)
    lib = _native.lib()
    calls = (("pi_robust_eval_sweeps", (8, 16, 24, None, 0, 10, 0.9, 1, None, None)),
             ("pi_robust_improve_sweep", (8, 24, None, 0, 10, 0.9, None, None)),
             ("pi_robust_value_sweep", (8, 16, 24, None, 0, 10, 0.9, None, None, None)))
    for fn, args in calls:
        assert getattr(lib, fn)(None, *args) != 0 and "null handle" in _native.last_error(), fn
        assert getattr(lib, fn)(eng._h, *args) != 0                                   # before pi_compile: the set comes first
        assert "pi_set_disturbances" in _native.last_error() and fn in _native.last_error()
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)
    for fn, args in calls:
        assert getattr(lib, fn)(eng._h, *args) != 0 and "pi_set_disturbances" in _native.last_error(), fn
    assert eng.set_disturbances([0.0, 0.5], np.zeros((2, 4), np.float32), [0.5, 0.5]) == 2
    for fn, args in calls:                                                            # a set, but no device
        assert getattr(lib, fn)(eng._h, *args) != 0 and "host-only" in _native.last_error(), fn
    for method, args in (("robust_eval_sweeps", (8, 16, 24, 0, 0, 10, 0.9, 1)), ("robust_improve_sweep", (8, 24, 0, 0, 10, 0.9)),
                         ("robust_value_sweep", (8, 16, 24, 0, 0, 10, 0.9))):
        with pytest.raises(_native.NativeError, match="host-only"):
            getattr(eng, method)(*args)
    assert eng.set_disturbances(None, None, None) == 0
    for fn, args in calls:                                                            # dropped: refused by name again
        assert getattr(lib, fn)(eng._h, *args) != 0 and "pi_set_disturbances" in _native.last_error(), fn
    eng.close()


def test_new_symbols_are_declared_commented_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    lib = _native.lib()
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(pi_handle\* h,", header, re.M), sym
        assert header.count(sym) >= 2, f"{sym} has no comment in the header"
        assert hasattr(lib, sym) and sym in _native.SIGNATURES
        assert _native.SIGNATURES[sym] == _native.SIGNATURES[sym.replace("pi_robust_", "pi_expect_")]
    for method in ("robust_eval_sweeps", "robust_improve_sweep", "robust_value_sweep"):
        assert callable(getattr(_native.Engine, method))
        from dynamicprogramming_amd.solver import HipSweepBackend
        assert callable(getattr(HipSweepBackend, method))
    for phrase in ("q_k < Q || q_k != q_k", "p_k == 0.0f takes no part"):
        assert phrase in header, phrase
    assert _native.ABI_VERSION == 12 and lib.pi_abi_version() == 12


@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_worst_case_kernels_are_in_the_one_expectation_module(name, tmp_path):
    shape = {2: (24, 17), 4: (9, 7, 11, 5), 6: (5, 4, 6, 4, 5, 4)}[envs.ENVS[name]._D]
    eng = H.host_engine(name, shape)
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)
    first = set(tmp_path.glob("pi_*.hsaco"))
    assert len(first) == 1
    assert not any(k.encode() in next(iter(first)).read_bytes() for k in KERNELS)      # the sweep unit is untouched
    assert eng.set_disturbances(None, None, [1.0]) == 1
    both = set(tmp_path.glob("pi_*.hsaco"))
    assert len(both) == 2 and first < both                                            # still one more object, not two
    image = (both - first).pop().read_bytes()
    for k in KERNELS | {"pi_expect_eval_kernel", "pi_expect_improve_kernel", "pi_expect_value_kernel"}:
        assert k.encode() in image, k
    eng.close()


# ---- 8. registers ------------------------------------------------------------------------------------------------------
def test_worst_case_kernels_do_not_spill(tmp_path):
    """No scratch and at most 512 VGPRs for the three pi_robust_* kernels in every D, by the method of
    tests/test_expect_host.py::test_expectation_kernels_do_not_spill.  The counts are printed: DESIGN quotes them."""
    import __graft_entry__ as G
    kernel = (ROOT / "dynamicprogramming_amd" / "csrc" / "pi_expect_kernels.hip").read_text()
    for name, bins in (("pendulum", 200), ("cartpole_swingup", 50), ("double_cartpole", 25), ("double_cartpole_swingup", 25)):
        eng, dyn = G._engine_for(name, bins)
        text = eng.kernel_source(dyn) + "\n" + kernel + "\n"
        n_actions = eng.info(Info.N_ACTIONS)
        eng.close()
        usage = H.kernel_resource_usage(text, tmp_path, name)
        mine = {fn: k for fn, k in usage.items() if fn.startswith("pi_robust_")}
        assert set(mine) == KERNELS
        for fn, k in mine.items():
            print(f"{fn} {name} {bins}^{envs.ENVS[name]._D} x {n_actions}: {k}")
            assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, fn, k)


# ---- 9. runner flag ----------------------------------------------------------------------------------------------------
def test_train_risk_flag(tmp_path, capsys, monkeypatch):
    from runners import _cli
    args = _cli.build_parser("cartpole", "x.npz").parse_args([])
    assert args.train_risk == "expected" and not _cli.training_noise_requested(args) and _cli.ignored_flags(args) == []
    args = _cli.build_parser("cartpole", "x.npz").parse_args(["--train-risk", "worst", "--train-state-noise", "0.1"])
    assert args.train_risk == "worst" and _cli.training_noise_requested(args) and _cli.ignored_flags(args) == []
    with pytest.raises(SystemExit):
        _cli.build_parser("cartpole", "x.npz").parse_args(["--train-risk", "cvar"])
    capsys.readouterr()

    def make(env_name, bins=None, **kw):                              # the env on the CPU backend, a short run
        cls = envs.ENVS[env_name]
        cfg = CudaPIConfig(**{**cls.CONFIG, "max_pi_iter": 1, "max_eval_iter": 2})
        return with_robust_backend(cls)(H.env_bins_space(env_name, (12, 11)), cls.ACTIONS, cfg)

    monkeypatch.setattr(envs, "make", make)
    path = tmp_path / "robust.npz"
    common = ["--save-path", str(path), "--retrain", "--train-state-noise", "0.2", "0.3", "--train-noise-points", "2"]
    pi = _cli.main("pendulum", str(path), common + ["--train-risk", "worst"])
    out = capsys.readouterr().out
    assert "worst-case training: max-min backup over 4 disturbance points" in out and "expected backup" not in out
    assert pi.risk == "worst" and pi._backend.calls["robust_eval"] == 2 and pi._backend.calls["expect_eval"] == 0
    assert str(np.load(path)["risk"]) == "worst" and envs.ENVS["pendulum"].load(path).risk == "worst"
    pi = _cli.main("pendulum", str(path), common)
    assert "noise-aware training: expected backup over 4 disturbance points" in capsys.readouterr().out
    assert pi.risk == "expected" and pi._backend.calls["expect_eval"] == 2 and "risk" not in np.load(path).files


def test_train_risk_without_a_training_noise_says_that_it_had_no_effect(tmp_path, capsys, monkeypatch):
    from runners import _cli

    def make(env_name, bins=None, **kw):
        cls = envs.ENVS[env_name]
        cfg = CudaPIConfig(**{**cls.CONFIG, "max_pi_iter": 1, "max_eval_iter": 2})
        return with_robust_backend(cls)(H.env_bins_space(env_name, (12, 11)), cls.ACTIONS, cfg)

    monkeypatch.setattr(envs, "make", make)
    path = tmp_path / "plain.npz"
    pi = _cli.main("pendulum", str(path), ["--save-path", str(path), "--retrain", "--train-risk", "worst"])
    out = capsys.readouterr().out
    assert "--train-risk worst" in out and "had no effect" in out and "worst-case training" not in out
    assert pi.risk == "expected" and pi.disturbances is None and pi._backend.calls["eval"] == 2
    assert "risk" not in np.load(path).files and "disturbances" not in np.load(path).files


def test_load_refuses_a_risk_entry_it_does_not_know(tmp_path):
    s = _solver(NAME, SHAPE, _cfg(max_pi_iter=1, max_eval_iter=2))
    s.set_disturbances(_set(), risk="worst")
    s.run()
    s.save(tmp_path / "good")
    data = dict(np.load(tmp_path / "good.npz"))
    np.savez(tmp_path / "bad.npz", **{**data, "risk": np.array("cvar")})
    with pytest.raises(ValueError, match="risk"):
        envs.ENVS[NAME].load(tmp_path / "bad")
    np.savez(tmp_path / "orphan.npz", **{k: v for k, v in data.items() if k != "disturbances"})
    with pytest.raises(ValueError, match="risk"):
        envs.ENVS[NAME].load(tmp_path / "orphan")
    assert envs.ENVS[NAME].load(tmp_path / "good").risk == "worst"
