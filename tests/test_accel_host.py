"""
CPU: Anderson-accelerated policy evaluation — the numpy twin of dynamicprogramming_amd.accel (the fixed reduction tree,
the combine, the host solve), the loop and its restart rule, the solver wiring on the CPU backend of
tests/accel_backend.py, the refusals of the two entry points on host-only handles, the build of
csrc/pi_accel_kernels.hip for gfx950, symbols and the runner's flag.
"""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np
import pytest

from dynamicprogramming_amd import _native, accel, envs
from dynamicprogramming_amd.noise import Disturbances
from dynamicprogramming_amd.solver import SYNC_INTERVAL, CudaPIConfig, _CudaPolicyIterationBase
from tests import helpers as H
from tests.accel_backend import AccelSweepBackend, with_accel_backend

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("pi_accel_update", "pi_accel_combine")


# ---- 1. the arithmetic ----------------------------------------------------------------------------------------------------
def _dot_by_the_rule(a, b):
    """The rule of include/pi_mi355.h spelled out in Python floats, one addition at a time."""
    n = len(a)

    def tree(v):
        v = list(v)
        for w in range(4):
            o = 32
            while o:
                for lane in range(o):
                    v[64 * w + lane] = v[64 * w + lane] + v[64 * w + lane + o]
                o >>= 1
        return (v[0] + v[128]) + (v[64] + v[192])

    tiles = []
    for t0 in range(0, n, 4096):
        threads = [0.0] * 256
        for c in range(4):
            for t in range(256):
                for i in range(4):
                    e = t0 + 1024 * c + 4 * t + i
                    if e < n:
                        threads[t] = threads[t] + float(a[e]) * float(b[e])
        tiles.append(tree(threads))
    threads = [0.0] * 256
    for k, v in enumerate(tiles):
        threads[k % 256] = threads[k % 256] + v
    return tree(threads)


def test_dot_follows_the_fixed_tree_on_a_hand_computed_case():
    """Three tiles whose products are 1e16 and 1 (thread 0 of tile 0), -1e16 (tile 1) and 1 (tile 2).  By the rule the first 1
    is absorbed inside thread 0 (1e16 + 1 = 1e16 in float64), the fold's lanes 0 and 2 add to 1e16 + 1 = 1e16 and lanes 0
    and 1 to 0: exactly 0.0, where the true sum is 2 and a left-to-right sum gives 1."""
    a, b = np.zeros(2 * 4096 + 5, np.float32), np.zeros(2 * 4096 + 5, np.float32)
    a[[0, 1, 4096, 8192]] = [1e8, 1.0, -1e8, 1.0]
    b[[0, 1, 4096, 8192]] = [1e8, 1.0, 1e8, 1.0]
    assert math.fsum(float(x) * float(y) for x, y in zip(a, b)) == 2.0
    assert accel.dot(a, b) == 0.0 == _dot_by_the_rule(a, b)
    # the second 1 in another thread of tile 0 survives the thread sum and is absorbed in the wave tree instead
    a[1], b[1], a[4], b[4] = 0.0, 0.0, 1.0, 1.0
    assert accel.dot(a, b) == 0.0 == _dot_by_the_rule(a, b)
    # ... and in tile 2 next to the other: 1 + 1 = 2 is representable beside 1e16
    a[4], b[4], a[8193], b[8193] = 0.0, 0.0, 1.0, 1.0
    assert accel.dot(a, b) == 2.0 == _dot_by_the_rule(a, b)


@pytest.mark.parametrize("n", [1, 255, 4097, 3 * 4096 + 5, 257 * 4096 + 3])
def test_dot_against_the_rule_and_fsum(n):
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    got = accel.dot(a, b)
    if n <= 3 * 4096 + 5:
        assert got == _dot_by_the_rule(a, b)                     # bit for bit
    # float64 products of float32 factors are exact (48 bits); every element passes through at most
    # 16 (thread) + 8 (tree) + ceil(tiles / 256) (fold) + 8 (tree) additions of relative error 2^-53 each
    prods = a.astype(np.float64) * b.astype(np.float64)
    depth = 16 + 8 + -(-(-(-n // 4096)) // 256) + 8
    assert abs(got - math.fsum(prods)) <= depth * 2.0 ** -53 * math.fsum(np.abs(prods)) * (1 + 1e-12)


def test_dots_is_the_update_of_the_ring():
    rng = np.random.default_rng(1)
    n, m = 5000, 3
    x, g, fp, gp = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    dF, dG = (rng.standard_normal((m, n)).astype(np.float32) for _ in range(2))
    keep = dF.copy(), dG.copy()
    out = accel.dots(x, g, fp, gp, dF, dG, 0, 0, True)           # first push: only (f_prev, g_prev) and f . f
    f = g - x
    assert out.shape == (1,) and out[0] == accel.dot(f, f)
    H.assert_bits_equal(fp, f, "f_prev")
    H.assert_bits_equal(gp, g, "g_prev")
    assert np.array_equal(dF, keep[0]) and np.array_equal(dG, keep[1])
    fp0, gp0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    fp[...], gp[...] = fp0, gp0
    out = accel.dots(x, g, fp, gp, dF, dG, 1, 3, False)
    H.assert_bits_equal(dF[1], f - fp0, "new column of dF")
    H.assert_bits_equal(dG[1], g - gp0, "new column of dG")
    assert np.array_equal(dF[[0, 2]], keep[0][[0, 2]]) and np.array_equal(dG[[0, 2]], keep[1][[0, 2]])
    want = [accel.dot(dF[j], f) for j in range(3)] + [accel.dot(dF[j], dF[1]) for j in range(3)] + [accel.dot(f, f)]
    assert out.tolist() == want
    for bad in (dict(slot=3, k_used=3, first=False), dict(slot=0, k_used=4, first=False), dict(slot=0, k_used=1, first=True),
                dict(slot=2, k_used=2, first=False), dict(slot=0, k_used=0, first=False)):
        with pytest.raises(ValueError):
            accel.dots(x, g, fp, gp, dF, dG, **bad)


def test_combine_with_zero_columns_returns_the_bits_of_g():
    g = np.float32([-0.0, 0.0, 1.5, -3.25e-40, np.float32(np.pi), -7.0])
    dG = np.zeros((3, len(g)), np.float32)
    dG[1, 1] = -0.0
    for coeffs in ([1.0, 2.0, 3.0], [-1.0, -2.5, 1e300], [0.0, -0.0, -1e-300]):
        out = accel.combine(g, dG, coeffs, 3)
        H.assert_bits_equal(out, g, f"combine with zero columns, coefficients {coeffs}")
    assert np.signbit(accel.combine(g, dG, [-1.0, -1.0, -1.0], 3)[0])
    # ... and with columns it is one rounding of the float64 expression; out may be g
    rng = np.random.default_rng(0)
    g, dG = rng.standard_normal(1000).astype(np.float32), rng.standard_normal((2, 1000)).astype(np.float32)
    want = (g.astype(np.float64) - ((0.0 + 0.25 * dG[0].astype(np.float64)) + -1.75 * dG[1].astype(np.float64))).astype(np.float32)
    H.assert_bits_equal(accel.combine(g, dG, [0.25, -1.75], 2), want, "combine")
    accel.combine(g, dG, [0.25, -1.75], 2, out=g)
    H.assert_bits_equal(g, want, "combine in place")
    with pytest.raises(ValueError, match="not finite"):
        accel.combine(g, dG, [0.25, float("nan")], 2)


def test_solve_a_hand_made_system_and_report_failure():
    c = accel.solve([[4.0, 2.0], [2.0, 3.0]], [2.0, 1.0])        # 4 * 0.5 + 2 * 0 = 2, 2 * 0.5 + 3 * 0 = 1
    assert abs(c[0] - 0.5) < 1e-10 and abs(c[1]) < 1e-10        # lambda = 7e-12 moves it by that much
    assert abs(accel.solve([[2.0]], [3.0])[0] - 3.0 / (2.0 + 2e-12)) < 1e-15       # sqrt twice: a few ulps
    # a Gram matrix of zero columns is singular whatever lambda = 1e-12 * trace adds; so is one that is not positive
    assert accel.solve([[0.0, 0.0], [0.0, 0.0]], [0.0, 0.0]) is None
    assert accel.solve([[0.0]], [1.0]) is None
    assert accel.solve([[1.0, 2.0], [2.0, 1.0]], [1.0, 1.0]) is None
    assert accel.solve([[-1.0]], [1.0]) is None
    assert accel.solve([[float("nan")]], [1.0]) is None and accel.solve([[1.0]], [float("inf")]) is None
    assert accel.solve([[float("inf")]], [1.0]) is None


def test_settings_are_validated():
    assert accel.Anderson().window == 4 and accel.Anderson().restart == 2.0
    for bad in (dict(window=0), dict(window=9), dict(window=2.5), dict(restart=0.0), dict(restart=float("nan"))):
        with pytest.raises(ValueError):
            accel.Anderson(**bad)


# ---- 2. the loop ----------------------------------------------------------------------------------------------------------
def _contraction(seed=0, n=64, gamma=0.99):
    rng = np.random.default_rng(seed)
    P = rng.random((n, n))
    P /= P.sum(axis=1, keepdims=True)
    r = rng.random(n).astype(np.float32).astype(np.float64)
    exact = np.linalg.solve(np.eye(n) - gamma * P, r)

    def sweep_batch(V, count):
        delta = float("inf")
        for _ in range(count):
            new = (r + gamma * (P @ V.astype(np.float64))).astype(np.float32)        # one rounding per sweep
            delta = float(np.abs(new - V).max())
            V[...] = new
        return delta
    return sweep_batch, exact, n, gamma


@pytest.mark.parametrize("window", [1, 4, 8])
def test_linear_contraction_ends_within_the_bound_in_fewer_sweeps(window):
    sweep_batch, exact, n, gamma = _contraction()
    theta = 1e-4
    plain, plain_sweeps, e0, r0 = accel.accelerated_evaluation(sweep_batch, np.zeros(n, np.float32), theta, 10_000, None)
    V, sweeps, extrapolations, restarts = accel.accelerated_evaluation(sweep_batch, np.zeros(n, np.float32), theta, 10_000,
                                                                       accel.Anderson(window=window))
    bound = gamma * theta / (1 - gamma)
    print(f"window {window}: {sweeps} sweeps ({extrapolations} extrapolations, {restarts} restarts) against {plain_sweeps}; "
          f"error {np.abs(V - exact).max():.3e} (plain {np.abs(plain - exact).max():.3e}), bound {bound:.3e}")
    assert (e0, r0) == (0, 0) and np.abs(plain - exact).max() < bound
    assert np.abs(V - exact).max() < bound
    assert sweeps < plain_sweeps and extrapolations >= 1
    assert sweeps % SYNC_INTERVAL == 1                            # the schedule 1, 25, 25, .. of the plain loop


class ScriptedOps:
    """`evaluate` against a script of residuals: records every call, answers benign dot products."""

    def __init__(self, deltas):
        self.deltas, self.log, self.pending = list(deltas), [], 0

    def snapshot(self):
        self.log.append("snapshot")

    def sweeps(self, n):
        self.log.append(("sweeps", n))

    def update(self, slot, k_used, first):
        self.log.append(("update", slot, k_used, first))

    def read(self, count):
        return self.deltas.pop(0), [0.5] * (count // 2) + [1.0] * (count // 2) + [1.0] * (count % 2)

    def combine(self, coeffs, k_used):
        self.log.append(("combine", k_used))


def test_a_batch_whose_residual_grows_clears_the_history():
    # batches: 1 sweep | first full | push, extrapolate | grows by more than kappa = 2: restart | first again | push | ends
    ops = ScriptedOps([1.0, 0.5, 0.4, 0.81, 0.7, 0.6, 1e-9])
    delta, sweeps, extrapolations, restarts, converged = accel.evaluate(ops, 1e-4, 10_000, accel.Anderson(window=2), SYNC_INTERVAL)
    assert (sweeps, extrapolations, restarts, converged) == (1 + 6 * 25, 2, 1, True) and delta == 1e-9
    updates = [e for e in ops.log if e[0] == "update"]
    assert updates == [("update", 0, 0, True), ("update", 0, 1, False), ("update", 1, 2, False), ("update", 0, 0, True),
                       ("update", 0, 1, False), ("update", 1, 2, False)]
    assert [e for e in ops.log if e[0] == "combine"] == [("combine", 1), ("combine", 1)]
    assert ops.log[:2] == [("sweeps", 1), "snapshot"]             # the one-sweep batch takes no part
    # exactly kappa times the previous residual is not a restart; the ring wraps at the window
    ops = ScriptedOps([1.0, 0.5, 0.4, 0.8, 0.7, 0.6, 1e-9])
    assert accel.evaluate(ops, 1e-4, 10_000, accel.Anderson(window=2), SYNC_INTERVAL)[2:4] == (4, 0)
    assert [e for e in ops.log if e[0] == "update"][3:] == [("update", 0, 2, False), ("update", 1, 2, False), ("update", 0, 2, False)]


def test_three_restarts_switch_the_acceleration_off():
    ops = ScriptedOps([1.0, 0.1, 1.0, 0.1, 1.0, 0.1, 1.0, 0.9, 0.8, 0.7])
    delta, sweeps, extrapolations, restarts, converged = accel.evaluate(ops, 1e-4, 1 + 9 * 25, accel.Anderson(), SYNC_INTERVAL)
    assert (sweeps, extrapolations, restarts, converged) == (226, 0, 3, False)
    assert ops.log.count("snapshot") == 6 and len([e for e in ops.log if e[0] == "update"]) == 6
    assert ops.log[-3:] == [("sweeps", 25)] * 3                   # plain from the third restart on
    # a truncated last batch takes no part either
    ops = ScriptedOps([1.0, 0.5, 0.4])
    assert accel.evaluate(ops, 1e-4, 40, accel.Anderson(), SYNC_INTERVAL)[1] == 40
    assert ops.log == [("sweeps", 1), "snapshot", ("sweeps", 25), ("update", 0, 0, True), ("sweeps", 14)]


def test_nan_in_v_gives_restarts_not_an_exception():
    sweep_batch, _, n, _ = _contraction()
    V0 = np.zeros(n, np.float32)
    V0[3] = np.nan
    V, sweeps, extrapolations, restarts = accel.accelerated_evaluation(sweep_batch, V0, 1e-4, 301, accel.Anderson())
    assert (sweeps, extrapolations, restarts) == (301, 0, accel.MAX_RESTARTS) and np.isnan(V).all()


# ---- 3. the solver on the CPU backend ---------------------------------------------------------------------------------
# two of the grids of profiles/r17/accelerated_evaluation.txt where the CPU table shows a clear win at the default window
GRIDS = {"pendulum": (50, 50), "cartpole_swingup": (9, 7, 11, 5)}


def _solver(name, shape=None, **cfg):
    cls = envs.ENVS[name]
    config = CudaPIConfig(**{**cls.CONFIG, **cfg})
    return with_accel_backend(cls)(H.env_bins_space(name, shape or GRIDS[name]), cls.ACTIONS, config)


_RUNS = {}


def _runs(name):
    """(plain, accelerated) solvers after run(), computed once per grid."""
    if name not in _RUNS:
        plain, fast = _solver(name), _solver(name)
        fast.set_acceleration(accel.Anderson())
        plain.run()
        fast.run()
        _RUNS[name] = (plain, fast)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(GRIDS))
def test_policy_evaluation_of_a_fixed_policy_within_the_bound_in_fewer_sweeps(name):
    plain, fast = _solver(name), _solver(name)
    for s in (plain, fast):
        s.policy_improvement()                                   # the greedy policy of V = 0, then fixed
    fast.set_acceleration(accel.Anderson())
    assert isinstance(fast._backend, AccelSweepBackend) and fast._accel_buffers is None
    d_plain, d_fast = plain.policy_evaluation(), fast.policy_evaluation()
    cfg = plain.config
    assert d_plain < cfg.theta and d_fast < cfg.theta
    bound = 2 * cfg.theta * cfg.gamma / (1 - cfg.gamma)
    gap = float((fast.d_value_function - plain.d_value_function).abs().max())
    print(f"{name}: {fast.stats['eval_sweeps']} sweeps against {plain.stats['eval_sweeps']}, max|dV| {gap:.3e}, bound {bound:.3e}, "
          f"{fast.stats['accel_extrapolations']} extrapolations, {fast.stats['accel_restarts']} restarts")
    assert gap < bound
    assert fast.stats["eval_sweeps"] < plain.stats["eval_sweeps"]
    assert fast.stats["sweeps_per_iter"] == [fast.stats["eval_sweeps"]] and fast.stats["eval_sweeps"] % SYNC_INTERVAL == 1
    assert fast.stats["accel_extrapolations"] == fast._backend.calls["accel_combine"] >= 1
    assert fast.stats["accel_per_iter"] == [(fast.stats["accel_extrapolations"], fast.stats["accel_restarts"])]
    assert fast._backend.calls["eval"] == fast.stats["eval_sweeps"] and plain._backend.calls["accel_update"] == 0
    n, m = fast.n_states, 4
    assert sum(t.numel() for k, t in fast._accel_buffers.items() if k != "dots") == (2 * m + 3) * n
    fast.set_acceleration(None)
    assert fast._accel_buffers is None and fast.acceleration is None


@pytest.mark.parametrize("name", list(GRIDS))
def test_run_converges_stable_with_fewer_sweeps(name):
    plain, fast = _runs(name)
    assert plain.stats["stable"] is True and fast.stats["stable"] is True
    assert fast.stats["eval_sweeps"] < plain.stats["eval_sweeps"]
    assert sum(fast.stats["sweeps_per_iter"]) == fast.stats["eval_sweeps"]
    assert len(fast.stats["accel_per_iter"]) == fast.stats["pi_iterations"]
    assert "accel_extrapolations" not in plain.stats
    cfg = plain.config
    assert np.abs(fast.value_function - plain.value_function).max() < 2 * cfg.theta * cfg.gamma / (1 - cfg.gamma)


def test_the_one_launch_shortcuts_and_the_bracket_are_not_taken():
    s = _solver("pendulum", (12, 11), max_pi_iter=2, max_eval_iter=60, theta=0.0)
    s.set_acceleration(accel.Anderson(window=2))
    s._backend.resident = True                                    # a backend that offers the one-launch shortcuts ...
    s._backend.whole_run = True
    s._backend.policy_evaluation = s._backend.policy_iteration = s._backend.eval_begin = None   # ... which must not be called
    s.run()
    assert s.stats["sweeps_per_iter"] == [60, 60] and s._backend.calls["accel_update"] == 4     # batches 1, 25, 25, 9


def test_set_acceleration_none_restores_the_plain_counts_and_bits():
    plain, _ = _runs("pendulum")
    back = _solver("pendulum")
    back.set_acceleration(accel.Anderson(window=8))
    back.policy_evaluation()
    assert back._backend.calls["accel_update"] > 0
    fresh = _solver("pendulum")
    fresh.set_acceleration(accel.Anderson())
    fresh.set_acceleration(None)
    fresh.run()
    assert fresh._backend.calls["accel_update"] == 0 and fresh._backend.calls["accel_combine"] == 0
    assert fresh.stats["sweeps_per_iter"] == plain.stats["sweeps_per_iter"]
    H.assert_bits_equal(fresh.value_function, plain.value_function, "V after set_acceleration(None)")
    assert np.array_equal(fresh.policy, plain.policy)


def test_expected_backup_is_accelerated_and_the_worst_case_is_refused_in_both_orders():
    name, shape = "pendulum", (12, 11)
    d = Disturbances.uniform(2, state_noise=[0.2, 0.3], action_noise=0.5, points=2)
    s = _solver(name, shape, max_pi_iter=1)
    s.set_disturbances(d)
    s.set_acceleration(accel.Anderson())
    s.run()
    assert s._backend.calls["expect_eval"] == s.stats["eval_sweeps"] and s._backend.calls["eval"] == 0
    assert s.stats["accel_extrapolations"] >= 1
    a = _solver(name, shape)
    a.set_acceleration(accel.Anderson())
    with pytest.raises(NotImplementedError, match="worst"):
        a.set_disturbances(d, risk="worst")
    assert a.disturbances is None and a.risk == "expected"
    a.set_disturbances(d)                                         # the expectation is fine
    b = _solver(name, shape)
    b.set_disturbances(d, risk="worst")
    with pytest.raises(NotImplementedError, match="worst"):
        b.set_acceleration(accel.Anderson())
    assert b.acceleration is None
    b.set_acceleration(None)
    with pytest.raises(TypeError):
        b.set_acceleration(4)


def test_sharded_solvers_refuse_and_subclasses_keep_their_own_evaluation():
    sharded = object.__new__(envs.PendulumCuda)
    sharded._comm, sharded.stats = object(), {}
    with pytest.raises(NotImplementedError, match="sharded"):
        sharded.set_acceleration(accel.Anderson())
    sharded.set_acceleration(None)

    calls = []

    class Own(envs.PendulumCuda):
        def policy_evaluation(self):
            calls.append("own")
            return 0.0
    s = with_accel_backend(Own)(H.env_bins_space("pendulum", (12, 11)), Own.ACTIONS, CudaPIConfig(max_pi_iter=2))
    s.set_acceleration(accel.Anderson())
    s.run()
    assert calls == ["own"] * s.stats["pi_iterations"] and s._backend.calls["accel_update"] == 0
    assert callable(_CudaPolicyIterationBase.set_acceleration)


# ---- 4. the C ABI on host-only handles ----------------------------------------------------------------------------------
def test_refusals_of_the_two_entry_points(tmp_path):
    """Every refusal is an error with its reason before anything could be launched: this handle has no device.  The
    pointers are never dereferenced."""
    eng = H.host_engine("pendulum", (24, 17))
    eng.compile(envs.dynamics_source("pendulum"), cache_dir=tmp_path)
    n, m = 1000, 4
    base = 1 << 20
    x, g, fp, gp, dF, dG, dots = (base + i * (1 << 16) for i in range(7))
    good = dict(x=x, g=g, f_prev=fp, g_prev=gp, dF=dF, dG=dG, m=m, slot=1, k_used=2, first=False, n=n, d_dots=dots)
    for key in ("x", "g", "f_prev", "g_prev", "dF", "dG", "d_dots"):
        with pytest.raises(_native.NativeError, match="null pointer"):
            eng.accel_update(**{**good, key: 0})
    for bad, why in ((dict(n=0), "n <= 0"), (dict(n=-5), "n <= 0"), (dict(m=0), r"window m must be in \[1, 8\]"),
                     (dict(m=9), r"window m"), (dict(k_used=-1), "k_used must be in"), (dict(k_used=9, m=8), "k_used must be in"),
                     (dict(k_used=5), "k_used must be in"), (dict(slot=4), "slot >= m"), (dict(slot=-1), "slot >= m"),
                     (dict(slot=2), "slot < k_used"), (dict(first=True), "first push takes k_used = 0"),
                     (dict(k_used=0), "k_used >= 1"), (dict(g=x), "must not overlap"), (dict(f_prev=x + 4 * (n - 1)), "must not overlap"),
                     (dict(dG=dF + 4 * n * (m - 1)), "must not overlap"), (dict(g_prev=dG + 4 * (m * n - 1)), "must not overlap")):
        with pytest.raises(_native.NativeError, match=why):
            eng.accel_update(**{**good, **bad})
    eng.accel_update(**good)                                      # in order: the checks and the build, no launch
    eng.accel_update(**{**good, "slot": 0, "k_used": 0, "first": True})
    eng.accel_update(**{**good, "f_prev": x + 4 * n})             # adjacent is not overlapping
    cgood = dict(g=g, dG=dG, coeffs=[0.5, -0.25], k_used=2, n=n, out=g)
    for key in ("g", "dG", "out"):
        with pytest.raises(_native.NativeError, match="null pointer"):
            eng.accel_combine(**{**cgood, key: 0})
    for bad, why in ((dict(n=0), "n <= 0"), (dict(k_used=-1), "k_used must be in"), (dict(k_used=9, coeffs=[0.0] * 9), "k_used must be in"),
                     (dict(coeffs=[0.5, float("nan")]), "coefficient 1 is not finite"),
                     (dict(coeffs=[float("inf"), 0.0]), "coefficient 0 is not finite"),
                     (dict(out=g + 4), "must not overlap"), (dict(out=dG + 4 * n), "must not overlap"), (dict(dG=g + 8), "must not overlap")):
        with pytest.raises(_native.NativeError, match=why):
            eng.accel_combine(**{**cgood, **bad})
    eng.accel_combine(**cgood)                                    # out == g is allowed
    eng.accel_combine(**{**cgood, "out": x})
    eng.accel_combine(**{**cgood, "k_used": 0, "coeffs": []})
    eng.close()


def test_new_symbols_are_declared_commented_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    lib = _native.lib()
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(pi_handle\* h,", header, re.M), sym
        assert header.count(sym) >= 2, f"{sym} has no comment in the header"
        assert hasattr(lib, sym) and sym in _native.SIGNATURES
    for method in ("accel_update", "accel_combine"):
        assert callable(getattr(_native.Engine, method))
    from dynamicprogramming_amd.solver import HipSweepBackend
    assert callable(HipSweepBackend.accel_update) and callable(HipSweepBackend.accel_combine)
    csrc = ROOT / "dynamicprogramming_amd" / "csrc"
    assert "pi_accel.cpp" in (csrc / "Makefile").read_text()
    assert "pi_accel.cpp" in (csrc / "pi_internal.h").read_text().split("#pragma once")[0]
    assert lib.pi_abi_version() == _native.ABI_VERSION
    # the reduction rule is written down where the ABI is
    for phrase in ("4 096", "(w0 + w2) + (w1 + w3)", "o = 32, 16, 8, 4, 2, 1"):
        assert phrase in header
    text = (ROOT / "dynamicprogramming_amd" / "accel.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(oracle|tests|torch)\b", text, re.M)


def test_module_builds_for_gfx950_once_for_every_handle_and_does_not_spill(tmp_path):
    """The acceleration module is one more object in the handle's cache, the same one for every grid and env (it is not
    specialised), built by the first call and by nothing before it; no private segment, the register counts are printed."""
    fake = dict(x=1 << 20, g=2 << 20, f_prev=3 << 20, g_prev=4 << 20, dF=5 << 20, dG=6 << 20, m=2, slot=0, k_used=0, first=True,
                n=100, d_dots=7 << 20)
    eng = H.host_engine("pendulum", (24, 17))
    eng.compile(envs.dynamics_source("pendulum"), cache_dir=tmp_path)
    first = sorted(tmp_path.glob("pi_*.hsaco"))
    assert len(first) == 1
    eng.accel_update(**fake)
    both = sorted(tmp_path.glob("pi_*.hsaco"))
    assert len(both) == 2 and set(first) < set(both)
    new = (set(both) - set(first)).pop()
    assert new.stat().st_size > 4096 and new.read_bytes()[:4] == b"\x7fELF"
    stamp = new.stat().st_mtime_ns
    eng.accel_combine(g=1 << 20, dG=2 << 20, coeffs=[1.0], k_used=1, n=10, out=1 << 20)
    eng.close()
    other = H.host_engine("cartpole_swingup", (9, 7, 11, 5))
    other.compile(envs.dynamics_source("cartpole_swingup"), cache_dir=tmp_path)
    other.accel_update(**fake)
    other.close()
    assert len(sorted(tmp_path.glob("pi_*.hsaco"))) == 3 and new.stat().st_mtime_ns == stamp
    usage = H.kernel_resource_usage((ROOT / "dynamicprogramming_amd" / "csrc" / "pi_accel_kernels.hip").read_text(), tmp_path, "accel")
    assert set(usage) == {"pi_accel_update_kernel", "pi_accel_update_vec_kernel", "pi_accel_fold_kernel",
                          "pi_accel_combine_kernel", "pi_accel_combine_vec_kernel"}
    for fn, k in usage.items():
        print(f"{fn}: {k}")
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (fn, k)
    # the sweep unit does not hold them: kernel_source_hash and the committed profiles stay valid
    assert "pi_accel" not in H.host_engine("pendulum", (24, 17)).kernel_source(envs.dynamics_source("pendulum"))


# ---- 5. the runner flag ---------------------------------------------------------------------------------------------------
def test_accelerate_flag_parses_and_reaches_train():
    import inspect
    from runners import _cli
    p = _cli.build_parser("pendulum", "results/pendulum_cuda_policy.npz")
    assert p.parse_args([]).accelerate is None
    assert p.parse_args(["--accelerate"]).accelerate == 4
    a = p.parse_args(["--accelerate", "8", "--bins", "50", "--retrain"])
    assert a.accelerate == 8 and a.bins == 50 and _cli.ignored_flags(a) == []
    with pytest.raises(SystemExit):
        p.parse_args(["--accelerate", "9"])
    assert inspect.signature(_cli.train).parameters["accelerate"].default is None
    assert "--accelerate" in (ROOT / "INTEGRATION.md").read_text()
