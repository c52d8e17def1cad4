"""
GPU: the robust lookahead and the adversary rollout (csrc/pi_adversary_kernels.hip through DevicePolicy.set_robust /
robust / adversary_rollout) against their numpy twins (dynamicprogramming_amd.noise.robust_action / adversary_rollout on
the checker's step), bit for bit, `worst` and trajectories included.  Grids, value functions and query points are those of
tests/expect_greedy_cases.py.  Every GPU step runs once; nothing retries.
"""
from __future__ import annotations

import numpy as np
import pytest

import utils.barycentric as B
from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd.noise import Disturbances
from tests import expect_greedy_cases as C
from tests import helpers as H
from tests.robust_cases import zero_weight_sets
from tests.test_gpu_expect import _make_set

pytestmark = pytest.mark.gpu

CASES = {name: C.case(name, shape) for name, shape in C.GRIDS}


def _policy(c):
    rng = np.random.default_rng(9)
    return rng.integers(0, len(c["acts"]), size=len(c["states"])).astype(np.int32)


def _sets(c):
    lo, hi, gshape, _ = c["grid"]
    cell = (hi.astype(np.float64) - lo.astype(np.float64)) / (np.asarray(gshape, np.float64) - 1)
    s3 = _make_set("S3", c["D"], cell, c["acts"])
    return {"multi": C.multi_point_set(c["name"]), "zero": Disturbances.none(c["D"]), "K64": s3,
            "zero-weight": zero_weight_sets(s3)[0]}


def _dp(c, dev, policy=True):
    dp = B.DevicePolicy(_policy(c) if policy else None, c["acts"], *c["grid"], c["bits"], device=dev)
    dp.set_values(c["V"])
    dp.set_dynamics(envs.dynamics_source(c["name"]))
    assert isinstance(dp.set_robust(), str)
    return dp


def _assert_query(got, want, what):
    got = [x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in got]
    assert len(got) == len(want)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), f"{what}: best"
    H.assert_bits_equal(got[1], want[1], f"{what}: action value")
    H.assert_bits_equal(got[2], want[2], f"{what}: best Q")
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]), f"{what}: worst"
    if len(want) == 5:
        H.assert_bits_equal(got[4], want[4], f"{what}: Q")


def _points(c, m, seed=1):
    """m of the 257 points of C.query_points (which needs room for its special rows), spread over them; all of them keep the
    far-outside row (index 128) and, when m > 3, the one with a NaN coordinate."""
    pts = C.query_points(c, 257, seed=seed)
    pick = pts[np.unique(np.r_[np.linspace(0, 256, m).astype(int), 128])[:m]] if m < 257 else pts
    if 3 < m < 257:
        pick[m - 2] = pts[255]
    return np.ascontiguousarray(pick)


def _same_rollout(a, b, starts, what):
    """C.assert_same_rollout, bit for bit, for every episode — except that in the episodes that START on a NaN coordinate
    (one per batch of more than 3) every NaN is replaced by ONE NaN first: such an episode carries NaNs through the plugin,
    and IEEE 754 pins neither the sign nor the payload of a NaN an operation produces.  Where its NaNs are is compared,
    which bits they have is not; its other values, and every other episode, are compared bit for bit."""
    from_nan = np.isnan(np.asarray(starts)).any(axis=1)

    def canon(r):
        def one(x, axis):
            if x is None:
                return None
            x = np.array(x.cpu().numpy() if hasattr(x, "cpu") else x)
            if x.dtype == np.float32 and from_nan.any():
                rows = x[from_nan] if axis == 0 else x[:, from_nan]
                rows = np.where(np.isnan(rows), np.float32(np.nan), rows).astype(np.float32)
                if axis == 0:
                    x[from_nan] = rows
                else:
                    x[:, from_nan] = rows
            return x
        return B.RolloutResult(one(r.states, 0), one(r.returns, 0), one(r.lengths, 0), one(r.terminated, 0), one(r.trajectory, 1))
    C.assert_same_rollout(canon(a), canon(b), what)


def _tables(c, V=None):
    return (c["V"] if V is None else V, c["acts"], *c["grid"])


@pytest.mark.parametrize("name", C.IDS)
def test_query_equals_the_twin(name, cuda_device):
    c = CASES[name]
    dp = _dp(c, cuda_device, policy=False)
    for label, d in _sets(c).items():
        dp.set_disturbances(d)                         # an upload between launches, never a rebuild
        for m in (1, 63, 64, 65, 257):
            pts = _points(c, m)
            want = noise.robust_action(c["chk"].step, pts, d, *_tables(c), c["gamma"], q_values=True)
            _assert_query(dp.robust(pts, c["gamma"], q_values=True), want, f"{name} {label} m={m}")
        if label == "multi":
            _assert_query(dp.robust(pts, c["gamma"]), want[:4], f"{name} without Q")
            assert (want[3] >= 0).any()
    # no winner: an all-NaN V gives best = 0, worst = -1
    dp.set_values(np.full_like(c["V"], np.nan))
    pts = _points(c, 65)
    got = dp.robust(pts, c["gamma"])
    want = noise.robust_action(c["chk"].step, pts, d, *_tables(c, np.full_like(c["V"], np.nan)), c["gamma"])
    live = np.isnan(want[2]) | (want[2] == np.float32(-1.0e30))
    _assert_query(got, want, f"{name} all-NaN V")
    nothing = want[2] == np.float32(-1.0e30)
    assert nothing.any() and (want[0][nothing] == 0).all() and (want[3][nothing] == -1).all() and live.any()
    dp.close()


@pytest.mark.parametrize("controller", ["policy", "robust"])
@pytest.mark.parametrize("name", C.IDS)
def test_rollout_equals_the_twin(name, controller, cuda_device):
    c = CASES[name]
    dp = _dp(c, cuda_device)
    policy = (_policy(c), c["acts"], *c["grid"], c["bits"])
    sets = _sets(c)
    runs = [("multi", m, 7, 3) for m in (1, 63, 64, 65, 257)] + [("multi", 65, 0, 0), ("multi", 65, 1, 1), ("multi", 65, 7, 0),
                                                                  ("multi", 65, 7, 1), ("K64", 65, 7, 3), ("zero-weight", 65, 7, 3)]
    for label, m, steps, every in runs:
        d = sets[label]
        dp.set_disturbances(d)
        starts = _points(c, m, seed=3)
        want = noise.adversary_rollout(c["chk"].step, starts, steps, d, *_tables(c), controller=controller, policy=policy,
                                       gamma=0.97, lookahead_gamma=c["gamma"], record_every=every)
        got = dp.adversary_rollout(starts, steps, gamma=0.97, record_every=every, controller=controller,
                                   lookahead_gamma=c["gamma"])
        _same_rollout(got, want, starts, f"{name} {controller} {label} m={m} steps={steps} every={every}")
    # the zero set: the adversary has one answer, and the rollouts are the deterministic ones
    dp.set_disturbances(sets["zero"])
    starts = _points(c, 65, seed=3)
    got = dp.adversary_rollout(starts, 7, gamma=0.97, record_every=1, controller=controller, lookahead_gamma=c["gamma"])
    if controller == "policy":
        same = dp.rollout(starts, 7, gamma=0.97, record_every=1)
    else:
        dp.set_greedy()
        same = dp.rollout(starts, 7, gamma=0.97, record_every=1, controller="greedy", lookahead_gamma=c["gamma"])
    _same_rollout(got, same, starts, f"{name} {controller} zero set")
    # no winner: the step of action 0 (its own worst point), as the twin takes it
    if controller == "robust":
        nan_V = np.full_like(c["V"], np.nan)
        dp.set_values(nan_V)
        dp.set_disturbances(sets["multi"])
        want = noise.adversary_rollout(c["chk"].step, starts, 3, sets["multi"], *_tables(c, nan_V), controller="robust",
                                       gamma=0.97, lookahead_gamma=c["gamma"], record_every=1)
        got = dp.adversary_rollout(starts, 3, gamma=0.97, record_every=1, controller="robust", lookahead_gamma=c["gamma"])
        _same_rollout(got, want, starts, f"{name} all-NaN V")
    dp.close()


def test_refusals_in_order(cuda_device):
    c = CASES["pendulum"]
    dp = B.DevicePolicy(None, c["acts"], *c["grid"], c["bits"], device=cuda_device)
    dp.set_values(c["V"])
    dp.set_dynamics(envs.dynamics_source("pendulum"))
    pts = C.query_points(c, 5)
    with pytest.raises(RuntimeError, match="set_robust"):
        dp.robust(pts, 0.9)
    eng = dp._engine
    with pytest.raises(_native.NativeError, match="pi_infer_set_robust"):          # the module first ...
        eng.robust(8, 5, 0.9, d_best=8)
    dp.set_robust()
    with pytest.raises(_native.NativeError, match="pi_infer_set_disturbances"):    # ... then the set
        eng.rollout_adversary(8, 5, 3, 0.9, 1, d_final=8)
    with pytest.raises(RuntimeError, match="set_disturbances"):
        dp.adversary_rollout(pts, 3, controller="robust", lookahead_gamma=0.9)
    dp.set_disturbances(Disturbances.none(2))
    for args, msg in (((8, 5, 3, float("nan"), 1), "lookahead_gamma is NaN"), ((8, 5, 3, 0.9, 2), "controller must be"),
                      ((8, 5, 3, 0.9, 0), "needs a policy")):
        with pytest.raises(_native.NativeError, match=msg):
            eng.rollout_adversary(*args, d_final=8)
    with pytest.raises(_native.NativeError, match="gamma is NaN"):
        eng.rollout_adversary(8, 5, 3, 0.9, 1, gamma=float("nan"), d_final=8)
    with pytest.raises(_native.NativeError, match="gamma is NaN"):
        eng.robust(8, 5, float("nan"), d_best=8)
    with pytest.raises(_native.NativeError, match="all five outputs"):
        eng.robust(8, 5, 0.9)
    with pytest.raises(RuntimeError, match="without a policy"):
        dp.adversary_rollout(pts, 3, controller="policy", lookahead_gamma=0.9)
    with pytest.raises(ValueError, match="controller"):
        dp.adversary_rollout(pts, 3, controller="greedy", lookahead_gamma=0.9)
    dp.set_dynamics(envs.dynamics_source("pendulum"))                             # drops the module
    with pytest.raises(RuntimeError, match="set_robust"):
        dp.robust(pts, 0.9)
    with pytest.raises(_native.NativeError, match="pi_infer_set_robust"):
        eng.robust(8, 5, 0.9, d_best=8)
    dp.close()


def test_solver_and_runner_run_the_adversary(cuda_device, tmp_path, capsys):
    """solver.adversary_rollout finds its set and arrays as rollout(controller="expected") does and equals the rollout set up
    by hand; --rollout --adversary prints rollout's lines."""
    from runners import _cli
    dist = Disturbances.uniform(2, state_noise=[0.0, 0.3], action_noise=0.4, points=2)
    solver = envs.make("pendulum", 25)
    solver.set_disturbances(dist, risk="worst")
    solver.run()
    starts = envs.ENVS["pendulum"].start_states(np.random.default_rng(5), 300)
    for controller in ("policy", "robust"):
        got = solver.adversary_rollout(starts, 60, controller=controller, gamma=0.99, record_every=20)
        dp = B.DevicePolicy(solver.policy, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape,
                            solver.strides, solver.corner_bits, device=cuda_device)
        dp.set_values(solver.value_function)
        dp.set_dynamics(envs.dynamics_source("pendulum"))
        dp.set_robust()
        dp.set_disturbances(dist)
        want = dp.adversary_rollout(starts, 60, gamma=0.99, record_every=20, controller=controller,
                                    lookahead_gamma=solver.config.gamma)
        dp.close()
        C.assert_same_rollout(got, want, f"solver.adversary_rollout({controller})")
        assert isinstance(got.states, np.ndarray) and got.trajectory.shape == (4, 300, 2)
    other = solver.adversary_rollout(starts, 60, disturbances=Disturbances.none(2), gamma=0.99)
    C.assert_same_rollout(other, solver.rollout(starts, 60, gamma=0.99), "disturbances= overrides the solver's set")
    solver.save(tmp_path / "robust")
    capsys.readouterr()
    _cli.main("pendulum", str(tmp_path / "robust.npz"), ["--save-path", str(tmp_path / "robust.npz"), "--rollout", "--adversary",
                                                         "robust", "--episodes", "3", "--steps", "20"])
    out = capsys.readouterr().out
    assert "adversary over 4 disturbance points, controller: robust" in out and out.count("Episode ") == 3
