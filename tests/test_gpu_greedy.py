"""
Value-greedy control on the device (csrc/pi_greedy_kernels.hip behind pi_infer_greedy / pi_infer_rollout_greedy,
DevicePolicy.greedy, DevicePolicy.rollout(controller="greedy"), solver.rollout(controller="greedy"), the runners'
--controller): the query must equal, bit for bit, the CPU checker's improvement backup at arbitrary points and the
numpy twin; the fused rollout the loop it replaces — one greedy launch and one pi_probe_step launch per time step with
ended episodes frozen on the host — and the twin on the checker's step.  Every GPU step runs once; nothing retries.
"""
from __future__ import annotations

import subprocess
import sys
from itertools import product
from pathlib import Path

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from tests import helpers as H
from utils import barycentric as B

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
LOOKAHEAD = 0.99


def _torch():
    import torch
    return torch


def _grid(name, shape):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return bins, (lo, hi, gshape, strides), bits


def _controller(name, grid, bits, actions, V, cuda_device):
    """A DevicePolicy WITHOUT a policy table, with values, plugin and the greedy module."""
    dp = B.DevicePolicy(None, actions, *grid, bits, device=cuda_device)
    dp.set_values(V)
    dp.set_dynamics(envs.dynamics_source(name))
    assert isinstance(dp.set_greedy(), str)
    return dp


def _reference(chk, pts, actions, V, grid, gamma):
    """(best, action value, best Q, Q matrix) from the checker: improve_points and, per action, eval_points."""
    best, q_best = chk.improve_points(pts, actions, V, *grid, gamma)
    Q = np.stack([chk.eval_points(pts, np.full(len(pts), u, np.float32), V, *grid, gamma) for u in actions], axis=1)
    return best, actions[best], q_best, Q


def _assert_query(got, want, what):
    assert np.array_equal(np.asarray(got[0]), want[0]), f"{what}: {int((np.asarray(got[0]) != want[0]).sum())} greedy indices differ"
    for k, label in ((1, "action value"), (2, "best Q"), (3, "Q matrix")):
        if len(got) > k:
            H.assert_bits_equal(np.asarray(got[k]), want[k], f"{what}: {label}")


def _query_case(name, shape, actions, cuda_device, gammas=(0.99, 1.0)):
    torch = _torch()
    bins, grid, bits = _grid(name, shape)
    actions = np.asarray(actions, np.float32)
    rng = np.random.default_rng(len(name))
    V = (30.0 * rng.standard_normal(int(np.prod(shape)))).astype(np.float32)
    m = 1000                                                                            # 3 * 256 + 232: ragged
    pts = H.sample_states(rng, bins, m)                                                 # up to 15 % outside the bounds
    pts[::97] *= 2.0                                                                    # ... and some far outside
    chk = H.oracle_for(name)
    dp = _controller(name, grid, bits, actions, V, cuda_device)
    d_pts = torch.from_numpy(pts).to(cuda_device)
    st = torch.cuda.current_stream(cuda_device).cuda_stream
    first = None
    for gamma in gammas:
        want = _reference(chk, pts, actions, V, grid, gamma)
        twin = B.greedy_action(chk.step, pts, V, actions, *grid, gamma, q_values=True)
        _assert_query(twin, want, f"{name} gamma={gamma} twin vs checker")
        got = dp.greedy(pts, gamma, q_values=True)                                      # numpy in -> numpy out, all together
        assert all(isinstance(x, np.ndarray) for x in got) and got[0].dtype == np.int32 and got[3].shape == (m, len(actions))
        _assert_query(got, want, f"{name} gamma={gamma} device vs checker")
        first = first or (gamma, got)
        # every output on its own: the others null
        outs = {"d_best": torch.full((m,), -7, dtype=torch.int32, device=cuda_device),
                "d_action": torch.full((m,), -7.0, device=cuda_device), "d_q_best": torch.full((m,), -7.0, device=cuda_device),
                "d_q_all": torch.full((m, len(actions)), -7.0, device=cuda_device)}
        for key, buf in outs.items():
            dp._engine.greedy(d_pts.data_ptr(), m, gamma, stream=st, **{key: buf.data_ptr()})
        torch.cuda.synchronize()
        _assert_query([outs[k].cpu().numpy() for k in ("d_best", "d_action", "d_q_best", "d_q_all")], want,
                      f"{name} gamma={gamma} each output alone")
        on_dev = dp.greedy(d_pts, gamma)                                                # a device tensor in -> tensors out
        assert len(on_dev) == 3 and all(torch.is_tensor(x) and x.device == d_pts.device for x in on_dev)
        _assert_query([x.cpu().numpy() for x in on_dev], want, f"{name} gamma={gamma} device tensor in")
    one = dp.greedy(pts[:1], gammas[0], q_values=True)                                  # m = 1
    _assert_query(one, [w[:1] for w in _reference(chk, pts[:1], actions, V, grid, gammas[0])], f"{name} m = 1")
    empty = dp.greedy(np.zeros((0, len(bins)), np.float32), gammas[0], q_values=True)
    assert empty[0].shape == (0,) and empty[3].shape == (0, len(actions))
    # neither the points nor the values were written: the first query again, same bits
    assert torch.equal(d_pts.cpu(), torch.from_numpy(pts))
    again = dp.greedy(pts, first[0], q_values=True)
    for a, b in zip(again, first[1]):
        H.assert_bits_equal(a, b, f"{name}: the first query repeated")
    return dp, pts, d_pts


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "double_pendulum_swingup", "double_cartpole",
                                  "double_cartpole_swingup"])
def test_greedy_query_equals_the_checker_and_the_twin(name, cuda_device):
    shape = tuple(int(g) for g in H.golden(name)["g0_shape"])
    dp, pts, d_pts = _query_case(name, shape, H.edge_actions(name), cuda_device)
    # a policy-table rollout on this handle still raises: it has no policy
    with pytest.raises(RuntimeError, match="without a policy"):
        dp.rollout(pts, 5)
    with pytest.raises(_native.NativeError, match="pi_infer_set_policy was never called"):
        dp._engine.rollout(d_pts.data_ptr(), len(pts), 5)
    with pytest.raises(RuntimeError, match="without a policy"):
        dp(pts)
    # a new plugin drops the module until set_greedy is called again
    dp.set_dynamics(envs.dynamics_source(name))
    with pytest.raises(RuntimeError, match="set_greedy"):
        dp.greedy(pts, 0.99)
    with pytest.raises(_native.NativeError, match="no greedy module"):
        dp._engine.greedy(d_pts.data_ptr(), len(pts), 0.99, d_best=d_pts.data_ptr())
    dp.close()


@pytest.mark.parametrize("case", ["act1", "act257"])
def test_greedy_query_with_one_action_and_with_257(case, cuda_device):
    """The action count is run-time data: a table of one action (the loop runs once, index 0 always) and one of 257, of
    which 65 + 65 clamp to the same torque (exact ties: the lowest index wins)."""
    _, name, shape, actions = {c[0]: c for c in H.EDGE_CASES}[case]
    acts = H.edge_actions(name, actions)
    assert len(acts) == int(case[3:])
    dp, pts, _ = _query_case(name, shape, acts, cuda_device, gammas=(0.99,))
    best = dp.greedy(pts, 0.99)[0]
    if len(acts) == 1:
        assert not best.any()
    else:
        assert len(np.unique(best)) > 2 and (best[best < 65] == 0).all()      # the clamped torques tie: index 0 wins
    dp.close()


@pytest.mark.parametrize("name,bins", [("pendulum", 25), ("cartpole", 6)])
def test_greedy_action_at_the_nodes_of_a_gpu_run_is_its_policy(name, bins, cuda_device):
    solver = envs.make(name, bins)
    solver.run()
    term, _ = H.terminal_mask(name, solver.states_space)
    live = ~term
    assert live.any()
    dp = B.DevicePolicy(None, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape, solver.strides,
                        solver.corner_bits, device=cuda_device)
    dp.set_values(solver.value_function)
    dp.set_dynamics(envs.dynamics_source(name))
    dp.set_greedy()
    best, act, _ = dp.greedy(np.ascontiguousarray(solver.states_space[live], np.float32), solver.config.gamma)
    dp.close()
    assert np.array_equal(best, solver.policy[live]), f"{int((best != solver.policy[live]).sum())} of {int(live.sum())} nodes differ"
    H.assert_bits_equal(act, np.asarray(solver.action_space, np.float32)[solver.policy[live]], "action values")


# ── fused rollout ─────────────────────────────────────────────────────────────────────────────────────────────────
def _step_engine(name, bins, actions, cuda_device):
    """The plugin's own step_dynamics, one launch per call (pi_probe_step)."""
    eng = _native.Engine(len(bins), [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins,
                         actions, device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    return eng


def _step_by_step(dp, eng, start, steps, gamma, every):
    """The loop the fused kernel replaces: per time step one greedy launch and one plugin-step launch, plus the
    bookkeeping of the rollout's definition on the host side (tests/test_gpu_rollout.py, _step_by_step)."""
    torch = _torch()
    dev = start.device
    m = start.shape[0]
    states = start.clone()
    nxt = torch.empty_like(states)
    rew = torch.empty(m, dtype=torch.float32, device=dev)
    done = torch.empty(m, dtype=torch.uint8, device=dev)
    ret = torch.zeros(m, dtype=torch.float32, device=dev)
    length = torch.zeros(m, dtype=torch.int32, device=dev)
    ended = torch.zeros(m, dtype=torch.bool, device=dev)
    disc, g = np.float32(1.0), np.float32(gamma)
    rows = [states.clone()]
    st = torch.cuda.current_stream(dev).cuda_stream
    for t in range(steps):
        act = dp.greedy(states, LOOKAHEAD)[1]
        eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
        run = ~ended
        gain = rew * float(disc)                                   # float32 multiply, then a separate float32 add
        ret = torch.where(run, ret + gain, ret)
        states = torch.where(run[:, None], nxt, states)
        length = torch.where(run, torch.full_like(length, t + 1), length)
        ended = ended | (run & (done != 0))
        disc = np.float32(disc * g)
        if every and (t + 1) % every == 0:
            rows.append(states.clone())
    return B.RolloutResult(states, ret, length, ended, torch.stack(rows) if every else None)


def _assert_same(got, want, what, trajectory=True):
    def host(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    H.assert_bits_equal(host(got.states), host(want.states), f"{what}: final states")
    H.assert_bits_equal(host(got.returns), host(want.returns), f"{what}: returns")
    assert np.array_equal(host(got.lengths), host(want.lengths)), f"{what}: lengths"
    assert np.array_equal(host(got.terminated), host(want.terminated)), f"{what}: terminated"
    if trajectory:
        assert (got.trajectory is None) == (want.trajectory is None), what
        if got.trajectory is not None:
            H.assert_bits_equal(host(got.trajectory), host(want.trajectory), f"{what}: trajectory")


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "double_pendulum_swingup", "double_cartpole"])
def test_fused_greedy_rollout_equals_the_step_by_step_loop_and_the_cpu_twin(name, gamma, cuda_device):
    torch = _torch()
    shape = tuple(int(g) for g in H.golden(name)["g0_shape"])
    bins, grid, bits = _grid(name, shape)
    actions = H.edge_actions(name)
    rng = np.random.default_rng(len(name))
    V = (30.0 * rng.standard_normal(int(np.prod(shape)))).astype(np.float32)
    m = 1000
    starts = H.sample_states(rng, bins, m)
    starts[::97] *= 2.0
    dp = _controller(name, grid, bits, actions, V, cuda_device)
    eng = _step_engine(name, bins, actions, cuda_device)
    chk = H.oracle_for(name)
    d_starts = torch.from_numpy(starts).to(cuda_device)
    # Measured with the numpy twin on exactly these inputs: every cart-pole has fallen by step 59 (951 of 1000 by step 10),
    # every double cart-pole by step 22 (989 by step 10).  So "ended and running episodes side by side" is asserted on a
    # second horizon of 10 steps for these two envs, as in tests/test_gpu_rollout.py.
    falls = name in ("cartpole", "double_cartpole")
    for steps in ((300, 10) if falls else (300,)):
        loop = _step_by_step(dp, eng, d_starts, steps, gamma, 7)
        twin = B.greedy_rollout(chk.step, starts, steps, V, actions, *grid, LOOKAHEAD, gamma=gamma, record_every=7)
        assert np.isfinite(twin.states).all() and np.isfinite(twin.returns).all()
        assert twin.trajectory.shape == (steps // 7 + 1, m, len(bins))
        for every in (0, 7):
            fused = dp.rollout(d_starts, steps, gamma=gamma, record_every=every, controller="greedy", lookahead_gamma=LOOKAHEAD)
            assert torch.is_tensor(fused.states) and fused.states.device == d_starts.device
            assert fused.lengths.dtype == torch.int32 and fused.terminated.dtype == torch.bool
            assert (fused.trajectory is None) == (every == 0)
            _assert_same(fused, loop, f"{name} {steps} steps gamma={gamma} every={every} fused vs loop", trajectory=every > 0)
            _assert_same(fused, twin, f"{name} {steps} steps gamma={gamma} every={every} fused vs numpy twin", trajectory=every > 0)
        assert torch.equal(d_starts.cpu(), torch.from_numpy(starts))                    # the start states are not written
        n_term = int(twin.terminated.sum())
        print(f"{name} {steps} steps gamma={gamma}: {n_term} of {m} episodes terminated, lengths {twin.lengths.min()} .. "
              f"{twin.lengths.max()}")
        if falls and steps == 10:
            assert 0 < n_term < m, "the freeze path needs ended and running episodes side by side"
        elif falls:
            assert n_term > 0 and twin.lengths.max() > twin.lengths.min() + 1          # they end on different steps
    # zero steps: the starts come back, nothing ran; numpy in -> numpy out
    none = dp.rollout(starts, 0, gamma=gamma, record_every=0, controller="greedy", lookahead_gamma=LOOKAHEAD)
    assert isinstance(none.states, np.ndarray) and np.array_equal(none.states, starts)
    assert not none.lengths.any() and not none.returns.any() and not none.terminated.any()
    with pytest.raises(ValueError, match="lookahead_gamma"):
        dp.rollout(starts, 5, controller="greedy")
    with pytest.raises(ValueError, match="controller"):
        dp.rollout(starts, 5, controller="argmax")
    with pytest.raises(_native.NativeError, match="lookahead_gamma is NaN"):
        dp._engine.rollout_greedy(d_starts.data_ptr(), m, 5, float("nan"))
    dp.close()
    eng.close()


# ── solver and runner ─────────────────────────────────────────────────────────────────────────────────────────────
def test_solver_greedy_rollout_and_the_runner_flag(cuda_device, tmp_path):
    """solver.rollout(controller="greedy") after run() equals DevicePolicy.rollout assembled by hand from V, the action
    table and the config's gamma; it also runs on the value function alone, after value_iteration(); the pendulum runner
    with --controller greedy prints one line per episode."""
    solver = envs.make("pendulum", 25)
    solver.run()
    starts = envs.PendulumCuda.start_states(np.random.default_rng(1), 300)
    got = solver.rollout(starts, 60, gamma=0.99, record_every=20, controller="greedy")
    dp = B.DevicePolicy(None, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape,
                        solver.strides, solver.corner_bits, device=cuda_device)
    dp.set_values(solver.value_function)
    dp.set_dynamics(envs.dynamics_source("pendulum"))
    dp.set_greedy()
    want = dp.rollout(starts, 60, gamma=0.99, record_every=20, controller="greedy", lookahead_gamma=solver.config.gamma)
    dp.close()
    _assert_same(got, want, "solver.rollout(controller='greedy')")
    assert isinstance(got.states, np.ndarray) and got.trajectory.shape == (4, 300, 2) and (got.lengths == 60).all()
    policy_run = solver.rollout(starts, 60, gamma=0.99, record_every=20)               # the default controller still works
    assert policy_run.trajectory.shape == (4, 300, 2)

    vi = envs.make("pendulum", 25)
    vi.value_iteration()
    assert getattr(vi, "value_function", None) is None                                  # nothing pulled to the host yet
    res = vi.rollout(starts[:10], 20, controller="greedy")
    assert res.states.shape == (10, 2) and (res.lengths == 20).all() and np.isfinite(res.returns).all()

    res = subprocess.run([sys.executable, str(ROOT / "runners" / "pendulum_cuda.py"), "--bins", "25", "--retrain", "--rollout",
                          "--controller", "greedy", "--episodes", "3", "--steps", "50", "--save-path", str(tmp_path / "p.npz")],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "accepted and ignored" not in res.stdout
    lines = [line for line in res.stdout.splitlines() if line.startswith("Episode ")]
    assert len(lines) == 3 and all("50 steps | return = " in line and "final state:" in line for line in lines)
