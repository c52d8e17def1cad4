"""
Stochastic rollouts on the device (csrc/pi_stochastic_kernels.hip behind pi_infer_rollout_stochastic /
pi_infer_random_words, DevicePolicy.rollout(epsilon=..., action_noise=..., state_noise=..., controller="random"),
DevicePolicy.random_words, solver.rollout, the runners' --rollout --random): the stream must equal the numpy Philox twin
word for word; the fused rollout the loop it replaces — per time step one pi_infer_query launch, the twin's words mixed
in with torch float32 operations, one pi_probe_step launch, torch state noise, ended episodes frozen on the host — and
the numpy twin on the checker's step, bit for bit.  Every GPU step runs once; nothing retries.
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
SEED = 0x5eed0123456789ab                # a non-zero high word
FIRST = 2 ** 32 - 500                    # the low counter word of the episode number carries inside a batch of 1000
EPSILON = 0.3


def _torch():
    import torch
    return torch


def _grid(name, shape):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return bins, (lo, hi, gshape, strides, bits)


def _inputs(name, shape=None, actions=None, m=1000):
    """The case of an env: its grid, a random policy table, m starts inside and beyond the grid, the noise levels —
    action noise a tenth of the action range, state noise 0.2 % of the span in every dimension but dimension 1."""
    shape = tuple(int(g) for g in H.golden(name)["g0_shape"]) if shape is None else shape
    bins, grid = _grid(name, shape)
    acts = H.edge_actions(name, actions)
    rng = np.random.default_rng(len(name))
    policy = rng.integers(0, len(acts), int(np.prod(shape))).astype(np.int32)
    starts = H.sample_states(rng, bins, m)
    a_noise = float(np.float32(0.1) * (acts.max() - acts.min()))
    s_noise = (np.float32(0.002) * (grid[1] - grid[0])).astype(np.float32)
    s_noise[1] = 0.0
    return bins, grid, acts, policy, starts, a_noise, s_noise


def _policy(name, grid, acts, policy, cuda_device, stochastic=True):
    dp = B.DevicePolicy(policy, acts, *grid, device=cuda_device)
    dp.set_dynamics(envs.dynamics_source(name))
    if stochastic:
        assert isinstance(dp.set_stochastic(), str)
    return dp


def _step_engine(name, bins, actions, cuda_device):
    """The plugin's own step_dynamics, one launch per call (pi_probe_step)."""
    eng = _native.Engine(len(bins), [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins,
                         actions, device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    return eng


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


# ── the stream ────────────────────────────────────────────────────────────────────────────────────────────────────
def test_random_words_equal_the_twin(cuda_device):
    bins, grid, acts, _, _, _, _ = _inputs("pendulum", (12, 9))
    dp = _policy("pendulum", grid, acts, None, cuda_device)                  # no policy: the module does not need one
    for seed, first, m in ((7, 0, 1000), (7, 0, 1), (SEED, 0, 1000), (SEED, FIRST, 1000), (2 ** 64 - 1, 2 ** 64 - 3, 7)):
        for step in (0, 299):
            for block in (0, 1, 2):
                got = dp.random_words(seed, first, m, step, block)
                assert got.dtype == np.uint32 and got.shape == (m, 4)
                want = B.random_words(seed, first, m, step, block)
                assert np.array_equal(got, want), (seed, first, m, step, block, int((got != want).sum()))
    assert B.random_words(SEED, FIRST, 1000, 0, 0)[:, 0].tolist() != B.random_words(SEED, 0, 1000, 0, 0)[:, 0].tolist()
    assert dp.random_words(SEED, 0, 0, 0, 0).shape == (0, 4)
    dp.set_dynamics(envs.dynamics_source("pendulum"))                       # a new plugin drops the module
    with pytest.raises(RuntimeError, match="set_stochastic"):
        dp.random_words(SEED, 0, 4, 0, 0)
    with pytest.raises(_native.NativeError, match="no stochastic module"):
        dp._engine.random_words(SEED, 0, 4, 0, 0, 4096)
    dp.close()


# ── fused rollout ─────────────────────────────────────────────────────────────────────────────────────────────────
def _step_by_step(dp, eng, acts, start, steps, gamma, every, epsilon, a_noise, s_noise, seed, first):
    """The loop the fused kernel replaces: per time step one query launch and one plugin-step launch; exploration,
    action noise, clamp and state noise from the twin's words in torch float32 operations, multiply and add kept
    separate; the bookkeeping of the rollout's definition on the host side."""
    torch = _torch()
    dev = start.device
    m, D = start.shape
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)          # noqa: E731
    f32 = lambda x: torch.tensor(float(np.float32(x)), dtype=torch.float32, device=dev)   # noqa: E731
    states = start.clone()
    nxt = torch.empty_like(states)
    rew = torch.empty(m, dtype=torch.float32, device=dev)
    done = torch.empty(m, dtype=torch.uint8, device=dev)
    ret = torch.zeros(m, dtype=torch.float32, device=dev)
    length = torch.zeros(m, dtype=torch.int32, device=dev)
    ended = torch.zeros(m, dtype=torch.bool, device=dev)
    disc, g = np.float32(1.0), np.float32(gamma)
    eps24 = B.explore_threshold(epsilon)
    a_lo, a_hi, a_amp = f32(acts.min()), f32(acts.max()), f32(a_noise)
    rows = [states.clone()]
    st = torch.cuda.current_stream(dev).cuda_stream
    for t in range(steps):
        act = dp(states)                                                      # pi_infer_query
        w0 = B.random_words(seed, first, m, t, 0)
        explore = up((w0[:, 0] >> 8) < eps24)
        act = torch.where(explore, up(acts[B.random_action_index(w0[:, 1], len(acts))]), act)
        if a_noise != 0:
            push = a_amp * up(B.sym(w0[:, 2]))
            act = act + push
            act = torch.fmin(torch.fmax(act, a_lo), a_hi)
        act = act.contiguous()
        eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
        if np.any(s_noise != 0):
            words = B.random_words(seed, first, m, t, 1)
            if D > 4:
                words = np.concatenate([words, B.random_words(seed, first, m, t, 2)], axis=1)
            go = done == 0
            disturbed = nxt.clone()
            for d in range(D):
                if s_noise[d] != 0:
                    push = f32(s_noise[d]) * up(B.sym(words[:, d]))
                    disturbed[:, d] = torch.where(go, nxt[:, d] + push, nxt[:, d])
            step_to = disturbed
        else:
            step_to = nxt
        run = ~ended
        gain = rew * float(disc)                                   # float32 multiply, then a separate float32 add
        ret = torch.where(run, ret + gain, ret)
        states = torch.where(run[:, None], step_to, states)
        length = torch.where(run, torch.full_like(length, t + 1), length)
        ended = ended | (run & (done != 0))
        disc = np.float32(disc * g)
        if every and (t + 1) % every == 0:
            rows.append(states.clone())
    return B.RolloutResult(states, ret, length, ended, torch.stack(rows) if every else None)


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("name", ["pendulum", "cartpole", "double_pendulum_swingup", "double_cartpole"])
def test_fused_stochastic_rollout_equals_the_step_by_step_loop_and_the_cpu_twin(name, gamma, cuda_device):
    torch = _torch()
    bins, grid, acts, policy, starts, a_noise, s_noise = _inputs(name)
    assert (s_noise != 0).sum() == len(bins) - 1 and a_noise > 0
    m = len(starts)
    dp = _policy(name, grid, acts, policy, cuda_device)
    eng = _step_engine(name, bins, acts, cuda_device)
    chk = H.oracle_for(name)
    d_starts = torch.from_numpy(starts).to(cuda_device)
    noisy = dict(epsilon=EPSILON, action_noise=a_noise, state_noise=s_noise, seed=SEED, first_episode=FIRST)
    # Measured with the numpy twin on exactly these inputs (random policy table, the noise above): every cart-pole has
    # fallen by step 72 (948 of 1000 by step 10), every double cart-pole by step 19 (994 by step 10).  So "ended and running episodes side by side" is asserted on a second horizon of 10 steps for these two envs, as in
    # tests/test_gpu_greedy.py.
    falls = name in ("cartpole", "double_cartpole")
    for steps in ((300, 10) if falls else (300,)):
        loop = _step_by_step(dp, eng, acts, d_starts, steps, gamma, 7, EPSILON, a_noise, s_noise, SEED, FIRST)
        twin = B.stochastic_rollout(chk.step, starts, steps, policy, acts, *grid, EPSILON, a_noise, s_noise, SEED,
                                    first_episode=FIRST, gamma=gamma, record_every=7)
        assert twin.trajectory.shape == (steps // 7 + 1, m, len(bins))
        for every in (0, 7):
            fused = dp.rollout(d_starts, steps, gamma=gamma, record_every=every, **noisy)
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
    # the noise did something: the deterministic rollout of the same batch differs
    plain = dp.rollout(d_starts, 10, gamma=gamma)
    assert not torch.equal(plain.states, dp.rollout(d_starts, 10, gamma=gamma, **noisy).states)
    dp.close()
    eng.close()


@pytest.mark.parametrize("case", ["act1", "act257"])
def test_random_controller_needs_no_policy(case, cuda_device):
    """controller="random" on a handle WITHOUT a policy table, over a table of one action and one of 257: the twin's
    bits; anything that would consult the policy is refused."""
    torch = _torch()
    _, name, shape, actions = {c[0]: c for c in H.EDGE_CASES}[case]
    bins, grid, acts, _, starts, a_noise, s_noise = _inputs(name, shape, actions)
    assert len(acts) == int(case[3:])
    dp = _policy(name, grid, acts, None, cuda_device)
    chk = H.oracle_for(name)
    for kw in (dict(), dict(action_noise=a_noise, state_noise=s_noise)):
        got = dp.rollout(starts, 60, gamma=0.99, record_every=7, controller="random", seed=SEED, first_episode=FIRST, **kw)
        assert isinstance(got.states, np.ndarray)                                       # numpy in -> numpy out
        want = B.stochastic_rollout(chk.step, starts, 60, None, acts, *grid, 1.0, kw.get("action_noise", 0.0),
                                    kw.get("state_noise"), SEED, first_episode=FIRST, gamma=0.99, record_every=7)
        _assert_same(got, want, f"{case} random controller {sorted(kw)}")
        same = dp.rollout(starts, 60, gamma=0.99, record_every=7, epsilon=1.0, seed=SEED, first_episode=FIRST, **kw)
        _assert_same(same, got, f"{case} epsilon = 1 is the random controller")
    d_starts = torch.from_numpy(starts).to(cuda_device)
    with pytest.raises(RuntimeError, match="without a policy"):
        dp.rollout(starts, 5, epsilon=0.5, seed=1)
    with pytest.raises(_native.NativeError, match="pi_infer_set_policy"):
        dp._engine.rollout_stochastic(d_starts.data_ptr(), len(starts), 5, epsilon=0.5)
    with pytest.raises(_native.NativeError, match="pi_infer_set_policy"):
        dp._engine.rollout_stochastic(d_starts.data_ptr(), len(starts), 5)
    dp.close()


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "double_cartpole"])
def test_defaults_are_the_deterministic_rollout(name, cuda_device):
    """Everything at zero through pi_infer_rollout_stochastic is pi_infer_rollout, bit for bit."""
    torch = _torch()
    bins, grid, acts, policy, starts, _, _ = _inputs(name)
    m, D = starts.shape
    dp = _policy(name, grid, acts, policy, cuda_device)
    d_starts = torch.from_numpy(starts).to(cuda_device)
    st = torch.cuda.current_stream(cuda_device).cuda_stream

    def buffers():
        return dict(d_final=torch.empty((m, D), device=cuda_device), d_return=torch.empty(m, device=cuda_device),
                    d_length=torch.empty(m, dtype=torch.int32, device=cuda_device),
                    d_terminated=torch.empty(m, dtype=torch.uint8, device=cuda_device),
                    d_traj=torch.empty((60 // 7 + 1, m, D), device=cuda_device))
    a, b, c = buffers(), buffers(), buffers()
    ptrs = lambda bufs: {k: v.data_ptr() for k, v in bufs.items()}             # noqa: E731
    dp._engine.rollout(d_starts.data_ptr(), m, 60, 0.99, traj_every=7, stream=st, **ptrs(a))
    dp._engine.rollout_stochastic(d_starts.data_ptr(), m, 60, 0.99, traj_every=7, stream=st, **ptrs(b))
    dp._engine.rollout_stochastic(d_starts.data_ptr(), m, 60, 0.99, state_noise=np.zeros(D, np.float32), seed=SEED,
                                  first_episode=FIRST, traj_every=7, stream=st, **ptrs(c))
    torch.cuda.synchronize()
    for other in (b, c):
        for key in a:
            H.assert_bits_equal(other[key].cpu().numpy(), a[key].cpu().numpy(), f"{name}: {key}")
    # ... and through the front end the default arguments do not even need the module
    plain = _policy(name, grid, acts, policy, cuda_device, stochastic=False)
    _assert_same(plain.rollout(d_starts, 60, gamma=0.99, record_every=7, seed=SEED, first_episode=5),
                 B.RolloutResult(a["d_final"], a["d_return"], a["d_length"], a["d_terminated"] != 0, a["d_traj"]), name)
    with pytest.raises(RuntimeError, match="set_stochastic"):
        plain.rollout(d_starts, 60, epsilon=0.1)
    plain.close()
    dp.close()


def test_batch_independence_and_fixed_seed_behaviour(cuda_device):
    torch = _torch()
    name = "cartpole"
    bins, grid, acts, policy, starts, a_noise, s_noise = _inputs(name)
    m, D = starts.shape
    dp = _policy(name, grid, acts, policy, cuda_device)
    d_starts = torch.from_numpy(starts).to(cuda_device)
    noisy = dict(epsilon=EPSILON, action_noise=a_noise, state_noise=s_noise, seed=SEED)
    whole = dp.rollout(d_starts, 10, gamma=0.99, record_every=3, first_episode=FIRST, **noisy)
    assert 0 < int(whole.terminated.sum()) < m
    head = dp.rollout(d_starts[:256], 10, gamma=0.99, record_every=3, first_episode=FIRST, **noisy)
    tail = dp.rollout(d_starts[256:], 10, gamma=0.99, record_every=3, first_episode=FIRST + 256, **noisy)
    joined = B.RolloutResult(*(torch.cat([x, y], dim=1 if x.dim() == 3 else 0) for x, y in zip(head, tail)))
    _assert_same(whole, joined, "one launch of 1000 against 256 + 744")
    _assert_same(dp.rollout(d_starts, 10, gamma=0.99, record_every=3, first_episode=FIRST, **noisy), whole, "the same seed twice")
    other = dp.rollout(d_starts, 10, gamma=0.99, record_every=3, first_episode=FIRST, **{**noisy, "seed": SEED + 1})
    assert not torch.equal(other.returns, whole.returns), "another seed, the same returns"
    shifted = dp.rollout(d_starts, 10, gamma=0.99, record_every=3, first_episode=FIRST + 1, **noisy)
    assert not torch.equal(shifted.returns, whole.returns), "first_episode must select the stream"
    assert torch.equal(d_starts.cpu(), torch.from_numpy(starts))                        # the start states are not written
    # zero steps: the starts come back, nothing ran; an empty batch: empty outputs
    none = dp.rollout(starts, 0, gamma=0.99, **noisy)
    assert isinstance(none.states, np.ndarray) and np.array_equal(none.states, starts)
    assert not none.lengths.any() and not none.returns.any() and not none.terminated.any()
    empty = dp.rollout(np.zeros((0, D), np.float32), 10, **noisy)
    assert empty.states.shape == (0, D) and empty.returns.shape == (0,) and empty.trajectory is None
    dp._engine.rollout_stochastic(0, 0, 10, epsilon=0.5)                               # m = 0: a no-op, buffers or not
    with pytest.raises(ValueError):
        dp.rollout(starts, 5, record_every=6, **noisy)
    with pytest.raises(_native.NativeError, match="traj_every > n_steps"):
        dp._engine.rollout_stochastic(d_starts.data_ptr(), m, 5, epsilon=0.5, d_traj=d_starts.data_ptr(), traj_every=6)
    with pytest.raises(_native.NativeError, match="epsilon"):
        dp._engine.rollout_stochastic(d_starts.data_ptr(), m, 5, epsilon=1.5)
    with pytest.raises(ValueError, match="greedy"):
        dp.rollout(starts, 5, controller="greedy", lookahead_gamma=0.99, epsilon=0.1)
    dp.set_dynamics(envs.dynamics_source(name))                                        # a new plugin drops the module
    with pytest.raises(RuntimeError, match="set_stochastic"):
        dp.rollout(starts, 5, **noisy)
    with pytest.raises(_native.NativeError, match="no stochastic module"):
        dp._engine.rollout_stochastic(d_starts.data_ptr(), m, 5, epsilon=0.5)
    dp.close()


# ── solver and runner ─────────────────────────────────────────────────────────────────────────────────────────────
def test_solver_stochastic_rollouts_and_the_runner_baseline(cuda_device, tmp_path):
    """solver.rollout(controller="random") on an instance that has never run; solver.rollout(epsilon=..., state_noise=...)
    after run() equals DevicePolicy.rollout assembled by hand; the pendulum runner with --rollout --random prints the
    reference's baseline lines and trains nothing."""
    fresh = envs.make("pendulum", 25)
    starts = envs.PendulumCuda.start_states(np.random.default_rng(1), 300)
    base = fresh.rollout(starts, 60, gamma=0.99, record_every=20, controller="random", seed=9)
    assert getattr(fresh, "policy", None) is None                                       # it never ran
    bins, grid = _grid("pendulum", (25, 25))
    want = B.stochastic_rollout(H.oracle_for("pendulum").step, starts, 60, None, fresh.action_space, *grid, 1.0, 0.0, None,
                                9, gamma=0.99, record_every=20)
    _assert_same(base, want, "solver.rollout(controller='random') on a fresh solver")
    assert isinstance(base.states, np.ndarray) and base.trajectory.shape == (4, 300, 2) and (base.lengths == 60).all()
    with pytest.raises(RuntimeError, match="trained policy"):
        fresh.rollout(starts, 60, epsilon=0.5)

    solver = envs.make("pendulum", 25)
    solver.run()
    kw = dict(epsilon=0.2, state_noise=[0.05, 0.0], seed=4, first_episode=100)
    got = solver.rollout(starts, 60, gamma=0.99, record_every=20, **kw)
    dp = B.DevicePolicy(solver.policy, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape,
                        solver.strides, solver.corner_bits, device=cuda_device)
    dp.set_dynamics(envs.dynamics_source("pendulum"))
    dp.set_stochastic()
    by_hand = dp.rollout(starts, 60, gamma=0.99, record_every=20, **kw)
    dp.close()
    _assert_same(got, by_hand, "solver.rollout(epsilon=..., state_noise=...)")
    assert not np.array_equal(got.returns, solver.rollout(starts, 60, gamma=0.99).returns)
    with pytest.raises(ValueError, match="greedy"):
        solver.rollout(starts, 60, controller="greedy", action_noise=0.1)

    res = subprocess.run([sys.executable, str(ROOT / "runners" / "pendulum_cuda.py"), "--rollout", "--random", "3", "--steps", "50",
                          "--save-path", str(tmp_path / "p.npz")], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [line for line in res.stdout.splitlines() if line.startswith("[random] Episode ")]
    assert len(lines) == 3 and all(": 50 steps | reward = " in line for line in lines), res.stdout[-2000:]
    assert "Training" not in res.stdout and "accepted and ignored" not in res.stdout and not (tmp_path / "p.npz").exists()
