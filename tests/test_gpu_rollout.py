"""
Fused closed-loop rollouts on the device (csrc/pi_rollout_kernels.hip behind pi_infer_rollout, DevicePolicy.rollout,
solver.rollout, the runners' --rollout): one launch per batch of episodes must equal, bit for bit, the loop it
replaces — one pi_infer_query and one pi_probe_step launch per time step with ended episodes frozen on the host — and
the numpy twin on the oracle's step.  Every GPU step runs once; nothing retries.
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


def _torch():
    import torch
    return torch


def _grid(name, shape):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return bins, (lo, hi, gshape, strides, bits)


def _step_engine(name, bins, actions, cuda_device):
    """The plugin's own step_dynamics, one launch per call (pi_probe_step)."""
    eng = _native.Engine(len(bins), [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins,
                         actions, device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    return eng


def _step_by_step(dp, eng, start, steps, gamma, every):
    """The loop the suite used before the fused kernel (tests/test_gpu_endtoend.py, _closed_loop): per time step one
    inference launch and one plugin-step launch, plus the bookkeeping of the rollout's definition on the host side —
    ended episodes keep their state, their return and their length."""
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
        act = dp(states)
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


@pytest.mark.parametrize("name", ["pendulum", "cartpole", "double_pendulum_swingup", "double_cartpole"])
def test_fused_rollout_equals_the_step_by_step_loop_and_the_cpu_twin(name, cuda_device):
    torch = _torch()
    shape = tuple(int(g) for g in H.golden(name)["g0_shape"])
    bins, (lo, hi, gshape, strides, bits) = _grid(name, shape)
    actions = np.asarray(envs.ENVS[name].ACTIONS, np.float32)
    rng = np.random.default_rng(len(name))
    policy = rng.integers(0, len(actions), int(np.prod(shape))).astype(np.int32)       # random, uploaded as is
    m, steps = 1000, 300                                                                # 1000 = 3 * 256 + 232: ragged
    starts = H.sample_states(rng, bins, m)                                              # up to 15 % outside the bounds
    starts[::97] *= 2.0                                                                 # ... and some far outside
    dp = B.DevicePolicy(policy, actions, lo, hi, gshape, strides, bits, device=cuda_device)
    assert dp.set_dynamics(envs.dynamics_source(name)) is not None
    eng = _step_engine(name, bins, actions, cuda_device)
    chk = H.oracle_for(name)
    d_starts = torch.from_numpy(starts).to(cuda_device)
    # Measured with the numpy twin: under a random policy EVERY cart-pole and double cart-pole of this batch has fallen long
    # before step 300 (about two thirds start outside the failure limits and end on step 1; the longest episode lasts 35
    # resp. 19 steps, and over 12 other policy seeds 142 resp. 32).  So in the 300-step run the frozen lanes sit next to running ones only while it
    # lasts — asserted below through the lengths — and "some episodes terminated, some did not" is asserted on a second
    # horizon of 10 steps, added for these two envs, everything else the same.
    falls = name in ("cartpole", "double_cartpole")
    for steps in ((steps, 10) if falls else (steps,)):
        for gamma in (1.0, 0.99):
            loop = _step_by_step(dp, eng, d_starts, steps, gamma, 7)
            twin = B.rollout(chk.step, starts, steps, policy, actions, lo, hi, gshape, strides, bits, gamma=gamma,
                             record_every=7)
            assert np.isfinite(twin.states).all() and np.isfinite(twin.returns).all()
            assert twin.trajectory.shape == (steps // 7 + 1, m, len(bins))
            for every in (0, 7):
                fused = dp.rollout(d_starts, steps, gamma=gamma, record_every=every)
                assert torch.is_tensor(fused.states) and fused.states.device == d_starts.device
                assert fused.lengths.dtype == torch.int32 and fused.terminated.dtype == torch.bool
                assert (fused.trajectory is None) == (every == 0)
                _assert_same(fused, loop, f"{name} {steps} steps gamma={gamma} every={every} fused vs loop", trajectory=every > 0)
                _assert_same(fused, twin, f"{name} {steps} steps gamma={gamma} every={every} fused vs numpy twin", trajectory=every > 0)
                from_host = dp.rollout(starts, steps, gamma=gamma, record_every=every)      # numpy in -> numpy out
                assert isinstance(from_host.states, np.ndarray) and from_host.terminated.dtype == bool
                _assert_same(from_host, fused, f"{name} numpy in", trajectory=True)
            assert torch.equal(d_starts.cpu(), torch.from_numpy(starts))                    # the start states are not written
            n_term = int(twin.terminated.sum())
            print(f"{name} {steps} steps gamma={gamma}: {n_term} of {m} episodes terminated, lengths {twin.lengths.min()} .. "
                  f"{twin.lengths.max()}, {len(np.unique(twin.lengths))} different")
            if falls and steps == 10:
                assert 0 < n_term < m, "the freeze path needs ended and running episodes side by side"
            elif falls:
                assert n_term > 0 and twin.lengths.max() > twin.lengths.min() + 1      # they end on different steps
    dp.close()
    eng.close()


def test_rollout_edge_cases(cuda_device):
    torch = _torch()
    name, shape = "cartpole", (9, 8, 11, 7)
    bins, (lo, hi, gshape, strides, bits) = _grid(name, shape)
    actions = np.asarray(envs.ENVS[name].ACTIONS, np.float32)
    rng = np.random.default_rng(17)
    policy = rng.integers(0, len(actions), int(np.prod(shape))).astype(np.int32)
    chk = H.oracle_for(name)
    dp = B.DevicePolicy(policy, actions, lo, hi, gshape, strides, bits, device=cuda_device)
    with pytest.raises(RuntimeError, match="set_dynamics"):
        dp.rollout(np.zeros((3, 4), np.float32), 5)
    with pytest.raises(_native.NativeError, match="pi_infer_set_dynamics was never called"):
        dp._engine.rollout(torch.zeros((3, 4), device=cuda_device).data_ptr(), 3, 5)
    dp.set_dynamics(envs.dynamics_source(name))
    starts = (rng.uniform(-1, 1, (257, 4)) * [1.0, 1.0, 0.15, 1.0]).astype(np.float32)
    for m in (1, 63, 64, 65, 257):
        for steps, every in ((0, 0), (1, 0), (1, 1), (40, 40), (40, 3)):
            got = dp.rollout(starts[:m], steps, gamma=0.9, record_every=every)
            want = B.rollout(chk.step, starts[:m], steps, policy, actions, lo, hi, gshape, strides, bits, gamma=0.9,
                             record_every=every)
            _assert_same(got, want, f"m={m} steps={steps} every={every}")
            if steps == 0:
                assert np.array_equal(got.states, starts[:m]) and not got.lengths.any() and not got.returns.any()
            if every == steps and every:
                assert got.trajectory.shape == (2, m, 4) and np.array_equal(got.trajectory[0], starts[:m])
                assert np.array_equal(got.trajectory[1], got.states)
    empty = dp.rollout(np.zeros((0, 4), np.float32), 10)
    assert empty.states.shape == (0, 4) and empty.returns.shape == (0,)
    # every output on its own: the others null
    d_starts = torch.from_numpy(starts).to(cuda_device)
    full = dp.rollout(d_starts, 40, gamma=0.9, record_every=4)
    m = len(starts)
    outs = {"d_final": torch.full((m, 4), -7.0, device=cuda_device), "d_return": torch.full((m,), -7.0, device=cuda_device),
            "d_length": torch.full((m,), -7, dtype=torch.int32, device=cuda_device),
            "d_terminated": torch.full((m,), 7, dtype=torch.uint8, device=cuda_device),
            "d_traj": torch.full((11, m, 4), -7.0, device=cuda_device)}
    st = torch.cuda.current_stream(cuda_device).cuda_stream
    for key, buf in outs.items():
        dp._engine.rollout(d_starts.data_ptr(), m, 40, 0.9, traj_every=4 if key == "d_traj" else 0, stream=st,
                           **{key: buf.data_ptr()})
    torch.cuda.synchronize()
    assert torch.equal(outs["d_final"], full.states) and torch.equal(outs["d_return"], full.returns)
    assert torch.equal(outs["d_length"], full.lengths) and torch.equal(outs["d_terminated"] != 0, full.terminated)
    assert torch.equal(outs["d_traj"], full.trajectory)
    # arguments
    for kw, msg in ((dict(n_steps=-1), "n_steps < 0"), (dict(traj_every=-1), "traj_every < 0"),
                    (dict(traj_every=41, d_traj=outs["d_traj"].data_ptr()), "traj_every > n_steps"),
                    (dict(traj_every=4), "d_traj is null"), (dict(m=-1), "m < 0"),
                    (dict(m=1 << 61, traj_every=1, d_traj=outs["d_traj"].data_ptr()), "63 bits"),
                    (dict(d_start=0), "d_start"), (dict(d_final=outs["d_final"].data_ptr() + 4), "aligned")):
        args = dict(d_start=d_starts.data_ptr(), m=m, n_steps=40, gamma=0.9)
        args.update(kw)
        with pytest.raises(_native.NativeError, match=msg):
            dp._engine.rollout(**args)
    with pytest.raises(ValueError, match="record_every"):
        dp.rollout(starts, 10, record_every=11)
    with pytest.raises(ValueError, match="float32"):
        dp.rollout(d_starts.double(), 10)
    # another plugin of the same D replaces the first: the crane's dynamics on the same grid and policy
    other = envs.dynamics_source("overhead_crane")
    dp.set_dynamics(other)
    swapped = dp.rollout(starts, 40, gamma=0.9)
    want = B.rollout(H.oracle_for("overhead_crane").step, starts, 40, policy, actions, lo, hi, gshape, strides, bits, gamma=0.9)
    _assert_same(swapped, want, "after a second set_dynamics")
    assert not np.array_equal(swapped.states, full.states.cpu().numpy())
    dp.close()
    # no policy: refused by the front end and by the library
    bare = B.DevicePolicy(None, None, lo, hi, gshape, strides, bits, device=cuda_device)
    bare.set_dynamics(envs.dynamics_source(name))
    with pytest.raises(RuntimeError, match="without a policy"):
        bare.rollout(starts, 5)
    with pytest.raises(_native.NativeError, match="pi_infer_set_policy was never called"):
        bare._engine.rollout(d_starts.data_ptr(), m, 5)
    bare.close()


def test_solver_rollout_and_the_runner_flag(cuda_device, tmp_path, monkeypatch):
    """The product path: solver.rollout after run() equals DevicePolicy.rollout on the same arrays; the pendulum
    runner with --rollout prints one line per episode, and the same lines again when it loads the archive it saved;
    the 6-D swing-up runner also writes the steady-state trajectory file."""
    solver = envs.make("pendulum", 50)
    solver.run()
    starts = envs.PendulumCuda.start_states(np.random.default_rng(1), 300)
    got = solver.rollout(starts, 200, gamma=0.99, record_every=50)
    dp = B.DevicePolicy(solver.policy, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape,
                        solver.strides, solver.corner_bits, device=cuda_device)
    dp.set_dynamics(envs.dynamics_source("pendulum"))
    _assert_same(got, dp.rollout(starts, 200, gamma=0.99, record_every=50), "solver.rollout")
    dp.close()
    assert isinstance(got.states, np.ndarray) and got.trajectory.shape == (5, 300, 2) and (got.lengths == 200).all()

    def runner(*extra):
        res = subprocess.run([sys.executable, str(ROOT / "runners" / "pendulum_cuda.py"), "--bins", "50", "--rollout",
                              "--episodes", "3", "--steps", "200", "--seed", "1", "--save-path", str(tmp_path / "p.npz"),
                              *extra], cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        assert "accepted and ignored" not in res.stdout
        return [line for line in res.stdout.splitlines() if line.startswith("Episode ")]
    trained = runner("--retrain")
    assert len(trained) == 3 and all("200 steps | return = " in line and "final state:" in line for line in trained)
    assert (tmp_path / "p.npz").exists() and not (tmp_path / "results").exists()
    assert runner() == trained                                    # loaded from the archive: same seed, same episodes

    from runners import _cli
    monkeypatch.chdir(tmp_path)
    pi = _cli.main("double_cartpole_swingup", "unused.npz", ["--bins", "6", "--retrain", "--rollout", "--episodes", "4",
                                                             "--steps", "150", "--save-path", str(tmp_path / "dc.npz")])
    d = np.load(tmp_path / "results" / "last_trajectory.npz")
    assert set(d.files) == {"traj", "n_episodes", "steps_per_episode"}
    assert int(d["n_episodes"]) == 4 and int(d["steps_per_episode"]) == 100
    traj = d["traj"]
    assert traj.dtype == np.float32 and traj.ndim == 2 and traj.shape[1] == 6 and 4 <= len(traj) <= 4 * 100
    # ... and it holds what the rollout produced: the last min(100, length + 1) states of every episode
    starts = envs.DoubleCartPoleSwingUpCuda.start_states(np.random.default_rng(42), 4)
    res = pi.rollout(starts, 150, record_every=1)
    want = np.concatenate([res.trajectory[max(0, n + 1 - 100):n + 1, ep] for ep, n in enumerate(res.lengths)])
    H.assert_bits_equal(traj, want, "last_trajectory.npz")


def test_rollout_handles_give_their_device_memory_back(cuda_device):
    """pi_infer_destroy unloads the rollout module too: 30 create / set_policy / set_dynamics / rollout / destroy cycles
    leave the device's free memory where it was (pattern: test_handles_give_their_device_memory_back)."""
    torch = _torch()
    name, shape = "cartpole_swingup", (14, 9, 12, 8)
    bins, (lo, hi, gshape, strides, bits) = _grid(name, shape)
    actions = np.asarray(envs.ENVS[name].ACTIONS, np.float32)
    policy = np.zeros(int(np.prod(shape)), np.int32)
    dyn = envs.dynamics_source(name)
    starts = torch.zeros((512, 4), dtype=torch.float32, device=cuda_device)
    final = torch.empty_like(starts)

    def cycle():
        inf = _native.InferenceEngine(lo, hi, gshape, strides, bits, device=cuda_device.index or 0)
        inf.set_policy(policy, actions)
        inf.set_dynamics(dyn)
        inf.rollout(starts.data_ptr(), 512, 20, d_final=final.data_ptr())
        torch.cuda.synchronize()
        inf.close()

    for _ in range(3):
        cycle()                                                  # warm the allocator pools and the caches
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(cuda_device)
    for _ in range(30):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(cuda_device)
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) / 2**20:.1f} MiB not returned after 30 handle cycles"


def test_fused_rollout_is_faster_than_the_loop_and_swings_the_pole_up(cuda_device):
    """CartPole swing-up 50^4, trained; 4 096 poles hanging down, 1 000 steps.  The fused call against the step-by-step
    loop in the same process, each after one warm-up, the better of two, timed with events: the loop is code this
    kernel replaces, so it is the baseline — the fused call must be faster.  And the fused result meets the criterion
    of tests/test_gpu_endtoend.py::test_trained_policies_solve_their_tasks_in_closed_loop: at least 0.99 of the poles up
    and held, the cart on the track."""
    torch = _torch()
    name, m, steps = "cartpole_swingup", 4096, 1000
    solver = envs.make(name, 50)
    solver.run()
    assert solver.stats["stable"]
    bins = [np.asarray(b, np.float32) for b in envs.ENVS[name].bins_space(50).values()]
    dp = B.DevicePolicy(solver.policy, solver.action_space, solver.bounds_low, solver.bounds_high, solver.grid_shape,
                        solver.strides, solver.corner_bits, device=cuda_device)
    dp.set_dynamics(envs.dynamics_source(name))
    eng = _step_engine(name, bins, solver.action_space, cuda_device)
    gen = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.rand((m, 4), generator=gen) * 2 - 1) * 0.05
    x[:, 2] += float(np.pi)
    starts = x.to(torch.float32).to(cuda_device)

    def timed(fn):
        fn()                                                     # warm-up
        best, out = float("inf"), None
        for _ in range(2):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            out = fn()
            t1.record()
            torch.cuda.synchronize()
            best = min(best, t0.elapsed_time(t1))
        return best, out
    t_fused, fused = timed(lambda: dp.rollout(starts, steps))
    t_loop, loop = timed(lambda: _step_by_step(dp, eng, starts, steps, 1.0, 0))
    print(f"{name} 50^4, m = {m}, {steps} steps: fused {t_fused:.2f} ms, step-by-step loop {t_loop:.2f} ms "
          f"({t_loop / t_fused:.1f}x), {m * steps / t_fused / 1e3:.1f} M episode-steps/s fused")
    _assert_same(fused, loop, "trained swing-up, fused vs loop", trajectory=False)
    assert t_fused < t_loop, f"fused {t_fused:.2f} ms is not faster than the loop's {t_loop:.2f} ms"
    s = fused.states
    theta = torch.atan2(torch.sin(s[:, 2]), torch.cos(s[:, 2])).abs()
    up = ((theta < 0.05) & (s[:, 3].abs() < 0.1) & ~fused.terminated).float().mean().item()
    assert up >= 0.99, f"only {up:.3f} of the poles were swung up and held"
    dp.close()
    eng.close()
