"""
Expected-value greedy control on the device (csrc/pi_expect_greedy_kernels.hip behind pi_infer_expect_greedy /
pi_infer_rollout_expect_greedy, DevicePolicy.expected_greedy, DevicePolicy.rollout(controller="expected"),
solver.rollout(controller="expected"), the runners' --controller expected): the query must equal, bit for bit, the numpy
twin on the checker's step, the greedy module with the zero set and the expectation improvement sweep of a solver handle
at the live nodes; the fused rollout the twin, the greedy and the stochastic rollouts where it reduces to them, and the
per-step loop it replaces.  Every GPU step runs once; nothing retries.

A NaN query coordinate makes a row of NaN in the Q matrix.  IEEE 754 leaves the sign and payload of a propagated NaN to
the implementation and the definition of Q does not set them, so those entries are compared as NaN (as
tests/test_gpu_endtoend.py compares the plugin's NaN results); every other entry, and every other output, by its bits.
"""
from __future__ import annotations

import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd.noise import Disturbances
from tests import expect_greedy_cases as C
from tests import helpers as H
from utils import barycentric as B

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
M, STEPS, EVERY = 300, 60, 7                       # 300 episodes: ragged against the 256-lane workgroup
SEED, FIRST = 2 ** 40 + 3, 2 ** 32 - 100           # the episode numbers carry into the counter's high word
WORLD = {"pendulum": dict(action_noise=0.5, state_noise=[0.02, 0.0]),
         "cartpole_swingup": dict(action_noise=2.0, state_noise=[0.01, 0.0, 0.02, 0.05]),
         "double_cartpole_swingup": dict(action_noise=3.0, state_noise=[0.01, 0.0, 0.02, 0.0, 0.01, 0.03])}


def _torch():
    import torch
    return torch


@lru_cache(maxsize=None)
def _case(name):
    c = C.case(name, dict(C.GRIDS)[name])
    c["starts"] = H.sample_states(np.random.default_rng(3), c["bins"], M)
    return c


def _setting(name, which):
    """(disturbance set, the noise of the world) of the rollout settings (a) .. (d)."""
    D = _case(name)["D"]
    return {"a": (Disturbances.none(D), {}), "b": (C.multi_point_set(name), {}),
            "c": (C.multi_point_set(name), dict(epsilon=0.3, **WORLD[name])),
            "d": (C.multi_point_set(name), dict(epsilon=1.0, **WORLD[name]))}[which]


@lru_cache(maxsize=None)
def _twin(name, which):
    """The numpy twin of one setting with the trajectory, computed once."""
    c = _case(name)
    dist, world = _setting(name, which)
    return noise.expected_greedy_rollout(c["chk"].step, c["starts"], STEPS, dist, c["V"], c["acts"], *c["grid"], c["gamma"],
                                         gamma=0.99, record_every=EVERY, seed=SEED, first_episode=FIRST, **world)


def _controller(c, cuda_device, greedy=False, stochastic=False):
    """A DevicePolicy WITHOUT a policy table, with values, plugin and the expected-greedy module."""
    dp = B.DevicePolicy(None, c["acts"], *c["grid"], c["bits"], device=cuda_device)
    dp.set_values(c["V"])
    dp.set_dynamics(envs.dynamics_source(c["name"]))
    assert isinstance(dp.set_expected_greedy(), str)
    if greedy:
        dp.set_greedy()
    if stochastic:
        dp.set_stochastic()
    return dp


def _assert_query(got, want, what):
    got = [x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in got]
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), \
        f"{what}: {int((got[0] != want[0]).sum())} greedy indices differ"
    H.assert_bits_equal(got[1], want[1], f"{what}: action value")
    H.assert_bits_equal(got[2], want[2], f"{what}: best Q")
    if len(got) > 3:
        nan = np.isnan(want[3])
        assert np.array_equal(np.isnan(got[3]), nan), f"{what}: NaN entries of the Q matrix"
        H.assert_bits_equal(got[3][~nan], want[3][~nan], f"{what}: Q matrix")


def _objects():
    return len(list(Path(_native.KERNEL_CACHE).glob("pi_*.hsaco")))


# ── 7. the query ──────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name", C.IDS)
def test_query_equals_the_twin_and_with_the_zero_set_the_greedy_module(name, cuda_device):
    torch = _torch()
    c = _case(name)
    dp = _controller(c, cuda_device, greedy=True)
    sets = [("zero set", Disturbances.none(c["D"])), ("multi-point set", C.multi_point_set(name))]
    if name == "pendulum":
        sets.append(("64 points", Disturbances.uniform(2, state_noise=[0.2, 0.3], points=8)))
        assert sets[-1][1].K == 64
    g = c["gamma"]
    objects = _objects()
    for label, dist in sets:
        dp.set_disturbances(dist)
        for m in (300, 5):
            pts = C.query_points(c, m)
            inside = (pts >= c["grid"][0]) & (pts <= c["grid"][1])
            assert np.isnan(pts).sum() == 1 and (~inside).sum() > 1               # one NaN, and points outside the bounds
            what = f"{name} {label} m={m}"
            want = noise.expected_greedy_action(c["chk"].step, pts, dist, c["V"], c["acts"], *c["grid"], g, q_values=True)
            assert np.isnan(want[3]).any() and not np.isnan(want[2]).any()
            got = dp.expected_greedy(pts, g, q_values=True)                          # numpy in -> numpy out
            assert all(isinstance(x, np.ndarray) for x in got) and got[3].shape == (m, len(c["acts"]))
            _assert_query(got, want, what)
            d_pts = torch.from_numpy(pts).to(cuda_device)
            on_dev = dp.expected_greedy(d_pts, g)                                    # a device tensor in -> tensors out
            assert len(on_dev) == 3 and all(torch.is_tensor(x) and x.device == d_pts.device for x in on_dev)
            _assert_query(on_dev, want, what + " device tensor in")
            assert torch.equal(d_pts.cpu().view(torch.int32), torch.from_numpy(pts).view(torch.int32))   # not written
            if dist.K == 1:
                _assert_query(got, dp.greedy(pts, g, q_values=True), what + " against DevicePolicy.greedy")
    empty = dp.expected_greedy(np.zeros((0, c["D"]), np.float32), g, q_values=True)
    assert empty[0].shape == (0,) and empty[3].shape == (0, len(c["acts"]))
    assert _objects() == objects, "another set is an upload, never a build"
    dp.close()


# ── 8. the sweep module against the inference module ──────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name", C.IDS)
def test_query_at_the_live_nodes_is_the_policy_of_the_expectation_sweep(name, cuda_device):
    torch = _torch()
    c = _case(name)
    dist = C.multi_point_set(name)
    bins = c["bins"]
    eng = _native.Engine(c["D"], [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins, c["acts"],
                         device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source(name))
    assert eng.set_disturbances(dist.action_offsets, dist.state_offsets, dist.weights) == dist.K

    def put(a):
        return torch.from_numpy(np.array(eng.to_memory(np.asarray(a)), order="C", copy=True)).to(cuda_device)
    n = len(c["states"])
    d_V, d_pol, d_term = put(c["V"]), put(np.zeros(n, np.int32)), put(c["term"].astype(np.uint8))
    eng.expect_improve_sweep(d_V.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), 0, n, c["gamma"])
    torch.cuda.synchronize()
    policy = np.ascontiguousarray(eng.to_user(d_pol.cpu().numpy()))
    eng.close()
    live = ~c["term"]
    dp = _controller(c, cuda_device)
    dp.set_disturbances(dist)
    best, act, _ = dp.expected_greedy(np.ascontiguousarray(c["states"][live], np.float32), c["gamma"])
    dp.close()
    assert np.array_equal(best, policy[live]), f"{int((best != policy[live]).sum())} of {int(live.sum())} nodes differ"
    H.assert_bits_equal(act, c["acts"][policy[live]], "action values")
    assert len(np.unique(best)) > 1


# ── 9. the fused rollout ──────────────────────────────────────────────────────────────────────────────────────────────
def _step_by_step(dp, eng, c, world):
    """The loop the fused kernel replaces: per time step one expected_greedy launch, the stream's words
    (random_words), one plugin-step launch (pi_probe_step) and the mixing of the rollout's definition on the host."""
    torch = _torch()
    dev = dp.device
    acts, m, D = c["acts"], M, c["D"]
    a_min, a_max = acts.min(), acts.max()
    eps24 = B.explore_threshold(world["epsilon"])
    an, sn = np.float32(world["action_noise"]), np.asarray(world["state_noise"], np.float32)
    s = c["starts"].copy()
    ret, length = np.zeros(m, np.float32), np.zeros(m, np.int32)
    ended = np.zeros(m, bool)
    disc, g = np.float32(1.0), np.float32(0.99)
    rows = [s.copy()]
    d_nxt = torch.empty((m, D), dtype=torch.float32, device=dev)
    d_rew = torch.empty(m, dtype=torch.float32, device=dev)
    d_done = torch.empty(m, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for t in range(STEPS):
        d_s = torch.from_numpy(s).to(dev)
        a = dp.expected_greedy(d_s, c["gamma"])[1].cpu().numpy()
        w0 = dp.random_words(SEED, FIRST, m, t, 0)
        explore = (w0[:, 0] >> np.uint32(8)) < eps24
        a = np.where(explore, acts[B.random_action_index(w0[:, 1], len(acts))], a).astype(np.float32)
        a = np.fmin(np.fmax(a + an * B.sym(w0[:, 2]), a_min), a_max)
        d_a = torch.from_numpy(a).to(dev)
        eng.probe_step(d_s.data_ptr(), d_a.data_ptr(), d_nxt.data_ptr(), d_rew.data_ptr(), d_done.data_ptr(), m, st)
        torch.cuda.synchronize()
        nxt, rew, done = d_nxt.cpu().numpy(), d_rew.cpu().numpy(), d_done.cpu().numpy() != 0
        words = dp.random_words(SEED, FIRST, m, t, 1)
        if D > 4:
            words = np.concatenate([words, dp.random_words(SEED, FIRST, m, t, 2)], axis=1)
        go = ~done
        for d in range(D):
            if sn[d] != 0:
                nxt[go, d] = nxt[go, d] + sn[d] * B.sym(words[go, d])
        run = ~ended
        ret[run] = ret[run] + disc * rew[run]
        s[run] = nxt[run]
        length[run] = t + 1
        ended |= run & done
        disc = np.float32(disc * g)
        if (t + 1) % EVERY == 0:
            rows.append(s.copy())
    return B.RolloutResult(s, ret, length, ended, np.stack(rows))


def _drop_trajectory(res):
    return B.RolloutResult(res.states, res.returns, res.lengths, res.terminated, None)


@pytest.mark.parametrize("name", C.IDS)
def test_fused_rollout_equals_the_twin_in_every_setting(name, cuda_device):
    torch = _torch()
    c = _case(name)
    starts, g = c["starts"], c["gamma"]
    dp = _controller(c, cuda_device, greedy=True, stochastic=True)
    d_starts = torch.from_numpy(starts).to(cuda_device)
    objects = _objects()
    run = lambda s, first=FIRST, every=EVERY, **kw: dp.rollout(                                      # noqa: E731
        s, STEPS, gamma=0.99, record_every=every, controller="expected", lookahead_gamma=g, seed=SEED, first_episode=first, **kw)
    fused = {}
    for which in "abcd":
        dist, world = _setting(name, which)
        twin = _twin(name, which)
        if which == "b" and name != "pendulum":                                  # the freeze path, asserted on the twin
            ends = twin.lengths[twin.terminated]
            print(f"{name}: {len(ends)} of {M} episodes terminated, on steps {ends.min()} .. {ends.max()}")
            assert 0 < len(ends) < M and len(np.unique(ends)) > 1, "episodes must end on different steps"
        dp.set_disturbances(dist)
        fused[which] = run(d_starts, **world)                                    # tensors in -> tensors out
        assert torch.is_tensor(fused[which].states) and fused[which].lengths.dtype == torch.int32
        C.assert_same_rollout(fused[which], twin, f"{name} ({which}) every={EVERY}")
        plain = run(starts, every=0, **world)                                    # numpy in -> numpy out, no trajectory
        assert isinstance(plain.states, np.ndarray) and plain.trajectory is None
        C.assert_same_rollout(plain, _drop_trajectory(twin), f"{name} ({which}) every=0")
        if which == "a":
            C.assert_same_rollout(fused["a"], dp.rollout(d_starts, STEPS, gamma=0.99, record_every=EVERY, controller="greedy",
                                                         lookahead_gamma=g), f"{name} (a) against the greedy rollout")
        if which == "d":
            C.assert_same_rollout(fused["d"], dp.rollout(d_starts, STEPS, gamma=0.99, record_every=EVERY, controller="random",
                                                         seed=SEED, first_episode=FIRST, **WORLD[name]),
                                  f"{name} (d) against the random baseline")
        if which == "c":                                                         # a cut batch equals the whole
            a, b = run(starts[:100], **world), run(starts[100:], first=FIRST + 100, **world)
            joined = B.RolloutResult(*(np.concatenate([x, y], axis=1 if x.ndim == 3 else 0) for x, y in zip(a, b)))
            C.assert_same_rollout(joined, twin, f"{name} (c) 100 + 200 episodes")
    assert not torch.equal(fused["a"].returns, fused["b"].returns), "another set must change the results"
    assert not torch.equal(fused["b"].returns, fused["c"].returns)
    assert _objects() == objects, "another set is an upload, never a build"
    assert torch.equal(d_starts.cpu(), torch.from_numpy(starts))                 # the start states are not written
    if name == "cartpole_swingup":                                               # ... and the loop it replaces
        bins = c["bins"]
        eng = _native.Engine(c["D"], [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins,
                             c["acts"], device=cuda_device.index or 0)
        eng.compile(envs.dynamics_source(name))
        dist, world = _setting(name, "c")
        dp.set_disturbances(dist)
        C.assert_same_rollout(fused["c"], _step_by_step(dp, eng, c, world), f"{name} (c) fused against the per-step loop")
        eng.close()
    zero = dp.rollout(starts, 0, controller="expected", lookahead_gamma=g)       # zero steps: the starts come back
    assert np.array_equal(zero.states, starts) and not zero.lengths.any() and not zero.terminated.any()
    # a new plugin drops the module (not the set) until set_expected_greedy is called again
    dp.set_dynamics(envs.dynamics_source(name))
    with pytest.raises(RuntimeError, match="set_expected_greedy"):
        run(starts)
    with pytest.raises(RuntimeError, match="set_expected_greedy"):
        dp.expected_greedy(starts, g)
    with pytest.raises(_native.NativeError, match="no expected-greedy module"):
        dp._engine.rollout_expect_greedy(d_starts.data_ptr(), M, 5, g)
    dp.close()


# ── 10. solver and runner ─────────────────────────────────────────────────────────────────────────────────────────────
def test_solver_expected_rollout_and_the_runner_flag(cuda_device, tmp_path):
    dist = Disturbances.uniform(2, state_noise=[0.05, 0.1], action_noise=0.3, points=2)
    world = dict(action_noise=0.3, state_noise=[0.05, 0.1], seed=7)
    starts = envs.PendulumCuda.start_states(np.random.default_rng(1), 300)

    def by_hand(pi, the_set):
        dp = B.DevicePolicy(None, pi.action_space, pi.bounds_low, pi.bounds_high, pi.grid_shape, pi.strides, pi.corner_bits,
                            device=cuda_device)
        dp.set_values(pi.value_function)
        dp.set_dynamics(envs.dynamics_source("pendulum"))
        dp.set_expected_greedy()
        dp.set_disturbances(the_set)
        out = dp.rollout(starts, 60, gamma=0.99, record_every=20, controller="expected", lookahead_gamma=pi.config.gamma,
                         **world)
        dp.close()
        return out
    solver = envs.make("pendulum", 25)
    solver.set_disturbances(dist)
    solver.run()
    got = solver.rollout(starts, 60, gamma=0.99, record_every=20, controller="expected", **world)
    C.assert_same_rollout(got, by_hand(solver, dist), "solver.rollout(controller='expected')")
    assert isinstance(got.states, np.ndarray) and got.trajectory.shape == (4, 300, 2) and (got.lengths == 60).all()
    other = solver.rollout(starts, 60, gamma=0.99, record_every=20, controller="expected", disturbances=Disturbances.none(2),
                           **world)
    C.assert_same_rollout(other, by_hand(solver, Disturbances.none(2)), "disturbances= overrides the solver's set")
    table = solver.rollout(starts, 60, gamma=0.99, record_every=20, **world)     # the policy table under the same noise
    assert table.trajectory.shape == (4, 300, 2)
    with pytest.raises(ValueError, match="stochastic greedy controller does not exist"):
        solver.rollout(starts, 60, controller="greedy", **world)
    solver.save(tmp_path / "noisy.npz")

    vi = envs.make("pendulum", 25)
    vi.set_disturbances(dist)
    vi.value_iteration()
    assert getattr(vi, "value_function", None) is None                           # nothing pulled to the host yet
    res = vi.rollout(starts[:10], 20, controller="expected", **world)
    assert res.states.shape == (10, 2) and (res.lengths == 20).all() and np.isfinite(res.returns).all()

    loaded = envs.PendulumCuda.load(tmp_path / "noisy.npz")                      # the archive carries its set
    assert loaded.disturbances is not None and loaded.disturbances.K == dist.K
    C.assert_same_rollout(loaded.rollout(starts, 60, gamma=0.99, record_every=20, controller="expected", **world),
                          by_hand(loaded, loaded.disturbances), "a load()ed archive")

    res = subprocess.run([sys.executable, str(ROOT / "runners" / "pendulum_cuda.py"), "--bins", "25", "--retrain", "--rollout",
                          "--controller", "expected", "--action-noise", "0.3", "--state-noise", "0.05", "0.1", "--episodes",
                          "3", "--steps", "50", "--save-path", str(tmp_path / "p.npz")],
                         cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "accepted and ignored" not in res.stdout and "expected lookahead over 27 disturbance points" in res.stdout
    lines = [line for line in res.stdout.splitlines() if line.startswith("Episode ")]
    assert len(lines) == 3 and all("50 steps | return = " in line and "final state:" in line for line in lines)
