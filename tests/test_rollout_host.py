"""
Closed-loop rollouts, the part that needs no GPU: the rollout kernel compiles for gfx950 behind every D, the
numpy twin (utils.barycentric.rollout) follows its definition, the envs' start distributions, the runner's
--rollout flag.  The device half is tests/test_gpu_rollout.py.
"""
from __future__ import annotations

from itertools import product

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from tests import helpers as H
from utils import barycentric as B


def _host_inference_engine(name, shape, cache_dir):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return _native.InferenceEngine(lo, hi, gshape, strides, bits, device=-1, cache_dir=cache_dir)


@pytest.mark.parametrize("name,shape", [("pendulum", (24, 17)), ("cartpole_swingup", (9, 7, 11, 5)),
                                        ("double_cartpole_swingup", (5, 4, 6, 4, 5, 4))])
def test_rollout_kernel_compiles_for_gfx950_without_a_gpu(name, shape, tmp_path):
    """pi_infer_set_dynamics on a host-only handle: grid + pi_math.h + plugin + csrc/pi_rollout_kernels.hip build through
    hipRTC into a second code object (next to the inference kernel's) that holds pi_rollout_kernel."""
    eng = _host_inference_engine(name, shape, tmp_path)
    before = set(tmp_path.glob("pi_*.hsaco"))
    assert len(before) == 1
    log = eng.set_dynamics(envs.dynamics_source(name))
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"pi_rollout_kernel" in blob
    eng.set_dynamics(envs.dynamics_source(name))                        # again: served from the cache, replaces
    assert len(list(tmp_path.glob("pi_*.hsaco"))) == 2
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.rollout(4096, 4, 10)
    eng.close()


def test_a_broken_plugin_is_reported_by_set_dynamics(tmp_path):
    eng = _host_inference_engine("pendulum", (8, 8), tmp_path)
    with pytest.raises(_native.NativeError) as exc:
        eng.set_dynamics("__device__ void step_dynamics(float a) { not valid C; }")
    assert "error" in str(exc.value).lower() and "rollout kernel compilation failed" in str(exc.value)
    assert len(list(tmp_path.glob("*.hsaco"))) == 1                      # the inference kernel only
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.rollout(4096, 4, 10)
    eng.close()


def test_rollout_kernel_does_not_spill(tmp_path):
    """The 6-D kernel keeps 64 weights and 64 indices live per lane next to the plugin's own registers: it must fit the
    512 registers a lane of a 256-thread workgroup may use without scratch; so must the others.  Checked on the
    ahead-of-time build of the translation unit pi_infer_set_dynamics hands to hipRTC (tests/helpers.inference_unit
    restates it from the header's description)."""
    for name, bins in (("pendulum", 200), ("cartpole_swingup", 50), ("double_cartpole", 25), ("double_cartpole_swingup", 25)):
        D = envs.ENVS[name]._D
        text = H.inference_unit(H.inference_grid(name, bins), name, "", ["pi_rollout_kernels.hip"])
        usage = H.kernel_resource_usage(text, tmp_path, name)
        k = usage["pi_rollout_kernel"]
        print(f"pi_rollout_kernel {name} {bins}^{D}: {k}")
        assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, k)


# ── the numpy twin ────────────────────────────────────────────────────────────────────────────────────────────────
def _stub_case():
    """A task on a 9 x 2 grid whose answer is known by hand: the policy names action +1 at every node, the stub env
    moves x by the (rounded: the interpolated sum of a constant may miss 1.0 by an ulp) action per step, pays the new x
    as reward and is done once x >= 3."""
    bits = np.array(list(product([0, 1], repeat=2)), dtype=np.int32)
    grid = dict(bounds_low=np.array([0.0, 0.0], np.float32), bounds_high=np.array([8.0, 1.0], np.float32),
                grid_shape=np.array([9, 2], np.int32), strides=np.array([2, 1], np.int32), corner_bits=bits)
    policy = np.ones(18, np.int32)                       # action index 1 -> value 1.0
    actions = np.array([-1.0, 1.0], np.float32)

    def step(states, acts):
        nxt = states.copy()
        nxt[:, 0] = states[:, 0] + np.round(acts)
        return nxt, nxt[:, 0].copy(), nxt[:, 0] >= 3.0
    return step, policy, actions, grid


def test_cpu_twin_follows_the_definition_on_a_hand_written_case():
    step, policy, actions, grid = _stub_case()
    starts = np.array([[0.0, 0.5], [2.0, 0.0], [-4.0, 1.0]], np.float32)      # the last one never reaches x = 3 in 5 steps
    res = B.rollout(step, starts, 5, policy, actions, gamma=0.5, record_every=2, **grid)
    assert isinstance(res, B.RolloutResult) and res._fields == ("states", "returns", "lengths", "terminated", "trajectory")
    # episode 0: x = 1, 2, 3 (done at step 3); episode 1: x = 3 (done at step 1); episode 2: x = -3 .. 1, not done
    assert res.lengths.dtype == np.int32 and res.lengths.tolist() == [3, 1, 5]
    assert res.terminated.dtype == bool and res.terminated.tolist() == [True, True, False]
    assert res.states.dtype == np.float32 and res.states.tolist() == [[3.0, 0.5], [3.0, 0.0], [1.0, 1.0]]
    # returns: sum_t 0.5^t x_{t+1}, float32 with exact terms here
    want = [1 + 0.5 * 2 + 0.25 * 3, 3.0, -3 - 0.5 * 2 - 0.25 * 1 + 0.125 * 0 + 0.0625 * 1]
    assert res.returns.dtype == np.float32 and res.returns.tolist() == want
    # rows after 0, 2, 4 steps; ended episodes repeat their last state
    assert res.trajectory.shape == (3, 3, 2) and res.trajectory.dtype == np.float32
    assert res.trajectory[:, :, 0].tolist() == [[0.0, 2.0, -4.0], [2.0, 3.0, -2.0], [3.0, 3.0, 0.0]]
    assert np.array_equal(res.trajectory[:, :, 1], np.broadcast_to(starts[:, 1], (3, 3)))
    assert np.array_equal(starts, np.array([[0.0, 0.5], [2.0, 0.0], [-4.0, 1.0]], np.float32))    # the input is not written
    # gamma = 1: the plain sum; no trajectory asked for, none returned; record_every == steps: start and end
    plain = B.rollout(step, starts, 5, policy, actions, **grid)
    assert plain.trajectory is None and plain.returns.tolist() == [6.0, 3.0, -5.0]
    ends = B.rollout(step, starts, 5, policy, actions, record_every=5, **grid)
    assert ends.trajectory.shape == (2, 3, 2) and np.array_equal(ends.trajectory[0], starts)
    assert np.array_equal(ends.trajectory[1], ends.states) and np.array_equal(ends.states, res.states)
    # zero steps: the start comes back, nothing ran
    none = B.rollout(step, starts, 0, policy, actions, record_every=0, **grid)
    assert np.array_equal(none.states, starts) and none.lengths.tolist() == [0, 0, 0] and not none.terminated.any()
    assert none.returns.tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        B.rollout(step, starts, 5, policy, actions, record_every=6, **grid)
    with pytest.raises(ValueError):
        B.rollout(step, starts, -1, policy, actions, **grid)


def test_cpu_twin_hands_the_step_only_running_episodes_and_sums_the_action_in_corner_order():
    """The action the twin feeds the env is the float32 sum over ascending corners (multiply, then add) of the module's
    own weights and indices; an ended episode is never stepped again."""
    name, shape = "cartpole", (7, 6, 9, 5)
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=4)), dtype=np.int32)
    rng = np.random.default_rng(3)
    actions = np.asarray(envs.ENVS[name].ACTIONS, np.float32)
    policy = rng.integers(0, len(actions), int(np.prod(shape))).astype(np.int32)
    chk = H.oracle_for(name)
    seen = []

    def step(states, acts):
        w, idx = B.get_barycentric_weights_and_indices(states, lo, hi, gshape, strides, bits)
        want = np.zeros(len(states), np.float32)
        for c in range(16):
            want = want + w[:, c] * actions[policy[idx[:, c]]]
        H.assert_bits_equal(acts, want, "action handed to the env")
        seen.append(len(states))
        return chk.step(states, acts)
    starts = H.sample_states(rng, bins, 200)
    res = B.rollout(step, starts, 60, policy, actions, lo, hi, gshape, strides, bits)
    assert res.terminated.any() and seen[0] == 200 and seen[-1] < 200 and all(a >= b for a, b in zip(seen, seen[1:]))
    assert np.array_equal(res.lengths == 60, ~res.terminated | (res.lengths == 60))
    assert (res.returns == res.lengths).all()                              # cartpole pays 1 per step, gamma = 1


def test_reference_mountain_car_policy_reaches_the_goal_from_every_evaluation_start():
    """The policy the REFERENCE produced for MountainCar-v0 (tests/golden/reference_results.npz), rolled out by the numpy
    twin on the plugin's dynamics from 64 of the env's own start states: every episode terminates — reaches the goal —
    within 200 steps, MountainCar-v0's own limit."""
    g = H.golden("reference_results")
    shape = tuple(int(x) for x in g["mountain_car_grid_shape"])
    bins = H.env_bins("mountain_car", shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=2)), dtype=np.int32)
    starts = envs.MountainCarCuda.start_states(np.random.default_rng(0), 64)
    res = B.rollout(H.oracle_for("mountain_car").step, starts, 200, g["mountain_car_policy"],
                    g["mountain_car_action_space"], lo, hi, gshape, strides, bits)
    print(f"mountain car: {int(res.terminated.sum())} of 64 reach the goal, steps {res.lengths.min()} .. {res.lengths.max()}")
    assert res.terminated.all(), f"only {int(res.terminated.sum())} of 64 starts reach the goal within 200 steps"
    assert (res.states[:, 0] >= 0.5).all() and res.lengths.max() <= 200
    assert np.array_equal(res.returns, -res.lengths.astype(np.float32))


# ── start distributions and the runner flag ───────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_start_states_of_every_env(name):
    cls = envs.ENVS[name]
    a = cls.start_states(np.random.default_rng(5), 500)
    assert a.shape == (500, cls._D) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(cls.DEFAULT_BINS).values()]
    lo, hi = np.array([t.min() for t in tabs]), np.array([t.max() for t in tabs])
    assert (a >= lo).all() and (a <= hi).all()
    assert np.array_equal(a, cls.start_states(np.random.default_rng(5), 500))
    assert not np.array_equal(a, cls.start_states(np.random.default_rng(6), 500))
    assert cls.start_states(np.random.default_rng(5), 0).shape == (0, cls._D)
    # the published ranges (gymnasium's resets; the reference runners' own numbers for the swing-ups and the crane)
    rng = {"pendulum": ([-np.pi, -1.0], [np.pi, 1.0]),
           "mountain_car": ([-0.6, 0.0], [-0.4, 0.0]), "continuous_mountain_car": ([-0.6, 0.0], [-0.4, 0.0]),
           "cartpole": ([-0.05] * 4, [0.05] * 4), "double_cartpole": ([-0.05] * 6, [0.05] * 6),
           "overhead_crane": ([2.4, 0.0, -0.05, 0.0], [2.6, 0.0, 0.05, 0.0])}.get(name)
    if rng is not None:
        assert (a >= np.float32(rng[0])).all() and (a <= np.float32(rng[1])).all()
        moving = np.float32(rng[0]) < np.float32(rng[1])
        assert (a.std(axis=0)[moving] > 0).all()
    else:                                                  # hanging down: angles within 0.05 of +-pi, at rest
        angles = {"cartpole_swingup": (2,), "double_pendulum_swingup": (0, 2), "double_cartpole_swingup": (2, 4)}[name]
        rest = [d for d in range(cls._D) if d not in angles and not (d == 0 and name != "double_pendulum_swingup")]
        assert (a[:, rest] == 0).all()
        for d in angles:
            assert (np.pi - np.abs(a[:, d].astype(np.float64)) <= 0.05 + 1e-6).all()
            assert (a[:, d] > 0).any() and (a[:, d] < 0).any()         # wrapped to both sides of the cut
        if name != "double_pendulum_swingup":
            assert (np.abs(a[:, 0]) <= np.float32(0.1)).all() and a[:, 0].std() > 0
    if name == "overhead_crane":
        b = cls.start_states(np.random.default_rng(5), 500, start_x=-1.0)
        assert (np.abs(b[:, 0] + 1.0) <= 0.1 + 1e-6).all() and np.array_equal(b[:, 1:], a[:, 1:])
        assert cls.start_states(np.random.default_rng(5), 50, start_x=9.0)[:, 0].max() <= np.float32(2.8)


@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_rollout_flag_is_off_by_default_and_claims_its_flags(name):
    from runners import _cli
    p = _cli.build_parser(name, f"results/{name}_cuda_policy.npz")
    assert p.parse_args([]).rollout is False
    argv = ["--episodes", "3", "--steps", "10", "--seed", "7", "--render", "--no-plot", "--record", "out.gif"]
    if name == "overhead_crane":
        argv += ["--start-x", "1.5"]
    without = _cli.ignored_flags(p.parse_args(argv))
    assert {"--episodes", "--steps", "--seed", "--render", "--no-plot", "--record"} <= set(without)
    assert ("--start-x" in without) == (name == "overhead_crane")
    a = p.parse_args(argv + ["--rollout"])
    assert a.rollout is True
    assert _cli.ignored_flags(a) == ["--render", "--record", "--no-plot"]


def test_solver_rollout_without_a_gpu_raises_instead_of_computing_elsewhere(tmp_path):
    """A load()ed instance has the rollout method; without a GPU it raises (no CPU fallback in the product)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    g = H.golden("reference_results")
    shape = tuple(int(x) for x in g["mountain_car_grid_shape"])
    bins = H.env_bins("mountain_car", shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    path = tmp_path / "mc.npz"
    np.savez(path, value_function=g["mountain_car_value_function"], policy=g["mountain_car_policy"], bounds_low=lo,
             bounds_high=hi, grid_shape=gshape, strides=strides,
             corner_bits=np.array(list(product([0, 1], repeat=2)), dtype=np.int32),
             action_space=g["mountain_car_action_space"], states_space=oracle.states_from_bins(bins))
    pi = envs.MountainCarCuda.load(path)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        pi.rollout(envs.MountainCarCuda.start_states(np.random.default_rng(0), 4), 10)
