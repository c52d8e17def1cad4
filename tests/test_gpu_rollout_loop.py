"""
The episode loop the five fused rollouts share (pi_rollout_episodes in csrc/pi_rollout_kernels.hip) under every controller
that runs on it — the policy table (pi_infer_rollout), two policies (pi_infer_rollout_hybrid), the lookahead
(pi_infer_rollout_greedy), the policy under noise (pi_infer_rollout_stochastic) and the expected lookahead under noise
(pi_infer_rollout_expect_greedy): the edge cases of tests/test_gpu_rollout.py::test_rollout_edge_cases on its grid, each
launch compared bit for bit with the controller's numpy twin on the oracle's step.  What a controller hands the loop
wrongly — the episode number of the random stream, the mode of the hybrid, the successor the lookahead kept — shows here
for the controllers whose own tests run ragged batches but not these shapes.  Every GPU step runs once; nothing retries.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from dynamicprogramming_amd import envs, noise
from dynamicprogramming_amd.noise import Disturbances
from tests import expect_greedy_cases as C
from tests import hybrid_cases
from utils import barycentric as B

pytestmark = pytest.mark.gpu
NAME, SHAPE = "cartpole", (9, 8, 11, 7)                   # 5 544 nodes
SHAPE2 = (6, 5, 7, 5)                                     # the hybrid partner: a narrower box round the upright pole
BOX2 = ((-1.2, -1.5, -0.1, -1.0), (1.2, 1.5, 0.1, 1.0))
ENTER, LEAVE = np.array([np.inf, np.inf, 0.05, 0.5], np.float32), np.array([np.inf, np.inf, 0.1, 1.0], np.float32)
GAMMA = 0.9
BATCHES = (1, 65, 257)                                    # one lane; one wave and a lane; one workgroup and a lane
HORIZONS = ((0, 0), (1, 1), (40, 3))                      # (n_steps, record_every)
NOISE = dict(epsilon=0.5, action_noise=2.0, state_noise=[0.01, 0.0, 0.02, 0.05], seed=2 ** 40 + 3,
             first_episode=2 ** 32 - 100)                 # the episode numbers carry into the counter's high word
CONTROLLERS = ("policy", "hybrid", "greedy", "stochastic", "expected")


@lru_cache(maxsize=None)
def _case():
    c = C.case(NAME, SHAPE)
    rng = np.random.default_rng(17)
    c["policy"] = rng.integers(0, len(c["acts"]), int(np.prod(SHAPE))).astype(np.int32)
    bins2 = [np.linspace(l, h, g, dtype=np.float32) for l, h, g in zip(*BOX2, SHAPE2)]
    acts2 = np.array([-5.0, 0.0, 5.0], np.float32)
    policy2 = rng.integers(0, len(acts2), int(np.prod(SHAPE2))).astype(np.int32)
    c["primary"] = (c["policy"], c["acts"], *c["grid"], c["bits"])
    c["secondary"] = (policy2, acts2) + hybrid_cases.tables(bins2)
    c["starts"] = (rng.uniform(-1, 1, (257, 4)) * [1.0, 1.0, 0.15, 1.0]).astype(np.float32)
    # a whole wave off the track: every episode of it ends on its first step; lane 64 (the next wave) goes on
    c["fallen"] = c["starts"][:65].copy()
    c["fallen"][:64, 0] = 5.0
    c["dist"] = Disturbances.uniform(4, state_noise=[0, 0.3, 0, 0.4], action_noise=2.0, points=2)
    return c


def _controller(kind, c, cuda_device):
    """(device rollout, numpy twin, handles to close): both take (starts, n_steps, record_every)."""
    step, g, kw = c["chk"].step, c["gamma"], dict(gamma=GAMMA)
    dyn = envs.dynamics_source(NAME)
    if kind in ("policy", "stochastic", "hybrid"):
        dp = B.DevicePolicy(*c["primary"], device=cuda_device)
        dp.set_dynamics(dyn)
    else:
        dp = B.DevicePolicy(None, c["acts"], *c["grid"], c["bits"], device=cuda_device)     # no policy table
        dp.set_values(c["V"])
        dp.set_dynamics(dyn)
    if kind == "policy":
        return (lambda s, n, e: dp.rollout(s, n, record_every=e, **kw),
                lambda s, n, e: B.rollout(step, s, n, *c["primary"], record_every=e, **kw), [dp])
    if kind == "hybrid":
        dp2 = B.DevicePolicy(*c["secondary"], device=cuda_device)
        hp = B.HybridPolicy(dp, dp2, ENTER, LEAVE)
        return (lambda s, n, e: hp.rollout(s, n, record_every=e, **kw),
                lambda s, n, e: B.hybrid_rollout(step, s, n, c["primary"], c["secondary"], ENTER, LEAVE, record_every=e, **kw),
                [dp, dp2])
    if kind == "greedy":
        dp.set_greedy()
        return (lambda s, n, e: dp.rollout(s, n, record_every=e, controller="greedy", lookahead_gamma=g, **kw),
                lambda s, n, e: B.greedy_rollout(step, s, n, c["V"], c["acts"], *c["grid"], g, record_every=e, **kw), [dp])
    if kind == "stochastic":
        dp.set_stochastic()
        return (lambda s, n, e: dp.rollout(s, n, record_every=e, **kw, **NOISE),
                lambda s, n, e: B.stochastic_rollout(step, s, n, *c["primary"], NOISE["epsilon"], NOISE["action_noise"],
                                                     NOISE["state_noise"], NOISE["seed"],
                                                     first_episode=NOISE["first_episode"], record_every=e, **kw), [dp])
    dp.set_expected_greedy()
    dp.set_disturbances(c["dist"])
    return (lambda s, n, e: dp.rollout(s, n, record_every=e, controller="expected", lookahead_gamma=g, **kw, **NOISE),
            lambda s, n, e: noise.expected_greedy_rollout(step, s, n, c["dist"], c["V"], c["acts"], *c["grid"], g,
                                                          record_every=e, **kw, **NOISE), [dp])


def _assert_same(got, want, what):
    C.assert_same_rollout(got, want, what)                   # bit patterns: -0.0 and NaN payloads count
    if hasattr(want, "secondary_steps"):
        assert np.array_equal(got.secondary_steps, want.secondary_steps), f"{what}: secondary_steps"
        assert np.array_equal(got.last_mode, want.last_mode), f"{what}: last_mode"


@pytest.mark.parametrize("kind", CONTROLLERS)
def test_every_controller_runs_the_shared_loop_to_its_twins_bits(kind, cuda_device):
    c = _case()
    device, twin, handles = _controller(kind, c, cuda_device)
    for m in BATCHES:
        for steps, every in HORIZONS:
            starts = c["starts"][:m]
            got, want = device(starts, steps, every), twin(starts, steps, every)
            _assert_same(got, want, f"{kind} m={m} steps={steps} every={every}")
            assert (got.trajectory is None) == (every == 0)
            if every:
                assert got.trajectory.shape == (steps // every + 1, m, 4) and np.array_equal(got.trajectory[0], starts)
            if steps == 0:
                assert np.array_equal(got.states, starts) and not got.lengths.any() and not got.returns.any()
                assert not got.terminated.any()
    # what the largest run exercised, from the twin: ended episodes beside running ones, and both of the hybrid's modes
    assert 0 < want.terminated.sum() < len(want.terminated) and len(np.unique(want.lengths)) > 2, kind
    if kind == "hybrid":
        assert 0 < want.last_mode.sum() < len(want.last_mode) and 0 < (want.secondary_steps > 0).sum()
    # a wave that leaves the loop after its first step with trajectory rows still to write: they repeat the last state
    got, want = device(c["fallen"], 40, 3), twin(c["fallen"], 40, 3)
    assert (want.lengths[:64] == 1).all() and want.terminated[:64].all() and want.lengths[64] > 3, kind
    _assert_same(got, want, f"{kind}: a whole wave ends on its first step")
    assert got.trajectory.shape == (14, 65, 4)
    assert (got.trajectory[1:, :64] == got.states[None, :64]).all() and not (got.trajectory[0, :64] == got.states[:64]).all()
    for h in handles:
        h.close()
