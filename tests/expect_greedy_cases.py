"""Inputs the expected-value greedy tests share (tests/test_expect_greedy_host.py, tests/test_gpu_expect_greedy.py): the
three grids, their multi-point disturbance sets and random value functions in the style of tests/test_expect_host.py."""
from __future__ import annotations

from itertools import product

import numpy as np

import oracle
from dynamicprogramming_amd import envs
from dynamicprogramming_amd.noise import Disturbances
from tests import helpers as H

GRIDS = [("pendulum", (24, 17)), ("cartpole_swingup", (9, 7, 11, 5)), ("double_cartpole_swingup", (5, 4, 6, 4, 5, 4))]
IDS = [name for name, _ in GRIDS]


def multi_point_set(name) -> Disturbances:
    """The multi-point rule of each grid: 8, 8 and 3 points."""
    if name == "pendulum":
        return Disturbances.uniform(2, state_noise=[0.2, 0.3], action_noise=0.5, points=2)
    if name == "cartpole_swingup":
        return Disturbances.uniform(4, state_noise=[0, 0.3, 0, 0.4], action_noise=2.0, points=2)
    return Disturbances.uniform(6, action_noise=3.0, points=3)


def case(name, shape, seed=0, scale=30.0) -> dict:
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    term, _ = H.terminal_mask(name, states)
    rng = np.random.default_rng(seed)
    V = (rng.standard_normal(len(states)) * scale).astype(np.float32)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return dict(name=name, bins=bins, grid=(lo, hi, gshape, strides), bits=bits, states=states, term=term, V=V,
                acts=H.edge_actions(name), gamma=float(np.float32(envs.ENVS[name].CONFIG["gamma"])),
                chk=H.oracle_for(name), D=len(bins))


def query_points(c, m, seed=1):
    """m points: inside, on nodes, up to 15 % outside the bounds (H.sample_states), one far outside, and — when there is
    room — one NaN coordinate."""
    pts = H.sample_states(np.random.default_rng(seed), c["bins"], m)
    pts[m // 2] *= 2.0
    if m > 3:
        pts[m - 2, c["D"] - 1] = np.nan
    return pts


def assert_same_rollout(a, b, what):
    def host(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    H.assert_bits_equal(host(a.states), host(b.states), f"{what}: final states")
    H.assert_bits_equal(host(a.returns), host(b.returns), f"{what}: returns")
    assert np.array_equal(host(a.lengths), host(b.lengths)), f"{what}: lengths"
    assert np.array_equal(host(a.terminated), host(b.terminated)), f"{what}: terminated"
    assert (a.trajectory is None) == (b.trajectory is None), what
    if a.trajectory is not None:
        H.assert_bits_equal(host(a.trajectory), host(b.trajectory), f"{what}: trajectory")
