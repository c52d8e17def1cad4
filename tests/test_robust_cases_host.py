"""
Without a GPU: the host-side helpers the worst-case edge tests lean on (tests/robust_cases.py) — the per-point q, the strict
fold and the three wrong folds that the GPU tests use to show that a case can tell them apart, and the fold's own sets.
"""
from __future__ import annotations

import numpy as np
import pytest

from dynamicprogramming_amd import envs, noise
from tests import helpers as H
from tests import robust_cases as RC
from tests.test_gpu_expect import _make_set
from tests.test_robust_host import _case

f32 = np.float32
NAN = f32(np.nan)


@pytest.mark.parametrize("name,shape", [("pendulum", (24, 17)), ("cartpole_swingup", (9, 7, 11, 5))])
def test_strict_fold_of_the_per_point_q_is_the_twin(name, shape):
    """Q and k* of robust_cases.fold over robust_cases.point_q equal noise.expected_q(risk="worst", worst_point=True), bit
    for bit, for S3 and for S3 with its 16 weight-0 rows; the fmin rule is np.fmin over the participating rows where no
    NaN and no zero is folded."""
    c = _case(name, shape)
    live = ~c["term"]
    pts, a = c["states"][live], c["acts"][c["pol"][live]]
    tables = (c["V"], c["acts"], *c["grid"], c["gamma"])
    s3 = _make_set("S3", c["D"], c["cell"], c["acts"])
    for d in (s3, RC.zero_weight_sets(s3)[0]):
        want_q, want_k = noise.expected_q(c["chk"].step, pts, a, d, *tables, risk="worst", worst_point=True)
        q = RC.point_q(c["chk"].step, pts, a, d, c["V"], c["acts"], c["grid"], c["gamma"])
        assert q.shape == (64, len(pts)) and np.isfinite(q).all() and (q != 0).all()
        got_q, got_k = RC.fold(q, d.weights)
        H.assert_bits_equal(got_q, want_q, f"{name}: Q of the host fold")
        assert np.array_equal(got_k, want_k)
        H.assert_bits_equal(RC.fold(q, d.weights, "fmin")[0], np.fmin.reduce(q[d.weights != 0], axis=0), f"{name}: fmin")
        H.assert_bits_equal(RC.fold(q, d.weights, "last-of-equals")[0], want_q, f"{name}: equal q have equal bits")


def test_the_folds_on_values_written_out():
    """One column per situation: a NaN in the middle, a NaN first, two NaNs, (+0, -0), (-0, +0), equal numbers, a smaller
    number under weight 0."""
    q = np.array([[1.0, NAN, 1.0, 0.0, -0.0, 2.0, 5.0],
                  [NAN, 1.0, NAN, -0.0, 0.0, 2.0, 1.0],
                  [0.5, 2.0, NAN, 0.0, -0.0, 2.0, 3.0]], f32)
    w = np.array([0.5, 0.0, 0.5], f32)
    every = np.full(3, 1.0 / 3.0, f32)

    def bits(rule, weights):
        Q, k = RC.fold(q, weights, rule)
        return [("nan" if np.isnan(x) else ("-0" if x == 0 and np.signbit(x) else float(x))) for x in Q], k.tolist()

    assert bits("strict", every) == (["nan", "nan", "nan", 0.0, "-0", 2.0, 1.0], [1, 0, 2, 0, 0, 0, 1])
    assert bits("fmin", every) == ([0.5, 1.0, 1.0, "-0", "-0", 2.0, 1.0], [2, 1, 0, 1, 0, 0, 1])
    assert bits("last-of-equals", every) == (["nan", "nan", "nan", 0.0, "-0", 2.0, 1.0], [1, 0, 2, 2, 2, 2, 1])
    assert bits("strict", w) == ([0.5, "nan", "nan", 0.0, "-0", 2.0, 3.0], [2, 0, 2, 0, 0, 0, 2])
    assert bits("zero-weight-rows-participate", w) == bits("strict", every)
    assert RC.differs(f32([NAN, 0.0, 1.0]), f32([-NAN, -0.0, 1.0])).tolist() == [False, True, False]


@pytest.mark.parametrize("name,shape", [("pendulum", (25, 41)), ("double_cartpole", (5, 4, 6, 4, 5, 4))])
def test_the_folds_own_sets_are_sets_the_library_takes(name, shape, tmp_path):
    """Weights of -0.0 and 1e-40, 63 rows of weight 0 with offsets of +-1e30: valid for noise.Disturbances (they were
    constructed) and for pi_set_disturbances on a host-only handle."""
    c = _case(name, shape)
    eng = H.host_engine(name, shape)
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)
    sets = RC.fold_sets(c["acts"], c["cell"], c["D"])
    assert set(sets) == {"last-row-only", "a-zero-a", "negative-zero-and-denormal-weights", "identical-rows"}
    for entry in sets.values():
        for d in entry if isinstance(entry, tuple) else (entry,):
            assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K
    d = sets["last-row-only"][0]
    assert d.K == 64 and (d.weights[:63] == 0).all() and d.weights[63] == 1
    d = sets["identical-rows"]
    assert np.array_equal(d.table()[0].view(np.uint32), d.table()[2].view(np.uint32))
    eng.close()
