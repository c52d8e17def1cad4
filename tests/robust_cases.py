"""Disturbance sets and host folds shared by the worst-case tests (tests/test_robust_host.py, tests/test_gpu_robust.py,
tests/test_gpu_robust_edges.py, tests/test_gpu_adversary_edges.py, tests/test_robust_cases_host.py)."""
from __future__ import annotations

import numpy as np

from dynamicprogramming_amd.noise import Disturbances

# Rows of a 64-point set whose da comes in runs of 8 (S3 of tests/test_gpu_expect.py) that are rewritten to weight 0:
# row 0, the first (8, 16, 40), inner (1, 5, 12, 27, 36, 50, 57) and last (15, 23, 31, 47, 63) rows of runs.
ZERO_ROWS = (0, 1, 5, 8, 12, 15, 16, 23, 27, 31, 36, 40, 47, 50, 57, 63)


def zero_weight_sets(full: Disturbances):
    """(set with zero-weight rows, the set without them, kept row indices) of a 64-point set `full`.  The 16 rows of
    ZERO_ROWS get weight 0 and offsets of +-1e30 — da and every dx, alternating in sign — which would change every result
    if they took part: da = +-1e30 clamps the action to an extreme and breaks every run it sits in, dx = +-1e30 clamps the
    successor to a border.  The other 48 keep their offsets and share the weights renormalised in float64; both sets
    hold the same float32 weights for them."""
    assert full.K == 64
    zero = np.zeros(64, bool)
    zero[list(ZERO_ROWS)] = True
    kept = np.flatnonzero(~zero)
    w = full.weights.astype(np.float64)
    w[zero] = 0.0
    w = (w / w.sum()).astype(np.float32)
    sign = np.where(np.arange(64) % 2 == 0, np.float32(1e30), np.float32(-1e30))
    da, dx = full.action_offsets.copy(), full.state_offsets.copy()
    da[zero] = sign[zero]
    dx[zero] = sign[zero, None] * np.where(np.arange(full.D) % 2 == 0, np.float32(1.0), np.float32(-1.0))[None, :]
    return Disturbances(da, dx, w), Disturbances(da[kept], dx[kept], w[kept]), kept


# ---- the fold on the host: per-point q and the point loop under the strict rule and under three wrong ones -------------
# (tests/test_gpu_robust_edges.py and tests/test_gpu_adversary_edges.py assert from these that a case can tell the rules apart)
FOLDS = ("strict", "fmin", "last-of-equals", "zero-weight-rows-participate")


def point_q(step, states, action_values, d, V, acts, grid, gamma):
    """(K, m) float32: q_k = r_k + gamma * E_k of EVERY row of `d` (weight 0 or not) at `states` under the action values
    `action_values` (m,) or a scalar — through the twin's own step and interpolation: noise.expected_q on the one-point
    set {(da_k, dx_k, 1)} with risk="worst", whose fold of one point is that point's q."""
    from dynamicprogramming_amd import noise
    pts = np.ascontiguousarray(np.atleast_2d(states), dtype=np.float32)
    q = np.empty((d.K, len(pts)), np.float32)
    for k in range(d.K):
        one = Disturbances(d.action_offsets[k:k + 1], d.state_offsets[k:k + 1], [1.0])
        q[k] = noise.expected_q(step, pts, action_values, one, V, acts, *grid, gamma, risk="worst")
    return q


def fold(q, weights, rule="strict"):
    """(Q (m,), k* (m,)) of the point loop over q (K, m) in ascending k.  "strict" is the definition: rows of weight 0
    are skipped, the first participating row gives Q, a later one replaces it where q < Q or q is NaN.  The wrong rules:
    "fmin": Q = fminf(Q, q) as the device's minimum instruction computes it — a NaN operand is dropped, -0 is below +0
    (np.fmin agrees wherever neither matters; it leaves the sign of a zero tie open, so it is spelt out here);
    "last-of-equals": q <= Q replaces; "zero-weight-rows-participate": the strict rule over every row."""
    assert rule in FOLDS
    K, m = q.shape
    Q, k_star, started = np.zeros(m, np.float32), np.full(m, -1, np.int32), False
    for k in range(K):
        if weights[k] == 0 and rule != "zero-weight-rows-participate":
            continue
        qk = q[k]
        with np.errstate(invalid="ignore"):
            if not started:
                take = np.ones(m, bool)
            elif rule == "fmin":
                take = ~np.isnan(qk) & (np.isnan(Q) | (qk < Q) | ((qk == Q) & np.signbit(qk) & ~np.signbit(Q)))
            elif rule == "last-of-equals":
                take = (qk <= Q) | (qk != qk)
            else:
                take = (qk < Q) | (qk != qk)
        Q, k_star, started = np.where(take, qk, Q), np.where(take, np.int32(k), k_star), True
    return Q, k_star


def differs(a, b):
    """Where two float32 arrays differ in bits, a NaN equal to a NaN of any payload."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def fold_sets(acts, cell, D, seed=31):
    """The sets that exist for the fold's own control flow (`started`, the skip of a weight-0 row, the runs of equal da),
    as {name: set or tuple of sets that must give the same bits}."""
    acts, cell = np.asarray(acts, np.float32), np.asarray(cell, np.float64)
    arange = float(acts.max() - acts.min()) or 1.0
    rng = np.random.default_rng(seed)
    f32 = np.float32
    sets = {}
    # (i) K = 64, rows 0 .. 62 at weight 0 with offsets of +-1e30, only row 63 takes part: that row alone at K = 1
    sign = np.where(np.arange(64) % 2 == 0, f32(1e30), f32(-1e30))
    da = sign.copy()
    dx = sign[:, None] * np.where(np.arange(D) % 2 == 0, f32(1.0), f32(-1.0))[None, :]
    w = np.zeros(64, f32)
    da[63], dx[63], w[63] = f32(0.19 * arange), (rng.uniform(-0.8, 0.8, size=D) * cell).astype(f32), 1.0
    sets["last-row-only"] = (Disturbances(da, dx, w), Disturbances(da[63:], dx[63:], [1.0]))
    # (ii) A, B (weight 0), A: the second A shares the first A's step — the two-row set A, A.  B would move every value
    A, B = f32(0.21 * arange), f32(-1e30)
    dx = (rng.uniform(-0.7, 0.7, size=(3, D)) * cell).astype(f32)
    dx[1] = f32(1e30)
    sets["a-zero-a"] = (Disturbances([A, B, A], dx, [0.5, 0.0, 0.5]), Disturbances([A, A], dx[[0, 2]], [0.5, 0.5]))
    # (iii) A, B, A with every weight non-zero is "a-b-a" of tests/test_gpu_expect_edges._edge_sets
    # (iv) weights -0.0 (== 0.0f: skipped) and a denormal (!= 0.0f: takes part); the twin decides
    dx = (rng.uniform(-0.9, 0.9, size=(4, D)) * cell).astype(f32)
    dx[0] = f32(1e30) * np.where(np.arange(D) % 2 == 0, f32(1.0), f32(-1.0))
    w = np.array([-0.0, 1e-40, 0.5, 0.5], f32)
    assert np.signbit(w[0]) and 0 < w[1] < np.finfo(f32).tiny
    sets["negative-zero-and-denormal-weights"] = Disturbances(np.array([1e30, -0.3, 0.0, 0.25], f32) * f32(arange), dx, w)
    # (v) two bit-identical rows, a different one between them
    dx = (rng.uniform(-0.7, 0.7, size=(3, D)) * cell).astype(f32)
    dx[2] = dx[0]
    sets["identical-rows"] = Disturbances([A, f32(0.0), A], dx, [0.25, 0.5, 0.25])
    return sets
