"""
Inputs the tests of the inference handle's edges share (tests/test_inference_utils.py, tests/test_gpu_infer_edges.py,
tests/test_gpu_infer_addr64.py): the reference-executed edge vectors of tests/golden/barycentric_edges.npz, source tables
in any memory order of the dimensions, start states with non-finite and boundary coordinates, and the comparison that
lets a GENERATED NaN differ in payload and sign between host and device while every other value is compared by its bits.
"""
from __future__ import annotations

from functools import lru_cache
from itertools import product

import numpy as np

from dynamicprogramming_amd import envs
from tests import helpers as H

EDGE_GRIDS = ("d2", "d4", "d6", "z2", "z4")
ZERO_GRIDS = ("z2", "z4")                                   # bounds with exact zeros: lo = +0, hi = +0, lo = -hi, lo = -0


def corner_bits(D):
    return np.array(list(product([0, 1], repeat=D)), dtype=np.int32)


def row_major(shape):
    return np.array([int(np.prod(shape[d + 1:], dtype=np.int64)) for d in range(len(shape))], dtype=np.int32)


def memory_strides(shape, order):
    """Element stride of every USER dimension when memory dimension k (0 = slowest) holds user dimension order[k]."""
    strides, step = np.zeros(len(shape), dtype=np.int64), 1
    for d in reversed(order):
        strides[d] = step
        step *= shape[d]
    return strides.astype(np.int32)


def to_memory(a, shape, order):
    """A table in the user's row-major order laid out in the memory order `order`."""
    return np.ascontiguousarray(np.asarray(a).reshape(shape).transpose(order)).reshape(-1)


@lru_cache(maxsize=None)
def edge_vectors():
    """{grid key: dict(lo, hi, gshape, strides, bits, bins, points, dim, cls, indices, weights, policy, actions,
    optimal_action)} and the class names, from the fixture alone."""
    gold = np.load(H.GOLDEN / "barycentric_edges.npz")
    classes = [str(x) for x in gold["classes"]]
    out = {}
    for key in (str(x) for x in gold["grids"]):
        gshape = gold[f"{key}_shape"]
        D = len(gshape)
        out[key] = dict(lo=gold[f"{key}_lo"], hi=gold[f"{key}_hi"], gshape=gshape, strides=row_major(gshape),
                        bits=corner_bits(D), bins=[gold[f"{key}_bins{d}"] for d in range(D)],
                        points=gold[f"{key}_points"], dim=gold[f"{key}_dim"], cls=gold[f"{key}_class"],
                        indices=gold[f"{key}_indices"], weights=gold[f"{key}_weights_numba"],
                        policy=gold[f"{key}_policy"], actions=gold[f"{key}_actions"],
                        optimal_action=gold[f"{key}_optimal_action"], D=D)
    return out, classes


def grid_of(v):
    """(lo, hi, gshape, strides, bits) of an edge_vectors() entry."""
    return v["lo"], v["hi"], v["gshape"], v["strides"], v["bits"]


def ascending_sum(w, idx, table, actions=None):
    """sum_c w[:, c] * x[idx[:, c]] in float32 from 0 over ASCENDING corners, multiply then add; x = actions[table[.]]
    when an action table is given, table[.] otherwise."""
    acc = np.zeros(len(w), np.float32)
    for c in range(w.shape[1]):
        x = table[idx[:, c]]
        acc = acc + w[:, c] * (x if actions is None else actions[x])
    return acc


def parent_clamp(pts, lo, hi):
    """The clamp the numpy twin had before it followed the reference's comparisons."""
    return np.maximum(lo, np.minimum(pts, hi))


def parent_clamp_with_zero(sign):
    """parent_clamp with the one choice IEEE 754 leaves to a maximum pinned: of two zeros of opposite sign it returns the
    one with `sign` (np.maximum returns either, depending on the loop numpy picks for the array)."""
    def clamp(pts, lo, hi):
        p = parent_clamp(pts, lo, hi)
        tie = (p == 0) & (np.asarray(pts) == 0) & (lo == 0) & (np.signbit(pts) != np.signbit(lo))
        return np.where(tie, np.float32(sign * 0.0), p)
    return clamp


def opposite_zero_rows(v):
    """Rows of an edge grid whose varied coordinate is a zero and meets a LOWER bound that is the zero of the other sign:
    there the sign of the clamped point reaches t and the weights.  (At an upper bound t is a difference from a node
    that is not zero, and the sign of the point is lost in it.)"""
    pts, dim = v["points"], v["dim"]
    rows = []
    for k in np.flatnonzero(dim >= 0):
        x, b = pts[k, dim[k]], v["lo"][dim[k]]
        if x == 0 and b == 0 and np.signbit(x) != np.signbit(b):
            rows.append(k)
    return np.asarray(rows, dtype=np.int64)


def assert_bits_equal_but_nan(got, want, what):
    """NaN at the same positions (host and device arithmetic may give a generated NaN another payload or sign), the
    same bit patterns everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other positions"
    H.assert_bits_equal(got[~nan], want[~nan], what)


def assert_same_rollout(got, want, what):
    """Every field of a rollout result: floats by assert_bits_equal_but_nan, the integer and flag fields exactly."""
    def host(x):
        return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    assert_bits_equal_but_nan(host(got.states), host(want.states), f"{what}: final states")
    assert_bits_equal_but_nan(host(got.returns), host(want.returns), f"{what}: returns")
    for field in ("lengths", "terminated", "secondary_steps", "last_mode", "switches"):
        if hasattr(want, field):
            assert np.array_equal(host(getattr(got, field)), host(getattr(want, field))), f"{what}: {field}"
    assert (got.trajectory is None) == (want.trajectory is None), what
    if want.trajectory is not None:
        assert_bits_equal_but_nan(host(got.trajectory), host(want.trajectory), f"{what}: trajectory")


def source(env, shape, order=None, seed=0, box=None, actions=None, bits=None):
    """A solution on a grid as the handle takes it: dict(env, D, shape, bins, lo, hi, gshape, strides, bits, policy, V,
    acts, tables, grid, chk, gamma).  `order`: the memory order of the dimensions the policy and V arrays are laid out
    in, with the strides to match (None: row-major); `box`: (lo, hi) instead of the env's own ranges.  `tables` is the
    tuple utils.barycentric.rollout takes, `grid` the four the lookahead twins take."""
    D = len(shape)
    if box is None:
        bins = H.env_bins(env, shape)
    else:
        bins = [np.linspace(l, h, g).astype(np.float32) for l, h, g in zip(*box, shape)]
    lo = np.array([b[0] for b in bins], np.float32)
    hi = np.array([b[-1] for b in bins], np.float32)
    gshape = np.asarray(shape, np.int32)
    n = int(np.prod(shape, dtype=np.int64))
    rng = np.random.default_rng(seed)
    acts = np.asarray(envs.ENVS[env].ACTIONS if actions is None else actions, np.float32)
    policy = rng.integers(0, len(acts), n).astype(np.int32)
    V = (rng.standard_normal(n) * 30.0).astype(np.float32)
    if order is None:
        strides = row_major(shape)
    else:
        strides = memory_strides(shape, order)
        policy, V = to_memory(policy, shape, order), to_memory(V, shape, order)
    bits = corner_bits(D) if bits is None else np.asarray(bits, np.int32)
    return dict(env=env, D=D, shape=tuple(shape), bins=bins, lo=lo, hi=hi, gshape=gshape, strides=strides, bits=bits,
                policy=policy, V=V, acts=acts, tables=(policy, acts, lo, hi, gshape, strides, bits),
                grid=(lo, hi, gshape, strides), chk=H.oracle_for(env),
                gamma=float(np.float32(envs.ENVS[env].CONFIG["gamma"])))


def ordinary_starts(rng, lo, hi, m, spread=1.0):
    """m points uniform over the box stretched by `spread` round its centre (spread > 1: some outside on both sides)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * spread
    return (mid + half * rng.uniform(-1.0, 1.0, size=(m, len(lo)))).astype(np.float32)


SPECIALS = ("nan", "inf_pos", "inf_neg", "lo", "hi", "zero_neg")


def special_starts(rng, lo, hi, m):
    """(starts (m, D), kind (m,) int8: index into SPECIALS or -1 for an ordinary episode).  Every (dimension, special)
    pair has one episode among the first 65 — NaN, +inf, -inf, the exact bounds and -0.0 in ONE coordinate, the others
    ordinary — and, for m > 65, another in the last wave; ordinary episodes sit beside them in the same waves."""
    D = len(lo)
    starts = ordinary_starts(rng, lo, hi, m, spread=0.6)
    kind = np.full(m, -1, np.int8)
    values = {"nan": lambda d: np.nan, "inf_pos": lambda d: np.inf, "inf_neg": lambda d: -np.inf,
              "lo": lambda d: lo[d], "hi": lambda d: hi[d], "zero_neg": lambda d: -0.0}
    pairs = [(d, s) for s in SPECIALS for d in range(D)]
    assert len(pairs) + 1 < 65 <= m
    for base in ((1,) if m <= 65 else (1, m - len(pairs) - 1)):
        for j, (d, s) in enumerate(pairs):
            starts[base + j, d] = np.float32(values[s](d))
            kind[base + j] = SPECIALS.index(s)
    return starts, kind
