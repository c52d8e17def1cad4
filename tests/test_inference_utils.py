"""utils/barycentric.py (inference-side helper): pinned bit for bit to
vectors produced by the reference's own function (tests/golden/barycentric_utils.npz, generated
by tests/golden/make_barycentric_golden.py in the build container); agrees with the training-side
interpolation up to the documented differences; get_optimal_action interpolates action values."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from tests import helpers as H
from tests import infer_cases as IC
from utils import barycentric as B
from utils.barycentric import get_barycentric_weights_and_indices, get_optimal_action
from itertools import product


GOLD = np.load(H.GOLDEN / "barycentric_utils.npz")


def test_matches_the_reference_function_bit_for_bit():
    """Same flat indices and bit-equal float32 weights as /root/reference/utils/barycentric.py:15-77
    (numba typing: float64 products rounded once) on 2 000 seeded points per dimension count,
    including out-of-range, exact-node and last-cell points; within 2 ulp of what the same function
    body gives under numpy-2 scalar promotion; get_optimal_action (:80-112) equal to 1e-12."""
    for D in (2, 4, 6):
        name, shape = str(GOLD[f"d{D}_env"]), tuple(int(x) for x in GOLD[f"d{D}_shape"])
        bins = H.env_bins(name, shape)
        lo, hi, gshape, strides = oracle.grid_metadata(bins)
        bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
        pts = GOLD[f"d{D}_points"]
        assert np.array_equal(pts.view(np.uint32), H.sample_states(np.random.default_rng(100 + D), bins, 2000).view(np.uint32))
        w, idx = get_barycentric_weights_and_indices(pts, lo, hi, gshape, strides, bits)
        assert np.array_equal(idx, GOLD[f"d{D}_indices"])
        assert np.array_equal(w.view(np.uint32), GOLD[f"d{D}_weights_numba"].view(np.uint32))
        plain = GOLD[f"d{D}_weights_plain"]
        ulp = np.spacing(np.maximum(np.abs(plain), np.float32(1e-30)))
        assert np.all(np.abs(w.astype(np.float64) - plain) <= 2.0 * D * ulp)
        policy, actions = GOLD[f"d{D}_policy"], GOLD[f"d{D}_actions"]
        got = np.array([get_optimal_action(pts[k], policy, actions, lo, hi, gshape, strides, bits)
                        for k in range(300)], dtype=np.float64)
        np.testing.assert_allclose(got, GOLD[f"d{D}_optimal_action"], rtol=0, atol=1e-12)


def _twin_on_edges(v):
    return get_barycentric_weights_and_indices(v["points"], *IC.grid_of(v))


def test_edge_vectors_pin_the_clamp_to_the_reference():
    """tests/golden/barycentric_edges.npz (the reference's function at the edges of `max(lo, min(x, hi))`, CPython
    comparison semantics): same indices, same weight bit patterns with the sign of every zero, no NaN anywhere — a NaN
    coordinate lands on the lower bound (base index 0 in that dimension, t = +0), +-inf on the bounds."""
    vectors, _ = IC.edge_vectors()
    assert set(vectors) == set(IC.EDGE_GRIDS)
    for key, v in vectors.items():
        w, idx = _twin_on_edges(v)
        assert not np.isnan(v["weights"]).any() and not np.isnan(w).any(), key
        assert idx.dtype == np.int32 and np.array_equal(idx, v["indices"]), key
        H.assert_bits_equal(w, v["weights"], f"{key}: weights, zero signs included")
        # get_optimal_action: a float32 dot product whose order BLAS chooses; 2^D products of |w| <= 1 and |a| <= 2,
        # each rounding at most 2^-24 relative of a partial sum <= 2: the bound is 2^D * 2 * 2^-24 * 2 against any order
        got = np.array([get_optimal_action(v["points"][k], v["policy"], v["actions"], *IC.grid_of(v))
                        for k in range(len(v["points"]))], dtype=np.float64)
        assert np.isfinite(got).all(), key
        assert np.max(np.abs(got - v["optimal_action"])) <= (1 << v["D"]) * 4.0 * 2.0 ** -24, key
        seq = IC.ascending_sum(v["weights"], v["indices"], v["policy"], v["actions"])
        assert np.max(np.abs(seq.astype(np.float64) - v["optimal_action"])) <= (1 << v["D"]) * 4.0 * 2.0 ** -24, key
        # what the NaN rows mean, from the fixture alone: cell 0 and weight 0 on every corner with the bit set
        for k in np.flatnonzero(np.isnan(v["points"]).any(axis=1)):
            for d in np.flatnonzero(np.isnan(v["points"][k])):
                up = v["bits"][:, d] == 1
                assert (v["weights"][k, up].view(np.uint32) << 1 == 0).all(), (key, k, d)
                assert ((v["indices"][k, ~up] // v["strides"][d]) % v["gshape"][d] == 0).all(), (key, k, d)


def test_edge_vectors_hold_every_point_class():
    """Asserted from the fixture alone: per grid and dimension the bounds and their neighbours, every node with both
    neighbours, both zeros, denormals, FLT_MIN, +-3.4e38, +-inf and NaN; NaN in all dimensions once; the two zero grids
    have a dimension with lo = 0, one with hi = 0 and one with lo = -hi."""
    vectors, classes = IC.edge_vectors()
    f = np.float32
    up, down = f(np.inf), f(-np.inf)
    tiny, fltmin = np.nextafter(f(0), up), np.finfo(np.float32).tiny
    fixed = {"zero_pos": f(0.0), "zero_neg": f(-0.0), "denorm_pos": tiny, "denorm_neg": -tiny, "fltmin_pos": fltmin,
             "fltmin_neg": -fltmin, "huge_pos": f(3.4e38), "huge_neg": f(-3.4e38), "inf_pos": up, "inf_neg": down}
    for key, v in vectors.items():
        pts, dim, cls = v["points"], v["dim"], v["cls"]
        for d in range(v["D"]):
            lo, hi = v["lo"][d], v["hi"][d]
            want = {"lo": [lo], "hi": [hi], "lo_below": [np.nextafter(lo, down)], "lo_above": [np.nextafter(lo, up)],
                    "hi_below": [np.nextafter(hi, down)], "hi_above": [np.nextafter(hi, up)],
                    "node": list(v["bins"][d]), "node_below": [np.nextafter(x, down) for x in v["bins"][d]],
                    "node_above": [np.nextafter(x, up) for x in v["bins"][d]]}
            want.update({name: [x] for name, x in fixed.items()})
            assert len(v["bins"][d]) == v["gshape"][d] and v["bins"][d][0] == lo and v["bins"][d][-1] == hi
            for name, values in want.items():
                rows = np.flatnonzero((dim == d) & (cls == classes.index(name)))
                have = pts[rows, d]
                assert len(have) == len(values), (key, d, name)
                H.assert_bits_equal(have, np.asarray(values, f), f"{key} dim {d} class {name}")
                others = np.delete(pts[rows], d, axis=1)
                assert np.isfinite(others).all() and (others > np.delete(v["lo"], d)).all() \
                    and (others < np.delete(v["hi"], d)).all(), (key, d, name)
            rows = np.flatnonzero((dim == d) & (cls == classes.index("nan")))
            assert len(rows) == 1 and np.isnan(pts[rows[0], d]) and np.isnan(pts[rows[0]]).sum() == 1, (key, d)
        rows = np.flatnonzero(cls == classes.index("nan_all"))
        assert len(rows) == 1 and dim[rows[0]] == -1 and np.isnan(pts[rows[0]]).all(), key
        assert len(pts) == sum(len(np.flatnonzero(dim == d)) for d in range(v["D"])) + 1
    for key in IC.ZERO_GRIDS:
        lo, hi = vectors[key]["lo"], vectors[key]["hi"]
        assert ((lo == 0) & (hi > 0)).any() and ((hi == 0) & (lo < 0)).any(), key
    assert any((vectors[key]["lo"] == -vectors[key]["hi"]).any() for key in IC.ZERO_GRIDS)
    assert all(len(IC.opposite_zero_rows(vectors[key])) >= 1 for key in IC.ZERO_GRIDS)


def test_edge_vectors_reach_what_the_former_clamp_got_wrong(monkeypatch):
    """With `np.maximum(lo, np.minimum(x, hi))` back in the twin, every NaN row differs from the reference, and so does
    every row where a zero coordinate meets a lower bound that is the zero of the other sign — under one of the two
    answers IEEE 754 allows a maximum of such zeros (np.maximum gives either, by the loop it picks; the reference gives
    the BOUND's zero, and the vectors hold one row with lo = +0 and one with lo = -0, so neither fixed answer passes).
    No other row differs: for every other input the clamp is unchanged."""
    vectors, _ = IC.edge_vectors()

    def wrong_rows(v, clamp):
        monkeypatch.setattr(B, "_clamp_point", clamp)
        with np.errstate(invalid="ignore"):
            w, idx = _twin_on_edges(v)
        return (w.view(np.uint32) != v["weights"].view(np.uint32)).any(axis=1) | (idx != v["indices"]).any(axis=1)

    lo_signs = set()
    for key, v in vectors.items():
        nan_rows = np.flatnonzero(np.isnan(v["points"]).any(axis=1))
        zero_rows = IC.opposite_zero_rows(v)
        wrong = wrong_rows(v, IC.parent_clamp)
        assert len(nan_rows) == v["D"] + 1 and wrong[nan_rows].all(), key
        assert set(np.flatnonzero(wrong)) <= set(nan_rows) | set(zero_rows), key
        plus, minus = wrong_rows(v, IC.parent_clamp_with_zero(+1.0)), wrong_rows(v, IC.parent_clamp_with_zero(-1.0))
        for k in zero_rows:
            negative_bound = bool(np.signbit(v["lo"][v["dim"][k]]))
            assert plus[k] == negative_bound and minus[k] == (not negative_bound), (key, k)
            lo_signs.add(negative_bound)
        assert set(np.flatnonzero(plus | minus)) == set(nan_rows) | set(zero_rows), key
    assert lo_signs == {False, True}


def test_package_reexports_like_the_reference():
    """`from utils import get_optimal_action` works as against the reference's utils/__init__.py."""
    import utils
    assert utils.get_optimal_action is get_optimal_action
    assert utils.get_barycentric_weights_and_indices is get_barycentric_weights_and_indices


def test_weights_and_indices_match_training_interpolation():
    for name, shape in (("pendulum", (11, 7)), ("cartpole", (5, 4, 6, 3)), ("double_cartpole", (3, 4, 2, 5, 3, 2))):
        bins = H.env_bins(name, shape)
        D = len(bins)
        lo, hi, gshape, strides = oracle.grid_metadata(bins)
        bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
        pts = H.sample_states(np.random.default_rng(D), bins, 2000)
        w, idx = get_barycentric_weights_and_indices(pts, lo, hi, gshape, strides, bits)
        assert w.dtype == np.float32 and idx.dtype == np.int32 and w.shape == (2000, 1 << D)
        np.testing.assert_allclose(w.sum(axis=1), 1.0, atol=1e-5)
        k_idx, k_w = H.oracle_for(name).interp(pts, lo, hi, gshape, strides)
        # same cell, same weights up to rounding; corner ORDER differs (MSB-first rows here)
        V = np.random.default_rng(1).standard_normal(int(np.prod(shape)))
        a = (w.astype(np.float64) * V[idx]).sum(axis=1)
        b = (k_w.astype(np.float64) * V[k_idx]).sum(axis=1)
        ok = np.abs(a - b) < 1e-4
        assert ok.mean() > 0.995          # cell-boundary points may pick the neighbouring cell
        same_cell = np.all(np.sort(idx, axis=1) == np.sort(k_idx, axis=1), axis=1)
        assert same_cell.mean() > 0.9         # exact nodes may sit in either adjacent cell


def test_get_optimal_action_interpolates_action_values():
    bins = [np.linspace(0, 1, 3, dtype=np.float32), np.linspace(0, 1, 3, dtype=np.float32)]
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=2)), dtype=np.int32)
    policy = np.arange(9, dtype=np.int32) % 3
    actions = np.array([-1.0, 0.0, 2.0], dtype=np.float32)
    assert get_optimal_action(np.array([0.0, 0.0]), policy, actions, lo, hi, gshape, strides, bits) == actions[0]
    mid = get_optimal_action(np.array([0.25, 0.25]), policy, actions, lo, hi, gshape, strides, bits)
    want = 0.25 * (actions[policy[0]] + actions[policy[1]] + actions[policy[3]] + actions[policy[4]])
    assert abs(mid - want) < 1e-6
    out = get_optimal_action(np.array([9.0, -9.0]), policy, actions, lo, hi, gshape, strides, bits)
    assert out == actions[policy[6]]          # clamped to the (1, 0) corner node
