"""
tests/golden/make_barycentric_golden.py — golden vectors for the inference helper, produced by the
REFERENCE'S OWN function (/root/reference/utils/barycentric.py:15-77, :80-112) run in this build
container.  The reference cannot travel, so only the outputs are committed
(tests/golden/barycentric_utils.npz); tests/test_inference_utils.py pins utils/barycentric.py to them.

The reference's function is a numba @njit kernel; numba is not installed here, so the module text is
executed with `njit` replaced by the identity decorator (nothing is copied into the repo; the text
is read, compiled and run in memory).  One typing difference matters for the last bit of the
weights: numba types the literal in `w = 1.0` / `1.0 - t[d]` as float64, so the corner weights are
float64 products rounded to float32 once, while numpy >= 2 treats a Python float as a weak scalar
and would keep those products in float32.  The generator therefore runs the function twice:
  * `numba` typing  — float literals wrapped in np.float64 (an AST transform of the in-memory copy),
                      i.e. what the deployed reference computes;        -> weights_numba
  * plain execution — the function body as numpy 2 evaluates it;       -> weights_plain
Indices are identical in both.

`--edges` writes a second file, tests/golden/barycentric_edges.npz (function `edges`): the same function at the edges of
its clamp `max(lo, min(x, hi))` — bounds, nodes and their float32 neighbours, signed zeros, denormals, +-3.4e38, +-inf,
NaN — on the three grids above and two whose bounds are exact zeros.  What is recorded there is Python's comparison
semantics for min / max (a NaN coordinate lands on the lower bound); numba is not installed, so that numba lowers them to
the same comparisons is read from its source, not run.
"""
from __future__ import annotations

import ast
import sys
from itertools import product
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests.helpers import env_bins, sample_states  # noqa: E402
import oracle  # noqa: E402

REF = Path("/root/reference/utils/barycentric.py")
OUT = Path(__file__).resolve().parent / "barycentric_utils.npz"
CASES = {2: ("pendulum", (11, 7)), 4: ("cartpole", (5, 4, 6, 3)), 6: ("double_cartpole", (3, 4, 2, 5, 3, 2))}


class _Float64Literals(ast.NodeTransformer):
    def visit_Constant(self, node):
        if isinstance(node.value, float):
            return ast.copy_location(
                ast.Call(func=ast.Attribute(value=ast.Name(id="np", ctx=ast.Load()), attr="float64", ctx=ast.Load()),
                         args=[node], keywords=[]), node)
        return node


def load_reference(numba_typing: bool):
    tree = ast.parse(REF.read_text())
    body = []
    for node in tree.body:          # drop `from numba import njit`; an identity decorator stands in
        if isinstance(node, ast.ImportFrom) and node.module == "numba":
            continue
        body.append(node)
    tree.body = body
    if numba_typing:
        tree = _Float64Literals().visit(tree)
    ast.fix_missing_locations(tree)
    ns = {"njit": lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))}
    exec(compile(tree, str(REF), "exec"), ns)
    return ns["get_barycentric_weights_and_indices"], ns["get_optimal_action"]


def main() -> None:
    if not REF.exists():
        raise SystemExit("/root/reference is not present: fixtures can only be generated in the build container")
    ref_numba, act_numba = load_reference(True)
    ref_plain, _ = load_reference(False)
    out = {}
    for D, (name, shape) in CASES.items():
        bins = env_bins(name, shape)
        lo, hi, gshape, strides = oracle.grid_metadata(bins)
        bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
        rng = np.random.default_rng(100 + D)
        pts = sample_states(rng, bins, 2000)
        w_n, idx_n = ref_numba(pts, lo, hi, gshape, strides, bits)
        w_p, idx_p = ref_plain(pts, lo, hi, gshape, strides, bits)
        assert np.array_equal(idx_n, idx_p)
        policy = rng.integers(0, 5, size=int(np.prod(shape))).astype(np.int32)
        actions = np.linspace(-2.0, 2.0, 5).astype(np.float32)
        acts = np.array([act_numba(pts[k], policy, actions, lo, hi, gshape, strides, bits) for k in range(300)],
                        dtype=np.float64)
        out.update({f"d{D}_env": np.array(name), f"d{D}_shape": np.asarray(shape, np.int32),
                    f"d{D}_points": pts, f"d{D}_indices": idx_n, f"d{D}_weights_numba": w_n,
                    f"d{D}_weights_plain": w_p, f"d{D}_policy": policy, f"d{D}_actions": actions,
                    f"d{D}_optimal_action": acts})
        print(f"D={D}: {len(pts)} points, weights differ between typings at "
              f"{int((w_n.view(np.uint32) != w_p.view(np.uint32)).sum())} of {w_n.size} entries")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, OUT.stat().st_size, "bytes")


# ── the edges of the clamp: barycentric_edges.npz ─────────────────────────────────────────────────────────────────────
# Grids: the three of CASES plus two whose bounds contain exact zeros (given as bounds, not bin tables, so the sign of
# a zero bound is what is written here): a dimension with lo = +0.0, one with hi = +0.0, one with lo = -hi and one with
# lo = -0.0.  Point classes, one row per (dimension, class member), the other coordinates seeded interior values:
EDGES_OUT = Path(__file__).resolve().parent / "barycentric_edges.npz"
EDGE_CLASSES = ("lo", "hi", "lo_below", "lo_above", "hi_below", "hi_above", "node", "node_below", "node_above",
                "zero_pos", "zero_neg", "denorm_pos", "denorm_neg", "fltmin_pos", "fltmin_neg", "huge_pos", "huge_neg",
                "inf_pos", "inf_neg", "nan", "nan_all")
ZERO_GRIDS = {
    "z2": (np.array([0.0, -1.5], np.float32), np.array([2.0, 0.0], np.float32), (5, 4)),
    "z4": (np.array([0.0, -2.5, -1.25, -0.0], np.float32), np.array([3.0, 0.0, 1.25, 1.0], np.float32), (4, 3, 5, 3)),
}


def edge_grids():
    """{key: (lo, hi, shape, bins)}: float32 bounds, the shape, and the float32 node coordinates per dimension."""
    grids = {}
    for D, (name, shape) in CASES.items():
        bins = env_bins(name, shape)
        lo, hi, _, _ = oracle.grid_metadata(bins)
        grids[f"d{D}"] = (np.asarray(lo, np.float32), np.asarray(hi, np.float32), shape, bins)
    for key, (lo, hi, shape) in ZERO_GRIDS.items():
        bins = [np.linspace(float(l), float(h), g).astype(np.float32) for l, h, g in zip(lo, hi, shape)]
        for b, l, h in zip(bins, lo, hi):
            b[0], b[-1] = l, h                       # linspace drops the sign of a -0.0 end point
        grids[key] = (lo, hi, shape, bins)
    return grids


def edge_points(rng, lo, hi, bins):
    """(points (m, D) float32, dim (m,) int8: the dimension a row varies or -1 for all, cls (m,) int8: index into
    EDGE_CLASSES)."""
    D = len(lo)
    f = np.float32
    up, down = f(np.inf), f(-np.inf)
    rows, dims, classes = [], [], []

    def interior():
        return np.array([l + (h - l) * u for l, h, u in zip(lo.astype(np.float64), hi.astype(np.float64),
                                                            rng.uniform(0.05, 0.95, size=D))], dtype=np.float32)

    def add(d, cls, value):
        p = interior()
        if d < 0:
            p[:] = value
        else:
            p[d] = value
        rows.append(p)
        dims.append(d)
        classes.append(EDGE_CLASSES.index(cls))

    for d in range(D):
        l, h = f(lo[d]), f(hi[d])
        add(d, "lo", l), add(d, "hi", h)
        add(d, "lo_below", np.nextafter(l, down)), add(d, "lo_above", np.nextafter(l, up))
        add(d, "hi_below", np.nextafter(h, down)), add(d, "hi_above", np.nextafter(h, up))
        for x in bins[d]:
            add(d, "node", f(x)), add(d, "node_below", np.nextafter(f(x), down)), add(d, "node_above", np.nextafter(f(x), up))
        tiny, fltmin = np.nextafter(f(0.0), up), np.finfo(np.float32).tiny
        add(d, "zero_pos", f(0.0)), add(d, "zero_neg", f(-0.0))
        add(d, "denorm_pos", tiny), add(d, "denorm_neg", -tiny)
        add(d, "fltmin_pos", fltmin), add(d, "fltmin_neg", -fltmin)
        add(d, "huge_pos", f(3.4e38)), add(d, "huge_neg", f(-3.4e38))
        add(d, "inf_pos", up), add(d, "inf_neg", down)
        add(d, "nan", f(np.nan))
    add(-1, "nan_all", f(np.nan))
    return np.stack(rows), np.asarray(dims, np.int8), np.asarray(classes, np.int8)


def edges() -> None:
    """tests/golden/barycentric_edges.npz: the reference's function at the edges of its clamp, both typings run (the
    numba-typing weights are stored; indices must agree between the two)."""
    if not REF.exists():
        raise SystemExit("/root/reference is not present: fixtures can only be generated in the build container")
    ref_numba, act_numba = load_reference(True)
    ref_plain, _ = load_reference(False)
    out = {"classes": np.array(EDGE_CLASSES)}
    for n, (key, (lo, hi, shape, bins)) in enumerate(edge_grids().items()):
        D = len(shape)
        gshape = np.asarray(shape, np.int32)
        strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
        bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
        rng = np.random.default_rng(700 + n)
        pts, dims, classes = edge_points(rng, lo, hi, bins)
        with np.errstate(all="ignore"):
            w_n, idx_n = ref_numba(pts, lo, hi, gshape, strides, bits)
            w_p, idx_p = ref_plain(pts, lo, hi, gshape, strides, bits)
        assert np.array_equal(idx_n, idx_p)
        policy = rng.integers(0, 5, size=int(np.prod(shape))).astype(np.int32)
        actions = np.linspace(-2.0, 2.0, 5).astype(np.float32)
        acts = np.array([act_numba(pts[k], policy, actions, lo, hi, gshape, strides, bits) for k in range(len(pts))],
                        dtype=np.float64)
        out.update({f"{key}_lo": lo, f"{key}_hi": hi, f"{key}_shape": gshape, f"{key}_points": pts, f"{key}_dim": dims,
                    f"{key}_class": classes, f"{key}_indices": idx_n, f"{key}_weights_numba": w_n,
                    f"{key}_policy": policy, f"{key}_actions": actions, f"{key}_optimal_action": acts})
        for d, b in enumerate(bins):
            out[f"{key}_bins{d}"] = b
        print(f"{key}: {len(pts)} points, NaN weights: {int(np.isnan(w_n).sum())}")
    out["grids"] = np.array(list(edge_grids()))
    np.savez_compressed(EDGES_OUT, **out)
    print("wrote", EDGES_OUT, EDGES_OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    if "--edges" in sys.argv[1:]:
        edges()
    else:
        main()
