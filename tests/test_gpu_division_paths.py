"""The three compiled forms of pi_locate (csrc/pi_sweep_kernels.hip) on the GPU, against the oracle, bit for bit (a NaN
matches any NaN).  Every backup of every sweep, one-launch and push kernel finds its successor's cell through pi_locate:

* every dimension proven for the reciprocal-multiply division — the form of all nine envs and the only one the other GPU
  files run.  Here: pi_probe_interp ON the run-time guard's own boundaries (`guard_points`), on a synthetic grid whose lower
  bounds are 0 so that a = s - lo is the coordinate itself: |a| = 2^-40 and the floats around it, the smallest normal, the
  largest denormal, +-0, sum |a| = 2^40 and the floats around it (as 2^39 + 2^39 and as 2^40 alone), every node of every
  dimension and its two neighbours (the top node: a quotient of exactly 1 and one ulp off on either side), one ulp below 0;
  each in each dimension alone and in all at once.  Compared with the oracle, with a float32 numpy restatement written
  below, with the PI_MI355_IEEE_DIV build and with the checked build;
* no dimension proven (PI_MI355_IEEE_DIV): the sweeps of the envs' small grids, the live list, a batch in the LDS-resident
  kernel;
* mixed — the `else` arm inside the fast branch — which needs a span outside [2^-30, 2^30] and which no env will ever
  have: synthetic grids with spans 5e-10 and 3e9 beside ordinary ones (`MIXED_SPANS`), a plugin without transcendental
  functions (`linear_plugin`), all three sweep kinds and the probe.  tests/test_block_sizes_host.py builds the same units
  without a device, pins their RECIPROCAL_DIV verdicts and checks on the CPU that most successors of the mixed grids lie
  strictly inside the grid (a test that only ever clamps proves nothing).

What the +-0 points found: for a coordinate of -0 (and for a negative denormal whose quotient rounds to -0) all three builds
return +0 where the oracle returned -0 in the weights of that dimension's upper corners — 88 of the 4 928 weights here.  The
oracle clamped with fmaxf(0.0f, n), for which C allows either zero when n is -0 (x86-64 returns the second operand); the
device's maximum orders -0 below +0.  No sweep result can show the difference (the chain of fmaf starts from +0), only the
probe does.  oracle/pi_oracle.cpp now pins +0, and so does the restatement below.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native
from dynamicprogramming_amd._native import Info, Option
from tests import helpers as H

pytestmark = pytest.mark.gpu

f32 = np.float32
SMALL_GRIDS = [("pendulum", (24, 17)), ("cartpole", (9, 7, 11, 5)), ("double_cartpole", (5, 4, 6, 4, 5, 4))]

# ---- the synthetic grids and their plugin -------------------------------------------------------------------------------
# 5e-10 < 2^-30 = 9.3e-10 and 3e9 > 2^30 = 1.07e9: pi_create keeps the IEEE division for those dimensions alone.
MIXED_SPANS = {2: [5e-10, 2.0], 4: [5e-10, 2.0, 3e9, 0.8]}
MIXED_SHAPES = {2: (24, 17), 4: (9, 7, 11, 5)}
MIXED_VERDICT = {2: [0, 1], 4: [0, 1, 0, 1]}
MIXED_ACTIONS = np.array([-2.0, -1.0, 0.0, 1.0, 2.0], dtype=f32)
MIXED_GAMMA = 0.95
# All spans pass the proof; lower bounds 0: the grid of the guard's edges.
GUARD_BINS = [np.linspace(0, 1.5, 9), np.linspace(0, 6.25, 7), np.linspace(0, 0.4, 11), np.linspace(0, 12, 5)]
# The plugin's coefficients, chosen on the CPU (tests/test_block_sizes_host.py measures the share of successors strictly
# inside the grid with the oracle's step: 2-D 0.879, 4-D 0.544): per unit of action a successor moves PUSH of its dimension's
# span and the cross term adds at most CROSS / 2 of it: 0.07 of the span at most, so that only nodes on or near a border can
# leave the grid, and an action of 0 in the middle of the next dimension lands exactly on a node.
PUSH, CROSS = 0.03, 0.02


def _lit(x) -> str:
    """A float32 value as a hexadecimal literal: the plugin text carries it exactly."""
    return float(f32(x)).hex() + "f"


def centred_bins(spans, shape):
    bins = [np.linspace(-0.5 * s, 0.5 * s, g).astype(f32) for s, g in zip(spans, shape)]
    assert all(np.all(np.diff(b) > 0) for b in bins), "float32 bins must be strictly increasing"
    return bins


def linear_plugin(spans) -> str:
    """n_x[d] = x[d] + (PUSH span_d) action + (CROSS span_d / span_e) x[e], e the next dimension (cyclic);
    reward = -sum (x[d] / span_d)^2 - 0.01 action^2; never terminates.  No sinf / cosf / fmodf: one instantiation."""
    D = len(spans)
    names = [f"x{d}" for d in range(D)]
    args = ", ".join(f"float {n}" for n in names)
    outs = ", ".join(f"float* n_{n}" for n in names)
    body, cost = [], []
    for d, n in enumerate(names):
        e = (d + 1) % D
        body.append(f"    *n_{n} = {n} + {_lit(PUSH * spans[d])} * action + {_lit(CROSS * spans[d] / spans[e])} * {names[e]};")
        cost.append(f"    {{ float u = {n} * {_lit(1.0 / spans[d])}; cost = cost + u * u; }}")
    return ("__device__ void step_dynamics(" + args + ", float action, " + outs + ", float* reward, bool* terminated) {\n"
            + "\n".join(body) + "\n    float cost = 0.01f * action * action;\n" + "\n".join(cost)
            + "\n    *reward = -cost;\n    *terminated = false;\n}\n")


def synthetic_engine(bins, src, device=-1, actions=MIXED_ACTIONS):
    return _native.Engine(len(bins), [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins],
                          [np.asarray(b, f32) for b in bins], actions, device=device)


def guard_bins():
    return [np.asarray(b, f32) for b in GUARD_BINS]


def guard_plugin() -> str:
    return linear_plugin([float(b[-1]) for b in guard_bins()])


# ---- the points on the guard's edges -----------------------------------------------------------------------------------
def _around(v):
    v = f32(v)
    return [np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]


def guard_points(bins) -> np.ndarray:
    """Rows of coordinates (lo = 0: the coordinate IS a = s - lo) on every boundary the docstring lists."""
    D = len(bins)
    hi = np.array([b[-1] for b in bins], f32)
    plain = (hi * f32(0.37)).astype(f32)                       # an ordinary point inside every dimension's grid
    tiny = f32(2.0) ** -40
    scalars = []
    for v in (tiny, -tiny):
        scalars += _around(v)
    scalars += [np.finfo(f32).tiny, np.nextafter(np.finfo(f32).tiny, f32(0)), -np.finfo(f32).tiny, f32(0.0), f32(-0.0),
                np.nextafter(f32(0), f32(-1)), np.nextafter(f32(0), f32(1))]      # ... one ulp below and above 0
    scalars += _around(f32(2.0) ** 40) + _around(f32(2.0) ** 39)
    rows = []
    for v in scalars:                                          # each in each dimension alone, and in all together
        for d in range(D):
            r = plain.copy()
            r[d] = v
            rows.append(r)
        rows.append(np.full(D, v, f32))
    # sum |a| exactly 2^40 and the floats on either side of it, from two coordinates of 2^39 (every pair of dimensions,
    # the others 0 or ordinary) and from 2^40 alone with the rest 0
    half = f32(2.0) ** 39
    for d in range(D):
        for e in range(D):
            if e != d:
                for v in _around(half):
                    for rest in (np.zeros(D, f32), plain):
                        r = rest.copy()
                        r[d], r[e] = half, v
                        rows.append(r)
        for v in _around(f32(2.0) ** 40):
            r = np.zeros(D, f32)
            r[d] = v
            rows.append(r)
    # every node of every dimension and the floats one ulp below and above it (the first node: 0 and one ulp below 0; the
    # last: hi, a quotient of exactly 1, and one ulp off on either side)
    for d in range(D):
        for node in bins[d]:
            for v in _around(node):
                r = plain.copy()
                r[d] = v
                rows.append(r)
    for i in range(max(len(b) for b in bins)):
        for k in range(3):
            rows.append(np.array([_around(b[min(i, len(b) - 1)])[k] for b in bins], f32))
    return np.ascontiguousarray(np.stack(rows).astype(f32))


def interp_float32(pts, bins):
    """get_barycentric_* restated in numpy, every operation rounded to float32: n = (s - lo) / (hi - lo) * (g - 1), the
    division in float64 and rounded once (exact for a quotient of two float32: 53 >= 2 * 24 + 2 bits); fminf / fmaxf
    semantics for the clamp (a NaN lands on the top border; the maximum of +0 and -0 is +0, as on the devices); truncation; frac = n - i; the corner weights multiplied left to
    right from 1.0f.  Corner c takes bit d of c for dimension d (2-D: dimension 1 toggles fastest)."""
    D, m = len(bins), len(pts)
    g = [len(b) for b in bins]
    stride = [int(np.prod(g[d + 1:])) for d in range(D)]
    cell, frac = [], []
    with np.errstate(all="ignore"):
        for d in range(D):
            lo, hi = f32(bins[d][0]), f32(bins[d][-1])
            a = (pts[:, d] - lo).astype(f32)
            span = f32(hi - lo)
            q = (a.astype(np.float64) / np.float64(span)).astype(f32)
            n = (q * f32(g[d] - 1)).astype(f32)
            top = f32(g[d] - 1)
            n = np.where(np.isnan(n), top, np.minimum(n, top))              # fminf(n, top)
            n = np.where(n > 0, n, f32(0.0)).astype(f32)                      # fmaxf(0, .) of no NaN; max(+0, -0) = +0
            i = np.minimum(n.astype(np.int32), g[d] - 2)
            cell.append(i)
            frac.append((n - i.astype(f32)).astype(f32))
        idx = np.zeros((m, 1 << D), np.int32)
        w = np.ones((m, 1 << D), f32)
        for c in range(1 << D):
            for d in range(D):
                bit = (c >> (1 - d)) & 1 if D == 2 else (c >> d) & 1
                idx[:, c] += (cell[d] + bit) * stride[d]
                w[:, c] = (w[:, c] * (frac[d] if bit else (f32(1.0) - frac[d]).astype(f32))).astype(f32)
    return idx, w


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == np.float32:
        ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    else:
        ok = a == b
    bad = np.argwhere(~ok)
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} differ, first at {bad[:5].tolist()}"


def _probe(eng, pts, dev):
    import torch
    m, C = len(pts), 1 << eng.D
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    d_idx = torch.full((m, C), -1, dtype=torch.int32, device=dev)
    d_w = torch.full((m, C), float("nan"), dtype=torch.float32, device=dev)
    eng.probe_interp(d_pts.data_ptr(), d_idx.data_ptr(), d_w.data_ptr(), m)
    torch.cuda.synchronize()
    return d_idx.cpu().numpy(), d_w.cpu().numpy()


# ---- all dimensions proven: the guard's own edges ------------------------------------------------------------------------
def test_probe_on_the_guards_own_boundaries(cuda_device, monkeypatch):
    bins, src = guard_bins(), guard_plugin()
    pts = guard_points(bins)
    meta = oracle.grid_metadata(bins)
    assert np.all(meta[0] == 0.0)                                # a = s - lo is the coordinate itself
    o_idx, o_w = oracle.build(4, src).interp(pts, *meta)
    n_idx, n_w = interp_float32(pts, bins)
    assert np.array_equal(o_idx, n_idx), "the numpy restatement and the oracle disagree on a cell"
    _same(o_w, n_w, "the numpy restatement against the oracle")
    got = {}
    for build, knob in (("default", None), ("ieee", "PI_MI355_IEEE_DIV"), ("checked", "PI_MI355_DEBUG")):
        monkeypatch.delenv("PI_MI355_IEEE_DIV", raising=False)
        monkeypatch.delenv("PI_MI355_DEBUG", raising=False)
        if knob:
            monkeypatch.setenv(knob, "1")
        eng = synthetic_engine(bins, src, cuda_device.index or 0)
        eng.compile(src)
        assert [eng.info(Info.RECIPROCAL_DIV + d) for d in range(4)] == ([0] * 4 if build == "ieee" else [1] * 4)
        assert eng.info(Info.DEBUG_CHECKS) == (build == "checked")
        got[build] = _probe(eng, pts, cuda_device)
        if build == "checked":
            assert eng.debug_report()["violations"] == 0
        eng.close()
    for build, (idx, w) in got.items():
        assert np.array_equal(idx, o_idx), f"{build} build: cells against the oracle, rows {np.flatnonzero((idx != o_idx).any(axis=1))[:5]}"
        _same(w, o_w, f"{build} build: weights against the oracle")
    assert np.array_equal(got["default"][0], n_idx)
    _same(got["default"][1], n_w, "default build against the numpy restatement")
    assert np.array_equal(got["default"][0], got["ieee"][0])
    _same(got["default"][1], got["ieee"][1], "default build against the IEEE_DIV build")


# ---- no dimension proven ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", SMALL_GRIDS, ids=[n for n, _ in SMALL_GRIDS])
def test_sweeps_with_ieee_division_in_every_dimension(name, shape, cuda_device, monkeypatch):
    import torch
    from tests.test_gpu_edges import _Case, _batches, _single_sweeps
    monkeypatch.setenv("PI_MI355_IEEE_DIV", "1")
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")
    c = _Case(name, shape, None, cuda_device)
    eng = c.eng
    try:
        assert [eng.info(Info.RECIPROCAL_DIV + d) for d in range(len(shape))] == [0] * len(shape)
        _single_sweeps(c)
        if name == "pendulum":                                   # 408 states: the LDS-resident kernel takes the batch
            assert eng.info(Info.RESIDENT_STATES_PER_THREAD) > 0
            _batches(c)
        if name == "cartpole":                                   # terminal states: the live-state list
            eng.set_option(Option.KEEP_LIVE_LIST, 1)
            assert c.term.any() and eng.prepare_mask(c.d_term.data_ptr()) == int((~c.term).sum()) == eng.info(Info.LIVE_STATES)
            d_p = c.d_pol.clone()
            d_changed = torch.full((1,), 77, dtype=torch.int32, device=cuda_device)
            eng.improve_sweep(c.d_V.data_ptr(), d_p.data_ptr(), c.d_term.data_ptr(), 0, c.n, c.gamma, d_changed.data_ptr())
            o_pol, o_changed = c.o_improve(c.pol)
            assert np.array_equal(d_p.cpu().numpy(), o_pol) and int(d_changed.item()) == o_changed
            eng.set_option(Option.RESIDENT, 0)                   # the batch over the list, not the LDS-resident kernel
            _batches(c)
    finally:
        eng.close()


# ---- mixed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 4])
def test_mixed_grids_against_the_oracle(D, cuda_device, monkeypatch):
    import torch
    monkeypatch.delenv("PI_MI355_IEEE_DIV", raising=False)
    spans, shape = MIXED_SPANS[D], MIXED_SHAPES[D]
    bins, src = centred_bins(spans, shape), linear_plugin(spans)
    eng = synthetic_engine(bins, src, cuda_device.index or 0)
    eng.compile(src)
    assert [eng.info(Info.RECIPROCAL_DIV + d) for d in range(D)] == MIXED_VERDICT[D]
    eng.set_option(Option.RESIDENT, 0)
    chk = oracle.build(D, src)
    meta = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    n = len(states)
    rng = np.random.default_rng(97 + D)
    V = (rng.standard_normal(n) * 3.0).astype(f32)
    pol = rng.integers(0, len(MIXED_ACTIONS), size=n).astype(np.int32)
    term = np.zeros(n, bool)
    dev = cuda_device
    d_V, d_pol = torch.from_numpy(V).to(dev), torch.from_numpy(pol).to(dev)
    d_term = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_delta = torch.full((1,), 123.0, dtype=torch.float32, device=dev)
    d_changed = torch.full((1,), 77, dtype=torch.int32, device=dev)
    try:
        pts = H.sample_states(rng, bins, 4096)
        idx, w = _probe(eng, pts, dev)
        o_idx, o_w = chk.interp(pts, *meta)
        assert np.array_equal(idx, o_idx)
        _same(w, o_w, "weights of the probe")
        args = (states, MIXED_ACTIONS, pol, V, term, *meta, MIXED_GAMMA)
        d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        eng.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), 0, n, MIXED_GAMMA, d_delta.data_ptr())
        o_Vn, o_delta = chk.eval_sweep(*args)
        H.assert_bits_equal(d_Vn.cpu().numpy(), o_Vn, "V' of the evaluation sweep")
        H.assert_bits_equal(f32(d_delta.item()), f32(o_delta), "its residual")
        d_p2 = d_pol.clone()
        eng.improve_sweep(d_V.data_ptr(), d_p2.data_ptr(), d_term.data_ptr(), 0, n, MIXED_GAMMA, d_changed.data_ptr())
        o_pol, o_changed = chk.improve_sweep(*args)
        assert np.array_equal(d_p2.cpu().numpy(), o_pol) and int(d_changed.item()) == o_changed > 0
        assert len(np.unique(o_pol)) > 1                         # V decides the action, not the grid's border
        d_p3, d_Vm = d_pol.clone(), torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        eng.value_sweep(d_V.data_ptr(), d_Vm.data_ptr(), d_p3.data_ptr(), d_term.data_ptr(), 0, n, MIXED_GAMMA,
                        d_delta.data_ptr(), d_changed.data_ptr())
        o_Vm, o_pol3, o_delta3, o_changed3 = chk.value_sweep(*args)
        H.assert_bits_equal(d_Vm.cpu().numpy(), o_Vm, "V' of the value sweep")
        assert np.array_equal(d_p3.cpu().numpy(), o_pol3) and int(d_changed.item()) == o_changed3
        H.assert_bits_equal(f32(d_delta.item()), f32(o_delta3), "the value sweep's residual")
    finally:
        eng.close()
