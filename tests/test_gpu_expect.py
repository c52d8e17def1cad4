"""
GPU: the expectation sweeps (csrc/pi_expect_kernels.hip through pi_set_disturbances / pi_expect_*) against their numpy
twins (dynamicprogramming_amd/noise.py on the checker's step): V', policy, residual and changed count bit for bit.

Per (grid, disturbance set) the twin runs ONCE over the whole grid (one evaluation sweep, one value sweep); what a
sub-range launch has to leave behind follows from those arrays, because every state's backup is independent of the others.
Every GPU step runs once; nothing retries.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd._native import Info
from dynamicprogramming_amd.noise import Disturbances
from dynamicprogramming_amd.solver import CudaPIConfig
from tests import helpers as H
from tests.noise_backend import with_noise_backend

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.0)


def _golden_shape(name):
    return tuple(int(g) for g in H.golden(name)["g0_shape"])


GRIDS = {
    "golden-2d": ("pendulum", None), "golden-4d": ("cartpole", None), "golden-6d": ("double_cartpole", None),
    "ragged-2d": ("pendulum", (24, 17)), "ragged-4d": ("cartpole_swingup", (9, 7, 11, 5)),
    "ragged-6d": ("double_cartpole", (5, 4, 6, 4, 5, 4)),
    "all2-2d": ("pendulum", (2, 2)), "all2-4d": ("double_pendulum_swingup", (2, 2, 2, 2)),
    "all2-6d": ("double_cartpole_swingup", (2,) * 6),
}
SETS = ("S1", "S2", "S3", "S4")


def _tensor_rule(D, axes):
    """Tensor Gauss-Legendre rule: axes = [("a" | dimension, amplitude, nodes)], first axis slowest."""
    K = int(np.prod([n for _, _, n in axes]))
    idx = np.indices([n for _, _, n in axes]).reshape(len(axes), K)
    da, dx, p = np.zeros(K), np.zeros((K, D)), np.ones(K)
    for j, (which, amp, n) in enumerate(axes):
        x, w = np.polynomial.legendre.leggauss(n)
        if which == "a":
            da = amp * x[idx[j]]
        else:
            dx[:, which] = amp * x[idx[j]]
        p = p * (w[idx[j]] / 2)
    return Disturbances(da.astype(np.float32), dx.astype(np.float32), p.astype(np.float32))


def _make_set(which, D, cell, acts):
    arange = float(acts.max() - acts.min()) or 1.0
    if which == "S1":
        return Disturbances.none(D)
    if which == "S2":       # 3 action nodes at 0.3 of the action range x 2 x 2 nodes at 0.6 cell widths in dimensions 0, 1
        return _tensor_rule(D, [("a", 0.3 * arange, 3), (0, 0.6 * cell[0], 2), (1, 0.6 * cell[1], 2)])
    rng = np.random.default_rng(11)
    if which == "S3":       # K = 64: offsets of up to 3 cells, random weights, da in runs alternating zero / non-zero
        dx = rng.uniform(-3.0, 3.0, size=(64, D)) * cell
        dx[rng.random((64, D)) < 0.2] = 0.0
        runs = np.repeat(np.where(np.arange(8) % 2 == 0, 0.0, rng.uniform(-0.7, 0.7, size=8) * arange), 8)
        p = rng.random(64) + 0.05
        return Disturbances(runs.astype(np.float32), dx.astype(np.float32), (p / p.sum()).astype(np.float32))
    dx = np.zeros((4, D))   # S4: everything must clamp
    dx[:, D - 1] = [1e30, -1e30, 1e30, -1e30]
    return Disturbances(np.array([1e3, 1e3, -1e3, -1e3], np.float32) * np.float32(arange), dx.astype(np.float32),
                        np.full(4, 0.25, np.float32))


_CASES = {}


def _case(grid, actions=None, chk=None, plugin=None, bins=None, gamma=None):
    """The case `grid`: a key of GRIDS, or (env, shape).  `actions`: the handle's action table instead of the env's own.
    `chk`, `plugin`, `bins`, `gamma`: a synthetic grid — the checker whose step is the twin's, the plugin source the engine
    compiles, its bin tables and its discount; such a grid has no terminal states.  Built once per distinct argument set."""
    key = (grid, None if actions is None else np.asarray(actions, np.float32).tobytes(), None if chk is None else id(chk),
           plugin, None if bins is None else tuple(np.asarray(b, np.float32).tobytes() for b in bins), gamma)
    if key in _CASES:
        return _CASES[key]
    name, shape = GRIDS[grid] if isinstance(grid, str) else grid
    if bins is None:
        shape = _golden_shape(name) if shape is None else shape
        bins = H.env_bins(name, shape)
    else:
        bins = [np.asarray(b, np.float32) for b in bins]
        shape = tuple(len(b) for b in bins)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    if plugin is None:
        term, tval = H.terminal_mask(name, states)
    else:
        term, tval = np.zeros(len(states), dtype=bool), 0.0
    rng = np.random.default_rng(3)
    V = (rng.standard_normal(len(states)) * 30.0).astype(np.float32)
    V[term] = np.float32(tval)
    acts = H.edge_actions(name, actions)
    pol = rng.integers(0, len(acts), size=len(states)).astype(np.int32)
    pol[term] = 0
    cell = (hi.astype(np.float64) - lo.astype(np.float64)) / (np.asarray(gshape, np.float64) - 1)
    for a in (V, pol, term):
        a.setflags(write=False)
    c = dict(name=name, shape=shape, bins=bins, grid=(lo, hi, gshape, strides), states=states, term=term, V=V, pol=pol,
             acts=acts, cell=cell, D=len(shape), n=len(states), chk=H.oracle_for(name) if chk is None else chk,
             src=envs.dynamics_source(name) if plugin is None else plugin,
             gamma=float(np.float32(envs.ENVS[name].CONFIG["gamma"] if gamma is None else gamma)))
    _CASES[key] = c
    return c


def _twin_of(c, d):
    """Whole-grid twin results of the case `c` under the set `d`: the set, V' of one evaluation sweep, V' and policy of one
    value sweep."""
    args = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    V_eval, _ = noise.expected_eval(c["chk"].step, c["states"], c["pol"], c["V"], *args)
    V_val, pol_val, _, _ = noise.expected_value_sweep(c["chk"].step, c["states"], c["pol"], c["V"], *args)
    for a in (V_eval, V_val, pol_val):
        a.setflags(write=False)
    return d, V_eval, V_val, pol_val


@lru_cache(maxsize=None)
def _twin(grid, which):
    """Whole-grid twin results for (grid, set): the set, V' of one evaluation sweep, V' and policy of one value sweep."""
    c = _case(grid)
    return _twin_of(c, _make_set(which, c["D"], c["cell"], c["acts"]))


def _residual(new, old):
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(new - old)
    return np.float32(np.fmax.reduce(d, initial=np.float32(0.0))) if len(d) else np.float32(0.0)


def _engine(c, dev, order=None, cache_dir=_native.KERNEL_CACHE, options=()):
    """`options`: (selector, value) pairs set before pi_compile."""
    bins = c["bins"]
    eng = _native.Engine(c["D"], [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins], bins, c["acts"],
                         device=dev.index or 0, order=order)
    for what, value in options:
        eng.set_option(what, value)
    eng.compile(c["src"], cache_dir=cache_dir)
    return eng


class _Device:
    """The arrays of one case on the device, in the engine's memory order, and the three sweeps on them."""

    def __init__(self, eng, c, dev, term=True):
        import torch
        self.torch, self.eng, self.c, self.dev = torch, eng, c, dev
        self.term = self.put(c["term"].astype(np.uint8)) if term else None

    def put(self, a):
        return self.torch.from_numpy(np.array(self.eng.to_memory(np.asarray(a)), order="C", copy=True)).to(self.dev)

    def get(self, t):
        return np.ascontiguousarray(self.eng.to_user(t.cpu().numpy()))

    def _outs(self, want_delta, want_changed):
        d_delta = self.torch.full((1,), 123.0, dtype=self.torch.float32, device=self.dev) if want_delta else None
        d_changed = self.torch.full((1,), 77, dtype=self.torch.int32, device=self.dev) if want_changed else None
        return d_delta, d_changed

    @staticmethod
    def _p(t):
        return 0 if t is None else t.data_ptr()

    def sweep(self, kind, a, b, V=None, pol=None, n_sweeps=1, want_delta=True, want_changed=True, expect=True):
        """Returns (Va, Vb, policy, residual | None, changed | None) after the call, host arrays in the user's order."""
        c, eng, p = self.c, self.eng, self._p
        d_Va = self.put(c["V"] if V is None else V)
        d_Vb = self.torch.full_like(d_Va, float(SENTINEL))
        d_pol = self.put(c["pol"] if pol is None else pol)
        d_delta, d_changed = self._outs(want_delta and kind != "improve", want_changed and kind != "eval")
        g = c["gamma"]
        if kind == "eval":
            fn = eng.expect_eval_sweeps if expect else eng.eval_sweeps
            fn(d_Va.data_ptr(), d_Vb.data_ptr(), d_pol.data_ptr(), p(self.term), a, b, g, n_sweeps, p(d_delta))
        elif kind == "improve":
            fn = eng.expect_improve_sweep if expect else eng.improve_sweep
            fn(d_Va.data_ptr(), d_pol.data_ptr(), p(self.term), a, b, g, p(d_changed))
        else:
            fn = eng.expect_value_sweep if expect else eng.value_sweep
            fn(d_Va.data_ptr(), d_Vb.data_ptr(), d_pol.data_ptr(), p(self.term), a, b, g, p(d_delta), p(d_changed))
        self.torch.cuda.synchronize()
        return (self.get(d_Va), self.get(d_Vb), self.get(d_pol),
                None if d_delta is None else np.float32(d_delta.item()),
                None if d_changed is None else int(d_changed.item()))


def _expected(c, twin, kind, a, b):
    """What a launch of `kind` over [a, b) leaves behind, from the whole-grid twin arrays: (Vb, policy, residual, changed)."""
    _, V_eval, V_val, pol_val = twin
    Vb = np.full(c["n"], SENTINEL, np.float32)
    pol = c["pol"].copy()
    newV = V_eval if kind == "eval" else V_val
    if kind != "improve":
        Vb[a:b] = newV[a:b]
    if kind != "eval":
        pol[a:b] = pol_val[a:b]
    return Vb, pol, _residual(newV[a:b], c["V"][a:b]), int((pol != c["pol"]).sum())


def _check(got, want, kind, what):
    Va, Vb, pol, delta, changed = got
    e_Vb, e_pol, e_delta, e_changed = want
    H.assert_bits_equal(Vb, e_Vb, f"{what} {kind}: V'")
    assert np.array_equal(pol, e_pol), f"{what} {kind}: policy"
    if delta is not None:
        assert delta == e_delta, f"{what} {kind}: residual {delta} vs {e_delta}"
    if changed is not None:
        assert changed == e_changed, f"{what} {kind}: changed {changed} vs {e_changed}"


@pytest.mark.parametrize("grid", list(GRIDS))
def test_sweeps_equal_the_twin_on_every_set(grid, cuda_device):
    """Each sweep kind on the whole grid and on an unaligned sub-range (states outside it untouched), for S1 .. S4 installed
    one after the other on ONE handle; for S1 also the deterministic entry points of the handle and the checker's sweeps."""
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device)
    dv = _Device(eng, c, cuda_device)
    sub = (37, n - 53) if n > 128 else (1, n - 1)
    for which in SETS:
        twin = _twin(grid, which)
        d = twin[0]
        assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K == eng.info(Info.DISTURBANCES)
        for kind in ("eval", "improve", "value"):
            for a, b in ((0, n), sub):
                got = dv.sweep(kind, a, b)
                H.assert_bits_equal(got[0], c["V"], f"{grid} {which} {kind}: the source buffer")
                _check(got, _expected(c, twin, kind, a, b), kind, f"{grid} {which} [{a}, {b})")
                if which == "S1":
                    _check(dv.sweep(kind, a, b, expect=False), _expected(c, twin, kind, a, b), kind,
                           f"{grid} deterministic entry point [{a}, {b})")
        if which == "S1":
            chk, targs = c["chk"], (c["states"], c["acts"], c["pol"], c["V"], c["term"], *c["grid"], c["gamma"])
            H.assert_bits_equal(chk.eval_sweep(*targs)[0], twin[1], f"{grid} checker eval")
            o_V, o_pol, _, _ = chk.value_sweep(*targs)
            H.assert_bits_equal(o_V, twin[2], f"{grid} checker value sweep")
            assert np.array_equal(o_pol, twin[3])
        elif which == "S2" and grid.startswith("golden"):
            # not vacuous: the set moves every Q and a share of the argmaxes (measured 10-28 % on these grids)
            base = _twin(grid, "S1")
            live = ~c["term"]
            assert (twin[1][live] != base[1][live]).mean() > 0.99
            assert (twin[3][live] != base[3][live]).mean() > 0.05
    eng.close()


@pytest.mark.parametrize("grid,term", [("golden-4d", True), ("golden-2d", False), ("golden-2d", True)])
def test_ping_pong_and_null_mask(grid, term, cuda_device):
    """n_sweeps = 1, 2, 3: the newest iterate is in Vb when odd, in Va when even, the one before it in the other buffer,
    the residual is the last sweep's.  Pendulum has no terminal states: with the mask and with term == NULL."""
    c = _case(grid)
    n = c["n"]
    d = _twin(grid, "S2")[0]
    eng = _engine(c, cuda_device)
    eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
    dv = _Device(eng, c, cuda_device, term=term)
    args = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    iterates, deltas = [c["V"]], [None]
    for _ in range(3):
        nxt, delta = noise.expected_eval(c["chk"].step, c["states"], c["pol"], iterates[-1], *args)
        iterates.append(nxt)
        deltas.append(delta)
    for k in (1, 2, 3):
        Va, Vb, _, delta, _ = dv.sweep("eval", 0, n, n_sweeps=k)
        newest, before = (Vb, Va) if k & 1 else (Va, Vb)
        H.assert_bits_equal(newest, iterates[k], f"{grid} {k} sweeps: newest iterate")
        H.assert_bits_equal(before, iterates[k - 1], f"{grid} {k} sweeps: the iterate before")
        assert delta == np.float32(deltas[k])
    for kind in ("improve", "value"):
        _check(dv.sweep(kind, 0, n), _expected(c, _twin(grid, "S2"), kind, 0, n), kind, f"{grid} term={term}")
    eng.close()


@pytest.mark.parametrize("grid,order", [("ragged-4d", (0, 2, 1, 3)), ("ragged-6d", (5, 4, 2, 3, 0, 1))])
def test_memory_orders(grid, order, cuda_device):
    """State offsets are given in the user's dimension order whatever the memory order of the handle."""
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device, order=order)
    dv = _Device(eng, c, cuda_device)
    for which in ("S3", "S2"):
        twin = _twin(grid, which)
        d = twin[0]
        eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
        for kind in ("eval", "improve", "value"):
            _check(dv.sweep(kind, 0, n), _expected(c, twin, kind, 0, n), kind, f"{grid} order {order} {which}")
    eng.close()


def test_every_nullable_output_alone(cuda_device):
    grid = "ragged-4d"
    c = _case(grid)
    n = c["n"]
    twin = _twin(grid, "S2")
    d = twin[0]
    eng = _engine(c, cuda_device)
    eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
    dv = _Device(eng, c, cuda_device)
    for kind, flags in (("eval", [(False, False)]), ("improve", [(False, False)]),
                        ("value", [(True, False), (False, True), (False, False)])):
        for want_delta, want_changed in flags:
            got = dv.sweep(kind, 37, n - 53, want_delta=want_delta, want_changed=want_changed)
            _check(got, _expected(c, twin, kind, 37, n - 53), kind, f"delta={want_delta} changed={want_changed}")
            assert (got[3] is not None) == (want_delta and kind != "improve")
            assert (got[4] is not None) == (want_changed and kind != "eval")
    eng.close()


def test_another_set_builds_nothing(cuda_device, tmp_path):
    """K is run-time data: a second pi_set_disturbances with another K leaves the cache directory as it is, and the sweeps
    that follow take their expectation over the new set."""
    grid = "golden-2d"
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device, cache_dir=tmp_path)
    assert len(list(tmp_path.glob("pi_*.hsaco"))) == 1
    dv = _Device(eng, c, cuda_device)
    listing = None
    for which in ("S2", "S3", "S1"):
        twin = _twin(grid, which)
        d = twin[0]
        assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K
        now = sorted((p.name, p.stat().st_mtime_ns) for p in tmp_path.iterdir())
        assert len(now) == 2 and (listing is None or now == listing)
        listing = now
        _check(dv.sweep("value", 0, n), _expected(c, twin, "value", 0, n), "value", f"after switching to {which}")
    eng.set_disturbances(None, None, None)
    with pytest.raises(_native.NativeError, match="pi_set_disturbances"):
        dv.sweep("eval", 0, n)
    eng.close()


@pytest.mark.parametrize("grid", ["golden-2d", "golden-4d"])
def test_solver_run_equals_the_checker_backend(grid, cuda_device):
    """run() with S2, capped at 50 sweeps per evaluation and 3 rounds: V, policy, sweep counts and the stable flag of the
    same loop on the CPU backend of tests/noise_backend.py.  After set_disturbances(None) the solver is a freshly
    constructed deterministic one, bit for bit."""
    c = _case(grid)
    cls = envs.ENVS[c["name"]]
    cfg = CudaPIConfig(**{**cls.CONFIG, "max_eval_iter": 50, "max_pi_iter": 3})
    d = _twin(grid, "S2")[0]
    space = H.env_bins_space(c["name"], c["shape"])

    def run(solver, noisy):
        if noisy is not None:
            solver.set_disturbances(d if noisy else None)
        solver.run()
        return solver

    gpu = run(cls(space, cls.ACTIONS, cfg, device=cuda_device, transport=False), True)
    cpu = run(with_noise_backend(cls)(space, cls.ACTIONS, cfg), True)
    assert gpu.stats["disturbances"] == 12 == cpu.stats["disturbances"]
    H.assert_bits_equal(gpu.value_function, cpu.value_function, f"{grid} V of the noise-aware run")
    assert np.array_equal(gpu.policy, cpu.policy)
    assert gpu.stats["sweeps_per_iter"] == cpu.stats["sweeps_per_iter"] and gpu.stats["pi_iterations"] == cpu.stats["pi_iterations"]
    assert gpu.stats["stable"] == cpu.stats["stable"] and gpu.stats["eval_sweeps"] == cpu.stats["eval_sweeps"]
    dropped = cls(space, cls.ACTIONS, cfg, device=cuda_device, transport=False)
    dropped.set_disturbances(d)
    fresh = run(cls(space, cls.ACTIONS, cfg, device=cuda_device, transport=False), None)
    run(dropped, False)
    assert dropped.stats["disturbances"] == 0
    H.assert_bits_equal(dropped.value_function, fresh.value_function, f"{grid} V after dropping the set")
    assert np.array_equal(dropped.policy, fresh.policy) and dropped.stats["sweeps_per_iter"] == fresh.stats["sweeps_per_iter"]
    assert not np.array_equal(gpu.value_function.view(np.uint32), fresh.value_function.view(np.uint32))
