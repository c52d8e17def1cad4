"""
GPU: the worst-case sweeps (the pi_robust_* kernels of csrc/pi_expect_kernels.hip through pi_robust_*) against their numpy
twins (dynamicprogramming_amd/noise.py with risk="worst" on the checker's step): V', policy, residual and changed count bit
for bit.

Per (grid, disturbance set) the twin runs ONCE over the whole grid (one evaluation sweep, one value sweep); what a
sub-range launch has to leave behind follows from those arrays, because every state's backup is independent of the others.
Grids, sets S1 .. S4, engines and the device arrays are those of tests/test_gpu_expect.py.  Every GPU step runs once;
nothing retries.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd._native import Info
from dynamicprogramming_amd.noise import Disturbances
from dynamicprogramming_amd.solver import CudaPIConfig
from tests import helpers as H
from tests.robust_backend import with_robust_backend
from tests.robust_cases import zero_weight_sets
from tests.test_gpu_expect import GRIDS, SENTINEL, _case, _check, _Device, _engine, _expected, _make_set

pytestmark = pytest.mark.gpu

SETS = ("S1", "S2", "S3", "S4", "Z")          # Z: S3 with 16 rows of weight 0 and offsets of +-1e30
PREFIX = {"robust": "robust_", "expect": "expect_", "deterministic": ""}


def _set(c, which):
    if which == "Z":
        return zero_weight_sets(_make_set("S3", c["D"], c["cell"], c["acts"]))[0]
    return _make_set(which, c["D"], c["cell"], c["acts"])


def _twin_of(c, d, risk="worst", V=None, term=True):
    """(set, V' of one evaluation sweep, V' and policy of one value sweep) over the whole grid."""
    V = c["V"] if V is None else V
    args = (c["term"] if term else None, d, c["acts"], *c["grid"], c["gamma"])
    V_eval, _ = noise.expected_eval(c["chk"].step, c["states"], c["pol"], V, *args, risk=risk)
    V_val, pol_val, _, _ = noise.expected_value_sweep(c["chk"].step, c["states"], c["pol"], V, *args, risk=risk)
    for a in (V_eval, V_val, pol_val):
        a.setflags(write=False)
    return d, V_eval, V_val, pol_val


@lru_cache(maxsize=None)
def _twin(grid, which, risk="worst"):
    c = _case(grid)
    return _twin_of(c, _set(c, which), risk)


class _Sweeps(_Device):
    """tests.test_gpu_expect._Device with the entry point chosen by name: "robust", "expect" or "deterministic"."""

    def sweep(self, kind, a, b, V=None, pol=None, n_sweeps=1, want_delta=True, want_changed=True, fold="robust"):
        c, eng, p = self.c, self.eng, self._p
        d_Va = self.put(c["V"] if V is None else V)
        d_Vb = self.torch.full_like(d_Va, float(SENTINEL))
        d_pol = self.put(c["pol"] if pol is None else pol)
        d_delta, d_changed = self._outs(want_delta and kind != "improve", want_changed and kind != "eval")
        g = c["gamma"]
        if kind == "eval":
            getattr(eng, PREFIX[fold] + "eval_sweeps")(d_Va.data_ptr(), d_Vb.data_ptr(), d_pol.data_ptr(), p(self.term), a, b,
                                                       g, n_sweeps, p(d_delta))
        elif kind == "improve":
            getattr(eng, PREFIX[fold] + "improve_sweep")(d_Va.data_ptr(), d_pol.data_ptr(), p(self.term), a, b, g, p(d_changed))
        else:
            getattr(eng, PREFIX[fold] + "value_sweep")(d_Va.data_ptr(), d_Vb.data_ptr(), d_pol.data_ptr(), p(self.term), a, b,
                                                       g, p(d_delta), p(d_changed))
        self.torch.cuda.synchronize()
        return (self.get(d_Va), self.get(d_Vb), self.get(d_pol),
                None if d_delta is None else np.float32(d_delta.item()),
                None if d_changed is None else int(d_changed.item()))


def _ranges(n):
    """The whole grid; [1, n - 1); a range that ends one state into its second 256-chunk; one that starts on the last state
    of a 256-chunk of the grid; the empty range.  On grids of fewer states the chunk ranges shrink to what exists."""
    out = [(0, n), (1, n - 1), (0, min(257, n)), (min(255, n - 1), n), (min(3, n), min(3, n))]
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("grid", list(GRIDS))
def test_sweeps_equal_the_twin_on_every_set_and_range(grid, cuda_device):
    """Each sweep kind over every range (states outside it untouched) for S1 .. S4 and Z installed one after the other on
    ONE handle; for S1 also the deterministic entry points of the handle."""
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    for which in SETS:
        twin = _twin(grid, which)
        d = twin[0]
        assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K == eng.info(Info.DISTURBANCES)
        for kind in ("eval", "improve", "value"):
            for a, b in _ranges(n):
                got = dv.sweep(kind, a, b)
                H.assert_bits_equal(got[0], c["V"], f"{grid} {which} {kind}: the source buffer")
                _check(got, _expected(c, twin, kind, a, b), kind, f"{grid} {which} [{a}, {b})")
                if which == "S1":
                    _check(dv.sweep(kind, a, b, fold="deterministic"), _expected(c, twin, kind, a, b), kind,
                           f"{grid} deterministic entry point [{a}, {b})")
        if which == "S2" and grid.startswith("golden"):
            # not vacuous: the minimum is not the expectation wherever the points' backups are not all equal (where every
            # point's step is done they are: cart-pole's Q = 1 at a third of its live nodes)
            mean = _twin(grid, "S2", "expected")
            live = ~c["term"]
            assert (twin[1][live] != mean[1][live]).mean() > 0.5
    eng.close()


def test_zero_weight_rows_equal_the_set_without_them(cuda_device):
    """On the device as in the twin: Z gives the bits of its 48 participating rows installed alone."""
    grid = "ragged-4d"
    c = _case(grid)
    n = c["n"]
    with_zeros, without, _ = zero_weight_sets(_make_set("S3", c["D"], c["cell"], c["acts"]))
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    got = {}
    for name, d in (("Z", with_zeros), ("48", without)):
        assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K
        got[name] = [dv.sweep(kind, 0, n) for kind in ("eval", "improve", "value")]
    for z, w, kind in zip(got["Z"], got["48"], ("eval", "improve", "value")):
        H.assert_bits_equal(z[1], w[1], f"{kind} V'")
        assert np.array_equal(z[2], w[2]) and z[3] == w[3] and z[4] == w[4], kind
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
    dv = _Sweeps(eng, c, cuda_device, term=term)
    args = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    iterates, deltas = [c["V"]], [None]
    for _ in range(3):
        nxt, delta = noise.expected_eval(c["chk"].step, c["states"], c["pol"], iterates[-1], *args, risk="worst")
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


def test_null_mask_on_a_grid_with_terminal_states(cuda_device):
    """term == NULL where the env has terminal states: every state is backed up, as the twin does with term=None."""
    grid = "ragged-4d"
    c = _case(grid)
    n = c["n"]
    assert c["term"].any()
    d = _set(c, "S2")
    twin = _twin_of(c, d, term=False)
    eng = _engine(c, cuda_device)
    eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
    dv = _Sweeps(eng, c, cuda_device, term=False)
    for kind in ("eval", "improve", "value"):
        _check(dv.sweep(kind, 1, n - 1), _expected(c, twin, kind, 1, n - 1), kind, f"{grid} term == NULL")
    eng.close()


def test_every_nullable_output_alone(cuda_device):
    grid = "ragged-4d"
    c = _case(grid)
    n = c["n"]
    twin = _twin(grid, "S2")
    d = twin[0]
    eng = _engine(c, cuda_device)
    eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
    dv = _Sweeps(eng, c, cuda_device)
    for kind, flags in (("eval", [(False, False)]), ("improve", [(False, False)]),
                        ("value", [(True, False), (False, True), (False, False)])):
        for want_delta, want_changed in flags:
            got = dv.sweep(kind, 37, n - 53, want_delta=want_delta, want_changed=want_changed)
            _check(got, _expected(c, twin, kind, 37, n - 53), kind, f"delta={want_delta} changed={want_changed}")
            assert (got[3] is not None) == (want_delta and kind != "improve")
            assert (got[4] is not None) == (want_changed and kind != "eval")
    eng.close()


@pytest.mark.parametrize("grid,order", [("ragged-4d", (0, 2, 1, 3)), ("ragged-6d", (5, 4, 2, 3, 0, 1))])
def test_memory_orders(grid, order, cuda_device):
    """State offsets are given in the user's dimension order whatever the memory order of the handle."""
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device, order=order)
    dv = _Sweeps(eng, c, cuda_device)
    for which in ("Z", "S2"):
        twin = _twin(grid, which)
        d = twin[0]
        eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
        for kind in ("eval", "improve", "value"):
            _check(dv.sweep(kind, 0, n), _expected(c, twin, kind, 0, n), kind, f"{grid} order {order} {which}")
    eng.close()


def test_alternating_expectation_and_worst_case_on_one_handle(cuda_device):
    """No mode lives on the handle: pi_expect_* and pi_robust_* calls alternate on one set, each giving its own twin."""
    grid = "ragged-4d"
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    for which in ("S2", "Z"):
        d = _twin(grid, which)[0]
        eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
        for kind in ("eval", "value", "improve"):
            for fold, risk in (("robust", "worst"), ("expect", "expected"), ("robust", "worst"), ("expect", "expected")):
                _check(dv.sweep(kind, 0, n, fold=fold), _expected(c, _twin(grid, which, risk), kind, 0, n), kind,
                       f"{grid} {which} {fold}")
    eng.close()


def test_refusals_on_a_device_handle(cuda_device):
    """After the set and pi_compile: the range, null pointers, Va == Vb and n_sweeps < 0, by return code."""
    grid = "golden-2d"
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    with pytest.raises(_native.NativeError, match="pi_set_disturbances"):
        dv.sweep("eval", 0, n)
    eng.set_disturbances(None, None, [1.0])
    import torch
    V = dv.put(c["V"])
    W = torch.empty_like(V)
    pol = dv.put(c["pol"])
    v, w, p = V.data_ptr(), W.data_ptr(), pol.data_ptr()
    for call in (lambda: eng.robust_eval_sweeps(v, w, p, 0, 0, n + 1, 0.9, 1), lambda: eng.robust_eval_sweeps(v, w, p, 0, 5, 4, 0.9, 1),
                 lambda: eng.robust_improve_sweep(v, p, 0, -1, n, 0.9), lambda: eng.robust_value_sweep(v, w, p, 0, 0, n + 1, 0.9)):
        with pytest.raises(_native.NativeError, match="outside"):
            call()
    for call in (lambda: eng.robust_eval_sweeps(0, w, p, 0, 0, n, 0.9, 1), lambda: eng.robust_eval_sweeps(v, w, 0, 0, 0, n, 0.9, 1),
                 lambda: eng.robust_improve_sweep(0, p, 0, 0, n, 0.9), lambda: eng.robust_improve_sweep(v, 0, 0, 0, n, 0.9),
                 lambda: eng.robust_value_sweep(v, 0, p, 0, 0, n, 0.9), lambda: eng.robust_value_sweep(v, w, 0, 0, 0, n, 0.9)):
        with pytest.raises(_native.NativeError, match="null device pointer"):
            call()
    with pytest.raises(_native.NativeError, match="different buffers"):
        eng.robust_eval_sweeps(v, v, p, 0, 0, n, 0.9, 1)
    with pytest.raises(_native.NativeError, match="different buffers"):
        eng.robust_value_sweep(v, v, p, 0, 0, n, 0.9)
    with pytest.raises(_native.NativeError, match="n_sweeps"):
        eng.robust_eval_sweeps(v, w, p, 0, 0, n, 0.9, -1)
    torch.cuda.synchronize()
    H.assert_bits_equal(dv.get(V), c["V"], "a refused call launches nothing")
    eng.close()


@pytest.mark.parametrize("where", [0, 1, 2])
def test_a_nan_under_one_point_makes_q_nan(where, cuda_device):
    """The case of tests/test_robust_host.py on the device: NaN on the planes of V around ONE point's successor of one
    state, that point first, middle or last.  The NaNs are where the twin has them and every other entry has its bits (the
    payload of a NaN an fmaf chain propagates is not pinned by IEEE 754, so it is not compared); a NaN Q never wins the
    argmax, and the residual, folded from 0 with '>', ignores it."""
    c = _case("ragged-2d")
    n = c["n"]
    lo = c["grid"][0]
    u_index = 1
    dx = np.zeros((3, 2), np.float32)
    dx[:, 0] = np.array([-4.0, 0.0, 4.0]) * c["cell"][0]
    d = Disturbances(None, dx, [0.25, 0.5, 0.25])
    nxt, _, done = c["chk"].step(c["states"], c["acts"][u_index])
    pos0 = (nxt[:, 0].astype(np.float64) - float(lo[0])) / c["cell"][0]
    ok = np.flatnonzero(~done & (pos0 > 7.0) & (pos0 < 15.0))
    s = ok[len(ok) // 2]
    plane = np.rint((c["states"][:, 0].astype(np.float64) - float(lo[0])) / c["cell"][0])
    V = c["V"].copy()
    V[np.abs(plane - (pos0[s] + 4.0 * (where - 1))) < 1.5] = np.nan
    pol = np.full(n, u_index, np.int32)
    case = dict(c, V=V, pol=pol)
    twin = _twin_of(case, d)
    assert np.isnan(twin[1][s]) and not np.isnan(twin[1]).all()
    eng = _engine(c, cuda_device)
    eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
    dv = _Sweeps(eng, case, cuda_device)
    for kind in ("eval", "value"):
        _, Vb, got_pol, delta, changed = dv.sweep(kind, 0, n)
        e_Vb, e_pol, e_delta, e_changed = _expected(case, twin, kind, 0, n)
        nan = np.isnan(e_Vb)
        assert np.array_equal(np.isnan(Vb), nan), kind
        H.assert_bits_equal(Vb[~nan], e_Vb[~nan], f"{kind}: entries that are not NaN")
        assert np.array_equal(got_pol, e_pol) and delta == e_delta, kind
        assert changed == (None if kind == "eval" else e_changed), kind        # an evaluation sweep counts no changes
    eng.close()


def test_solver_run_equals_the_checker_backend(cuda_device):
    """Cart-pole swing-up 9 x 7 x 11 x 5 with its 8-point set (action noise 2.0, state noise 0.3 / 0.4 in dimensions 1
    and 3, 2 nodes each), risk="worst", capped at 3 rounds x 50 sweeps: V, policy, sweep counts and the stable flag of the
    same run on the CPU backend of tests/robust_backend.py."""
    name, shape = "cartpole_swingup", (9, 7, 11, 5)
    cls = envs.ENVS[name]
    cfg = CudaPIConfig(**{**cls.CONFIG, "max_eval_iter": 50, "max_pi_iter": 3})
    d = Disturbances.uniform(4, state_noise=[0.0, 0.3, 0.0, 0.4], action_noise=2.0, points=2)
    assert d.K == 8
    space = H.env_bins_space(name, shape)
    gpu = cls(space, cls.ACTIONS, cfg, device=cuda_device, transport=False)
    cpu = with_robust_backend(cls)(space, cls.ACTIONS, cfg)
    for s in (gpu, cpu):
        s.set_disturbances(d, risk="worst")
        s.run()
    assert gpu.stats["risk"] == "worst" == cpu.stats["risk"] and gpu.stats["disturbances"] == 8
    assert cpu._backend.calls["robust_eval"] == cpu.stats["eval_sweeps"] > 0 and cpu._backend.calls["expect_eval"] == 0
    H.assert_bits_equal(gpu.value_function, cpu.value_function, "V of the worst-case run")
    assert np.array_equal(gpu.policy, cpu.policy)
    assert gpu.stats["sweeps_per_iter"] == cpu.stats["sweeps_per_iter"] and gpu.stats["pi_iterations"] == cpu.stats["pi_iterations"]
    assert gpu.stats["stable"] == cpu.stats["stable"] and gpu.stats["eval_sweeps"] == cpu.stats["eval_sweeps"]
    mean = cls(space, cls.ACTIONS, cfg, device=cuda_device, transport=False)
    mean.set_disturbances(d)
    mean.run()
    assert "risk" not in mean.stats
    assert not np.array_equal(mean.value_function.view(np.uint32), gpu.value_function.view(np.uint32))
