"""
Grid continuation on the device: the resample kernel (csrc/pi_resample_kernels.hip behind pi_infer_resample) against its
numpy twin (utils.barycentric.resample), solver.continue_from against a checker-backend solver whose arrays were filled
from the twin, and the runner's --coarse-bins.  Every comparison is bitwise.  The host half is
tests/test_continuation_host.py.
"""
from __future__ import annotations

import ctypes
from functools import lru_cache
from itertools import product

import numpy as np
import pytest

from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd.solver import CudaPIConfig
from tests import helpers as H
from utils import barycentric as B

pytestmark = pytest.mark.gpu

POISON_V, POISON_P = np.float32(-12345.5), np.int32(-7)
# source shape -> destination shape: ragged against the wave (64) and the workgroup (256)
KERNEL_SHAPES = {2: ((11, 13), (37, 41)), 4: ((5, 4, 6, 3), (9, 7, 11, 5)), 6: ((3, 3, 4, 2, 3, 3), (5, 4, 6, 3, 5, 4))}
ORDERS = {2: (1, 0), 4: (2, 0, 3, 1), 6: (5, 4, 2, 3, 0, 1)}


def _bits(D):
    return np.array(list(product([0, 1], repeat=D)), dtype=np.int32)


def _row_major(shape):
    return np.array([int(np.prod(shape[d + 1:])) for d in range(len(shape))], dtype=np.int64)


def _memory_strides(shape, order):
    """Element stride of every USER dimension when memory dimension k (0 = slowest) holds user dimension order[k]."""
    strides, step = np.zeros(len(shape), dtype=np.int64), 1
    for d in reversed(order):
        strides[d] = step
        step *= int(shape[d])
    return strides


def _to_memory(a, shape, order):
    return np.ascontiguousarray(a.reshape(shape).transpose(order)).reshape(-1)


@lru_cache(maxsize=None)
def _source(D, src_shape):
    """A seeded solution on a grid with other bounds in every dimension: random V, random policy over five actions."""
    rng = np.random.default_rng(100 + D)
    lo = np.float32([-(1.0 + 0.25 * d) for d in range(D)])
    hi = np.float32([1.0 + 0.5 * d for d in range(D)])
    n = int(np.prod(src_shape))
    actions = np.float32([-2.0, -0.5, 0.0, 0.5, 2.0])
    return dict(V=rng.standard_normal(n).astype(np.float32), P=rng.integers(0, len(actions), n).astype(np.int32),
                actions=actions, grid=dict(bounds_low=lo, bounds_high=hi, grid_shape=np.int32(src_shape),
                                           strides=_row_major(src_shape).astype(np.int32), corner_bits=_bits(D)))


@lru_cache(maxsize=None)
def _destination(D, src_shape, dst_shape, bounds):
    """Bin tables of the destination — wider than the source's bounds (nodes clamp) or narrower — with uneven spacing,
    a seeded terminal mask, and the twin's answer in the USER's order with and without an action map."""
    src = _source(D, src_shape)
    rng = np.random.default_rng(7 * D + len(bounds))
    lo, hi = src["grid"]["bounds_low"].astype(np.float64), src["grid"]["bounds_high"].astype(np.float64)
    scale = 1.3 if bounds == "wider" else 0.6
    mid, half = (lo + hi) / 2 + (0.0 if bounds == "wider" else 0.1), (hi - lo) / 2 * scale
    bins = []
    for d, g in enumerate(dst_shape):
        inner = np.sort(rng.uniform(mid[d] - half[d], mid[d] + half[d], g - 2))
        bins.append(np.concatenate([[mid[d] - half[d]], inner, [mid[d] + half[d]]]).astype(np.float32))
    mask = rng.random(int(np.prod(dst_shape))) < 0.2
    dst_actions = np.float32([-1.0, 0.0, 1.0])
    amap = B.action_map(src["actions"], dst_actions)
    assert amap.tolist() == [0, 0, 1, 1, 2]
    V, P = B.resample(src["V"], src["P"], bins=bins, **src["grid"])
    _, P_mapped = B.resample(None, src["P"], bins=bins, action_map=amap, **src["grid"])
    for a in (V, P, P_mapped, mask):
        a.setflags(write=False)
    return dict(bins=bins, mask=mask, amap=amap, n_dst_actions=len(dst_actions), V=V, P=P, P_mapped=P_mapped)


def _device_policy(src, cuda_device):
    g = src["grid"]
    dp = B.DevicePolicy(src["P"], src["actions"], g["bounds_low"], g["bounds_high"], g["grid_shape"], g["strides"],
                        g["corner_bits"], device=cuda_device)
    dp.set_values(src["V"])
    return dp


def _run_kernel(dp, dst, shape, order, cuda_device, *, mask, mapped, want_V=True, want_P=True):
    """One launch into poisoned outputs; returns (V, policy) as numpy arrays in MEMORY order (None where not asked for)."""
    import torch
    n = int(np.prod(shape))
    out_V = torch.full((n,), float(POISON_V), dtype=torch.float32, device=cuda_device) if want_V else None
    out_P = torch.full((n,), int(POISON_P), dtype=torch.int32, device=cuda_device) if want_P else None
    term = torch.from_numpy(np.array(_to_memory(dst["mask"].view(np.uint8), shape, order))).to(cuda_device) if mask else None
    dp.resample(dst["bins"], _memory_strides(shape, order), term, out_V, out_P,
                action_map=dst["amap"] if mapped else None, n_actions=dst["n_dst_actions"] if mapped else None)
    torch.cuda.synchronize(cuda_device)
    return (None if out_V is None else out_V.cpu().numpy()), (None if out_P is None else out_P.cpu().numpy())


def _expected(dst, shape, order, *, mask, mapped):
    V, P = dst["V"], dst["P_mapped"] if mapped else dst["P"]
    if mask:
        V, P = np.where(dst["mask"], POISON_V, V), np.where(dst["mask"], POISON_P, P)
    return _to_memory(V, shape, order), _to_memory(P.astype(np.int32), shape, order)


@pytest.mark.parametrize("bounds", ["wider", "narrower"])
@pytest.mark.parametrize("D", [2, 4, 6])
def test_kernel_equals_the_twin(D, bounds, cuda_device):
    """V and policy of random source tables, bit for bit: the user's memory order and a permuted one, with a mask
    (masked nodes keep the poison they held) and without, identity and non-identity action map, V-only and policy-only."""
    src_shape, dst_shape = KERNEL_SHAPES[D]
    src, dst = _source(D, src_shape), _destination(D, src_shape, dst_shape, bounds)
    clamped = sum(int(((b < l) | (b > h)).sum()) for b, l, h in zip(dst["bins"], src["grid"]["bounds_low"], src["grid"]["bounds_high"]))
    assert (clamped > 0) == (bounds == "wider")
    dp = _device_policy(src, cuda_device)
    try:
        for order in (tuple(range(D)), ORDERS[D]):
            for mask in (False, True):
                for mapped in (False, True):
                    what = f"{D}-D {bounds} order {order} mask {mask} map {mapped}"
                    want_V, want_P = _expected(dst, dst_shape, order, mask=mask, mapped=mapped)
                    got_V, got_P = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=mask, mapped=mapped)
                    H.assert_bits_equal(got_V, want_V, what + ": V")
                    H.assert_bits_equal(got_P, want_P, what + ": policy")
            want_V, want_P = _expected(dst, dst_shape, order, mask=True, mapped=True)
            got_V, none = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=True, mapped=True, want_P=False)
            assert none is None
            H.assert_bits_equal(got_V, want_V, f"{D}-D {bounds} order {order}: V alone")
            none, got_P = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=True, mapped=True, want_V=False)
            assert none is None
            H.assert_bits_equal(got_P, want_P, f"{D}-D {bounds} order {order}: policy alone")
    finally:
        dp.close()


def test_policy_alone_needs_no_values_and_values_alone_no_policy(cuda_device):
    src_shape, dst_shape = KERNEL_SHAPES[4]
    src, dst = _source(4, src_shape), _destination(4, src_shape, dst_shape, "wider")
    g = src["grid"]
    order = tuple(range(4))
    args = (g["bounds_low"], g["bounds_high"], g["grid_shape"], g["strides"], g["corner_bits"])
    dp = B.DevicePolicy(src["P"], src["actions"], *args, device=cuda_device)               # never saw set_values
    try:
        _, got_P = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=False, mapped=False, want_V=False)
        H.assert_bits_equal(got_P, dst["P"], "policy from a handle without values")
        with pytest.raises(RuntimeError, match="set_values"):
            _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=False, mapped=False)
    finally:
        dp.close()
    dp = B.DevicePolicy(None, None, *args, device=cuda_device)
    try:
        dp.set_values(src["V"])
        got_V, _ = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=False, mapped=False, want_P=False)
        H.assert_bits_equal(got_V, dst["V"], "V from a handle without a policy")
        with pytest.raises(RuntimeError, match="without a policy table"):
            _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=False, mapped=False)
    finally:
        dp.close()


def test_the_library_refuses_a_map_entry_out_of_range_and_a_short_identity(cuda_device):
    """pi_infer_resample's own checks of the action map need the source's action count, which only a device handle with a
    policy knows; the binding's check is bypassed here."""
    import torch
    src_shape, dst_shape = KERNEL_SHAPES[2]
    src, dst = _source(2, src_shape), _destination(2, src_shape, dst_shape, "wider")
    dp = _device_policy(src, cuda_device)
    try:
        out = torch.full((int(np.prod(dst_shape)),), int(POISON_P), dtype=torch.int32, device=cuda_device)
        shape = np.int32(dst_shape)
        strides = _row_major(dst_shape)
        bins = np.concatenate(dst["bins"])
        i32p, f32p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_float, ctypes.c_int64))

        def call(amap, n_actions):
            m = None if amap is None else np.int32(amap)
            return _native.lib().pi_infer_resample(dp._engine._h, shape.ctypes.data_as(i32p), strides.ctypes.data_as(i64p),
                                                   bins.ctypes.data_as(f32p), None if m is None else m.ctypes.data_as(i32p),
                                                   n_actions, None, None, out.data_ptr(), None)
        assert call([0, 0, 1, 3, 2], 3) != 0 and "action_map[3] = 3 is not an index" in _native.last_error()
        assert call([0, -1, 1, 1, 2], 3) != 0 and "action_map[1] = -1 is not an index" in _native.last_error()
        assert call(None, 4) != 0 and "at least the source's 5 actions" in _native.last_error()
        torch.cuda.synchronize(cuda_device)
        assert (out.cpu().numpy() == POISON_P).all()                                  # refused: nothing was launched
        assert call(None, 5) == 0
        torch.cuda.synchronize(cuda_device)
        H.assert_bits_equal(out.cpu().numpy(), dst["P"], "identity map")
    finally:
        dp.close()


@pytest.mark.parametrize("D", [2, 4, 6])
def test_source_with_two_bins_in_every_dimension(D, cuda_device):
    """One source cell: base index 0 everywhere, every destination node between the same 2^D corners."""
    _, dst_shape = KERNEL_SHAPES[D]
    src_shape = (2,) * D
    src, dst = _source(D, src_shape), _destination(D, src_shape, dst_shape, "wider")
    dp = _device_policy(src, cuda_device)
    try:
        for order in (tuple(range(D)), ORDERS[D]):
            want_V, want_P = _expected(dst, dst_shape, order, mask=True, mapped=False)
            got_V, got_P = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=True, mapped=False)
            H.assert_bits_equal(got_V, want_V, f"{D}-D from 2 bins, order {order}: V")
            H.assert_bits_equal(got_P, want_P, f"{D}-D from 2 bins, order {order}: policy")
    finally:
        dp.close()


@pytest.mark.parametrize("dst_shape", [(2, 2046), (2, 2047), (2100, 2)])
def test_bin_tables_at_the_threshold_between_the_two_entry_points(dst_shape, cuda_device):
    """2 048 table floats are the last size pi_resample_kernel stages, 2 049 the first that takes pi_resample_wide_kernel."""
    src_shape = KERNEL_SHAPES[2][0]
    src, dst = _source(2, src_shape), _destination(2, src_shape, dst_shape, "wider")
    dp = _device_policy(src, cuda_device)
    try:
        for order in ((0, 1), (1, 0)):
            want_V, want_P = _expected(dst, dst_shape, order, mask=True, mapped=True)
            got_V, got_P = _run_kernel(dp, dst, dst_shape, order, cuda_device, mask=True, mapped=True)
            H.assert_bits_equal(got_V, want_V, f"{dst_shape} order {order}: V")
            H.assert_bits_equal(got_P, want_P, f"{dst_shape} order {order}: policy")
    finally:
        dp.close()


def test_64_bit_positions(cuda_device):
    """A destination of 182^4 = 1 097 199 376 nodes (>= 2^30: byte offsets beyond 2^32) in a permuted memory order from a
    6^4 source: 2^18 scattered memory positions and the last 4 096 against the twin, masked nodes among them."""
    import gc
    import torch
    D, src_shape, dst_shape, order = 4, (6, 6, 6, 6), (182,) * 4, (2, 0, 3, 1)
    n = int(np.prod(dst_shape, dtype=np.int64))
    assert n >= 1 << 30 and 4 * n >= 1 << 32
    src = _source(D, src_shape)
    lo, hi = src["grid"]["bounds_low"], src["grid"]["bounds_high"]
    bins = [np.linspace(1.1 * l, 1.1 * h, g, dtype=np.float32) for l, h, g in zip(lo, hi, dst_shape)]
    # the mask per dimension, as the solver builds it: node (i0, i1, i2, i3) is terminal iff i0 % 5 == 0 and i3 % 3 == 1
    small = (np.arange(182) % 5 == 0).reshape(-1, 1, 1, 1) & (np.arange(182) % 3 == 1).reshape(1, 1, 1, -1)
    term = torch.from_numpy(small).to(cuda_device).expand(dst_shape).permute(*order).contiguous().reshape(-1).to(torch.uint8)
    out_V = torch.full((n,), float(POISON_V), dtype=torch.float32, device=cuda_device)
    out_P = torch.full((n,), int(POISON_P), dtype=torch.int32, device=cuda_device)
    dp = _device_policy(src, cuda_device)
    try:
        dp.resample(bins, _memory_strides(dst_shape, order), term, out_V, out_P)
        torch.cuda.synchronize(cuda_device)
    finally:
        dp.close()
    rng = np.random.default_rng(64)
    at_mem = np.concatenate([np.sort(rng.integers(0, n, 1 << 18)), np.arange(n - 4096, n)]).astype(np.int64)
    assert (at_mem >= 1 << 30).sum() > 4096
    im = np.stack(np.unravel_index(at_mem, [dst_shape[d] for d in order]), axis=1)
    iu = np.empty_like(im)
    for k, d in enumerate(order):
        iu[:, d] = im[:, k]
    at_user = np.ravel_multi_index(tuple(iu.T), dst_shape)
    masked = (iu[:, 0] % 5 == 0) & (iu[:, 3] % 3 == 1)
    assert 100 < masked.sum() < len(masked) // 4
    want_V, want_P = B.resample(src["V"], src["P"], bins=bins, at=at_user, **src["grid"])
    pick = torch.from_numpy(at_mem).to(cuda_device)
    got_V, got_P, got_term = out_V[pick].cpu().numpy(), out_P[pick].cpu().numpy(), term[pick].cpu().numpy()
    del out_V, out_P, term, pick
    gc.collect()
    torch.cuda.empty_cache()
    assert np.array_equal(got_term != 0, masked)
    H.assert_bits_equal(got_V, np.where(masked, POISON_V, want_V), "182^4: V")
    H.assert_bits_equal(got_P, np.where(masked, POISON_P, want_P).astype(np.int32), "182^4: policy")


# ── solver level ──────────────────────────────────────────────────────────────────────────────────────────────────
SOLVER_CASES = {
    "pendulum": ((25, 25), (50, 50), {}),
    "mountain_car": ((30, 30), (60, 60), {}),
    "cartpole": ((6,) * 4, (12,) * 4, {}),
    "double_cartpole": ((5,) * 6, (7,) * 6, dict(max_pi_iter=3, max_eval_iter=200)),      # bounded: the checker's time
}


def _config(name, overrides):
    return CudaPIConfig(**{**envs.ENVS[name].CONFIG, **overrides})


def _make(cls, name, shape, overrides, checker=False):
    klass = H.with_checker_backend(cls) if checker else cls
    return klass(H.env_bins_space(name, shape), cls.ACTIONS, _config(name, overrides))


def _solution(solver):
    return dict(V=solver.value_function, policy=solver.policy, rounds=solver.stats["pi_iterations"],
                sweeps=list(solver.stats["sweeps_per_iter"]), stable=solver.stats.get("stable"))


def _fill_from_twin(checker, source, policy=True):
    """What continue_from does, restated with the twin on a checker-backend solver: non-terminal nodes take the
    interpolated V (both buffers) and the nearest node's action, in the solver's memory order."""
    n = checker.n_states
    V, P = B.resample(source.value_function, source.policy if policy else None, source.bounds_low, source.bounds_high,
                      source.grid_shape, source.strides, source.corner_bits, checker._bins,
                      action_map=B.action_map(source.action_space, checker.action_space))
    live = ~checker._to_user(checker.d_terminal_mask.numpy()[:n]).astype(bool)
    V_now = np.array(checker._to_user(checker.d_value_function.numpy()[:n]))
    V_now[live] = V[live]
    checker.d_value_function.numpy()[:n] = checker._to_memory(V_now)
    checker.d_new_value_function.copy_(checker.d_value_function)
    if policy:
        P_now = np.array(checker._to_user(checker.d_policy.numpy()[:n]))
        P_now[live] = P[live]
        checker.d_policy.numpy()[:n] = checker._to_memory(P_now)


@lru_cache(maxsize=None)
def _coarse(name):
    coarse_shape, _, overrides = SOLVER_CASES[name]
    solver = _make(envs.ENVS[name], name, coarse_shape, overrides)
    solver.run()
    return solver


@lru_cache(maxsize=None)
def _continued(name):
    _, fine_shape, overrides = SOLVER_CASES[name]
    solver = _make(envs.ENVS[name], name, fine_shape, overrides)
    solver.continue_from(_coarse(name))
    assert solver.stats["continued_from"]["grid_shape"] == list(SOLVER_CASES[name][0])
    assert solver.stats["continued_from"]["seconds"] > 0
    solver.run()
    return solver


@pytest.mark.parametrize("name", list(SOLVER_CASES))
def test_continue_from_then_run_equals_the_checker_filled_from_the_twin(name, cuda_device):
    _, fine_shape, overrides = SOLVER_CASES[name]
    got = _solution(_continued(name))
    checker = _make(envs.ENVS[name], name, fine_shape, overrides, checker=True)
    _fill_from_twin(checker, _coarse(name))
    checker.run()
    want = _solution(checker)
    print(f"[continuation] {name} {SOLVER_CASES[name][0]} -> {fine_shape}: rounds {got['rounds']} (checker {want['rounds']}), "
          f"sweeps {sum(got['sweeps'])} (checker {sum(want['sweeps'])}), stable {got['stable']}")
    assert got["rounds"] == want["rounds"] and got["sweeps"] == want["sweeps"] and got["stable"] == want["stable"]
    H.assert_bits_equal(got["V"], want["V"], f"{name}: V")
    H.assert_bits_equal(got["policy"], want["policy"], f"{name}: policy")


@pytest.mark.parametrize("name", ["pendulum", "mountain_car"])
def test_continued_run_converges_in_fewer_sweeps_to_the_cold_run_s_solution(name, cuda_device):
    """Both runs stop at a residual below theta, not at the fixed point: each is within theta * gamma / (1 - gamma) of
    it, so they are within twice that of each other."""
    _, fine_shape, overrides = SOLVER_CASES[name]
    cold = _make(envs.ENVS[name], name, fine_shape, overrides)
    cold.run()
    warm = _continued(name)
    cfg = warm.config
    bound = 2.0 * cfg.theta * cfg.gamma / (1.0 - cfg.gamma)
    gap = float(np.abs(warm.value_function - cold.value_function).max())
    agree = float((warm.policy == cold.policy).mean())
    print(f"[continuation] {name}: cold {cold.stats['eval_sweeps']} sweeps in {cold.stats['pi_iterations']} rounds, continued "
          f"{warm.stats['eval_sweeps']} in {warm.stats['pi_iterations']}; max|dV| {gap:.3g} (bound {bound:.3g}), policy agreement {agree:.4f}")
    assert warm.stats["stable"] and cold.stats["stable"]
    assert warm.stats["eval_sweeps"] < cold.stats["eval_sweeps"]
    assert gap <= bound


def test_continue_from_in_an_explicit_memory_order(cuda_device):
    """A subclass with a MEMORY_ORDER of its own, applied at this size: the device arrays are filled in that order."""
    name = "cartpole"
    _, fine_shape, overrides = SOLVER_CASES[name]

    class Ordered(envs.ENVS[name]):
        MEMORY_ORDER = (2, 0, 3, 1)
        _ORDER_MIN_STATES = 0
    solver = _make(Ordered, name, fine_shape, overrides)
    assert solver._order == (2, 0, 3, 1)
    solver.continue_from(_coarse(name))
    checker = _make(Ordered, name, fine_shape, overrides, checker=True)
    assert checker._order == (2, 0, 3, 1)
    _fill_from_twin(checker, _coarse(name))
    n = solver.n_states
    H.assert_bits_equal(solver.d_value_function[:n].cpu().numpy(), checker.d_value_function.numpy()[:n], "V in memory order")
    H.assert_bits_equal(solver.d_new_value_function[:n].cpu().numpy(), checker.d_value_function.numpy()[:n], "second buffer")
    H.assert_bits_equal(solver.d_policy[:n].cpu().numpy(), checker.d_policy.numpy()[:n], "policy in memory order")
    solver.run()
    got, want = _solution(solver), _solution(_continued(name))                          # results never depend on the order
    assert got["rounds"] == want["rounds"] and got["sweeps"] == want["sweeps"]
    H.assert_bits_equal(got["V"], want["V"], "V after run()")
    H.assert_bits_equal(got["policy"], want["policy"], "policy after run()")


def test_values_only_and_the_three_kinds_of_source(tmp_path, cuda_device):
    name = "mountain_car"
    _, fine_shape, overrides = SOLVER_CASES[name]
    cls = envs.ENVS[name]
    coarse = _coarse(name)
    n = int(np.prod(fine_shape))
    # policy=False: V as before, the policy stays what construction made it
    solver = _make(cls, name, fine_shape, overrides)
    solver.continue_from(coarse, policy=False)
    checker = _make(cls, name, fine_shape, overrides, checker=True)
    _fill_from_twin(checker, coarse, policy=False)
    assert not checker.d_policy.numpy().any()
    H.assert_bits_equal(solver.d_value_function[:n].cpu().numpy(), checker.d_value_function.numpy()[:n], "policy=False: V")
    H.assert_bits_equal(solver.d_policy[:n].cpu().numpy(), checker.d_policy.numpy()[:n], "policy=False: policy")
    solver.run()
    checker.run()
    assert solver.stats["sweeps_per_iter"] == checker.stats["sweeps_per_iter"]
    H.assert_bits_equal(solver.value_function, checker.value_function, "policy=False: V after run()")
    H.assert_bits_equal(solver.policy, checker.policy, "policy=False: policy after run()")
    # ... after run() the device arrays are gone
    with pytest.raises(RuntimeError, match="before run"):
        solver.continue_from(coarse)
    # a save() archive by its path, and a load()ed instance: the same fill as from the solver itself
    checker = _make(cls, name, fine_shape, overrides, checker=True)
    _fill_from_twin(checker, coarse)
    coarse.save(tmp_path / "coarse.npz")
    for source in (tmp_path / "coarse.npz", str(tmp_path / "coarse"), cls.load(tmp_path / "coarse.npz")):
        fresh = _make(cls, name, fine_shape, overrides)
        fresh.continue_from(source)
        H.assert_bits_equal(fresh.d_value_function[:n].cpu().numpy(), checker.d_value_function.numpy()[:n], f"{type(source).__name__}: V")
        H.assert_bits_equal(fresh.d_policy[:n].cpu().numpy(), checker.d_policy.numpy()[:n], f"{type(source).__name__}: policy")
        fresh._backend.close()


def test_runner_coarse_bins_writes_the_solver_level_result(tmp_path, cuda_device, capsys):
    from runners import _cli
    path = tmp_path / "pendulum_policy.npz"
    pi = _cli.main("pendulum", str(path), ["--bins", "50", "--coarse-bins", "25", "--retrain"])
    out = capsys.readouterr().out
    assert "continuation level 25 bins" in out and "eval sweeps" in out
    want = _continued("pendulum")
    assert pi.stats["continued_from"]["grid_shape"] == [25, 25] and pi.stats["sweeps_per_iter"] == want.stats["sweeps_per_iter"]
    data = np.load(path)
    H.assert_bits_equal(data["value_function"], want.value_function, "archive: V")
    H.assert_bits_equal(data["policy"], want.policy, "archive: policy")
    assert data["grid_shape"].tolist() == [50, 50]
