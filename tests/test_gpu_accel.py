"""
GPU: the two kernels of csrc/pi_accel_kernels.hip (through pi_accel_update / pi_accel_combine) against the numpy twin of
dynamicprogramming_amd.accel, bit for bit — sizes around every boundary of the reduction tree, every shape of the ring,
misaligned views, `out` aliasing `g`, column offsets past 2^32 bytes — and the accelerated solver against the same loop
on the CPU backend of tests/accel_backend.py: V, policy, rounds, sweeps per round, extrapolations and restarts all equal,
with no tolerance (sweeps = oracle, kernels = twin, the solve is the same host code).
"""
from __future__ import annotations

import numpy as np
import pytest

from dynamicprogramming_amd import _native, accel, envs
from dynamicprogramming_amd.noise import Disturbances
from dynamicprogramming_amd.solver import CudaPIConfig
from tests import helpers as H
from tests.accel_backend import with_accel_backend

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 8193, 256 * 4096 + 5]
# (m, slot, k_used, first): the first push; one column; slot 0 and slot m - 1 of a full window; a wrapped ring (the slot in
# the middle of a full window); a window that is filling
RINGS = [(4, 0, 0, True), (1, 0, 1, False), (8, 0, 8, False), (8, 7, 8, False), (8, 3, 8, False), (4, 2, 3, False)]


@pytest.fixture(scope="module")
def engine(cuda_device):
    import torch
    bins = H.env_bins("pendulum", (24, 17))
    eng = _native.Engine(2, [24, 17], [b.min() for b in bins], [b.max() for b in bins], bins, envs.PendulumCuda.ACTIONS,
                         device=cuda_device.index or 0)
    eng.compile(envs.dynamics_source("pendulum"))                 # gives the handle its code-object cache
    yield eng
    torch.cuda.synchronize()
    eng.close()


def _arrays(rng, n, m, offset):
    """Host arrays and their device copies; `offset` = 1: every device array is a view one element into its allocation."""
    import torch
    host = {k: rng.standard_normal(n).astype(np.float32) for k in ("x", "g", "f_prev", "g_prev")}
    host.update({k: rng.standard_normal((m, n)).astype(np.float32) for k in ("dF", "dG")})
    dev = {}
    for k, a in host.items():
        flat = torch.zeros(a.size + offset, dtype=torch.float32, device="cuda")
        view = flat[offset:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        dev[k] = view
        assert view.data_ptr() % 16 == (4 * offset) % 16
    return host, dev


@pytest.mark.parametrize("n", SIZES)
def test_update_and_combine_equal_the_twin(n, engine, cuda_device):
    import torch
    st = torch.cuda.current_stream(cuda_device).cuda_stream
    rng = np.random.default_rng(n)
    # the size that crosses the second level of the tree: the first push and the wrapped full window (the twin's 17 dot
    # products over a million elements are what takes the time)
    for m, slot, k, first in (RINGS if n < 1 << 20 else [RINGS[0], RINGS[4]]):
        for offset in (0, 1):
            host, dev = _arrays(rng, n, m, offset)
            d_dots = torch.full((17,), -1.0, dtype=torch.float64, device=cuda_device)
            engine.accel_update(dev["x"].data_ptr(), dev["g"].data_ptr(), dev["f_prev"].data_ptr(), dev["g_prev"].data_ptr(),
                                dev["dF"].data_ptr(), dev["dG"].data_ptr(), m, slot, k, first, n, d_dots.data_ptr(), st)
            want = accel.dots(host["x"], host["g"], host["f_prev"], host["g_prev"], host["dF"], host["dG"], slot, k, first)
            got = d_dots.cpu().numpy()
            what = f"n={n} m={m} slot={slot} k={k} first={first} offset={offset}"
            H.assert_bits_equal(got[:2 * k + 1], want, f"dots, {what}")
            assert (got[2 * k + 1:] == -1.0).all(), what
            for key in ("f_prev", "g_prev", "dF", "dG", "x", "g"):
                H.assert_bits_equal(dev[key].cpu().numpy(), host[key], f"{key}, {what}")
            # the combine over the same ring: into another array, then in place
            coeffs = rng.standard_normal(k).tolist()
            out = torch.zeros(n + offset, dtype=torch.float32, device=cuda_device)[offset:]
            engine.accel_combine(dev["g"].data_ptr(), dev["dG"].data_ptr(), coeffs, k, n, out.data_ptr(), st)
            expect = accel.combine(host["g"], host["dG"], coeffs, k)
            H.assert_bits_equal(out.cpu().numpy(), expect, f"combine, {what}")
            engine.accel_combine(dev["g"].data_ptr(), dev["dG"].data_ptr(), coeffs, k, n, dev["g"].data_ptr(), st)
            H.assert_bits_equal(dev["g"].cpu().numpy(), expect, f"combine with out == g, {what}")


def test_zero_columns_keep_the_bits_of_g_on_the_device(engine, cuda_device):
    import torch
    st = torch.cuda.current_stream(cuda_device).cuda_stream
    g = np.float32([-0.0, 0.0, 1.5, -3.25e-40, np.pi, -7.0] * 700)
    d_g = torch.from_numpy(g).to(cuda_device)
    d_dG = torch.zeros((3, len(g)), dtype=torch.float32, device=cuda_device)
    engine.accel_combine(d_g.data_ptr(), d_dG.data_ptr(), [-1.0, -2.5, 1e300], 3, len(g), d_g.data_ptr(), st)
    H.assert_bits_equal(d_g.cpu().numpy(), g, "combine with zero columns")


def test_column_offsets_past_2_pow_32_bytes(engine, cuda_device):
    """n = 2^27 + 3 at m = 8: the last column of the (m, n) rings ends 96 bytes past 2^32.  The arrays are zero except their
    first and last 5 000 elements, so the twin needs only the tiles that hold data: every other tile sum is exactly 0.0."""
    import torch
    st = torch.cuda.current_stream(cuda_device).cuda_stream
    n, m, edge = (1 << 27) + 3, 8, 5000
    assert 4 * m * n > 1 << 32 and 4 * (m - 1) * n < 1 << 32
    rng = np.random.default_rng(27)
    tiles = -(-n // accel.TILE)
    tail0 = ((n - edge) // accel.TILE) * accel.TILE               # tile-aligned start of the tail region
    spans = [(0, 2 * accel.TILE), (tail0, n)]
    host, dev = {}, {}
    for key, rows in (("x", 1), ("g", 1), ("f_prev", 1), ("g_prev", 1), ("dF", m), ("dG", m)):
        d = torch.zeros((rows, n), dtype=torch.float32, device=cuda_device)
        host[key] = []
        for lo, hi in spans:
            a = np.zeros((rows, hi - lo), np.float32)
            keep = slice(0, edge) if lo == 0 else slice(n - edge - lo, hi - lo)
            a[:, keep] = rng.standard_normal((rows, edge)).astype(np.float32)
            d[:, lo:hi] = torch.from_numpy(a).to(cuda_device)
            host[key].append(a if rows > 1 else a[0])
        dev[key] = d if rows > 1 else d[0]
    slot, k = m - 1, m
    d_dots = torch.zeros(17, dtype=torch.float64, device=cuda_device)
    engine.accel_update(dev["x"].data_ptr(), dev["g"].data_ptr(), dev["f_prev"].data_ptr(), dev["g_prev"].data_ptr(),
                        dev["dF"].data_ptr(), dev["dG"].data_ptr(), m, slot, k, False, n, d_dots.data_ptr(), st)
    got = d_dots.cpu().numpy()
    parts = {q: np.zeros(tiles, np.float64) for q in range(2 * k + 1)}
    for r, (lo, hi) in enumerate(spans):
        h = {key: host[key][r] for key in host}
        f = h["g"] - h["x"]
        h["dF"][slot] = f - h["f_prev"]
        h["dG"][slot] = h["g"] - h["g_prev"]
        t0, t1 = lo // accel.TILE, -(-hi // accel.TILE)
        for j in range(k):
            parts[j][t0:t1] = accel._tile_sums(h["dF"][j], f)
            parts[k + j][t0:t1] = accel._tile_sums(h["dF"][j], h["dF"][slot])
        parts[2 * k][t0:t1] = accel._tile_sums(f, f)
        H.assert_bits_equal(dev["dF"][slot, lo:hi].cpu().numpy(), h["dF"][slot], f"new column of dF, elements {lo}..{hi}")
        H.assert_bits_equal(dev["dG"][slot, lo:hi].cpu().numpy(), h["dG"][slot], f"new column of dG, elements {lo}..{hi}")
        H.assert_bits_equal(dev["f_prev"][lo:hi].cpu().numpy(), f, f"f_prev, elements {lo}..{hi}")
    want = np.array([accel._fold(parts[q]) for q in range(2 * k + 1)])
    assert np.all(want[[slot, k + slot, 2 * k]] != 0.0)
    H.assert_bits_equal(got, want, "dots at n = 2^27 + 3, m = 8")
    assert float(dev["dF"][slot, 2 * accel.TILE:tail0].abs().max()) == 0.0
    coeffs = rng.standard_normal(k).tolist()
    engine.accel_combine(dev["g"].data_ptr(), dev["dG"].data_ptr(), coeffs, k, n, dev["g"].data_ptr(), st)
    for r, (lo, hi) in enumerate(spans):
        expect = accel.combine(host["g"][r], host["dG"][r], coeffs, k)
        H.assert_bits_equal(dev["g"][lo:hi].cpu().numpy(), expect, f"combine, elements {lo}..{hi}")


# ---- the solver -----------------------------------------------------------------------------------------------------------
GRIDS = [("pendulum", (50, 50)), ("cartpole_swingup", (9, 7, 11, 5)), ("double_cartpole", (5,) * 6)]


def _pair(name, shape, cuda_device, prepare, **limits):
    cls = envs.ENVS[name]
    cfg = CudaPIConfig(**{**cls.CONFIG, **limits})
    space = H.env_bins_space(name, shape)
    gpu = cls(space, cls.ACTIONS, cfg, device=cuda_device, transport=False)
    cpu = with_accel_backend(cls)(space, cls.ACTIONS, cfg)
    for s in (gpu, cpu):
        prepare(s)
    return gpu, cpu


def _same_books(gpu, cpu, what):
    for key in ("eval_sweeps", "sweeps_per_iter", "pi_iterations", "accel_extrapolations", "accel_restarts", "accel_per_iter"):
        assert gpu.stats[key] == cpu.stats[key], (what, key, gpu.stats[key], cpu.stats[key])
    assert gpu.stats["accel_extrapolations"] >= 1, what


@pytest.mark.parametrize("name,shape", GRIDS)
def test_policy_evaluation_equals_the_checker_backend(name, shape, cuda_device):
    def prepare(s):
        s.policy_improvement()                                   # the greedy policy of V = 0, then fixed
        s.set_acceleration(accel.Anderson())
    gpu, cpu = _pair(name, shape, cuda_device, prepare)
    d_gpu, d_cpu = gpu.policy_evaluation(), cpu.policy_evaluation()
    assert d_gpu == d_cpu < gpu.config.theta
    _same_books(gpu, cpu, name)
    n = gpu.n_states
    H.assert_bits_equal(gpu._to_user(gpu.d_value_function[:n].cpu().numpy()), cpu._to_user(cpu.d_value_function[:n].numpy()),
                        f"{name} V of the accelerated evaluation")


@pytest.mark.parametrize("name,shape", GRIDS)
def test_run_equals_the_checker_backend(name, shape, cuda_device):
    gpu, cpu = _pair(name, shape, cuda_device, lambda s: s.set_acceleration(accel.Anderson()))
    gpu.run()
    cpu.run()
    _same_books(gpu, cpu, name)
    assert gpu.stats["stable"] == cpu.stats["stable"]
    H.assert_bits_equal(gpu.value_function, cpu.value_function, f"{name} V of the accelerated run")
    assert np.array_equal(gpu.policy, cpu.policy)


def test_expected_backup_equals_the_checker_backend(cuda_device):
    d = Disturbances.uniform(4, state_noise=[0.05, 0.0, 0.05, 0.0], action_noise=0.5, points=2)
    assert d.K == 8

    def prepare(s):
        s.set_disturbances(d)
        s.set_acceleration(accel.Anderson())
    # two rounds of at most 301 sweeps: the 8-point twin on the CPU is what takes the time
    gpu, cpu = _pair("cartpole_swingup", (9, 7, 11, 5), cuda_device, prepare, max_pi_iter=2, max_eval_iter=301)
    gpu.run()
    cpu.run()
    _same_books(gpu, cpu, "expected backup")
    assert gpu.stats["stable"] == cpu.stats["stable"] and gpu.stats["disturbances"] == 8
    H.assert_bits_equal(gpu.value_function, cpu.value_function, "V of the accelerated noise-aware run")
    assert np.array_equal(gpu.policy, cpu.policy)


def test_acceleration_off_again_is_the_plain_run_and_the_one_launch_path(cuda_device):
    """Pendulum 50^2 qualifies for the one-launch run.  With acceleration it goes batch by batch; after set_acceleration(None)
    it is the plain solver bit for bit, in one launch again."""
    name, shape = "pendulum", (50, 50)
    cls = envs.ENVS[name]
    space = H.env_bins_space(name, shape)
    make = lambda: cls(space, cls.ACTIONS, CudaPIConfig(**cls.CONFIG), device=cuda_device, transport=False)   # noqa: E731
    plain = make()
    assert plain._backend.whole_run
    plain.run()
    assert plain._backend.whole_runs == 1 and "accel_extrapolations" not in plain.stats
    fast = make()
    fast.set_acceleration(accel.Anderson())
    fast.run()
    assert fast._backend.whole_runs == 0 and fast._backend.xcd_evaluations == 0
    assert fast.stats["accel_extrapolations"] >= 1 and fast.stats["eval_sweeps"] < plain.stats["eval_sweeps"]
    back = make()
    back.set_acceleration(accel.Anderson(window=8))
    back.policy_evaluation()
    assert back._accel_buffers is not None
    back.set_acceleration(None)
    assert back._accel_buffers is None
    fresh = make()
    fresh.set_acceleration(accel.Anderson())
    fresh.set_acceleration(None)
    fresh.run()
    assert fresh._backend.whole_runs == 1
    assert fresh.stats["sweeps_per_iter"] == plain.stats["sweeps_per_iter"]
    H.assert_bits_equal(fresh.value_function, plain.value_function, "V after set_acceleration(None)")
    assert np.array_equal(fresh.policy, plain.policy)
