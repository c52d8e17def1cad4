"""
Grid continuation, the part that needs no GPU: the numpy twin (utils.barycentric.resample) on a case computed by hand,
the action map, the resample kernel compiling for gfx950 behind every D without scratch, the new entry points of the C
ABI and what they refuse, the runner's --coarse-bins flag.  The device half is tests/test_gpu_continuation.py.
"""
from __future__ import annotations

import re
from itertools import product
from pathlib import Path

import numpy as np
import pytest

from dynamicprogramming_amd import _native
from utils import barycentric as B

ROOT = Path(__file__).resolve().parents[1]


def _bits(D):
    return np.array(list(product([0, 1], repeat=D)), dtype=np.int32)


def _row_major(shape):
    return [int(np.prod(shape[d + 1:])) for d in range(len(shape))]


# ── the numpy twin ────────────────────────────────────────────────────────────────────────────────────────────────
def test_twin_on_a_hand_computed_case():
    """Source: 3 x 2 nodes on [0, 2] x [0, 1], V[i, j] = 10 i + j, policy[i, j] = 2 i + j.  Every weight below is a
    dyadic fraction, so the float32 sums are exact and the expected values are written out."""
    grid = dict(bounds_low=np.float32([0, 0]), bounds_high=np.float32([2, 1]), grid_shape=np.int32([3, 2]),
                strides=np.int32([2, 1]), corner_bits=_bits(2))
    V = np.float32([0, 1, 10, 11, 20, 21])
    P = np.arange(6, dtype=np.int32)
    bins = [np.float32([-1.0, 0.25, 1.5, 5.0]), np.float32([0.5, 0.75, 2.0])]
    got_V, got_P = B.resample(V, P, bins=bins, **grid)
    assert got_V.dtype == np.float32 and got_P.dtype == np.int32 and got_V.shape == got_P.shape == (12,)
    # x = -1 clamps to 0 (cell 0, t = 0), 0.25 lies in cell 0 (t = .25), 1.5 in cell 1 (t = .5), 5 clamps to 2 (cell 1,
    # t = 1); y = .5 -> t = .5, .75 -> t = .75, 2 clamps to 1 (t = 1): V = 10 x_clamped + y_clamped
    xs, ys = [0.0, 0.25, 1.5, 2.0], [0.5, 0.75, 1.0]
    assert got_V.reshape(4, 3).tolist() == [[10 * x + y for y in ys] for x in xs]
    # largest weight, the FIRST corner on ties (corner order (0,0) (0,1) (1,0) (1,1)): y = .5 ties towards j = 0,
    # x = 1.5 ties towards i = 1; a clamped coordinate sits on the upper node of the last cell
    assert got_P.reshape(4, 3).tolist() == [[0, 1, 1], [0, 1, 1], [2, 3, 3], [4, 5, 5]]
    # restricted to chosen nodes, in the order asked for; either table alone
    at = np.array([11, 0, 4])
    sub_V, sub_P = B.resample(V, P, bins=bins, at=at, **grid)
    assert sub_V.tolist() == got_V[at].tolist() and sub_P.tolist() == got_P[at].tolist()
    only_V, none = B.resample(V, None, bins=bins, **grid)
    assert none is None and np.array_equal(only_V, got_V)
    none, only_P = B.resample(None, P, bins=bins, chunk=5, **grid)
    assert none is None and np.array_equal(only_P, got_P)
    # an action map sends the source's indices through
    amap = np.int32([5, 4, 3, 2, 1, 0])
    assert B.resample(None, P, bins=bins, action_map=amap, **grid)[1].tolist() == (5 - got_P).tolist()


def test_twin_from_a_source_of_two_bins_per_dimension():
    """One cell: every destination node interpolates between the same four corners."""
    grid = dict(bounds_low=np.float32([-1, -1]), bounds_high=np.float32([1, 1]), grid_shape=np.int32([2, 2]),
                strides=np.int32([2, 1]), corner_bits=_bits(2))
    V = np.float32([0, 4, 8, 12])                       # V = 6 + 4 x + 2 y
    P = np.int32([3, 2, 1, 0])
    bins = [np.float32([-1, -0.5, 0, 1]), np.float32([-3, 0.5, 1])]
    got_V, got_P = B.resample(V, P, bins=bins, **grid)
    assert got_V.reshape(4, 3).tolist() == [[6 + 4 * x + 2 * max(y, -1) for y in (-3, 0.5, 1)] for x in (-1, -0.5, 0, 1)]
    assert got_P.reshape(4, 3).tolist() == [[3, 2, 2], [3, 2, 2], [3, 2, 2], [1, 0, 0]]


def test_action_map():
    same = np.linspace(-2, 2, 21, dtype=np.float32)
    assert B.action_map(same, same.copy()) is None                                    # equal tables: the identity
    # ties go to the lowest index: -0.5 is as far from -1 as from 0, 0.5 as far from 0 as from 1
    m = B.action_map([-2.0, -0.5, 0.5, 2.0], [-1.0, 0.0, 1.0])
    assert m.dtype == np.int32 and m.tolist() == [0, 0, 1, 2]
    # a coarser action set: the nearest value
    fine, coarse = np.linspace(-2, 2, 21, dtype=np.float32), np.float32([-2, 0, 2])
    assert B.action_map(fine, coarse).tolist() == [0] * 5 + [0] + [1] * 9 + [1] + [2] * 5
    assert B.action_map(coarse, fine).tolist() == [0, 10, 20]
    assert B.action_map([1.0, 2.0], [1.0, 2.0, 3.0]).tolist() == [0, 1]               # another length is never "equal"


# ── the kernel builds ─────────────────────────────────────────────────────────────────────────────────────────────
SHAPES = {2: (11, 13), 4: (5, 4, 6, 3), 6: (3, 3, 4, 2, 3, 3)}


def _host_handle(D, cache_dir):
    shape = SHAPES[D]
    return _native.InferenceEngine([-1.0] * D, [1.0] * D, shape, _row_major(shape), _bits(D), device=-1, cache_dir=cache_dir)


@pytest.mark.parametrize("D", [2, 4, 6])
def test_resample_module_compiles_for_gfx950_without_a_gpu(D, tmp_path):
    """pi_infer_set_values on a host-only handle: the handle's grid + csrc/pi_resample_kernels.hip build through hipRTC
    into a further code object that holds both entry points of the kernel."""
    eng = _host_handle(D, tmp_path)
    before = set(tmp_path.glob("pi_*.hsaco"))
    assert len(before) == 1
    log = eng.set_values(np.zeros(int(np.prod(SHAPES[D])), np.float32))
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"pi_resample_kernel" in blob and b"pi_resample_wide_kernel" in blob
    eng.set_values(np.zeros(int(np.prod(SHAPES[D])), np.float32))                    # again: nothing new is built
    assert len(list(tmp_path.glob("pi_*.hsaco"))) == 2
    eng.close()


def test_resample_kernel_does_not_spill(tmp_path):
    """The 6-D kernel holds 64 weights, 64 indices and 64 source values per lane: no scratch in any D, on the
    ahead-of-time build of the translation unit pi_infer_set_values hands to hipRTC (tests/helpers.inference_unit restates
    it from the header's description), for the BASELINE grids as sources."""
    from dynamicprogramming_amd import envs
    from tests import helpers as H
    for name, bins in (("pendulum", 200), ("double_pendulum_swingup", 40), ("double_cartpole", 13)):
        D = envs.ENVS[name]._D
        text = H.inference_unit(H.inference_grid(name, bins), None, "", ["pi_resample_kernels.hip"])
        usage = H.kernel_resource_usage(text, tmp_path, name)
        print(f"{name} {bins}^{D}: {usage}")
        assert set(usage) == {"pi_resample_kernel", "pi_resample_wide_kernel"}
        for k in usage.values():
            assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, usage)
        assert usage["pi_resample_kernel"]["lds"] == 4 * 2048 and usage["pi_resample_wide_kernel"]["lds"] == 60 * 1024


# ── the C ABI ─────────────────────────────────────────────────────────────────────────────────────────────────────
def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pi_mi355.h").read_text(), flags=re.S)
    lib = _native.lib()
    for name in ("pi_infer_set_values", "pi_infer_resample"):
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared in pi_mi355.h"
        assert hasattr(lib, name) and name in _native.SIGNATURES
    assert lib.pi_abi_version() == _native.ABI_VERSION == 12
    assert "#define PI_MI355_ABI_VERSION 12" in (ROOT / "include" / "pi_mi355.h").read_text()
    assert callable(_native.InferenceEngine.set_values) and callable(_native.InferenceEngine.resample)
    assert callable(B.DevicePolicy.set_values) and callable(B.DevicePolicy.resample)
    from dynamicprogramming_amd.solver import _CudaPolicyIterationBase
    assert callable(_CudaPolicyIterationBase.continue_from)


def test_refusals_of_set_values_and_resample(tmp_path):
    """Every refusal is an error with its reason, before anything could be launched: these handles have no device."""
    eng = _host_handle(2, tmp_path)
    n = int(np.prod(SHAPES[2]))
    with pytest.raises(_native.NativeError, match=f"length {n + 1} != grid size {n}"):
        eng.set_values(np.zeros(n + 1, np.float32))
    bins = [np.linspace(-2, 2, 37, dtype=np.float32), np.linspace(-0.5, 0.5, 41, dtype=np.float32)]
    good = dict(dst_shape=[37, 41], dst_strides=[41, 1], dst_bins=bins)
    with pytest.raises(_native.NativeError, match="both outputs are null"):
        eng.resample(**good)
    # strides that are no dense layout of the shape in any order of the dimensions
    for strides in ([41, 2], [42, 1], [37, 1], [0, 1], [41, -1], [1, 1]):
        with pytest.raises(_native.NativeError, match="not the element strides of a dense array"):
            eng.resample(**{**good, "dst_strides": strides}, d_values=4096)
    with pytest.raises(_native.NativeError, match="at least 2 bins"):
        eng.resample([1, 41], [41, 1], [bins[0][:1], bins[1]], d_values=4096)
    # values without set_values, a policy without set_policy
    with pytest.raises(_native.NativeError, match="pi_infer_set_values was never called"):
        eng.resample(**good, d_values=4096)
    with pytest.raises(_native.NativeError, match="pi_infer_set_policy was never called"):
        eng.resample(**good, d_policy=4096, n_actions=3)
    eng.set_values(np.zeros(n, np.float32))
    with pytest.raises(_native.NativeError, match="pi_infer_set_policy was never called"):
        eng.resample(**good, d_values=4096, d_policy=8192, n_actions=3)
    # tables beyond the 60 KiB pi_create admits: 15 361 floats
    wide = [np.linspace(-1, 1, 15359, dtype=np.float32), np.float32([0, 1])]
    with pytest.raises(_native.NativeError, match="exceed the 60 KiB LDS budget"):
        eng.resample([15359, 2], [2, 1], wide, d_values=4096)
    # a map entry that is no index into the destination's actions (the binding looks first; the library's own check needs
    # a policy on the device: tests/test_gpu_continuation.py)
    for bad in ([0, 3, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="indices into the destination's 3 actions"):
            eng.resample(**good, d_policy=8192, action_map=bad, n_actions=3)
    # the column-major layout and everything else in order: only the missing device is left to refuse
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.resample(**{**good, "dst_strides": [1, 37]}, d_values=4096)
    wide[0] = wide[0][:15358]                                                       # 15 360 floats: admitted
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.resample([15358, 2], [2, 1], wide, d_values=4096)
    eng.close()


def test_continue_from_is_refused_where_it_cannot_work():
    """Without device arrays (after run(), or on a load()ed instance) and on a sharded solver; another D is a ValueError."""
    from dynamicprogramming_amd import envs

    class Arrays:
        device = "cpu"
    done = object.__new__(envs.PendulumCuda)
    with pytest.raises(RuntimeError, match="before run"):
        done.continue_from("nowhere.npz")
    sharded = object.__new__(envs.PendulumCuda)
    sharded.d_value_function, sharded._comm = Arrays(), object()
    with pytest.raises(NotImplementedError, match="multi-GPU path is frozen"):
        sharded.continue_from("nowhere.npz")
    fresh = object.__new__(envs.PendulumCuda)
    fresh.d_value_function, fresh._comm = Arrays(), None
    other = object.__new__(envs.ENVS["cartpole"])
    other.value_function, other.policy = np.zeros(16, np.float32), np.zeros(16, np.int32)
    other.grid_shape = np.int32([2, 2, 2, 2])
    with pytest.raises(ValueError, match="4 dimensions, this solver 2"):
        fresh.continue_from(other)
    untrained = object.__new__(envs.PendulumCuda)
    with pytest.raises(RuntimeError, match="run\\(\\) or load\\(\\)"):
        fresh.continue_from(untrained)


# ── the runner flag ───────────────────────────────────────────────────────────────────────────────────────────────
def test_coarse_bins_flag_parses_and_defaults_to_none():
    import inspect
    from runners import _cli
    p = _cli.build_parser("pendulum", "results/pendulum_cuda_policy.npz")
    assert p.parse_args([]).coarse_bins == []
    assert p.parse_args(["--bins", "50", "--coarse-bins", "25"]).coarse_bins == [25]
    a = p.parse_args(["--coarse-bins", "20", "40", "--bins", "80", "--retrain"])
    assert a.coarse_bins == [20, 40] and a.bins == 80 and a.retrain
    assert _cli.ignored_flags(a) == []
    assert inspect.signature(_cli.train).parameters["coarse_bins"].default == ()
