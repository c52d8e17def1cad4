"""
Rollouts that switch between two policies, the part that needs no GPU: the numpy twin (utils.barycentric.hybrid_rollout)
follows the reference's switch rule step for step (tests/golden/hybrid_switch.npz) and degenerates to the single-policy
twin, the hybrid kernel compiles for gfx950 behind every D without scratch, the new entry points are exported, bound
and refuse what they must, the runner takes the reference's flags.  The device half is tests/test_gpu_hybrid_rollout.py.
"""
from __future__ import annotations

import re
from itertools import product
from pathlib import Path

import numpy as np
import pytest

from dynamicprogramming_amd import _native, envs
from tests import helpers as H
from tests import hybrid_cases as C
from utils import barycentric as B

ROOT = Path(__file__).resolve().parents[1]
INF = np.inf
# the reference's rule as the box of the definition (include/pi_mi355.h): (x, x', th1, w1, th2, w2)
REF_ENTER = np.array([INF, INF, 0.32, 4.0, 0.32, 4.0], np.float32)
REF_LEAVE = np.array([INF, INF, 0.38, 5.0, 0.38, 5.0], np.float32)


# ── the switch rule ───────────────────────────────────────────────────────────────────────────────────────────────
def test_switch_rule_follows_the_reference_on_every_step_of_the_fixture():
    """states in, modes out of the reference's own _use_balance (tests/golden/make_hybrid_switch_golden.py): the twin's
    rule, in float32 with the thresholds of the definition, gives the same mode on every step of every sequence.
    Nothing is left out: the generator emits no state within 1e-5 of a threshold."""
    g = H.golden("hybrid_switch")
    states, modes, thr = g["states"], g["modes"], g["thresholds"]
    assert states.dtype == np.float32 and states.shape[2] == 6 and modes.shape == states.shape[:2] and len(states) >= 4
    assert states.shape[1] >= 2000
    assert thr.tolist() == [0.32, 4.0, 0.38, 5.0]
    assert np.array_equal(REF_ENTER[2:], np.float32([thr[0], thr[1]] * 2)) and np.array_equal(REF_LEAVE[2:], np.float32([thr[2], thr[3]] * 2))
    mag = np.abs(states[:, :, 2:].astype(np.float64))
    for j in range(4):
        for level in (thr[j % 2], thr[2 + j % 2]):
            assert (np.abs(mag[:, :, j] - level) > 1e-5).all()
            above = mag[:, :, j] > level
            assert (~above[:, :-1] & above[:, 1:]).any() and (above[:, :-1] & ~above[:, 1:]).any()   # crossed both ways
    mode = np.zeros(len(states), bool)
    for t in range(states.shape[1]):
        mode = B.switch_mode(mode, states[:, t], REF_ENTER, REF_LEAVE)
        assert np.array_equal(mode, modes[:, t]), f"step {t}"
    prev = np.concatenate([np.zeros((len(modes), 1), bool), modes[:, :-1]], axis=1)
    assert (~prev & modes).sum() > 50 and (prev & ~modes).sum() > 50


def test_switch_rule_edges():
    s = np.array([[0.5, -0.5], [1.0, 0.0], [np.nan, 0.0], [-2.0, 0.0], [3.0, 3.0]], np.float32)
    enter, leave = np.float32([1.0, INF]), np.float32([2.0, INF])
    assert B.switch_mode(np.zeros(5, bool), s, enter, leave).tolist() == [True, False, False, False, False]   # strict <
    assert B.switch_mode(np.ones(5, bool), s, enter, leave).tolist() == [True, True, True, True, False]       # strict >
    # mode 1 that leaves does not re-enter on the same step; inf takes no part either way
    assert B.switch_mode(np.ones(1, bool), np.float32([[0.1, 9.0]]), np.float32([1.0, 10.0]), np.float32([2.0, 5.0])).tolist() == [False]


# ── the numpy twin ────────────────────────────────────────────────────────────────────────────────────────────────
def _same(got, want, what):
    H.assert_bits_equal(got.states, want.states, f"{what}: states")
    H.assert_bits_equal(got.returns, want.returns, f"{what}: returns")
    assert np.array_equal(got.lengths, want.lengths) and np.array_equal(got.terminated, want.terminated), what
    H.assert_bits_equal(got.trajectory, want.trajectory, f"{what}: trajectory")


@pytest.mark.parametrize("D", [2, 4, 6])
def test_twin_degenerates_to_the_single_policy_twin(D):
    c = C.build(D)
    step = H.oracle_for(c["env"]).step
    starts = c["starts"][:200]
    zero, inf = np.zeros(D, np.float32), np.full(D, INF, np.float32)
    never = B.hybrid_rollout(step, starts, 60, c["primary"], c["secondary"], zero, c["leave"], gamma=0.99, record_every=7)
    assert isinstance(never, B.HybridRolloutResult)
    assert never._fields == B.RolloutResult._fields + ("secondary_steps", "last_mode")
    _same(never, B.rollout(step, starts, 60, *c["primary"], gamma=0.99, record_every=7), "enter = 0")
    assert never.secondary_steps.dtype == np.int32 and not never.secondary_steps.any()
    assert never.last_mode.dtype == np.uint8 and not never.last_mode.any()
    always = B.hybrid_rollout(step, starts, 60, c["primary"], c["secondary"], inf, inf, gamma=0.99, record_every=7)
    _same(always, B.rollout(step, starts, 60, *c["secondary"], gamma=0.99, record_every=7), "enter = leave = inf")
    finite = np.isfinite(starts).all(axis=1)
    assert np.array_equal(always.secondary_steps[finite], always.lengths[finite]) and always.last_mode[finite].all()
    # zero steps: nothing ran
    none = B.hybrid_rollout(step, starts, 0, c["primary"], c["secondary"], inf, inf)
    assert np.array_equal(none.states, starts) and not none.lengths.any() and not none.secondary_steps.any()
    assert not none.last_mode.any() and none.trajectory is None
    with pytest.raises(ValueError):
        B.hybrid_rollout(step, starts, 5, c["primary"], c["secondary"], inf, inf, record_every=6)


def test_twin_counts_secondary_steps_and_last_mode_on_a_hand_written_case():
    """x moves by the action per step: +1 on the primary table, -1 on the secondary; enter |x| < 1.5 ... wait for it to
    leave at |x| > 2.5.  From x = 0: mode 1 at once, x = -1, -2, -3 (left on the 4th step: mode 0), then +1 again."""
    bits = np.array(list(product([0, 1], repeat=2)), dtype=np.int32)
    grid = (np.float32([-8.0, 0.0]), np.float32([8.0, 1.0]), np.array([17, 2], np.int32), np.array([2, 1], np.int32), bits)
    up = (np.zeros(34, np.int32), np.float32([1.0])) + grid
    down = (np.zeros(34, np.int32), np.float32([-1.0])) + grid

    def step(states, acts):
        nxt = states.copy()
        nxt[:, 0] = states[:, 0] + np.round(acts)
        return nxt, np.ones(len(states), np.float32), nxt[:, 0] >= 6.0
    starts = np.float32([[0.0, 0.5], [4.0, 0.5], [-3.0, 0.0]])
    res = B.hybrid_rollout(step, starts, 6, up, down, np.float32([1.5, INF]), np.float32([2.5, INF]), record_every=1)
    # episode 0: x = 0 (m1) -1 (m1) -2 (m1) -3 (m0) -2 (m0) -1 (m1) -> -2
    assert res.trajectory[:, 0, 0].tolist() == [0.0, -1.0, -2.0, -3.0, -2.0, -1.0, -2.0]
    # episode 1: never inside, done at x = 6 after 2 steps; episode 2: -3 -2 (m0) -1 (m1) -2 (m1) -3 (m0) -2 (m0) -> -1
    assert res.lengths.tolist() == [6, 2, 6] and res.terminated.tolist() == [False, True, False]
    assert res.trajectory[:, 2, 0].tolist() == [-3.0, -2.0, -1.0, -2.0, -3.0, -2.0, -1.0]
    assert res.secondary_steps.tolist() == [4, 0, 2] and res.last_mode.tolist() == [1, 0, 0]
    assert res.returns.tolist() == [6.0, 2.0, 6.0]


# ── the kernel, compiled without a GPU ────────────────────────────────────────────────────────────────────────────
def _host_pair(D, cache_dir):
    c = C.build(D)
    a = _native.InferenceEngine(*c["primary"][2:], device=-1, cache_dir=cache_dir)
    b = _native.InferenceEngine(*c["secondary"][2:], device=-1, cache_dir=cache_dir)
    return c, a, b


@pytest.mark.parametrize("D", [2, 4, 6])
def test_hybrid_kernel_compiles_for_gfx950_without_a_gpu(D, tmp_path):
    """pi_infer_set_partner on host-only handles: primary grid + secondary grid + pi_math.h + the plugin + the rollout
    helpers + csrc/pi_hybrid_kernels.hip build through hipRTC into a third code object that holds
    pi_hybrid_rollout_kernel (and not the single-policy kernel)."""
    c, a, b = _host_pair(D, tmp_path)
    with pytest.raises(_native.NativeError, match="pi_infer_set_dynamics was never called"):
        a.set_partner(b)
    a.set_dynamics(envs.dynamics_source(c["env"]))
    before = set(tmp_path.glob("pi_*.hsaco"))
    log = a.set_partner(b)
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"pi_hybrid_rollout_kernel" in blob and b"pi_rollout_kernel" not in blob
    a.set_partner(b)                                                      # again: served from the cache
    assert set(tmp_path.glob("pi_*.hsaco")) - before == {obj}
    with pytest.raises(_native.NativeError, match="host-only"):
        a.rollout_hybrid(b, 4096, 4, 10, c["enter"], c["leave"])
    a.close()
    b.close()


def test_hybrid_kernel_does_not_spill(tmp_path):
    """Selecting a lane's grid costs registers next to the 2^D weights and indices: on the full-size grids (the 6-D pair
    is the hybrid runner's) the kernel must stay without scratch, like pi_rollout_kernel
    (tests/test_rollout_host.py::test_rollout_kernel_does_not_spill).  Checked on the ahead-of-time build of the
    translation unit pi_infer_set_partner hands to hipRTC, restated by tests/helpers.inference_unit from the kernel file's
    description of it."""
    for name, bins, name2, bins2 in (("pendulum", 200, "pendulum", 50), ("cartpole_swingup", 50, "cartpole_swingup", 30),
                                     ("double_cartpole_swingup", 25, "double_cartpole", 25)):
        text = H.inference_unit(H.inference_grid(name, bins), name, "#define PI_HYBRID 1\n",
                                ["pi_rollout_kernels.hip", "pi_hybrid_kernels.hip"], second_grid=H.inference_grid(name2, bins2))
        usage = H.kernel_resource_usage(text, tmp_path, name)
        assert set(usage) == {"pi_hybrid_rollout_kernel"}
        k = usage["pi_hybrid_rollout_kernel"]
        print(f"pi_hybrid_rollout_kernel {name} {bins}^D + {name2} {bins2}^D: {k}")
        assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, k)


# ── the ABI ───────────────────────────────────────────────────────────────────────────────────────────────────────
def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pi_mi355.h").read_text(), flags=re.S)
    lib = _native.lib()
    for name in ("pi_infer_set_partner", "pi_infer_rollout_hybrid"):
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in pi_mi355.h"
        assert hasattr(lib, name) and name in _native.SIGNATURES
    assert len(_native.SIGNATURES["pi_infer_rollout_hybrid"][1]) == 17 and len(_native.SIGNATURES["pi_infer_set_partner"][1]) == 4
    assert "#define PI_MI355_ABI_VERSION 12" in text and lib.pi_abi_version() == 12 == _native.ABI_VERSION
    assert hasattr(_native.InferenceEngine, "set_partner") and hasattr(_native.InferenceEngine, "rollout_hybrid")
    assert hasattr(B, "HybridPolicy") and hasattr(B, "HybridRolloutResult") and hasattr(B, "hybrid_rollout")


def test_argument_errors_that_need_no_gpu(tmp_path):
    c, a, b = _host_pair(4, tmp_path)
    c2, a2, _b2 = _host_pair(2, tmp_path)
    _b2.close()
    a.set_dynamics(envs.dynamics_source(c["env"]))
    with pytest.raises(_native.NativeError, match="differ in D"):
        a.set_partner(a2)
    lo, hi, gshape, strides, bits = c["secondary"][2:]
    flipped = _native.InferenceEngine(lo, hi, gshape, strides, bits[::-1].copy(), device=-1, cache_dir=tmp_path)
    with pytest.raises(_native.NativeError, match="corner_bits"):
        a.set_partner(flipped)
    L = _native.lib()
    assert L.pi_infer_set_partner(a._h, None, None, 0) != 0 and "null handle" in _native.last_error()
    assert L.pi_infer_set_partner(None, b._h, None, 0) != 0 and "null handle" in _native.last_error()
    assert L.pi_infer_rollout_hybrid(None, b._h, None, 1, 1, 1.0, None, None, None, None, None, None, None, None, None, 0,
                                     None) != 0 and "null handle" in _native.last_error()
    with pytest.raises(_native.NativeError, match="null handle"):
        a.rollout_hybrid(None, 4096, 4, 10, c["enter"], c["leave"])
    a.set_partner(b)
    with pytest.raises(_native.NativeError, match="host-only"):
        a.rollout_hybrid(b, 4096, 4, 10, c["enter"], c["leave"])
    with pytest.raises(ValueError, match="4 thresholds"):
        a.rollout_hybrid(b, 4096, 4, 10, c["enter"][:3], c["leave"])
    # a broken plugin never reaches the hybrid module: set_dynamics refuses it and keeps the previous one
    with pytest.raises(_native.NativeError, match="compilation failed"):
        a.set_dynamics("__device__ void step_dynamics(float a) { not valid C; }")
    a.set_partner(b)
    for e in (a, b, a2, flipped):
        e.close()


# ── the runner ────────────────────────────────────────────────────────────────────────────────────────────────────
def test_runner_accepts_the_reference_flag_set_and_names_what_it_ignores(tmp_path, capsys):
    from runners import hybrid_double_cartpole as R
    p = R.build_parser()
    d = p.parse_args([])
    assert (d.episodes, d.steps, d.seed, d.render, d.record, d.random, d.bins, d.no_plot, d.retrain, d.save_path) == \
        (5, 1000, 42, False, None, None, None, False, False, None)
    assert d.swingup_path == Path("results/double_cartpole_swingup_cuda_policy.npz")
    assert d.balance_path == Path("results/double_cartpole_cuda_policy.npz")
    assert R.ignored_flags(d) == []
    a = p.parse_args(["--render", "--record", "out.gif", "--episodes", "3", "--steps", "10", "--seed", "7", "--random",
                      "--bins", "6", "--no-plot", "--retrain", "--save-path", "x.npz"])
    assert (a.episodes, a.steps, a.seed, a.random, a.bins) == (3, 10, 7, 5, 6)
    assert R.ignored_flags(a) == ["--render", "--record", "--random", "--bins", "--no-plot", "--retrain", "--save-path"]
    assert p.parse_args(["--random", "9"]).random == 9
    assert np.array_equal(np.float32(R.ENTER), REF_ENTER) and np.array_equal(np.float32(R.LEAVE), REF_LEAVE)
    # the reference's starts: [0, 0, pi, 0, pi, 0], x and x' moved by U(-0.05, 0.05) in episode order
    s = R.start_states(7, 3)
    rng = np.random.default_rng(7)
    want = np.tile(np.float32([0, 0, np.pi, 0, np.pi, 0]), (3, 1))
    for ep in range(3):
        want[ep, :2] += rng.uniform(-0.05, 0.05, size=2).astype(np.float32)
    assert s.dtype == np.float32 and np.array_equal(s, want)
    # missing archives: a clear message that names the training commands
    with pytest.raises(SystemExit) as exc:
        R.main(["--swingup-path", str(tmp_path / "a.npz"), "--balance-path", str(tmp_path / "b.npz"), "--no-plot"])
    msg = str(exc.value)
    assert "a.npz" in msg and "b.npz" in msg and "runners/double_cartpole_swingup_cuda.py" in msg
    assert "runners/double_cartpole_cuda.py" in msg
    assert "--no-plot" in capsys.readouterr().out
