"""
Value-greedy control, the part that needs no GPU: the numpy twin (utils.barycentric.greedy_action / greedy_rollout)
agrees bit for bit with the CPU checker's backup at arbitrary points, its fmaf emulation is exact, the greedy kernels
compile for gfx950 behind every D without spilling, the C ABI declares, exports and binds the three entry points and
refuses what it must, the runners parse --controller.  The device half is tests/test_gpu_greedy.py.
"""
from __future__ import annotations

import ctypes
import re
from itertools import product
from pathlib import Path

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from tests import helpers as H
from utils import barycentric as B

ROOT = Path(__file__).resolve().parents[1]
GAMMA = 0.99
# the grids of the twin-against-checker comparison: odd, unequal shapes in every D, and the 9 actions of the 6-D swing-up
TWIN_GRIDS = [("pendulum", (31, 29)), ("mountain_car", (30, 27)), ("cartpole", (7, 6, 9, 8)),
              ("double_cartpole", (4, 5, 4, 5, 4, 5)), ("double_cartpole_swingup", (4,) * 6)]


def _grid(name, shape):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    return bins, (lo, hi, gshape, strides)


def _host_engine(name, shape, cache_dir):
    bins, (lo, hi, gshape, strides) = _grid(name, shape)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return _native.InferenceEngine(lo, hi, gshape, strides, bits, device=-1, cache_dir=cache_dir)


# ── the numpy twin against the checker ────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name,shape", TWIN_GRIDS, ids=[n for n, _ in TWIN_GRIDS])
def test_twin_equals_the_checkers_backup_at_arbitrary_points(name, shape):
    """greedy_action against oracle.improve_points (index, best Q) and, action by action, oracle.eval_points (the whole
    Q matrix): 20 000 points inside, beyond and on the borders of the grid, V ~ 30 N(0, 1)."""
    bins, grid = _grid(name, shape)
    rng = np.random.default_rng(len(name))
    V = (30.0 * rng.standard_normal(int(np.prod(shape)))).astype(np.float32)
    pts = H.sample_states(rng, bins, 20000)
    acts = H.edge_actions(name)
    chk = H.oracle_for(name)
    before = (pts.copy(), V.copy())
    best, act, q_best, Q = B.greedy_action(chk.step, pts, V, acts, *grid, GAMMA, q_values=True)
    assert best.dtype == np.int32 and act.dtype == q_best.dtype == Q.dtype == np.float32 and Q.shape == (len(pts), len(acts))
    want_best, want_q = chk.improve_points(pts, acts, V, *grid, GAMMA)
    assert np.array_equal(best, want_best), f"{int((best != want_best).sum())} greedy indices differ"
    H.assert_bits_equal(q_best, want_q, f"{name}: best Q")
    H.assert_bits_equal(act, acts[want_best], f"{name}: action value")
    for a, u in enumerate(acts):
        H.assert_bits_equal(Q[:, a], chk.eval_points(pts, np.full(len(pts), u, np.float32), V, *grid, GAMMA), f"{name}: Q[:, {a}]")
    H.assert_bits_equal(Q[np.arange(len(pts)), best], q_best, f"{name}: Q at the greedy index")
    short = B.greedy_action(chk.step, pts, V, acts, *grid, GAMMA)
    assert len(short) == 3 and np.array_equal(short[0], best)
    assert np.array_equal(pts, before[0]) and np.array_equal(V, before[1])            # inputs are not written


def _stub():
    """A 3 x 2 grid over [0, 2] x [0, 1] with V = 0 .. 5 in row-major order and a stub env: x moves by the action, the
    reward is -|a| (NaN for a NaN state), done once x' >= 2.5."""
    grid = (np.array([0.0, 0.0], np.float32), np.array([2.0, 1.0], np.float32), np.array([3, 2], np.int32),
            np.array([2, 1], np.int32))
    V = np.arange(6, dtype=np.float32)
    actions = np.array([-1.0, 0.0, 1.0], np.float32)

    def step(states, acts):
        nxt = states.copy()
        nxt[:, 0] = states[:, 0] + acts
        return nxt, states[:, 0] * np.float32(0.0) - np.abs(acts), nxt[:, 0] >= 2.5
    return step, V, actions, grid


def test_twin_on_a_hand_computed_case():
    """gamma = 0.5, every number exact in float32.
    (0.5, 0.25): a = -1 lands at x = -0.5, clamped onto the border cell: E = 0.75 * V[0] + 0.25 * V[1] = 0.25,
    Q = -1 + 0.125; a = 0: cell 0, fractions (0.5, 0.25), E = 0.125 * 1 + 0.375 * 2 + 0.125 * 3 = 1.25, Q = 0.625;
    a = +1: cell 1, E = 0.375 * 2 + 0.125 * 3 + 0.375 * 4 + 0.125 * 5 = 3.25, Q = -1 + 1.625 = 0.625: a tie, the lower index wins.
    (2, 1), the far corner: a = -1 reads V[3] = 3: Q = 0.5; a = 0 reads V[5] = 5: Q = 2.5; a = +1 is done: Q = -1.
    A NaN state: every Q is NaN, nothing wins: index 0 with Q = -1e30."""
    step, V, actions, grid = _stub()
    pts = np.array([[0.5, 0.25], [2.0, 1.0], [np.nan, 0.5]], np.float32)
    best, act, q_best, Q = B.greedy_action(step, pts, V, actions, *grid, 0.5, q_values=True)
    assert Q[0].tolist() == [-0.875, 0.625, 0.625] and Q[1].tolist() == [0.5, 2.5, -1.0] and np.isnan(Q[2]).all()
    assert best.tolist() == [1, 1, 0] and act.tolist() == [0.0, 0.0, -1.0]
    assert q_best.tolist() == [0.625, 2.5, float(np.float32(-1.0e30))]
    # in 2-D dimension 1 toggles fastest: with V that tells the corners apart the weights must sit on the right ones
    step0 = lambda s, a: (s.copy(), np.zeros(len(s), np.float32), np.zeros(len(s), bool))      # noqa: E731
    _, _, q, _ = B.greedy_action(step0, np.array([[0.25, 0.75]], np.float32), V, actions[:1], *grid, 1.0, q_values=True)
    assert q.tolist() == [0.75 * 0.25 * 0 + 0.75 * 0.75 * 1 + 0.25 * 0.25 * 2 + 0.25 * 0.75 * 3]
    # the closed loop on it: always a = 0 from (0.5, 0.25) (ties to the lower index), so the state stays
    res = B.greedy_rollout(step, pts[:2], 3, V, actions, *grid, 0.5, gamma=1.0, record_every=1)
    assert isinstance(res, B.RolloutResult) and res.trajectory.shape == (4, 2, 2)
    assert res.states.tolist() == [[0.5, 0.25], [2.0, 1.0]] and res.lengths.tolist() == [3, 3]
    assert res.returns.tolist() == [0.0, 0.0] and not res.terminated.any()
    with pytest.raises(ValueError):
        B.greedy_rollout(step, pts[:2], 3, V, actions, *grid, 0.5, record_every=4)


def test_fmaf_emulation_rounds_once():
    """Triples whose float64 sum a * b + c lands exactly on the midpoint of two float32 values and only the bits the
    float64 sum has already dropped say which side the true value lies on — a float64 sum rounded to nearest and then
    to float32 goes the wrong way on them.  Worked out by hand: with x = 1 + 2^-23, y = 1 - 2^-23, x * y = 1 - 2^-46, so
    2^-4 x * y = 2^-4 - 2^-50, and 2^-50 is below the float64 resolution 2^-32 at 2^20.  c = 2^20 + 2^-3 has an odd last
    float32 bit (the spacing there is 2^-3); the midpoints around it are c -+ 2^-4."""
    x, y = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23)
    c = np.float32(2.0 ** 20 + 2.0 ** -3)
    lo_, hi_ = np.float32(2.0 ** 20), np.float32(2.0 ** 20 + 2.0 ** -2)
    h = np.float32(2.0 ** -4)
    cases = [
        (h * x, y, c, c),              # c + 2^-4 - 2^-50: just below the upper midpoint (ties-to-even would go up to hi_)
        (-(h * x), y, c, c),           # c - 2^-4 + 2^-50: just above the lower midpoint (ties-to-even would go down to lo_)
        (h, np.float32(1.0), c, hi_),  # exactly the upper midpoint: the tie goes to the even neighbour
        (-h, np.float32(1.0), c, lo_),             # exactly the lower midpoint: likewise
        (-(h * x), y, -c, -c), (h * x, y, -c, -c),                 # mirrored
        (h * x, y, lo_, lo_),          # 2^20 + 2^-4 - 2^-50: below the midpoint above an EVEN value (both roundings agree)
        (np.float32(3.0), np.float32(5.0), np.float32(7.0), np.float32(22.0)),
        (np.float32(0.0), np.float32(5.0), np.float32(-0.0), np.float32(0.0)),
    ]
    assert float(h * x) == 2.0 ** -4 * (1 + 2.0 ** -23)          # the operands are float32 values
    a, b, cc, want = (np.array(v, np.float32) for v in zip(*cases))
    H.assert_bits_equal(B._fmaf(a, b, cc), want, "fmaf emulation")
    naive = (a.astype(np.float64) * b.astype(np.float64) + cc.astype(np.float64)).astype(np.float32)
    assert naive[0] == hi_ and naive[1] == lo_, "the first two triples are the ones a double rounding gets wrong"
    # scalars and infinities pass through
    assert B._fmaf(np.float32(2.0), np.float32(3.0), np.float32(1.0)) == np.float32(7.0)
    assert np.isinf(B._fmaf(np.float32(3e38), np.float32(10.0), np.float32(0.0)))
    # and the processor's own fmaf agrees on random operands of mixed magnitude
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(7)
    t = (rng.standard_normal((3, 4000)) * np.exp2(rng.integers(-30, 30, (3, 4000)))).astype(np.float32)
    t[2, ::2] = -(t[0, ::2] * t[1, ::2])                         # heavy cancellation
    want = np.array([libm.fmaf(*(float(v) for v in t[:, k])) for k in range(t.shape[1])], np.float32)
    H.assert_bits_equal(B._fmaf(t[0], t[1], t[2]), want, "fmaf emulation against libm")


@pytest.mark.parametrize("name,bins", [("pendulum", 50), ("mountain_car", 60)])
def test_greedy_action_at_the_nodes_of_a_converged_run_is_its_policy(name, bins):
    """The lookahead is the improvement backup: at every non-terminal node of a converged checker run it returns
    policy[node]."""
    tabs, grid = _grid(name, (bins, bins))
    states = oracle.states_from_bins(tabs)
    term, term_value = H.terminal_mask(name, states)
    acts = H.edge_actions(name)
    chk = H.oracle_for(name)
    cfg = envs.CudaPIConfig(gamma=GAMMA, theta=1e-4)
    ref = chk.run(states, acts, term, *grid, gamma=cfg.gamma, theta=cfg.theta, max_eval_iter=cfg.max_eval_iter,
                  max_pi_iter=cfg.max_pi_iter, terminal_value=term_value)
    assert ref["stable"]
    live = ~term
    best, _, _ = B.greedy_action(chk.step, states[live], ref["value_function"], acts, *grid, cfg.gamma)
    assert live.sum() > 0.9 * len(states) and np.array_equal(best, ref["policy"][live])


# ── the module ────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name,shape", [("pendulum", (24, 17)), ("cartpole_swingup", (9, 7, 11, 5)),
                                        ("double_cartpole_swingup", (5, 4, 6, 4, 5, 4))])
def test_greedy_kernels_compile_for_gfx950_without_a_gpu(name, shape, tmp_path):
    """pi_infer_set_greedy on a host-only handle: grid + pi_math.h + plugin + rollout helpers + csrc/pi_greedy_kernels.hip
    build through hipRTC into one more code object in the handle's cache, holding both kernels."""
    eng = _host_engine(name, shape, tmp_path)
    eng.set_values(np.zeros(int(np.prod(shape)), np.float32))
    eng.set_dynamics(envs.dynamics_source(name))
    before = set(tmp_path.glob("pi_*.hsaco"))
    assert len(before) == 3
    log = eng.set_greedy(H.edge_actions(name))
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"pi_greedy_kernel" in blob and b"pi_greedy_rollout_kernel" in blob
    assert b"pi_rollout_kernel" not in blob.replace(b"pi_greedy_rollout_kernel", b"")      # the helpers only
    eng.set_greedy(H.edge_actions(name)[:1])                           # again: served from the cache, replaces
    assert len(list(tmp_path.glob("pi_*.hsaco"))) == 4
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.greedy(4096, 4, GAMMA, d_best=4096)
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.rollout_greedy(4096, 4, 10, GAMMA)
    eng.close()


def test_greedy_kernels_do_not_spill(tmp_path):
    """Per action the 6-D lookahead holds 64 values and the weights and offsets of 64 corners next to the plugin's own
    registers: both kernels must fit the 512 registers a lane of a 256-thread workgroup may use, without scratch, in
    every D.  Checked on the ahead-of-time build of the translation unit pi_infer_set_greedy hands to hipRTC
    (tests/helpers.inference_unit restates it from the header's description), the method of
    test_resample_kernel_does_not_spill."""
    for name, bins in (("pendulum", 200), ("cartpole_swingup", 50), ("double_cartpole", 25), ("double_cartpole_swingup", 25)):
        D = envs.ENVS[name]._D
        text = H.inference_unit(H.inference_grid(name, bins), name, "#define PI_GREEDY 1\n",
                                ["pi_rollout_kernels.hip", "pi_greedy_kernels.hip"])
        usage = H.kernel_resource_usage(text, tmp_path, name)
        assert set(usage) == {"pi_greedy_kernel", "pi_greedy_rollout_kernel"}
        for fn, k in usage.items():
            print(f"{fn} {name} {bins}^{D}: {k}")
            assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, fn, k)


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    lib = _native.lib()
    for sym in ("pi_infer_set_greedy", "pi_infer_greedy", "pi_infer_rollout_greedy"):
        assert re.search(rf"^int {sym}\(pi_infer\* h,", header, re.M), sym
        assert header.count(sym) >= 2, f"{sym} has no comment in the header"
        assert hasattr(lib, sym) and sym in _native.SIGNATURES
    for method in ("set_greedy", "greedy", "rollout_greedy"):
        assert callable(getattr(_native.InferenceEngine, method))
    for method in ("set_greedy", "greedy"):
        assert callable(getattr(B.DevicePolicy, method))
    assert lib.pi_abi_version() == _native.ABI_VERSION
    makefile = (ROOT / "dynamicprogramming_amd" / "csrc" / "Makefile").read_text()
    assert "pi_greedy.cpp" in makefile and "pi_greedy.cpp" in (ROOT / "dynamicprogramming_amd" / "csrc" / "pi_internal.h").read_text()
    # the profiles stay tied to the sweep kernels: the new device file is not part of their fingerprint
    import hashlib
    sweeps = ROOT / "dynamicprogramming_amd" / "csrc" / "pi_sweep_kernels.hip"
    want = hashlib.sha256(sweeps.read_bytes() + (ROOT / "include" / "pi_math.h").read_bytes()).hexdigest()[:16]
    assert _native.kernel_source_hash() == want


def test_refusals_are_error_codes(tmp_path):
    name, shape = "pendulum", (12, 9)
    acts = H.edge_actions(name)
    dyn = envs.dynamics_source(name)
    V = np.zeros(int(np.prod(shape)), np.float32)
    eng = _host_engine(name, shape, tmp_path)
    with pytest.raises(_native.NativeError, match="no greedy module"):
        eng.greedy(4096, 4, GAMMA, d_best=4096)
    with pytest.raises(_native.NativeError, match="pi_infer_set_values was never called"):
        eng.set_greedy(acts)
    eng.set_values(V)
    with pytest.raises(_native.NativeError, match="pi_infer_set_dynamics was never called"):
        eng.set_greedy(acts)
    eng.close()
    eng = _host_engine(name, shape, tmp_path)
    eng.set_dynamics(dyn)
    with pytest.raises(_native.NativeError, match="pi_infer_set_values was never called"):
        eng.set_greedy(acts)
    eng.set_values(V)
    with pytest.raises(_native.NativeError, match="at least one action"):
        eng.set_greedy(np.zeros(0, np.float32))
    with pytest.raises(_native.NativeError, match="action_space"):
        eng.set_greedy(None)
    with pytest.raises(_native.NativeError, match="no greedy module"):
        eng.rollout_greedy(4096, 4, 10, GAMMA)
    eng.set_greedy(acts)
    with pytest.raises(_native.NativeError, match="all four outputs are null"):
        eng.greedy(4096, 4, GAMMA)
    with pytest.raises(_native.NativeError, match="gamma is NaN"):
        eng.greedy(4096, 4, float("nan"), d_best=4096)
    with pytest.raises(_native.NativeError, match="m < 0"):
        eng.greedy(4096, -1, GAMMA, d_best=4096)
    eng.greedy(0, 0, GAMMA)                                            # m = 0: a no-op that succeeds, buffers or not
    with pytest.raises(_native.NativeError, match="lookahead_gamma is NaN"):
        eng.rollout_greedy(4096, 4, 10, float("nan"))
    with pytest.raises(_native.NativeError, match="gamma is NaN"):
        eng.rollout_greedy(4096, 4, 10, GAMMA, gamma=float("nan"))
    eng.set_values(V + 1)                                              # new values: the module stays
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.greedy(4096, 4, GAMMA, d_best=4096)
    eng.set_dynamics(dyn)                                              # a new plugin drops it
    with pytest.raises(_native.NativeError, match="no greedy module.*pi_infer_set_greedy"):
        eng.greedy(4096, 4, GAMMA, d_best=4096)
    with pytest.raises(_native.NativeError, match="no greedy module"):
        eng.rollout_greedy(4096, 4, 10, GAMMA)
    eng.close()
    # a null handle
    assert _native.lib().pi_infer_greedy(None, None, 0, 0.5, None, None, None, None, None) == 1
    assert _native.lib().pi_infer_set_greedy(None, None, 0, None, 0) == 1


def test_front_end_refusals_need_no_gpu(tmp_path):
    """The controller argument is checked before anything touches a device."""
    dp = object.__new__(B.DevicePolicy)
    with pytest.raises(ValueError, match="lookahead_gamma"):
        dp.rollout(np.zeros((2, 2), np.float32), 5, controller="greedy")
    with pytest.raises(ValueError, match="controller"):
        dp.rollout(np.zeros((2, 2), np.float32), 5, controller="argmax")
    g = H.golden("reference_results")
    shape = tuple(int(x) for x in g["mountain_car_grid_shape"])
    bins, (lo, hi, gshape, strides) = _grid("mountain_car", shape)
    path = tmp_path / "mc.npz"
    np.savez(path, value_function=g["mountain_car_value_function"], policy=g["mountain_car_policy"], bounds_low=lo,
             bounds_high=hi, grid_shape=gshape, strides=strides,
             corner_bits=np.array(list(product([0, 1], repeat=2)), dtype=np.int32),
             action_space=g["mountain_car_action_space"], states_space=oracle.states_from_bins(bins))
    pi = envs.MountainCarCuda.load(path)
    with pytest.raises(ValueError, match="controller"):
        pi.rollout(envs.MountainCarCuda.start_states(np.random.default_rng(0), 4), 10, controller="argmax")


@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_controller_flag_parses_and_defaults_to_policy(name):
    from runners import _cli
    p = _cli.build_parser(name, f"results/{name}_cuda_policy.npz")
    assert p.parse_args([]).controller == "policy"
    assert p.parse_args(["--rollout", "--controller", "greedy"]).controller == "greedy"
    assert p.parse_args(["--rollout", "--controller", "policy"]).controller == "policy"
    with pytest.raises(SystemExit):
        p.parse_args(["--controller", "argmax"])
    assert _cli.ignored_flags(p.parse_args(["--rollout", "--controller", "greedy"])) == []
    assert _cli.ignored_flags(p.parse_args(["--controller", "greedy"])) == ["--controller"]
