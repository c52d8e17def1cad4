"""
Stochastic rollouts, the part that needs no GPU: the numpy twin of the random stream (utils.barycentric.philox4x32,
random_words, sym, explore_threshold, random_action_index) reproduces the published Philox4x32-10 answers, the twin of
the rollout (stochastic_rollout) reduces to the deterministic one, does not depend on how a batch is cut, explores and
picks actions at the right frequencies and applies clamp and noise in the documented order; the kernels compile for
gfx950 behind every D without scratch; the C ABI declares, exports and binds the three entry points and refuses what it
must; the runners parse the new flags.  The device half is tests/test_gpu_stochastic.py.
"""
from __future__ import annotations

import math
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


def _grid(name, shape):
    bins = H.env_bins(name, shape)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    bits = np.array(list(product([0, 1], repeat=len(bins))), dtype=np.int32)
    return bins, (lo, hi, gshape, strides, bits)


def _host_engine(name, shape, cache_dir):
    _, grid = _grid(name, shape)
    return _native.InferenceEngine(*grid, device=-1, cache_dir=cache_dir)


# ── the stream ────────────────────────────────────────────────────────────────────────────────────────────────────
def test_philox_known_answers_and_the_exact_conversions():
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in cases:
        got = B.philox4x32(counter, key)
        assert got.dtype == np.uint32 and got.tolist() == list(want), [hex(int(x)) for x in got]
    # vectorised: all three at once give the same rows
    got = B.philox4x32(np.array([c for c, _, _ in cases], np.uint32), np.array([k for _, k, _ in cases], np.uint32))
    assert got.tolist() == [list(w) for _, _, w in cases]
    # random_words is philox on (low e, high e, t, j; low seed, high seed), e carrying into its high word
    seed, first = 0x0123456789abcdef, 2 ** 32 - 2
    words = B.random_words(seed, first, 4, 7, 2)
    for row in range(4):
        e = first + row
        assert words[row].tolist() == B.philox4x32([e & 0xffffffff, e >> 32, 7, 2], [seed & 0xffffffff, seed >> 32]).tolist()
    assert B.random_words(seed, first, 0, 0, 0).shape == (0, 4)
    s = B.sym(np.array([0, 0xffffffff, 0x80000000, 0x800000ff], np.uint32))
    assert s.dtype == np.float32 and s.tolist() == [-1.0, 1.0 - 2.0 ** -23, 0.0, 0.0]
    for n in (1, 3, 257):
        assert B.random_action_index(np.array([0, 0xffffffff], np.uint32), n).tolist() == [0, n - 1]
    assert B.explore_threshold(0.0) == 0 and B.explore_threshold(1.0) == 1 << 24 and B.explore_threshold(0.25) == 1 << 22
    assert B.explore_threshold(0.3) == int(np.rint(float(np.float32(0.3)) * 2.0 ** 24))      # the float32 the library is handed
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            B.explore_threshold(bad)


def _case(name, shape, m, seed=0):
    bins, grid = _grid(name, shape)
    rng = np.random.default_rng(seed + len(name))
    acts = H.edge_actions(name)
    policy = rng.integers(0, len(acts), int(np.prod(shape))).astype(np.int32)
    starts = H.sample_states(rng, bins, m)
    return H.oracle_for(name), starts, policy, acts, grid


def _same(a, b, what):
    H.assert_bits_equal(a.states, b.states, f"{what}: final states")
    H.assert_bits_equal(a.returns, b.returns, f"{what}: returns")
    assert np.array_equal(a.lengths, b.lengths) and np.array_equal(a.terminated, b.terminated), what
    assert (a.trajectory is None) == (b.trajectory is None)
    if a.trajectory is not None:
        H.assert_bits_equal(a.trajectory, b.trajectory, f"{what}: trajectory")


@pytest.mark.parametrize("name,shape", [("pendulum", (31, 29)), ("cartpole_swingup", (7, 6, 9, 8))])
def test_twin_without_noise_is_the_deterministic_rollout(name, shape):
    chk, starts, policy, acts, grid = _case(name, shape, 200)
    for gamma, every in ((1.0, 0), (0.99, 7)):
        want = B.rollout(chk.step, starts, 40, policy, acts, *grid, gamma=gamma, record_every=every)
        got = B.stochastic_rollout(chk.step, starts, 40, policy, acts, *grid, 0.0, 0.0, None, seed=5, gamma=gamma,
                                   record_every=every)
        _same(got, want, f"{name} gamma={gamma}")
        zeros = B.stochastic_rollout(chk.step, starts, 40, policy, acts, *grid, 0.0, 0.0, np.zeros(len(shape)), seed=9,
                                     first_episode=77, gamma=gamma, record_every=every)
        _same(zeros, want, f"{name} gamma={gamma}, zero noise vector")


def test_twin_does_not_depend_on_how_the_batch_is_cut():
    name, shape = "cartpole", (7, 6, 9, 8)              # episodes end on different steps: the live set shrinks
    chk, starts, policy, acts, grid = _case(name, shape, 700)
    kw = dict(epsilon=0.3, action_noise=2.0, state_noise=[0.01, 0.0, 0.02, 0.05], seed=2 ** 40 + 3, gamma=0.99, record_every=5)
    run = lambda s, first: B.stochastic_rollout(chk.step, s, 30, policy, acts, *grid, first_episode=first, **kw)   # noqa: E731
    whole, a, b = run(starts, 0), run(starts[:300], 0), run(starts[300:], 300)
    assert 0 < whole.terminated.sum() < 700
    joined = B.RolloutResult(*(np.concatenate([x, y], axis=1 if x.ndim == 3 else 0) for x, y in zip(a, b)))
    _same(whole, joined, "700 episodes against 300 + 400")
    other = B.stochastic_rollout(chk.step, starts[300:], 30, policy, acts, *grid, first_episode=0, **kw)
    assert not np.array_equal(other.returns, b.returns), "first_episode must select the stream"
    again = run(starts, 0)
    _same(again, whole, "the same seed twice")
    assert not np.array_equal(B.stochastic_rollout(chk.step, starts, 30, policy, acts, *grid, **{**kw, "seed": 4}).returns,
                              whole.returns)


def _chi2_bound(dof, p):
    """x with P(chi^2_dof > x) = p for even dof: the survival function is exp(-x/2) * sum_{i < dof/2} (x/2)^i / i!,
    solved by bisection."""
    assert dof % 2 == 0
    surv = lambda x: math.exp(-x / 2) * sum((x / 2) ** i / math.factorial(i) for i in range(dof // 2))   # noqa: E731
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if surv(mid) > p else (lo, mid)
    return hi


def test_exploration_and_action_frequencies():
    """2^16 (episode, step) pairs, 256 x 256, under a fixed seed: the coin at epsilon = 0.25 within 4 sigma
    (sigma = sqrt(0.25 * 0.75 / 65536) = 0.00169: 0.007), the index over 11 actions under the chi-square bound of its
    10 degrees of freedom at p = 1e-6 (46.86; the closed form of the survival function for even degrees of freedom)."""
    words = np.concatenate([B.random_words(20261019, 1000, 256, t, 0) for t in range(256)])
    assert words.shape == (1 << 16, 4)
    explore = (words[:, 0] >> 8) < B.explore_threshold(0.25)
    print(f"explore fraction {explore.mean():.5f}")
    assert abs(explore.mean() - 0.25) < 0.007
    idx = B.random_action_index(words[:, 1], 11)
    assert idx.min() == 0 and idx.max() == 10
    counts = np.bincount(idx, minlength=11)
    expected = len(idx) / 11
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    bound = _chi2_bound(10, 1e-6)
    print(f"chi-square {chi2:.2f}, bound {bound:.2f}")
    # the derivation reproduces the printed tables of the distribution: 18.307 at p = 0.05, 29.588 at p = 0.001
    assert abs(_chi2_bound(10, 0.05) - 18.307) < 1e-3 and abs(_chi2_bound(10, 0.001) - 29.588) < 1e-3
    assert chi2 < bound
    # the noise words are spread over [-1, 1): mean 0 +- 4 sigma (sigma = 1 / sqrt(3 * 65536)), both halves of the range hit
    u = B.sym(words[:, 2])
    assert abs(float(u.mean())) < 4 / math.sqrt(3 * 65536) and u.min() < -0.999 and u.max() > 0.999


def test_clamp_and_order_on_a_stub_step():
    """A stub whose reward IS the action shows what the step was handed; its successor holds -0.0 and a payload in the
    dimensions without noise, and it reports `done` for half the batch."""
    m = 4096
    acts = np.array([-1.0, 0.25, 1.0], np.float32)
    grid = (np.zeros(4, np.float32), np.ones(4, np.float32), np.full(4, 2, np.int32), np.array([8, 4, 2, 1], np.int32),
            np.array(list(product([0, 1], repeat=4)), np.int32))
    starts = np.zeros((m, 4), np.float32)
    starts[:, 0] = np.arange(m) % 2                          # odd rows end on their first step

    def step(states, a):
        nxt = np.empty_like(states)
        nxt[:, 0] = states[:, 0]
        nxt[:, 1] = -0.0
        nxt[:, 2] = 3.0
        nxt[:, 3] = a
        return nxt, a.copy(), states[:, 0] > 0.5
    seed, first = 11, 2 ** 33
    w0, w1 = B.random_words(seed, first, m, 0, 0), B.random_words(seed, first, m, 0, 1)
    picked = acts[B.random_action_index(w0[:, 1], 3)]
    # epsilon = 1, no policy, no noise: the table's values, unclamped bits
    res = B.stochastic_rollout(step, starts, 1, None, acts, *grid, 1.0, 0.0, None, seed, first_episode=first)
    H.assert_bits_equal(res.returns, picked, "random actions")
    assert set(np.unique(res.returns)) == {-1.0, 0.25, 1.0}
    # action noise: multiply, then add, then the clamp to the table's extremes — both ends are reached
    res = B.stochastic_rollout(step, starts, 1, None, acts, *grid, 1.0, 0.5, None, seed, first_episode=first)
    want = np.fmin(np.fmax(picked + np.float32(0.5) * B.sym(w0[:, 2]), np.float32(-1.0)), np.float32(1.0))
    H.assert_bits_equal(res.returns, want, "noisy actions")
    assert res.returns.min() == -1.0 and res.returns.max() == 1.0 and (res.returns == -1.0).sum() > 10 and (res.returns == 1.0).sum() > 10
    assert len(np.unique(res.returns)) > 1000
    # state noise in dimensions 0 and 2 only; a done step's successor is stored as the step returned it
    noise = np.array([0.125, 0.0, 0.5, 0.0], np.float32)
    res = B.stochastic_rollout(step, starts, 1, None, acts, *grid, 1.0, 0.0, noise, seed, first_episode=first)
    done = starts[:, 0] > 0.5
    assert np.array_equal(res.terminated, done) and done.sum() == m // 2
    H.assert_bits_equal(res.states[:, 1], np.full(m, -0.0, np.float32), "a dimension without noise keeps its bits (-0.0)")
    H.assert_bits_equal(res.states[:, 3], picked, "a dimension without noise keeps its bits (payload)")
    H.assert_bits_equal(res.states[done][:, [0, 2]], np.tile(np.array([1.0, 3.0], np.float32), (m // 2, 1)), "done successors")
    go = ~done
    H.assert_bits_equal(res.states[go, 0], np.float32(0.0) + noise[0] * B.sym(w1[go, 0]), "dimension 0 noise")
    H.assert_bits_equal(res.states[go, 2], np.float32(3.0) + noise[2] * B.sym(w1[go, 2]), "dimension 2 noise")
    assert np.abs(res.states[go, 2] - 3.0).max() > 0.49                      # not clamped to the grid's [0, 1]
    # one value stands for every dimension; the disturbed state is what the next step starts from
    res2 = B.stochastic_rollout(step, starts[::2], 2, None, acts, *grid, 1.0, 0.0, 0.125, seed, first_episode=first,
                                record_every=1)
    assert res2.trajectory.shape == (3, m // 2, 4) and (res2.lengths == 2).all()
    w1b = B.random_words(seed, first, m // 2, 1, 1)            # the sub-batch's rows number its episodes
    H.assert_bits_equal(res2.trajectory[2][:, 0], res2.trajectory[1][:, 0] + np.float32(0.125) * B.sym(w1b[:, 0]),
                        "step 1 starts from the disturbed state")
    # refusals of the twin
    for kw in (dict(epsilon=0.5), dict(action_noise=-1.0), dict(state_noise=[0.1, 0.1]), dict(state_noise=float("inf")),
               dict(action_noise=float("nan"))):
        args = {"epsilon": 1.0, "action_noise": 0.0, "state_noise": None, **kw}
        with pytest.raises(ValueError):
            B.stochastic_rollout(step, starts, 1, None, acts, *grid, args["epsilon"], args["action_noise"],
                                 args["state_noise"], seed)


# ── the module ────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name,shape", [("pendulum", (24, 17)), ("cartpole_swingup", (9, 7, 11, 5)),
                                        ("double_cartpole_swingup", (5, 4, 6, 4, 5, 4))])
def test_stochastic_kernels_compile_for_gfx950_without_a_gpu(name, shape, tmp_path):
    """pi_infer_set_stochastic on a host-only handle: grid + pi_math.h + plugin + rollout helpers +
    csrc/pi_stochastic_kernels.hip build through hipRTC into one more code object in the handle's cache, holding both
    kernels.  Neither a policy nor values are needed."""
    eng = _host_engine(name, shape, tmp_path)
    eng.set_dynamics(envs.dynamics_source(name))
    before = set(tmp_path.glob("pi_*.hsaco"))
    assert len(before) == 2
    log = eng.set_stochastic(H.edge_actions(name))
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"pi_stochastic_rollout_kernel" in blob and b"pi_random_words_kernel" in blob
    assert b"pi_rollout_kernel" not in blob                                # the helpers only
    eng.set_stochastic(H.edge_actions(name)[:1])                           # again: served from the cache, replaces
    assert len(list(tmp_path.glob("pi_*.hsaco"))) == 3
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.rollout_stochastic(4096, 4, 10, epsilon=1.0)
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.random_words(1, 0, 4, 0, 0, 4096)
    eng.close()


def test_stochastic_kernels_do_not_spill(tmp_path):
    """Both kernels without scratch in every D, on the ahead-of-time build of the translation unit
    pi_infer_set_stochastic hands to hipRTC (tests/helpers.inference_unit restates it from the header's description), the
    method of tests/test_greedy_host.py::test_greedy_kernels_do_not_spill.  The register counts are printed: the kernel file's
    header quotes them."""
    for name, bins in (("pendulum", 200), ("cartpole_swingup", 50), ("double_cartpole", 25), ("double_cartpole_swingup", 25)):
        D = envs.ENVS[name]._D
        text = H.inference_unit(H.inference_grid(name, bins), name, "#define PI_STOCHASTIC 1\n",
                                ["pi_rollout_kernels.hip", "pi_stochastic_kernels.hip"])
        usage = H.kernel_resource_usage(text, tmp_path, name)
        assert set(usage) == {"pi_stochastic_rollout_kernel", "pi_random_words_kernel"}
        for fn, k in usage.items():
            print(f"{fn} {name} {bins}^{D}: {k}")
            assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, fn, k)


def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    lib = _native.lib()
    for sym in ("pi_infer_set_stochastic", "pi_infer_rollout_stochastic", "pi_infer_random_words"):
        assert re.search(rf"^int {sym}\(pi_infer\* h,", header, re.M), sym
        assert header.count(sym) >= 2, f"{sym} has no comment in the header"
        assert hasattr(lib, sym) and sym in _native.SIGNATURES
    for method in ("set_stochastic", "rollout_stochastic", "random_words"):
        assert callable(getattr(_native.InferenceEngine, method))
    for method in ("set_stochastic", "random_words"):
        assert callable(getattr(B.DevicePolicy, method))
    assert lib.pi_abi_version() == _native.ABI_VERSION == 12
    assert re.search(r"#define PI_MI355_ABI_VERSION 12\b", header)
    makefile = (ROOT / "dynamicprogramming_amd" / "csrc" / "Makefile").read_text()
    assert "pi_stochastic.cpp" in makefile
    assert "pi_stochastic.cpp" in (ROOT / "dynamicprogramming_amd" / "csrc" / "pi_internal.h").read_text()
    # the profiles stay tied to the sweep kernels: the new device file is not part of their fingerprint
    import hashlib
    sweeps = ROOT / "dynamicprogramming_amd" / "csrc" / "pi_sweep_kernels.hip"
    want = hashlib.sha256(sweeps.read_bytes() + (ROOT / "include" / "pi_math.h").read_bytes()).hexdigest()[:16]
    assert _native.kernel_source_hash() == want


def test_refusals_are_error_codes(tmp_path):
    name, shape = "pendulum", (12, 9)
    acts = H.edge_actions(name)
    dyn = envs.dynamics_source(name)
    eng = _host_engine(name, shape, tmp_path)
    with pytest.raises(_native.NativeError, match="no stochastic module"):
        eng.rollout_stochastic(4096, 4, 10, epsilon=1.0)
    with pytest.raises(_native.NativeError, match="no stochastic module"):
        eng.random_words(1, 0, 4, 0, 0, 4096)
    with pytest.raises(_native.NativeError, match="pi_infer_set_dynamics was never called"):
        eng.set_stochastic(acts)
    eng.set_dynamics(dyn)
    with pytest.raises(_native.NativeError, match="at least one action"):
        eng.set_stochastic(np.zeros(0, np.float32))
    with pytest.raises(_native.NativeError, match="action_space"):
        eng.set_stochastic(None)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(_native.NativeError, match=r"action_space\[1\] is not finite"):
            eng.set_stochastic(np.array([0.0, bad, 1.0], np.float32))
    eng.set_stochastic(acts)                                               # needs neither a policy nor values
    ok = dict(epsilon=1.0, action_noise=0.0, state_noise=None)
    for kw, why in ((dict(epsilon=-0.01), "epsilon"), (dict(epsilon=1.01), "epsilon"), (dict(epsilon=float("nan")), "epsilon"),
                    (dict(action_noise=-1.0), "action_noise"), (dict(action_noise=float("inf")), "action_noise"),
                    (dict(action_noise=float("nan")), "action_noise"),
                    (dict(state_noise=[0.0, -0.5]), r"state_noise\[1\]"), (dict(state_noise=[float("inf"), 0.0]), r"state_noise\[0\]"),
                    (dict(state_noise=[0.0, float("nan")]), r"state_noise\[1\]"), (dict(gamma=float("nan")), "gamma is NaN")):
        with pytest.raises(_native.NativeError, match=why):
            eng.rollout_stochastic(4096, 4, 10, **{**ok, **kw})
    with pytest.raises(ValueError, match="state_noise"):
        eng.rollout_stochastic(4096, 4, 10, state_noise=[0.1, 0.1, 0.1], **{k: v for k, v in ok.items() if k != "state_noise"})
    with pytest.raises(_native.NativeError, match="host-only"):              # everything valid: only the handle is in the way
        eng.rollout_stochastic(4096, 4, 10, **ok)
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.rollout_stochastic(4096, 4, 10, epsilon=0.5)
    with pytest.raises(_native.NativeError, match="m < 0"):
        eng.random_words(1, 0, -1, 0, 0, 4096)
    eng.set_dynamics(dyn)                                                  # a new plugin drops the module
    with pytest.raises(_native.NativeError, match="no stochastic module.*pi_infer_set_stochastic"):
        eng.rollout_stochastic(4096, 4, 10, **ok)
    with pytest.raises(_native.NativeError, match="no stochastic module.*pi_infer_set_stochastic"):
        eng.random_words(1, 0, 4, 0, 0, 4096)
    eng.close()
    lib = _native.lib()
    assert lib.pi_infer_set_stochastic(None, None, 0, None, 0) == 1          # a null handle
    assert lib.pi_infer_rollout_stochastic(None, None, 0, 0, 1.0, 0.0, 0.0, None, 0, 0, None, None, None, None, None, 0, None) == 1
    assert lib.pi_infer_random_words(None, 0, 0, 0, 0, 0, None, None) == 1


def test_front_end_refusals_need_no_gpu(tmp_path):
    """The stochastic arguments are checked before anything touches a device."""
    dp = object.__new__(B.DevicePolicy)
    pts = np.zeros((2, 2), np.float32)
    for kw in (dict(epsilon=0.1), dict(action_noise=0.5), dict(state_noise=0.1), dict(state_noise=[0.0, 0.2])):
        dp.D = 2
        with pytest.raises(ValueError, match="greedy"):
            dp.rollout(pts, 5, controller="greedy", lookahead_gamma=0.99, **kw)
    with pytest.raises(ValueError, match="controller"):
        dp.rollout(pts, 5, controller="uniform")
    with pytest.raises(ValueError, match="epsilon"):
        dp.rollout(pts, 5, epsilon=1.5)
    with pytest.raises(ValueError, match="epsilon"):
        dp.rollout(pts, 5, controller="random", epsilon=0.5)
    with pytest.raises(ValueError, match="action_noise"):
        dp.rollout(pts, 5, action_noise=-1.0)
    with pytest.raises(ValueError, match="state_noise"):
        dp.rollout(pts, 5, state_noise=[0.1, 0.2, 0.3])
    with pytest.raises(RuntimeError, match="set_stochastic"):
        dp.rollout(pts, 5, controller="random")
    with pytest.raises(RuntimeError, match="set_stochastic"):
        dp.random_words(1, 0, 4, 0, 0)
    g = H.golden("reference_results")
    shape = tuple(int(x) for x in g["mountain_car_grid_shape"])
    bins, (lo, hi, gshape, strides, bits) = _grid("mountain_car", shape)
    path = tmp_path / "mc.npz"
    np.savez(path, value_function=g["mountain_car_value_function"], policy=g["mountain_car_policy"], bounds_low=lo,
             bounds_high=hi, grid_shape=gshape, strides=strides, corner_bits=bits,
             action_space=g["mountain_car_action_space"], states_space=oracle.states_from_bins(bins))
    pi = envs.MountainCarCuda.load(path)
    starts = envs.MountainCarCuda.start_states(np.random.default_rng(0), 4)
    with pytest.raises(ValueError, match="greedy"):
        pi.rollout(starts, 10, controller="greedy", epsilon=0.2)
    with pytest.raises(ValueError, match="controller"):
        pi.rollout(starts, 10, controller="uniform")
    from dynamicprogramming_amd import solver as S
    if not S.GPU_AVAILABLE:
        with pytest.raises(RuntimeError, match="GPU"):
            pi.rollout(starts, 10, controller="random")
        with pytest.raises(RuntimeError, match="GPU"):
            envs.make("pendulum", 25)


@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_stochastic_flags_parse(name):
    from runners import _cli
    D = envs.ENVS[name]._D
    p = _cli.build_parser(name, f"results/{name}_cuda_policy.npz")
    d = p.parse_args([])
    assert (d.epsilon, d.action_noise, d.state_noise) == (0.0, 0.0, None) and _cli.ignored_flags(d) == []
    a = p.parse_args(["--rollout", "--epsilon", "0.1", "--action-noise", "0.5", "--state-noise", "0.01", "--seed", "3"])
    assert (a.epsilon, a.action_noise, a.state_noise, a.seed) == (0.1, 0.5, [0.01], 3) and _cli.ignored_flags(a) == []
    per_dim = [str(0.01 * (k + 1)) for k in range(D)]
    assert len(p.parse_args(["--rollout", "--state-noise", *per_dim]).state_noise) == D
    a = p.parse_args(["--epsilon", "0.1", "--action-noise", "0.5", "--state-noise", "0.01"])
    assert _cli.ignored_flags(a) == ["--epsilon", "--action-noise", "--state-noise"]
    a = p.parse_args(["--rollout", "--random", "3", "--steps", "50"])
    assert a.random == 3 and a.rollout and _cli.ignored_flags(a) == []
    with pytest.raises(SystemExit):
        p.parse_args(["--epsilon", "often"])


def test_random_without_rollout_still_does_nothing(capsys):
    from runners import _cli
    assert _cli.main("mountain_car", "unused.npz", ["--random"]) is None
    out = capsys.readouterr().out
    assert "nothing to do here" in out and "[random]" not in out
    assert _cli.main("pendulum", "unused.npz", ["--random", "4", "--epsilon", "0.5"]) is None
    assert "--epsilon" in capsys.readouterr().out                           # listed as ignored
