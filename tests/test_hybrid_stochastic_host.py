"""
Hybrid rollouts under noise, the part that needs no GPU: the numpy twin (utils.barycentric.stochastic_hybrid_rollout)
against a scalar restatement of the definition (include/pi_mi355.h) on a hand-written case and against the twins it must
degenerate to, the kernel compiled for gfx950 behind every D without scratch, the two entry points declared, exported,
bound and refusing what they must, the runner's flags and lines.  The device half is tests/test_gpu_hybrid_stochastic.py,
which takes the common inputs (`noisy_case`, `twin`) from here.
"""
from __future__ import annotations

import re
from functools import lru_cache
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
EPSILON, SEED, GAMMA = 0.25, 7, 0.99
SYMBOLS = ("pi_infer_set_partner_stochastic", "pi_infer_rollout_hybrid_stochastic")


# ── the common inputs of the mixed-batch tests ────────────────────────────────────────────────────────────────────
@lru_cache(maxsize=None)
def noisy_case(D):
    """A pair of tests/hybrid_cases.py with the noise every mixed-batch test runs under: epsilon 0.25, action noise a
    quarter of the primary's largest action, state noise half a primary-grid cell in every dimension, the primary's
    actions as the exploration table, seed 7."""
    c = C.build(D)
    acts = np.asarray(c["primary"][1], np.float32)
    a_noise = float(np.float32(0.25) * np.abs(acts).max())
    s_noise = np.array([np.float32(0.5) * (b[1] - b[0]) for b in c["bins"]], np.float32)
    assert a_noise == {2: 0.5, 4: 5.0, 6: 15.0}[D] and (s_noise > 0).all()
    return dict(c, table=acts, noise=dict(epsilon=EPSILON, action_noise=a_noise, state_noise=s_noise, seed=SEED))


def run_twin(D, starts=None, steps=C.STEPS, enter=None, leave=None, first_episode=0, gamma=GAMMA, record_every=0, **over):
    c = noisy_case(D)
    kw = dict(c["noise"], **over)
    table = kw.pop("table", c["table"])
    return B.stochastic_hybrid_rollout(H.oracle_for(c["env"]).step, c["starts"] if starts is None else starts, steps,
                                       kw.pop("primary", c["primary"]), kw.pop("secondary", c["secondary"]),
                                       c["enter"] if enter is None else enter, c["leave"] if leave is None else leave,
                                       table, kw["epsilon"], kw["action_noise"], kw["state_noise"], kw["seed"],
                                       first_episode=first_episode, gamma=gamma, record_every=record_every)


@lru_cache(maxsize=None)
def twin(D, first_episode=0):
    """The whole batch under the common noise with one trajectory row per step, computed once and shared (read only)."""
    res = run_twin(D, first_episode=first_episode, record_every=1)
    for x in res:
        x.setflags(write=False)
    return res


def switches_from_trajectory(res, enter, leave):
    """`switches` and `secondary_steps` recomputed from a record_every = 1 trajectory by tests/hybrid_cases.py's rule."""
    modes, took = C.modes_per_step(res, enter, leave)
    prev = np.concatenate([np.zeros((1, modes.shape[1]), bool), modes[:-1]])
    return ((modes != prev) & took).sum(axis=0).astype(np.int32), modes.sum(axis=0).astype(np.int32)


def same(got, want, what, fields=None):
    for f in fields or want._fields:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), f"{what}: {f}"
        if a is not None:
            H.assert_bits_equal(np.asarray(a), np.asarray(b), f"{what}: {f}")


# the counts the batches were chosen for (the numpy composition of the definition, first_episode = 0)
CENSUS = {2: dict(entered_late=859, left=855, never=138, mixed=4776, terminated=0, lengths=(300, 300)),
          4: dict(entered_late=161, left=132, never=797, mixed=1171, terminated=999, lengths=(1, 300)),
          6: dict(entered_late=59, left=57, never=927, mixed=296, terminated=1000, lengths=(1, 198))}


@pytest.mark.parametrize("D", [2, 4, 6])
def test_the_noisy_batches_exercise_every_path(D):
    c, res = noisy_case(D), twin(D)
    cen = C.census(res, c["enter"], c["leave"])
    print(f"D={D} {c['env']}: {cen}, {int(res.terminated.sum())} terminated, lengths {res.lengths.min()} .. "
          f"{res.lengths.max()}, {int(res.switches.sum())} switches (most in one episode: {int(res.switches.max())})")
    for key in ("entered_late", "left", "never", "mixed"):
        assert cen[key] > 0, key
        assert cen[key] == CENSUS[D][key], (key, cen[key])
    assert int(res.terminated.sum()) == CENSUS[D]["terminated"]
    assert (int(res.lengths.min()), int(res.lengths.max())) == CENSUS[D]["lengths"]
    assert res.switches.dtype == np.int32 and res.switches.max() > 1          # the hysteresis is crossed more than once
    sw, sec = switches_from_trajectory(res, c["enter"], c["leave"])
    assert np.array_equal(sw, res.switches) and np.array_equal(sec, res.secondary_steps)
    assert isinstance(res, B.StochasticHybridRolloutResult)
    assert res._fields == B.HybridRolloutResult._fields + ("switches",)


# ── the twin against a scalar restatement of the definition ───────────────────────────────────────────────────────
def test_twin_on_a_hand_written_case():
    """x moves by the action per step: +1 on the primary table, -1 on the secondary; enter |x| < 1.5, leave |x| > 2.5;
    `done` at x >= 6.  Words from random_words, one episode and one step at a time, every float32 operation written out:
    the twin must give the same modes, counters, actions and states, and the case must hold exploring steps, clamped
    actions, episodes that switch more than once and a `done` step, whose successor stays undisturbed."""
    f32 = np.float32
    bits = np.array(list(product([0, 1], repeat=2)), dtype=np.int32)
    grid = (f32([-8.0, 0.0]), f32([8.0, 1.0]), np.array([17, 2], np.int32), np.array([2, 1], np.int32), bits)
    up = (np.zeros(34, np.int32), f32([1.0])) + grid
    down = (np.zeros(34, np.int32), f32([-1.0])) + grid
    enter, leave = f32([1.5, INF]), f32([2.5, INF])
    table = f32([-3.0, 0.5, 3.0])
    eps, a_noise, s_noise, seed, first, steps, gamma = 0.4, f32(0.75), f32([0.3, 0.0]), 11, 2 ** 40 + 3, 14, f32(0.9)

    def step(states, acts):
        nxt = states.copy()
        nxt[:, 0] = states[:, 0] + acts
        return nxt, np.ones(len(states), np.float32), nxt[:, 0] >= 6.0
    starts = f32([[0.0, 0.5], [4.5, 0.5], [-3.0, 0.0], [2.0, 1.0], [5.5, 0.0], [-1.0, 0.25]])
    res = B.stochastic_hybrid_rollout(step, starts, steps, up, down, enter, leave, table, eps, a_noise, s_noise, seed,
                                      first_episode=first, gamma=gamma, record_every=1)
    eps24 = B.explore_threshold(eps)
    seen = dict(explored=0, clamped=0, done=0, modes=set())
    for e, s0 in enumerate(starts):
        s, mode, sec, sw, ret, disc, length, term = s0.copy(), False, 0, 0, f32(0), f32(1), 0, False
        for t in range(steps):
            assert np.array_equal(res.trajectory[t, e], s), (e, t)
            inside, outside = abs(s[0]) < enter[0], abs(s[0]) > leave[0]
            now = (not outside) if mode else bool(inside)
            sw, mode, sec = sw + (now != mode), now, sec + now
            seen["modes"].add(now)
            w0 = B.random_words(seed, first + e, 1, t, 0)[0]
            if (int(w0[0]) >> 8) < eps24:
                a = table[(int(w0[1]) * len(table)) >> 32]
                seen["explored"] += 1
            else:
                a = B._interpolated_actions(s[None], *(down if mode else up))[0]
                assert a == (-1.0 if mode else 1.0)
            a = f32(a + f32(a_noise * B.sym(w0[2:3])[0]))
            seen["clamped"] += abs(a) > 3.0
            a = min(max(a, f32(-3.0)), f32(3.0))
            nxt = f32([s[0] + a, s[1]])
            done = nxt[0] >= 6.0
            if not done:
                w1 = B.random_words(seed, first + e, 1, t, 1)[0]
                nxt[0] = f32(nxt[0] + f32(s_noise[0] * B.sym(w1[0:1])[0]))
            ret, disc, s, length = f32(ret + f32(disc * f32(1))), f32(disc * gamma), nxt, t + 1
            if done:
                term = True
                seen["done"] += 1
                assert s[0] == f32(res.trajectory[t, e, 0] + a)              # the successor of a `done` step is not disturbed
                break
        assert np.array_equal(res.states[e], s) and res.returns[e] == ret, e
        assert (res.lengths[e], res.terminated[e], res.secondary_steps[e], res.last_mode[e], res.switches[e]) == \
            (length, term, sec, int(mode), sw), e
        assert np.array_equal(res.trajectory[length:, e], np.tile(s, (steps + 1 - length, 1)))   # a frozen episode repeats
    print(f"hand-written case: {seen}, switches {res.switches.tolist()}, lengths {res.lengths.tolist()}")
    assert seen["explored"] > 5 and seen["clamped"] > 0 and seen["done"] > 0 and seen["modes"] == {False, True}
    assert res.switches.max() > 1 and 0 < res.terminated.sum() < len(starts)
    assert res.secondary_steps.dtype == np.int32 and res.last_mode.dtype == np.uint8 and res.switches.dtype == np.int32


# ── the twins it degenerates to ───────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("D", [2, 4, 6])
def test_twin_with_zero_noise_is_the_hybrid_twin(D):
    c = noisy_case(D)
    step = H.oracle_for(c["env"]).step
    for seed in (0, 12345):
        got = run_twin(D, record_every=7, epsilon=0.0, action_noise=0.0, state_noise=None, seed=seed)
        want = B.hybrid_rollout(step, c["starts"], C.STEPS, c["primary"], c["secondary"], c["enter"], c["leave"], gamma=GAMMA,
                                record_every=7)
        same(got, want, f"D={D} zero noise, seed {seed}")
    one = run_twin(D, record_every=1, epsilon=0.0, action_noise=0.0, state_noise=None)
    sw, _ = switches_from_trajectory(one, c["enter"], c["leave"])
    assert np.array_equal(one.switches, sw) and sw.any()


@pytest.mark.parametrize("D", [2, 4, 6])
def test_twin_with_degenerate_boxes_is_the_single_policy_stochastic_twin(D):
    c = noisy_case(D)
    step, n = H.oracle_for(c["env"]).step, c["noise"]
    starts = c["starts"][:300]
    zero, inf = np.zeros(D, np.float32), np.full(D, INF, np.float32)
    args = (n["epsilon"], n["action_noise"], n["state_noise"], n["seed"])
    never = run_twin(D, starts=starts, steps=80, enter=zero, first_episode=9, record_every=7)
    want = B.stochastic_rollout(step, starts, 80, *c["primary"], *args, first_episode=9, gamma=GAMMA, record_every=7)
    same(never, want, f"D={D} enter = 0")
    assert not never.switches.any() and not never.secondary_steps.any() and not never.last_mode.any()
    # always secondary: the exploration table is the secondary's, as the single-policy twin's is
    table2 = np.asarray(c["secondary"][1], np.float32)
    always = run_twin(D, starts=starts, steps=80, enter=inf, leave=inf, first_episode=9, record_every=7, table=table2)
    want = B.stochastic_rollout(step, starts, 80, *c["secondary"], *args, first_episode=9, gamma=GAMMA, record_every=7)
    same(always, want, f"D={D} enter = leave = inf")
    finite = np.isfinite(starts).all(axis=1)
    assert finite.all() and np.array_equal(always.switches, (always.lengths > 0).astype(np.int32))
    assert np.array_equal(always.secondary_steps, always.lengths)
    # the same policy on both sides: whatever the box, the single-policy twin
    twice = run_twin(D, starts=starts, steps=80, first_episode=9, record_every=7, secondary=c["primary"])
    want = B.stochastic_rollout(step, starts, 80, *c["primary"], *args, first_episode=9, gamma=GAMMA, record_every=7)
    same(twice, want, f"D={D} twice the same policy")
    assert twice.switches.any()


@pytest.mark.parametrize("D", [2, 4, 6])
def test_twin_is_invariant_under_cutting_the_batch(D):
    whole = twin(D, first_episode=5)
    head = run_twin(D, starts=noisy_case(D)["starts"][:300], first_episode=5, record_every=1)
    tail = run_twin(D, starts=noisy_case(D)["starts"][300:], first_episode=305, record_every=1)
    for f in whole._fields:
        axis = 1 if f == "trajectory" else 0
        H.assert_bits_equal(np.concatenate([getattr(head, f), getattr(tail, f)], axis=axis), getattr(whole, f), f"D={D}: {f}")
    assert not H.bits_equal(whole.states, twin(D).states)                     # first_episode is part of the counter


@pytest.mark.parametrize("D", [2, 4, 6])
def test_twin_at_epsilon_one_does_not_read_the_policies(D):
    c = noisy_case(D)
    rng = np.random.default_rng(3)
    starts = c["starts"][:300]
    a = run_twin(D, starts=starts, steps=80, epsilon=1.0)
    other = tuple((rng.integers(0, len(t[1]), len(t[0])).astype(np.int32),) + tuple(t[1:]) for t in (c["primary"], c["secondary"]))
    b = run_twin(D, starts=starts, steps=80, epsilon=1.0, primary=other[0], secondary=other[1])
    same(a, b, f"D={D} epsilon = 1")
    assert a.secondary_steps.any() and a.switches.any()                       # the mode is still counted
    assert not H.bits_equal(a.states, run_twin(D, starts=starts, steps=80).states)


def test_twin_refuses_what_the_stochastic_twin_refuses():
    c = noisy_case(2)
    for kw, msg in ((dict(epsilon=1.5), "epsilon"), (dict(action_noise=-1.0), "action_noise"),
                    (dict(state_noise=[0.1, 0.2, 0.3]), "state_noise"), (dict(table=np.float32([np.inf])), "finite"),
                    (dict(record_every=C.STEPS + 1), "record_every")):
        with pytest.raises(ValueError, match=msg):
            run_twin(2, starts=c["starts"][:4], **kw)


# ── the kernel, compiled without a GPU ────────────────────────────────────────────────────────────────────────────
def _host_pair(D, cache_dir):
    c = noisy_case(D)
    a = _native.InferenceEngine(*c["primary"][2:], device=-1, cache_dir=cache_dir)
    b = _native.InferenceEngine(*c["secondary"][2:], device=-1, cache_dir=cache_dir)
    return c, a, b


@pytest.mark.parametrize("D", [2, 4, 6])
def test_stochastic_hybrid_kernel_compiles_for_gfx950_without_a_gpu(D, tmp_path):
    """pi_infer_set_partner_stochastic on host-only handles: one more code object, which holds the new kernel and none of
    the kernels of the files it takes its functions from; the hybrid and the stochastic module still build from them."""
    c, a, b = _host_pair(D, tmp_path)
    with pytest.raises(_native.NativeError, match="pi_infer_set_dynamics was never called"):
        a.set_partner_stochastic(b, c["table"])
    a.set_dynamics(envs.dynamics_source(c["env"]))
    before = set(tmp_path.glob("pi_*.hsaco"))
    log = a.set_partner_stochastic(b, c["table"])
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and b"pi_hybrid_stochastic_rollout_kernel" in blob
    for other in (b"pi_hybrid_rollout_kernel", b"pi_stochastic_rollout_kernel", b"pi_random_words_kernel", b"pi_rollout_kernel"):
        assert other not in blob, other
    a.set_partner_stochastic(b, c["table"][::-1].copy())                  # another table: an upload, the same code object
    assert set(tmp_path.glob("pi_*.hsaco")) - before == {obj}
    a.set_partner(b)
    a.set_stochastic(c["table"])
    assert len(set(tmp_path.glob("pi_*.hsaco")) - before) == 3
    with pytest.raises(_native.NativeError, match="host-only"):
        a.rollout_hybrid_stochastic(b, 4096, 4, 10, c["enter"], c["leave"], **c["noise"])
    a.close()
    b.close()


def test_stochastic_hybrid_kernel_does_not_spill(tmp_path):
    """On the full-size grids (the 6-D pair is the hybrid runner's) the kernel stays without scratch, read as
    tests/test_hybrid_host.py reads it for the hybrid kernel: the ahead-of-time build of the translation unit
    pi_infer_set_partner_stochastic hands to hipRTC, restated from the kernel file's header.  The register counts are
    printed: the kernel file's header quotes them."""
    for name, bins, name2, bins2 in (("pendulum", 200, "pendulum", 50), ("cartpole_swingup", 50, "cartpole_swingup", 30),
                                     ("double_cartpole_swingup", 25, "double_cartpole", 25)):
        text = H.inference_unit(H.inference_grid(name, bins), name,
                                "#define PI_HYBRID_STOCHASTIC 1\n#define PI_HYBRID 1\n#define PI_STOCHASTIC 1\n",
                                ["pi_rollout_kernels.hip", "pi_hybrid_kernels.hip", "pi_stochastic_kernels.hip",
                                 "pi_hybrid_stochastic_kernels.hip"], second_grid=H.inference_grid(name2, bins2))
        usage = H.kernel_resource_usage(text, tmp_path, name)
        assert set(usage) == {"pi_hybrid_stochastic_rollout_kernel"}
        k = usage["pi_hybrid_stochastic_rollout_kernel"]
        print(f"pi_hybrid_stochastic_rollout_kernel {name} {bins}^D + {name2} {bins2}^D: {k}")
        assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, k)


# ── the ABI ───────────────────────────────────────────────────────────────────────────────────────────────────────
def test_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.lib()
    for name in SYMBOLS:
        assert re.search(rf"^int {name}\(pi_infer\* h, pi_infer\* partner,", text, re.M), f"{name} is not declared in pi_mi355.h"
        assert header.count(name) >= 2, f"{name} has no comment in the header"
        assert hasattr(lib, name) and name in _native.SIGNATURES
    assert len(_native.SIGNATURES["pi_infer_set_partner_stochastic"][1]) == 6
    assert len(_native.SIGNATURES["pi_infer_rollout_hybrid_stochastic"][1]) == 23
    assert "#define PI_MI355_ABI_VERSION 12" in text and lib.pi_abi_version() == 12 == _native.ABI_VERSION
    for method in ("set_partner_stochastic", "rollout_hybrid_stochastic"):
        assert callable(getattr(_native.InferenceEngine, method))
    assert callable(B.stochastic_hybrid_rollout) and B.StochasticHybridRolloutResult._fields[-1] == "switches"
    import inspect
    params = inspect.signature(B.HybridPolicy.rollout).parameters
    for key in ("epsilon", "action_noise", "state_noise", "seed", "first_episode", "action_space"):
        assert params[key].kind is inspect.Parameter.KEYWORD_ONLY and params[key].default is None, key
    assert "set_partner_stochastic" in (ROOT / "__graft_entry__.py").read_text()


def test_refusals_are_error_codes(tmp_path):
    Err = _native.NativeError
    c, a, b = _host_pair(4, tmp_path)
    c2, a2, b2 = _host_pair(2, tmp_path)
    table, dyn = c["table"], envs.dynamics_source(c["env"])
    L = _native.lib()
    run = lambda h=a, partner=b, **kw: h.rollout_hybrid_stochastic(                       # noqa: E731
        partner, 4096, 4, 10, kw.pop("enter", c["enter"]), kw.pop("leave", c["leave"]), **dict(c["noise"], **kw))
    # the builder: the handles, the pair, the plugin, the table
    assert L.pi_infer_set_partner_stochastic(a._h, None, None, 0, None, 0) != 0 and "null handle" in _native.last_error()
    assert L.pi_infer_set_partner_stochastic(None, b._h, None, 0, None, 0) != 0 and "null handle" in _native.last_error()
    a.set_dynamics(dyn)
    with pytest.raises(Err, match="differ in D"):
        a.set_partner_stochastic(a2, table)
    lo, hi, gshape, strides, bits = c["secondary"][2:]
    flipped = _native.InferenceEngine(lo, hi, gshape, strides, bits[::-1].copy(), device=-1, cache_dir=tmp_path)
    with pytest.raises(Err, match="corner_bits"):
        a.set_partner_stochastic(flipped, table)
    with pytest.raises(Err, match="action_space"):
        a.set_partner_stochastic(b, None)
    with pytest.raises(Err, match="at least one action"):
        a.set_partner_stochastic(b, np.zeros(0, np.float32))
    with pytest.raises(Err, match=r"pi_infer_set_partner_stochastic: action_space\[1\] is not finite"):
        a.set_partner_stochastic(b, np.float32([0.0, np.nan]))
    # the launch: the handles, the pair, the module
    none = (None,) * 8
    assert L.pi_infer_rollout_hybrid_stochastic(None, b._h, None, 1, 1, 1.0, None, None, 0.0, 0.0, None, 0, 0, *none, 0,
                                                None) != 0 and "null handle" in _native.last_error()
    with pytest.raises(Err, match="null handle"):
        run(partner=None)
    with pytest.raises(Err, match="differ in D"):
        run(partner=a2)
    with pytest.raises(Err, match="corner_bits"):
        run(partner=flipped)
    with pytest.raises(Err, match=r"no hybrid module: call pi_infer_set_partner_stochastic \(again after every pi_infer_set_dynamics\)"):
        run()
    a.set_partner(b)                                                       # the deterministic module is not the one asked for
    with pytest.raises(Err, match="pi_infer_set_partner_stochastic"):
        run()
    a.set_partner_stochastic(b, table)
    other = _native.InferenceEngine(lo, hi, [5, 6, 4, 7], [168, 28, 7, 1], bits, device=-1, cache_dir=tmp_path)
    with pytest.raises(Err, match="another partner grid: call pi_infer_set_partner_stochastic"):
        run(partner=other)
    # the box
    nan = c["enter"].copy()
    nan[2] = np.nan
    for kw, msg in ((dict(enter=nan), "threshold 2 is NaN"), (dict(leave=nan), "threshold 2 is NaN"),
                    (dict(enter=c["leave"], leave=c["enter"]), r"enter\[2\] > leave\[2\]"), (dict(enter=None), "null argument"),
                    # the noise
                    (dict(epsilon=1.5), "epsilon must lie in"), (dict(epsilon=np.nan), "epsilon must lie in"),
                    (dict(action_noise=-0.5), "action_noise must be finite"), (dict(action_noise=np.inf), "action_noise must be finite"),
                    (dict(state_noise=np.float32([0, 0, -1, 0])), r"state_noise\[2\] must be finite"),
                    (dict(gamma=np.nan), "gamma is NaN")):
        with pytest.raises(Err, match=msg):
            run(**kw)
        assert "pi_infer_rollout_hybrid_stochastic" in _native.last_error() or "null argument" in _native.last_error()
    with pytest.raises(ValueError, match="4 thresholds"):
        run(enter=c["enter"][:3])
    with pytest.raises(ValueError, match="4 values"):
        run(state_noise=np.zeros(3, np.float32))
    with pytest.raises(Err, match="host-only"):                            # everything else passed: only the device is missing
        run()
    a.set_dynamics(dyn)                                                    # a new plugin drops the module
    with pytest.raises(Err, match="no hybrid module: call pi_infer_set_partner_stochastic"):
        run()
    for e in (a, b, a2, b2, flipped, other):
        e.close()


# ── the runner ────────────────────────────────────────────────────────────────────────────────────────────────────
class _FakePolicy:
    """Stands in for HybridPolicy in the runner: records the call and returns fixed numpy results."""
    class _Closed:
        def close(self):
            pass
    primary = secondary = _Closed()

    def __init__(self):
        self.calls = []

    def rollout(self, states, steps, **kw):
        self.calls.append((np.array(states), steps, kw))
        m = len(states)
        fields = (np.tile(np.float32([0.1, 0.0, 0.5, -1.25, -0.25, 2.5]), (m, 1)), np.float32([10.4] * m),
                  np.full(m, steps, np.int32), np.arange(m) % 2 == 1, None, np.arange(m, dtype=np.int32) * 3,
                  (np.arange(m) % 2).astype(np.uint8))
        if kw:
            return B.StochasticHybridRolloutResult(*fields, np.arange(m, dtype=np.int32) + 1)
        return B.HybridRolloutResult(*fields)


def test_runner_takes_the_noise_flags_and_is_unchanged_without_them(tmp_path, capsys, monkeypatch):
    from runners import _cli
    from runners import hybrid_double_cartpole as R
    p = R.build_parser()
    d = p.parse_args([])
    assert (d.epsilon, d.action_noise, d.state_noise) == (0.0, 0.0, None) and not R.noise_requested(d)
    a = p.parse_args(["--epsilon", "0.1", "--action-noise", "2.5", "--state-noise", "0.01", "0", "0.02", "0", "0.02", "0"])
    assert (a.epsilon, a.action_noise, a.state_noise) == (0.1, 2.5, [0.01, 0.0, 0.02, 0.0, 0.02, 0.0]) and R.noise_requested(a)
    assert R.ignored_flags(a) == [] and R.ignored_flags(p.parse_args(["--random", "--epsilon", "0.5"])) == ["--random"]
    assert all(R.noise_requested(p.parse_args(f)) for f in (["--epsilon", "1"], ["--action-noise", "1"], ["--state-noise", "0"]))
    # names, types and meaning of the other runners' flags (runners/_cli.py); the stream is seeded by --seed there and here
    theirs = {x.dest: x for x in _cli.build_parser("pendulum", "x.npz")._actions}
    ours = {x.dest: x for x in p._actions}
    for dest in ("epsilon", "action_noise", "state_noise"):
        assert (ours[dest].option_strings, ours[dest].type, ours[dest].default, ours[dest].nargs, ours[dest].metavar) == \
            (theirs[dest].option_strings, theirs[dest].type, theirs[dest].default, theirs[dest].nargs, theirs[dest].metavar)
        assert ours[dest].help == theirs[dest].help.replace("(extension, with --rollout)", "(extension)")
    assert "noise_seed" not in theirs and "noise_seed" not in ours
    sw, ba = tmp_path / "a.npz", tmp_path / "b.npz"
    sw.write_bytes(b"")
    ba.write_bytes(b"")
    fake = _FakePolicy()
    monkeypatch.setattr(R, "hybrid_policy", lambda *args, **kw: fake)
    paths = ["--swingup-path", str(sw), "--balance-path", str(ba), "--episodes", "2", "--steps", "30", "--seed", "3"]
    # without the flags: today's call, today's lines
    R.main(paths + ["--random"])
    out = capsys.readouterr().out.splitlines()
    assert out == [f"[{R.ENV}] note: --random belong to the rollout / plot harness or to training, which this runner does not "
                   "do; accepted and ignored",
                   "Ep 1: 30 steps | reward=10 | balance_steps=0 | last_mode=SWINGUP | th1=+28.6° th2=-14.3° w1=-1.25 w2=+2.50",
                   "Ep 2: 30 steps | reward=10 | balance_steps=3 | last_mode=BALANCE | th1=+28.6° th2=-14.3° w1=-1.25 w2=+2.50"]
    assert fake.calls[0][1] == 30 and fake.calls[0][2] == {} and np.array_equal(fake.calls[0][0], R.start_states(3, 2))
    # with them: the keywords of HybridPolicy.rollout, switches= in every line and the summary
    R.main(paths + ["--epsilon", "0.1", "--state-noise", "0.01"])
    out = capsys.readouterr().out.splitlines()
    assert fake.calls[1][2] == dict(epsilon=0.1, action_noise=0.0, state_noise=[0.01], seed=3)
    assert out == ["Ep 1: 30 steps | reward=10 | balance_steps=0 | switches=1 | last_mode=SWINGUP | th1=+28.6° th2=-14.3° "
                   "w1=-1.25 w2=+2.50",
                   "Ep 2: 30 steps | reward=10 | balance_steps=3 | switches=2 | last_mode=BALANCE | th1=+28.6° th2=-14.3° "
                   "w1=-1.25 w2=+2.50",
                   "Summary: 2 episodes | mean reward=10.4 | terminated=0.50 | ending in BALANCE=0.50 | mean switches=1.50"]
