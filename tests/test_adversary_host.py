"""
The robust lookahead and the adversary rollout without a GPU: the numpy twins (dynamicprogramming_amd.noise.robust_action /
adversary_rollout) against the twins they must agree with, the adversary module of the inference handle on host-only
handles (build, cache objects, refusals in the documented order), the register budget of
csrc/pi_adversary_kernels.hip, symbols and the runner's flag.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import utils.barycentric as B
from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd.noise import Disturbances
from tests import expect_greedy_cases as C
from tests import helpers as H

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("pi_infer_set_robust", "pi_infer_robust", "pi_infer_rollout_adversary")
KERNELS = {"pi_robust_greedy_kernel", "pi_adversary_rollout_kernel"}


def _policy_tables(c):
    pol = np.random.default_rng(9).integers(0, len(c["acts"]), size=len(c["states"])).astype(np.int32)
    return (pol, c["acts"], *c["grid"], c["bits"])


# ---- 1. the twins ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", C.GRIDS, ids=C.IDS)
def test_zero_set_twins_are_the_deterministic_twins(name, shape):
    """With the one-point zero set the adversary has one answer: controller "policy" is ``rollout`` and controller "robust"
    is ``greedy_rollout``, bit for bit, trajectories included; the query is ``greedy_action`` with worst = 0 where an
    action won."""
    c = C.case(name, shape)
    d0 = Disturbances.none(c["D"])
    tables = (c["V"], c["acts"], *c["grid"])
    starts = C.query_points(c, 65, seed=3)
    policy = _policy_tables(c)
    kw = dict(gamma=0.97, record_every=1)
    got = noise.adversary_rollout(c["chk"].step, starts, 7, d0, *tables, controller="policy", policy=policy,
                                  lookahead_gamma=c["gamma"], **kw)
    C.assert_same_rollout(got, B.rollout(c["chk"].step, starts, 7, *policy, **kw), f"{name} policy")
    got = noise.adversary_rollout(c["chk"].step, starts, 7, d0, *tables, controller="robust", lookahead_gamma=c["gamma"], **kw)
    C.assert_same_rollout(got, B.greedy_rollout(c["chk"].step, starts, 7, *tables, c["gamma"], **kw), f"{name} robust")
    best, act, qb, worst, Q = noise.robust_action(c["chk"].step, starts, d0, *tables, c["gamma"], q_values=True)
    g_best, g_act, g_qb, g_Q = B.greedy_action(c["chk"].step, starts, *tables, c["gamma"], q_values=True)
    assert np.array_equal(best, g_best) and np.array_equal(worst, np.where(qb > np.float32(-1.0e30), 0, -1))
    for a, b, what in ((act, g_act, "action"), (qb, g_qb, "best Q"), (Q, g_Q, "Q")):
        H.assert_bits_equal(a, b, f"{name} {what}")


@pytest.mark.parametrize("name,shape", C.GRIDS, ids=C.IDS)
def test_lookahead_columns_are_the_worst_case_q_and_the_step_is_the_worst_points(name, shape):
    """Q(., a) of the query is ``expected_q(risk="worst")`` and ``worst`` its k* for the winner; one adversary step under
    the policy table lands where that point's own one-point set lands (its successor, reward and flag)."""
    c = C.case(name, shape)
    d = C.multi_point_set(name)
    tables = (c["V"], c["acts"], *c["grid"])
    pts = C.query_points(c, 65)
    best, act, qb, worst, Q = noise.robust_action(c["chk"].step, pts, d, *tables, c["gamma"], q_values=True)
    for i, u in enumerate(c["acts"]):
        q, k = noise.expected_q(c["chk"].step, pts, u, d, *tables, c["gamma"], risk="worst", worst_point=True)
        H.assert_bits_equal(q, Q[:, i], f"{name} Q(., {u})")
    won = qb > np.float32(-1.0e30)
    for i, u in enumerate(c["acts"]):                  # where an action won, worst is the k* of the fold under that action
        _, k = noise.expected_q(c["chk"].step, pts, u, d, *tables, c["gamma"], risk="worst", worst_point=True)
        rows = won & (best == i)
        assert np.array_equal(worst[rows], k[rows]), f"{name} worst under action {i}"
    assert len(np.unique(best[won])) > 1, "more than one action wins somewhere: the loop above is not about one action"
    assert won.any() and (worst[won] >= 0).all() and (worst[~won] == -1).all() and (best[~won] == 0).all()
    policy = _policy_tables(c)
    one = noise.adversary_rollout(c["chk"].step, pts, 1, d, *tables, controller="policy", policy=policy, lookahead_gamma=c["gamma"])
    a = B._interpolated_actions(np.ascontiguousarray(pts, np.float32), *policy)
    _, k = noise.expected_q(c["chk"].step, pts, a, d, *tables, c["gamma"], risk="worst", worst_point=True)
    for j in np.unique(k):
        rows = k == j
        alone = Disturbances(d.action_offsets[j:j + 1], d.state_offsets[j:j + 1], [1.0])
        want = noise.adversary_rollout(c["chk"].step, pts[rows], 1, alone, *tables, controller="policy", policy=policy,
                                       lookahead_gamma=c["gamma"])
        H.assert_bits_equal(one.states[rows], want.states, f"{name} successor of point {j}")
        H.assert_bits_equal(one.returns[rows], want.returns, f"{name} reward of point {j}")
        assert np.array_equal(one.terminated[rows], want.terminated)
    with pytest.raises(ValueError, match="controller"):
        noise.adversary_rollout(c["chk"].step, pts, 1, d, *tables, controller="greedy")
    with pytest.raises(ValueError, match="policy"):
        noise.adversary_rollout(c["chk"].step, pts, 1, d, *tables, controller="policy")


# ---- 2. the module on host-only handles -------------------------------------------------------------------------------
def _host_engine(name, shape, cache_dir):
    c = C.case(name, shape)
    return c, _native.InferenceEngine(*c["grid"], c["bits"], device=-1, cache_dir=cache_dir)


@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_adversary_module_builds_for_gfx950_and_is_one_more_cache_object(name, tmp_path):
    shape = {2: (24, 17), 4: (9, 7, 11, 5), 6: (5, 4, 6, 4, 5, 4)}[envs.ENVS[name]._D]
    c, eng = _host_engine(name, shape, tmp_path)
    eng.set_values(np.zeros(len(c["states"]), np.float32))
    eng.set_dynamics(envs.dynamics_source(name))
    before = set(tmp_path.glob("pi_*.hsaco"))
    log = eng.set_robust(c["acts"])
    assert isinstance(log, str) and "error" not in log.lower()
    (obj,) = set(tmp_path.glob("pi_*.hsaco")) - before                      # one more cache object
    blob = obj.read_bytes()
    assert blob[:4] == b"\x7fELF" and all(k.encode() in blob for k in KERNELS)
    for other in (b"pi_rollout_kernel", b"pi_greedy_kernel", b"pi_greedy_rollout_kernel"):
        assert other not in blob, other                                        # the shared functions only
    d = Disturbances.none(c["D"])
    assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == 1     # an upload: no build
    eng.set_greedy(c["acts"])                                                  # the greedy module still builds from its file
    assert len(list(tmp_path.glob("pi_*.hsaco"))) == len(before) + 2
    with pytest.raises(_native.NativeError, match="host-only"):
        eng.robust(4096, 4, 0.99, d_best=4096)
    eng.set_dynamics(envs.dynamics_source(name))                               # drops the module
    with pytest.raises(_native.NativeError, match="pi_infer_set_robust"):
        eng.robust(4096, 4, 0.99, d_best=4096)
    eng.close()


def test_refusals_in_the_documented_order_on_a_host_only_handle(tmp_path):
    c, eng = _host_engine("pendulum", (24, 17), tmp_path)
    lib = _native.lib()
    assert lib.pi_infer_robust(None, 8, 4, 0.9, 8, None, None, None, None, None) != 0 and "null handle" in _native.last_error()
    with pytest.raises(_native.NativeError, match="pi_infer_set_values"):
        eng.set_robust(c["acts"])
    eng.set_values(np.zeros(len(c["states"]), np.float32))
    with pytest.raises(_native.NativeError, match="pi_infer_set_dynamics"):
        eng.set_robust(c["acts"])
    eng.set_dynamics(envs.dynamics_source("pendulum"))
    with pytest.raises(_native.NativeError):
        eng.set_robust(np.array([0.0, np.nan], np.float32))                    # a table that is not finite
    query = lambda **kw: eng.robust(8, 4, kw.pop("gamma", 0.9), **{"d_best": 8, **kw})                    # noqa: E731
    run = lambda controller=1, lg=0.9, **kw: eng.rollout_adversary(8, 4, 3, lg, controller, **{"d_final": 8, **kw})   # noqa: E731
    for call in (query, run):                                                  # a missing module ...
        with pytest.raises(_native.NativeError, match="pi_infer_set_robust"):
            call()
    eng.set_robust(c["acts"])
    for call in (query, run):                                                  # ... then a missing set
        with pytest.raises(_native.NativeError, match="pi_infer_set_disturbances"):
            call()
    eng.set_disturbances(None, None, [1.0])
    with pytest.raises(_native.NativeError, match="gamma is NaN"):             # NaN discounts
        query(gamma=float("nan"))
    with pytest.raises(_native.NativeError, match="gamma is NaN"):
        run(gamma=float("nan"))
    with pytest.raises(_native.NativeError, match="lookahead_gamma is NaN"):
        run(lg=float("nan"))
    for bad in (2, -1):                                                        # a controller other than 0 or 1
        with pytest.raises(_native.NativeError, match="controller must be"):
            run(controller=bad)
    with pytest.raises(_native.NativeError, match="needs a policy"):           # controller 0 without a policy
        run(controller=0)
    with pytest.raises(_native.NativeError, match="all five outputs"):
        eng.robust(8, 4, 0.9)
    with pytest.raises(_native.NativeError, match="host-only"):
        run()
    eng.close()


def test_symbols_are_declared_commented_exported_and_bound():
    header = (ROOT / "include" / "pi_mi355.h").read_text()
    lib = _native.lib()
    for sym in SYMBOLS:
        assert re.search(rf"^int {sym}\(pi_infer\* h,", header, re.M), sym
        assert header.count(sym) >= 2, f"{sym} has no comment in the header"
        assert hasattr(lib, sym) and sym in _native.SIGNATURES
    for method in ("set_robust", "robust", "rollout_adversary"):
        assert callable(getattr(_native.InferenceEngine, method))
    for method in ("set_robust", "robust", "adversary_rollout"):
        assert callable(getattr(B.DevicePolicy, method))
    assert _native.ABI_VERSION == 12 and lib.pi_abi_version() == 12
    csrc = ROOT / "dynamicprogramming_amd" / "csrc"
    assert "pi_adversary.cpp" in (csrc / "Makefile").read_text()
    assert "pi_adversary.cpp" in (csrc / "pi_internal.h").read_text().split("#pragma once")[0]
    text = (csrc / "pi_adversary_kernels.hip").read_text()
    assert not re.search(r"s_sleep|while\s*\(\s*(true|1)\s*\)|__builtin_amdgcn_s_waitcnt", text)     # no waits, no polls


# ---- 3. registers --------------------------------------------------------------------------------------------------------
def test_adversary_kernels_do_not_spill(tmp_path):
    """Both kernels without scratch and within 512 VGPRs in every D, on the ahead-of-time build of the translation unit
    pi_infer_set_robust hands to hipRTC (tests/helpers.inference_unit restates it from the kernel file's header).  The
    register counts are printed: the kernel file's header and DESIGN quote them."""
    for name, bins in (("pendulum", 200), ("cartpole_swingup", 50), ("double_cartpole", 25), ("double_cartpole_swingup", 25)):
        text = H.inference_unit(H.inference_grid(name, bins), name, "#define PI_ADVERSARY 1\n#define PI_GREEDY 1\n",
                                ["pi_rollout_kernels.hip", "pi_greedy_kernels.hip", "pi_adversary_kernels.hip"])
        usage = H.kernel_resource_usage(text, tmp_path, name)
        assert set(usage) == KERNELS
        for fn, k in usage.items():
            print(f"{fn} {name} {bins}^{envs.ENVS[name]._D}: {k}")
            assert k["scratch"] == 0 and k["vgpr"] <= 512, (name, fn, k)


# ---- 4. the runner's flag ------------------------------------------------------------------------------------------------
def test_adversary_flag(tmp_path, capsys):
    from dynamicprogramming_amd.solver import CudaPIConfig
    from runners import _cli
    from tests.robust_backend import with_robust_backend
    parse = _cli.build_parser("cartpole", "x.npz").parse_args
    assert parse([]).adversary is None and _cli.ignored_flags(parse([])) == []
    assert parse(["--rollout", "--adversary"]).adversary == "policy" and parse(["--rollout", "--adversary", "robust"]).adversary == "robust"
    assert _cli.ignored_flags(parse(["--rollout", "--adversary"])) == [] and _cli.ignored_flags(parse(["--adversary"])) == ["--adversary"]
    with pytest.raises(SystemExit):
        parse(["--adversary", "greedy"])
    # an archive without a set and no --train-*-noise flag: the runner says what is missing; with a set (the archive's, or
    # the flags') evaluate() hands it and the controller to the policy's adversary_rollout and prints rollout's lines
    cls = envs.ENVS["pendulum"]
    cfg = CudaPIConfig(**{**cls.CONFIG, "max_pi_iter": 1, "max_eval_iter": 2})
    s = with_robust_backend(cls)(H.env_bins_space("pendulum", (12, 11)), cls.ACTIONS, cfg)
    s.run()
    s.save(tmp_path / "plain")
    with pytest.raises(SystemExit, match="--adversary needs a disturbance set"):
        _cli.main("pendulum", str(tmp_path / "plain.npz"), ["--save-path", str(tmp_path / "plain.npz"), "--rollout", "--adversary"])
    calls = []

    class Stub:
        disturbances = Disturbances.none(2)

        def adversary_rollout(self, starts, steps, **kw):
            calls.append((len(starts), steps, kw))
            m = len(starts)
            return B.RolloutResult(np.zeros((m, 2), np.float32), np.ones(m, np.float32), np.full(m, steps, np.int32),
                                   np.zeros(m, bool), None)
    capsys.readouterr()
    _cli.evaluate("pendulum", Stub(), 3, 10, 42, adversary="robust", disturbances=Stub.disturbances)
    out = capsys.readouterr().out
    assert out.count("Episode ") == 3 and "10 steps | return = 1.000" in out
    assert calls == [(3, 10, dict(controller="robust", gamma=1.0, record_every=0, disturbances=Stub.disturbances))]
