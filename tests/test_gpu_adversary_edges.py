"""
GPU: pi_robust_greedy_kernel and pi_adversary_rollout_kernel (csrc/pi_adversary_kernels.hip) at their edges, both
controllers, against dynamicprogramming_amd.noise.robust_action / adversary_rollout on the checker's step — bit for bit,
`worst` and trajectories included, with `_assert_query` and `_same_rollout` of tests/test_gpu_adversary.py.  Grids, start
vectors and source tables are those of tests/infer_cases.py, the shapes those of tests/test_gpu_infer_edges.py.  Every GPU
step runs once.  What a case exercises is asserted from the twin (the per-point q of tests/robust_cases.point_q and its
host folds), never from the device result.

The adversary fold returns k*, so an exact tie between two points is visible here and not in the sweeps: the first of
equal points must win.  Where values are not finite, a NaN the arithmetic GENERATES may differ in payload and sign between
host and device: in those tests, and only there, every NaN of both sides is replaced by one NaN before the comparison
(positions are compared, bits of a NaN are not), and `_same_rollout` is told which episodes start on a non-finite state.

What would have to be wrong in the kernel for a test to fail.  OBSERVED: failed in the mutation run (pi_adversary_worst's
`q < Q` replaced by `q <= Q`, run once, not committed); JUDGED: written from the code, not run.

- every test of this file.  OBSERVED: all 19 fail under `q <= Q`, on `worst` or on a trajectory: beside the tie sets,
  points beyond a bound (their disturbed successors clamp to one border cell) and `done` steps (q = r for every row of a
  run) tie as well.  Of the earlier tests, 7 of the 9 twin comparisons of tests/test_gpu_adversary.py fail too (the 6-D
  rollouts do not).
- ties for k* (test_ties_*).  OBSERVED: `q <= Q` — the last of equal points wins: `worst` of the query and, through
  dx_{k*}, the trajectories differ.  JUDGED: k_star / best_k updated on `>=` in the action loop (the later of two tied
  actions would report its own k*), wn / wr / wdone copied from the last point instead of the worst.
- non-finite and boundary states (test_non_finite_and_boundary_states).  JUDGED: a NaN or infinite coordinate reaching
  pi_greedy_expect's cell search without its clamp, -0.0 against a bound of the other sign, lanes of one wave with NaN and
  ordinary states diverging in the point loop (the table words are wave-uniform, the branches on q are not).
- non-finite V (test_non_finite_values).  JUDGED: `q != q` dropped (a NaN point never taken: k* and the successor
  differ), fminf in place of the comparison, best_k kept from a NaN action, `worst` not -1 where no action won, the
  rollout keeping another action's successor than action 0's where nothing wins.
- one-cell, ragged and permuted grids (test_one_cell_and_ragged_grids, test_value_table_on_a_permuted_memory_order).
  JUDGED: base index or stride arithmetic of pi_greedy_expect under the point loop (dx added in the user's dimension
  order, strides of the memory order), a 2-bin dimension's clamp `min(i, g - 2)`.
- batch geometry (test_batch_geometry).  JUDGED: `i >= m` off by one at m = 255, 256, 257 and 1, a second workgroup's
  lanes reading past `points`, the episode loop's bound at a one-episode batch.

Measured on an MI355X (this module alone, `pytest -m gpu --durations=0`; every handle compiles its modules in the call):
19 tests in 13.3 s.  Slowest calls: boundary states 6-D 1.4 s, permuted order 6-D 1.2 s, one cell 2^6 1.2 s, ties 2-D 0.9 s,
ties 4-D, the ragged grids and permuted order 4-D 0.7 s each, everything else 0.6 s or less.
Not built: the robust query beside the greedy one in tests/test_gpu_infer_addr64.py (the optional item).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import utils.barycentric as B
from dynamicprogramming_amd import envs, noise
from dynamicprogramming_amd.noise import Disturbances
from tests import infer_cases as IC
from tests import robust_cases as RC
from tests.test_gpu_adversary import _assert_query, _same_rollout
from tests.test_gpu_infer_edges import GRIDS, ORDERS, SHAPES

pytestmark = pytest.mark.gpu

f32 = np.float32
CONTROLLERS = ("policy", "robust")
RETURN_GAMMA = 0.97


@lru_cache(maxsize=None)
def _source(D, order=None):
    g = GRIDS[D]
    return IC.source(g["env"], g["shape"], order=order, seed=3)


def _cell(src):
    return (src["hi"].astype(np.float64) - src["lo"].astype(np.float64)) / (np.asarray(src["gshape"], np.float64) - 1)


def _multi(src):
    """Action noise of a tenth of the action range and state noise of 0.7 cells in the first and the last dimension, two
    nodes each: K = 8, da in two runs of four."""
    D = src["D"]
    amp = np.zeros(D)
    amp[[0, D - 1]] = 0.7 * _cell(src)[[0, D - 1]]
    d = Disturbances.uniform(D, state_noise=amp, action_noise=0.1 * float(src["acts"].max() - src["acts"].min()), points=2)
    assert d.K == 8
    return d


def _dp(src, dev, V=None):
    dp = B.DevicePolicy(src["policy"], src["acts"], src["lo"], src["hi"], src["gshape"], src["strides"], src["bits"], device=dev)
    dp.set_values(src["V"] if V is None else V)
    dp.set_dynamics(envs.dynamics_source(src["env"]))
    assert isinstance(dp.set_robust(), str)
    return dp


def _one_nan(x):
    x = np.array(x.cpu().numpy() if hasattr(x, "cpu") else x)
    return np.where(np.isnan(x), f32(np.nan), x).astype(f32) if x.dtype == np.float32 else x


def _want(src, d, pts, V=None):
    """The twin's (best, action, q_best, worst, Q) of the query."""
    with np.errstate(all="ignore"):
        return noise.robust_action(src["chk"].step, pts, d, src["V"] if V is None else V, src["acts"], *src["grid"],
                                   src["gamma"], q_values=True)


def _query(dp, src, d, pts, what, V=None, non_finite=False, want=None):
    """The query with the Q matrix against the twin (`want`: computed before, where a test asserts its conditions from it
    before anything is launched); returns the twin's result."""
    want = _want(src, d, pts, V) if want is None else want
    got = dp.robust(pts, src["gamma"], q_values=True)
    if non_finite:
        got, want_c = [_one_nan(x) for x in got], [_one_nan(x) for x in want]
        _assert_query(got, want_c, what)
    else:
        _assert_query(got, want, what)
    return want


def _rollout_wants(src, d, starts, steps, V=None):
    """The twin's rollouts by controller, every state recorded."""
    with np.errstate(all="ignore"):
        return {controller: noise.adversary_rollout(src["chk"].step, starts, steps, d, src["V"] if V is None else V, src["acts"],
                                                    *src["grid"], controller=controller, policy=src["tables"], gamma=RETURN_GAMMA,
                                                    lookahead_gamma=src["gamma"], record_every=1) for controller in CONTROLLERS}


def _rollouts(dp, src, d, starts, steps, what, V=None, non_finite=False, wants=None):
    """Both controllers, every state recorded, against the twin (`wants`: computed before)."""
    wants = _rollout_wants(src, d, starts, steps, V) if wants is None else wants
    marks = np.where(np.isfinite(starts), starts, f32(np.nan)) if non_finite else np.zeros_like(starts)
    for controller in CONTROLLERS:
        got = dp.adversary_rollout(starts, steps, gamma=RETURN_GAMMA, record_every=1, controller=controller,
                                   lookahead_gamma=src["gamma"])
        _same_rollout(got, wants[controller], marks, f"{what} {controller} steps={steps}")
    return wants


def _fold_at(src, d, pts, action_values, V=None):
    """(per-point q (K, m), Q, k*) of the strict fold at `pts` under `action_values`, on the host."""
    with np.errstate(all="ignore"):
        q = RC.point_q(src["chk"].step, pts, action_values, d, src["V"] if V is None else V, src["acts"], src["grid"], src["gamma"])
    return (q, *RC.fold(q, d.weights))


def _tied_for_the_minimum(q, weights):
    """Per query point: at least two participating rows hold the minimum, with bit-equal q."""
    part = q[np.asarray(weights) != 0]
    least = part.min(axis=0)
    return ((part == least[None, :]) & (part.view(np.uint32) == least.view(np.uint32)[None, :])).sum(axis=0) >= 2


def _starts(src, m, seed):
    return IC.ordinary_starts(np.random.default_rng(seed), src["lo"], src["hi"], m, spread=1.3)


# ---- ties for k* ----------------------------------------------------------------------------------------------------------
def _tie_sets(src):
    """Sets with bit-identical rows at different positions, and one whose rows differ only in a dx of dimension 0 that is
    clamped to the same border by the interpolation."""
    D, cell = src["D"], _cell(src)
    arange = float(src["acts"].max() - src["acts"].min())
    rng = np.random.default_rng(17)
    X, Y, Z = ((f32(a * arange), (rng.uniform(-0.8, 0.8, size=D) * cell).astype(f32)) for a in (0.15, -0.2, 0.0))

    def rows(*r):
        return Disturbances([x[0] for x in r], np.stack([x[1] for x in r]), np.full(len(r), 1.0 / len(r)))
    beyond = np.zeros((3, D), f32)
    beyond[:, 0] = [1e30, 2e30, 3e30]
    return {"two-identical": rows(X, X), "two-identical-after-another": rows(Y, X, X), "three-identical-apart": rows(X, Y, X, Z, X),
            "clamped-to-one-border": Disturbances(None, beyond, np.full(3, 1.0 / 3.0))}


@pytest.mark.parametrize("D", (2, 4))
def test_ties_between_points_take_the_first(D, cuda_device):
    """Query at 257 points and 7-step rollouts of 65 episodes under sets with exact ties for the minimum.  From the twin:
    under every set at least a quarter of the query points have a tie for the minimum under the winning action, the
    strict fold's k* is the first of the tied rows there, and `<=` would report another row."""
    src = _source(D)
    pts = _starts(src, 257, 50 + D)
    sets, wants = _tie_sets(src), {}
    for label, d in sets.items():                            # the conditions, from the twin, before anything is launched
        want = wants[label] = _want(src, d, pts)
        q, Q, k = _fold_at(src, d, pts, want[1])
        tied = _tied_for_the_minimum(q, d.weights)
        assert tied.mean() >= 0.25, f"{D}-D {label}: a tie for the minimum at only {tied.mean():.3f} of the points"
        won = want[3] >= 0
        assert np.array_equal(k[won], want[3][won]) and won.mean() > 0.9
        last = RC.fold(q, d.weights, "last-of-equals")[1]
        assert (last[tied & won] != k[tied & won]).all() and (k[tied & won] < last[tied & won]).all()
    dp = _dp(src, cuda_device)
    for label, d in sets.items():
        dp.set_disturbances(d)
        _query(dp, src, d, pts, f"{D}-D {label}", want=wants[label])
        _rollouts(dp, src, d, pts[:65], 7, f"{D}-D {label}")
    dp.close()


PENDULUM_TIED_ACTIONS = np.array([-3.0, -2.5, 2.5, 3.0], f32)       # the plugin clamps its torque to +-2: -3 and -2.5 tie


def test_ties_between_actions_report_the_lowest_index_and_its_point(cuda_device):
    """Pendulum with the torques -3, -2.5, 2.5, 3 and the rows da = (+0.75, 0): action 0 becomes -2.25 and -3, both
    clamped to -2 by the plugin, so its two points tie and k* = 0; action 1 becomes -1.75 and -2.5 -> -2, so where the
    second point is its minimum Q(1) has the bits of Q(0) and k* = 1.  The strict argmax keeps action 0 and reports ITS
    point.  From the twin: such points exist where action 0 is the winner."""
    src = IC.source("pendulum", GRIDS[2]["shape"], seed=5, actions=PENDULUM_TIED_ACTIONS)
    d = Disturbances([0.75, 0.0], np.zeros((2, 2), f32), [0.5, 0.5])
    pts = _starts(src, 257, 61)
    want = _want(src, d, pts)
    k0, k1 = (_fold_at(src, d, pts, a)[2] for a in PENDULUM_TIED_ACTIONS[:2])
    Q = want[4]
    tie = (Q[:, 0].view(np.uint32) == Q[:, 1].view(np.uint32)) & (want[0] == 0) & (k0 == 0) & (k1 == 1)
    print(f"[adversary edges] tied actions with different k*: {int(tie.sum())} of {len(pts)} points")
    assert tie.sum() >= 16 and (want[3][tie] == 0).all()
    dp = _dp(src, cuda_device)
    dp.set_disturbances(d)
    _query(dp, src, d, pts, "tied actions", want=want)
    _rollouts(dp, src, d, pts[:65], 7, "tied actions")
    dp.close()


# ---- non-finite and boundary states ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (2, 4, 6))
def test_non_finite_and_boundary_states(D, cuda_device):
    """The rows of infer_cases.special_starts — NaN, +-inf, the exact bounds and -0.0 in one coordinate, ordinary points in
    the same waves — and points up to 30 % beyond both bounds, as query points and as episode starts (1 and 5 steps)."""
    src = _source(D)
    d = _multi(src)
    cases = {}
    for m in (65, 257):                                      # the conditions, from the twin, before anything is launched
        starts, special = IC.special_starts(np.random.default_rng(m), src["lo"], src["hi"], m)
        assert all((special == IC.SPECIALS.index(s)).sum() >= D for s in IC.SPECIALS)
        want = _want(src, d, starts)
        assert (want[3][special < 0] >= 0).all(), "an ordinary point without a winner"
        runs = {steps: _rollout_wants(src, d, starts, steps) for steps in ((1, 5) if m == 65 else ())}
        for want_r in runs.get(5, {}).values():              # a NaN state stays in play beside ordinary episodes
            assert (want_r.lengths[np.isnan(starts).any(axis=1)] >= 1).any() and (want_r.lengths[special < 0] == 5).any()
        cases[m] = (starts, want, runs)
    beyond = _starts(src, 257, 70 + D)
    assert ((beyond < src["lo"]).any(axis=0) & (beyond > src["hi"]).any(axis=0)).all()
    dp = _dp(src, cuda_device)
    dp.set_disturbances(d)
    for m, (starts, want, runs) in cases.items():
        _query(dp, src, d, starts, f"{D}-D special m={m}", non_finite=True, want=want)
        for steps, wants in runs.items():
            _rollouts(dp, src, d, starts, steps, f"{D}-D special m={m}", non_finite=True, wants=wants)
    _query(dp, src, d, beyond, f"{D}-D beyond the bounds")
    _rollouts(dp, src, d, beyond[:65], 5, f"{D}-D beyond the bounds")
    dp.close()


# ---- non-finite V ---------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _poisoned_values(D):
    """The source's V with NaN on the lower third of dimension 0 and +inf, -inf and NaN at scattered nodes elsewhere."""
    src = _source(D)
    V = np.array(src["V"])
    first = np.unravel_index(np.arange(len(V)), src["shape"])[0]
    V[first < max(src["shape"][0] // 3, 2)] = np.nan
    rng = np.random.default_rng(23)
    at = rng.choice(len(V), size=3 * max(len(V) // 150, 6), replace=False).reshape(3, -1)
    for nodes, v in zip(at, (np.inf, -np.inf, np.nan)):
        V[nodes] = f32(v)
    V.setflags(write=False)
    return V


@pytest.mark.parametrize("D", (2, 4, 6))
def test_non_finite_values(D, cuda_device):
    """V with a NaN region and scattered +-inf and NaN nodes.  From the twin: at some query points every action's Q is NaN
    (best 0, Q = -1e30, worst -1) and at others an action wins; under the policy's action some start states fold a NaN
    that is not their first point (it has to be TAKEN) and some fold two (only the second NaN replaces the first), and
    there fminf would report another k* — the rollout under the policy controller moves by that point's dx."""
    src = _source(D)
    V = _poisoned_values(D)
    d = _multi(src)
    pts = _starts(src, 257, 80 + D)
    want = _want(src, d, pts, V)
    nothing = want[2] == f32(-1.0e30)
    assert np.isnan(want[4]).all(axis=1).any() and (want[0][nothing] == 0).all() and (want[3][nothing] == -1).all()
    with np.errstate(invalid="ignore"):                      # where nothing wins every Q is NaN or -inf
        assert (np.isnan(want[4][nothing]) | (want[4][nothing] <= f32(-1.0e30))).all()
    assert (~nothing).sum() > len(pts) // 4 and (want[3][~nothing] >= 0).all() and np.isinf(want[4]).any()
    with np.errstate(all="ignore"):
        a = B._interpolated_actions(pts, *src["tables"])
    q, Q, k = _fold_at(src, d, pts, a, V=V)
    nan = np.isnan(q)
    mixed = nan.any(axis=0) & ~nan.all(axis=0)
    pick = np.argsort(~mixed, kind="stable")[:65]            # the episodes: the points that fold NaN and numbers first
    starts, nan, k, q = np.ascontiguousarray(pts[pick]), nan[:, pick], k[pick], q[:, pick]
    assert (nan.any(axis=0) & ~nan[0]).any(), "no NaN that has to be taken"
    assert ((nan.sum(axis=0) >= 2) & ~nan.all(axis=0)).any() and nan.all(axis=0).any() and (~nan.any(axis=0)).any()
    assert (RC.fold(q, d.weights, "fmin")[1] != k).any()
    dp = _dp(src, cuda_device, V=V)
    dp.set_disturbances(d)
    _query(dp, src, d, pts, f"{D}-D non-finite V", V=V, non_finite=True, want=want)
    for steps in (1, 5):
        _rollouts(dp, src, d, starts, steps, f"{D}-D non-finite V", V=V, non_finite=True)
    dp.close()


# ---- one-cell and ragged grids, a permuted memory order -------------------------------------------------------------------
@pytest.mark.parametrize("env,shape", SHAPES, ids=["x".join(map(str, s)) for _, s in SHAPES])
def test_one_cell_and_ragged_grids(env, shape, cuda_device):
    """2 bins in every dimension (one cell) and the ragged shapes of tests/test_gpu_infer_edges.py; points outside the box
    on both sides; the multi-point set and the tie set whose rows are clamped to one border."""
    src = IC.source(env, shape, seed=20 + len(shape))
    pts = _starts(src, 257, 30 + len(shape))
    _, idx = B.get_barycentric_weights_and_indices(pts, *src["grid"], src["bits"])
    assert idx.min() == 0 and idx.max() == len(src["V"]) - 1
    dp = _dp(src, cuda_device)
    for label, d in (("multi", _multi(src)), ("clamped", _tie_sets(src)["clamped-to-one-border"])):
        dp.set_disturbances(d)
        want = _query(dp, src, d, pts, f"{shape} {label}")
        if label == "clamped":
            assert (want[3] <= 0).all() and (want[3] == 0).any()
        _rollouts(dp, src, d, pts[:65], 5, f"{shape} {label}")
    dp.close()


@pytest.mark.parametrize("D", (4, 6))
def test_value_table_on_a_permuted_memory_order(D, cuda_device):
    """V and the policy table laid out in another memory order of the dimensions, the strides to match; state offsets stay
    in the user's dimension order.  From the twin: read as row-major the same arrays give other answers."""
    src = _source(D, ORDERS[D])
    assert not np.array_equal(src["strides"], IC.row_major(src["shape"]))
    d = _multi(src)
    pts = _starts(src, 257, 40 + D)
    dp = _dp(src, cuda_device)
    dp.set_disturbances(d)
    want = _query(dp, src, d, pts, f"{D}-D order {ORDERS[D]}")
    res = _rollouts(dp, src, d, pts[:65], 5, f"{D}-D order {ORDERS[D]}")
    assert all((r.lengths == 5).any() for r in res.values())
    other = noise.robust_action(src["chk"].step, pts, d, src["V"], src["acts"], src["lo"], src["hi"], src["gshape"],
                                IC.row_major(src["shape"]), src["gamma"])
    # (measured 0.42 and 0.33 of the best Q, 0.17 and 0.18 of the best actions: the other points' steps are done or clamped)
    assert (other[2] != want[2]).mean() > 0.25 and (other[0] != want[0]).mean() > 0.1
    dp.close()


# ---- batch geometry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (2, 6))
def test_batch_geometry(D, cuda_device):
    """Query and episode batches of 1, 255, 256 and 257 (one lane, one short of a workgroup, exactly one, one lane of a
    second), 9 steps."""
    src = _source(D)
    d = _multi(src)
    dp = _dp(src, cuda_device)
    dp.set_disturbances(d)
    every = _starts(src, 257, 90 + D)
    for m in (1, 255, 256, 257):
        pts = np.ascontiguousarray(every[257 - m:])
        want = _query(dp, src, d, pts, f"{D}-D m={m}")
        assert len(want[0]) == m
        res = _rollouts(dp, src, d, pts, 9, f"{D}-D m={m}")
        assert all(r.trajectory.shape == (10, m, D) for r in res.values())
    dp.close()
