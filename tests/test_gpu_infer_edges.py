"""
The kernels of the inference handle (pi_infer_*) where the sweep kernels have long been tested and they had not: non-finite
and boundary states on the policy-table path, strides of a permuted memory order, permuted corner tables, one-cell and
ragged grids.  Every launch is compared with its numpy twin on the oracle's step — bit patterns, except that a NaN the
arithmetic GENERATES may differ in payload and sign between host and device (tests/infer_cases.py) — or, for the clamp,
with vectors the reference's own function produced (tests/golden/barycentric_edges.npz).  What a case exercised is asserted
from the twin or the fixture, never from the device result.  Nothing launches with an index that can leave a table: every
grid passes pi_infer_create's checks and every buffer is sized for its launch.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from dynamicprogramming_amd import envs, noise
from dynamicprogramming_amd.noise import Disturbances
from tests import helpers as H
from tests import infer_cases as IC
from utils import barycentric as B

pytestmark = pytest.mark.gpu
INF = np.inf
GAMMA = 0.9
SEED, FIRST = 2 ** 40 + 3, 2 ** 32 - 100                    # the episode numbers carry into the counter's high word
POLICY_KINDS = ("policy", "hybrid", "stochastic", "hybrid_stochastic")
ALL_KINDS = POLICY_KINDS + ("greedy", "expected")
# per D: env, primary shape, secondary shape, the secondary's box as a share of the primary's, its action table, and the
# switch box as shares of the primary's upper bounds (inf: the dimension takes no part)
GRIDS = {
    2: dict(env="pendulum", shape=(31, 29), shape2=(17, 13), acts2=np.linspace(-2.0, 2.0, 5, dtype=np.float32),
            enter=(0.4, 0.4), leave=(0.55, 0.6)),
    4: dict(env="cartpole", shape=(9, 8, 11, 7), shape2=(6, 5, 7, 5), acts2=np.array([-5.0, 0.0, 5.0], np.float32),
            enter=(INF, INF, 0.4, 0.4), leave=(INF, INF, 0.55, 0.6)),
    6: dict(env="double_cartpole", shape=(5, 4, 6, 4, 5, 4), shape2=(4, 3, 4, 3, 4, 3),
            acts2=np.array([-8.0, 0.0, 8.0], np.float32), enter=(INF, INF, 0.5, 0.5, 0.5, 0.5),
            leave=(INF, INF, 0.6, 0.7, 0.6, 0.7)),
}
ORDERS = {4: (2, 0, 3, 1), 6: (4, 2, 0, 5, 3, 1)}


def _pair(env, shape, shape2, acts2, enter, leave, order=None, order2=None, bits=None, bits2=None, seed=0):
    """dict(p, s, enter, leave, noise, dist): the primary source, the secondary on the inner 70 % of its box, the switch
    box and the noise every stochastic controller runs under."""
    p = IC.source(env, shape, order=order, seed=seed, bits=bits)
    box2 = ((p["lo"].astype(np.float64) * 0.7).astype(np.float32), (p["hi"].astype(np.float64) * 0.7).astype(np.float32))
    s = IC.source(env, shape2, order=order2, seed=seed + 1, box=box2, actions=acts2, bits=bits2)
    span = (p["hi"] - p["lo"]).astype(np.float64)
    a_span = float(p["acts"].max() - p["acts"].min())
    nz = dict(epsilon=0.25, action_noise=float(np.float32(0.1 * a_span)), state_noise=(0.01 * span).astype(np.float32),
              seed=SEED, first_episode=FIRST)
    dist = Disturbances.uniform(p["D"], action_noise=0.1 * a_span, points=2)
    assert dist.K == 2
    return dict(p=p, s=s, enter=(np.asarray(enter) * p["hi"]).astype(np.float32),
                leave=(np.asarray(leave) * p["hi"]).astype(np.float32), noise=nz, dist=dist)


@lru_cache(maxsize=None)
def _grid_pair(D):
    g = GRIDS[D]
    return _pair(g["env"], g["shape"], g["shape2"], g["acts2"], g["enter"], g["leave"])


def _policy_handle(src, dev, bits=None):
    return B.DevicePolicy(src["policy"], src["acts"], src["lo"], src["hi"], src["gshape"], src["strides"],
                          src["bits"] if bits is None else bits, device=dev)


def _controller(kind, c, dev):
    """(device rollout, numpy twin, handles to close) of one controller on the pair c; both take (starts, steps, every)."""
    p, s, nz = c["p"], c["s"], c["noise"]
    step, kw = p["chk"].step, dict(gamma=GAMMA)
    dp = _policy_handle(p, dev)
    dp.set_dynamics(envs.dynamics_source(p["env"]))
    handles = [dp]
    if kind == "policy":
        return (lambda x, n, e: dp.rollout(x, n, record_every=e, **kw),
                lambda x, n, e: B.rollout(step, x, n, *p["tables"], record_every=e, **kw), handles)
    if kind == "stochastic":
        dp.set_stochastic()
        return (lambda x, n, e: dp.rollout(x, n, record_every=e, **kw, **nz),
                lambda x, n, e: B.stochastic_rollout(step, x, n, *p["tables"], nz["epsilon"], nz["action_noise"],
                                                     nz["state_noise"], nz["seed"], first_episode=nz["first_episode"],
                                                     record_every=e, **kw), handles)
    if kind in ("hybrid", "hybrid_stochastic"):
        dp2 = _policy_handle(s, dev)
        handles.append(dp2)
        hp = B.HybridPolicy(dp, dp2, c["enter"], c["leave"])
        if kind == "hybrid":
            return (lambda x, n, e: hp.rollout(x, n, record_every=e, **kw),
                    lambda x, n, e: B.hybrid_rollout(step, x, n, p["tables"], s["tables"], c["enter"], c["leave"],
                                                     record_every=e, **kw), handles)
        return (lambda x, n, e: hp.rollout(x, n, record_every=e, **kw, **nz),
                lambda x, n, e: B.stochastic_hybrid_rollout(step, x, n, p["tables"], s["tables"], c["enter"], c["leave"],
                                                            p["acts"], nz["epsilon"], nz["action_noise"], nz["state_noise"],
                                                            nz["seed"], first_episode=nz["first_episode"], record_every=e,
                                                            **kw), handles)
    dp.set_values(p["V"])
    if kind == "greedy":
        dp.set_greedy()
        return (lambda x, n, e: dp.rollout(x, n, record_every=e, controller="greedy", lookahead_gamma=p["gamma"], **kw),
                lambda x, n, e: B.greedy_rollout(step, x, n, p["V"], p["acts"], *p["grid"], p["gamma"], record_every=e, **kw),
                handles)
    assert kind == "expected"
    dp.set_expected_greedy()
    dp.set_disturbances(c["dist"])
    return (lambda x, n, e: dp.rollout(x, n, record_every=e, controller="expected", lookahead_gamma=p["gamma"], **kw, **nz),
            lambda x, n, e: noise.expected_greedy_rollout(step, x, n, c["dist"], p["V"], p["acts"], *p["grid"], p["gamma"],
                                                          record_every=e, **kw, **nz), handles)


def _twin_quiet(twin, *args):
    with np.errstate(all="ignore"):
        return twin(*args)


def _assert_lookahead(got, want, what):
    """(best, action, q_best, Q) of a lookahead query: NaN positions of Q equal, bit patterns elsewhere."""
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), f"{what}: greedy indices"
    H.assert_bits_equal(got[1], want[1], f"{what}: action value")
    IC.assert_bits_equal_but_nan(got[2], want[2], f"{what}: best Q")
    IC.assert_bits_equal_but_nan(got[3], want[3], f"{what}: Q matrix")


def _queries_and_resample(c, dev, pts, what, bits=None):
    """The query, both lookahead queries and the resample with c's primary as the source, each against its twin given the
    same strides (and corner table)."""
    torch = __import__("torch")
    p = c["p"]
    bits = p["bits"] if bits is None else bits
    step = p["chk"].step
    dp = _policy_handle(p, dev, bits)
    w, idx = dp.weights_and_indices(pts)
    wn, idxn = B.get_barycentric_weights_and_indices(pts, p["lo"], p["hi"], p["gshape"], p["strides"], bits)
    assert np.array_equal(idx, idxn), f"{what}: indices"
    H.assert_bits_equal(w, wn, f"{what}: weights")
    H.assert_bits_equal(dp(pts), IC.ascending_sum(wn, idxn, p["policy"], p["acts"]), f"{what}: action")
    dp.set_dynamics(envs.dynamics_source(p["env"]))
    dp.set_values(p["V"])
    dp.set_greedy()
    dp.set_expected_greedy()
    dp.set_disturbances(c["dist"])
    with np.errstate(all="ignore"):
        want_g = B.greedy_action(step, pts, p["V"], p["acts"], *p["grid"], p["gamma"], q_values=True)
        want_e = noise.expected_greedy_action(step, pts, c["dist"], p["V"], p["acts"], *p["grid"], p["gamma"], q_values=True)
    got_g, got_e = dp.greedy(pts, p["gamma"], q_values=True), dp.expected_greedy(pts, p["gamma"], q_values=True)
    _assert_lookahead(got_g, want_g, f"{what}: greedy query")
    _assert_lookahead(got_e, want_e, f"{what}: expected-greedy query")
    # resample: a destination that reaches beyond the source's box on both sides, 3 bins per dimension but 4 in the last
    dst_shape = (3,) * (p["D"] - 1) + (4,)
    bins = [np.linspace(1.2 * l, 1.2 * h, g).astype(np.float32) for l, h, g in zip(p["lo"], p["hi"], dst_shape)]
    n = int(np.prod(dst_shape))
    out_V = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    out_P = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dp.resample(bins, IC.row_major(dst_shape).astype(np.int64), None, out_V, out_P)
    want_V, want_P = B.resample(p["V"], p["policy"], p["lo"], p["hi"], p["gshape"], p["strides"], bits, bins)
    H.assert_bits_equal(out_V.cpu().numpy(), want_V, f"{what}: resampled V")
    assert np.array_equal(out_P.cpu().numpy(), want_P), f"{what}: resampled policy"
    dp.close()
    return got_g, got_e


# ── a. the query on the reference's edge vectors ─────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("key", IC.EDGE_GRIDS)
def test_query_equals_the_reference_on_the_edge_vectors(key, cuda_device):
    """Indices equal, weights bit-equal to the reference's (zero signs included, no NaN), the action bit-equal to the
    ascending-corner float32 sum over the reference's weights and indices."""
    v = IC.edge_vectors()[0][key]
    dp = B.DevicePolicy(v["policy"], v["actions"], *IC.grid_of(v), device=cuda_device)
    w, idx = dp.weights_and_indices(v["points"])
    assert idx.dtype == np.int32 and np.array_equal(idx, v["indices"]), key
    H.assert_bits_equal(w, v["weights"], f"{key}: device weights against the reference's")
    act = dp(v["points"])
    assert not np.isnan(act).any()
    H.assert_bits_equal(act, IC.ascending_sum(v["weights"], v["indices"], v["policy"], v["actions"]), f"{key}: device action")
    dp.close()


# ── b. non-finite and boundary starts under the four policy-table controllers ────────────────────────────────────────────
@pytest.mark.parametrize("D", (2, 4, 6))
@pytest.mark.parametrize("kind", POLICY_KINDS)
def test_rollouts_from_non_finite_and_boundary_states(kind, D, cuda_device):
    """NaN, +-inf, the exact bounds and -0.0 in one coordinate of the start, ordinary episodes in the same waves: batches
    of 65 and 257, 1 and 5 steps, every state recorded."""
    c = _grid_pair(D)
    p = c["p"]
    device, twin, handles = _controller(kind, c, cuda_device)
    for m in (65, 257):
        starts, special = IC.special_starts(np.random.default_rng(m), p["lo"], p["hi"], m)
        for steps in (1, 5):
            want = _twin_quiet(twin, starts, steps, 1)
            got = device(starts, steps, 1)
            what = f"{kind} {D}-D m={m} steps={steps}"
            IC.assert_same_rollout(got, want, what)
            assert got.trajectory.shape == (steps + 1, m, D)
            # from the twin alone: an episode acted on its policy table from a NaN state, and one from an infinite state
            acted = want.lengths >= 1
            if "stochastic" in kind:                         # an exploring step does not read the table
                words = B.random_words(SEED, FIRST, m, 0, 0)
                acted &= (words[:, 0] >> np.uint32(8)) >= B.explore_threshold(c["noise"]["epsilon"])
            assert (acted & np.isnan(starts).any(axis=1)).any() and (acted & np.isinf(starts).any(axis=1)).any(), what
            for name in ("lo", "hi", "zero_neg"):
                assert (acted & (special == IC.SPECIALS.index(name))).any(), (what, name)
            assert (acted & (special < 0)).sum() > m // 4, what
        if steps == 5:
            # a NaN state stays in play: some episode acts from a state the dynamics made non-finite, too
            later = ~np.isfinite(want.trajectory[1:steps]).all(axis=2) & (want.lengths[None, :] > np.arange(1, steps)[:, None])
            assert later.any(), what
    if kind.startswith("hybrid"):
        assert 0 < (want.secondary_steps > 0).sum() < m, f"{kind} {D}-D: both modes"
    for h in handles:
        h.close()


# ── c. the resample on the zero-bounded sources, onto nodes that are zeros of either sign ────────────────────────────────
@pytest.mark.parametrize("key", IC.ZERO_GRIDS)
def test_resample_onto_signed_zero_and_non_finite_nodes(key, cuda_device, monkeypatch):
    """A destination whose bin tables hold -0.0 and +0.0 nodes, nodes beyond the source's box, NaN and +-inf, from the
    sources whose bounds are exact zeros."""
    torch = __import__("torch")
    v = IC.edge_vectors()[0][key]
    D, n_src = v["D"], int(np.prod(v["gshape"]))
    V = (np.random.default_rng(5).standard_normal(n_src) * 30.0).astype(np.float32)
    bins = []
    for d in range(D):
        # ascending: beyond both bounds, the bounds, the middle, and both zeros where 0 sorts; then the nodes a
        # destination can hold that no source box contains: NaN (lands on the source's lower bound) and +-inf
        l, h = float(v["lo"][d]), float(v["hi"][d])
        finite = np.array(sorted({l - 1.0, l, h, h + 1.0, 0.5 * (l + h)} - {0.0}), np.float32)
        at = int(np.searchsorted(finite, 0.0))
        bins.append(np.concatenate([finite[:at], [-0.0, 0.0], finite[at:], [np.nan, np.inf, -np.inf]]).astype(np.float32))
        zero = bins[-1] == 0
        assert (zero & np.signbit(bins[-1])).sum() == 1 and (zero & ~np.signbit(bins[-1])).sum() == 1
    shape = [len(b) for b in bins]
    n = int(np.prod(shape))
    dp = B.DevicePolicy(v["policy"], v["actions"], *IC.grid_of(v), device=cuda_device)
    dp.set_values(V)
    out_V = torch.full((n,), float("nan"), dtype=torch.float32, device=cuda_device)
    out_P = torch.full((n,), -7, dtype=torch.int32, device=cuda_device)
    dp.resample(bins, IC.row_major(shape).astype(np.int64), None, out_V, out_P)
    want_V, want_P = B.resample(V, v["policy"], *IC.grid_of(v), bins)
    H.assert_bits_equal(out_V.cpu().numpy(), want_V, f"{key}: resampled V")
    assert np.array_equal(out_P.cpu().numpy(), want_P), f"{key}: resampled policy"
    # from the twin alone: no NaN comes out although NaN nodes went in, and the clamp matters to the result — with the
    # former one (a NaN coordinate to the UPPER bound, as fminf / fmaxf send it) the twin gives other values
    assert not np.isnan(want_V).any()
    with monkeypatch.context() as mp:
        mp.setattr(B, "_clamp_point", lambda x, lo, hi: np.fmax(lo, np.fmin(x, hi)))
        other_V, _ = B.resample(V, v["policy"], *IC.grid_of(v), bins)
    assert (other_V.view(np.uint32) != want_V.view(np.uint32)).sum() > n // 10
    dp.close()


# ── d. strides of a permuted memory order, permuted corner tables ────────────────────────────────────────────────────────
@lru_cache(maxsize=None)
def _permuted_pair(D, corner_perm):
    g = GRIDS[D]
    rng = np.random.default_rng(40 + D)
    bits = IC.corner_bits(D)[rng.permutation(1 << D)] if corner_perm else None
    bits2 = bits                                             # a hybrid walks ONE corner order on both grids (checked by the library)
    order2 = tuple(reversed(ORDERS[D]))
    c = _pair(g["env"], g["shape"], g["shape2"], g["acts2"], g["enter"], g["leave"], order=ORDERS[D], order2=order2,
              bits=bits, bits2=bits2, seed=7)
    assert not np.array_equal(c["p"]["strides"], IC.row_major(g["shape"]))
    assert not np.array_equal(c["s"]["strides"], IC.row_major(g["shape2"]))
    return c


def _starts(c, m, seed):
    """m starts over the primary's box stretched by 1.3: points outside on both sides in every dimension."""
    p = c["p"]
    x = IC.ordinary_starts(np.random.default_rng(seed), p["lo"], p["hi"], m, spread=1.3)
    assert ((x < p["lo"]).any(axis=0) & (x > p["hi"]).any(axis=0)).all()
    return x


@pytest.mark.parametrize("D", (4, 6))
def test_every_kernel_on_strides_of_a_permuted_memory_order(D, cuda_device):
    """Query, the six rollouts, both lookahead queries and the resample on sources whose tables lie in a permuted memory
    order (the partner of the hybrids in another one), each against its twin given the same strides."""
    c = _permuted_pair(D, False)
    starts = _starts(c, 257, D)
    _queries_and_resample(c, cuda_device, starts, f"{D}-D order {ORDERS[D]}")
    for kind in ALL_KINDS:
        device, twin, handles = _controller(kind, c, cuda_device)
        want = _twin_quiet(twin, starts, 5, 1)
        IC.assert_same_rollout(device(starts, 5, 1), want, f"{kind} {D}-D order {ORDERS[D]}")
        assert (want.lengths == 5).any()
        for h in handles:
            h.close()
    # the strides matter: the twin on the same arrays read as row-major gives other actions
    p = c["p"]
    w, idx = B.get_barycentric_weights_and_indices(starts, p["lo"], p["hi"], p["gshape"], p["strides"], p["bits"])
    _, idx_rm = B.get_barycentric_weights_and_indices(starts, p["lo"], p["hi"], p["gshape"], IC.row_major(p["shape"]), p["bits"])
    assert (IC.ascending_sum(w, idx, p["policy"], p["acts"]) != IC.ascending_sum(w, idx_rm, p["policy"], p["acts"])).mean() > 0.5


@pytest.mark.parametrize("D", (4, 6))
def test_permuted_corner_tables_under_the_rollouts_and_ignored_by_the_lookaheads(D, cuda_device):
    """The four policy-table rollouts with a permuted corner table (both handles of a hybrid share it, as the library
    demands) on permuted strides; and the documented fact that the lookaheads ignore corner_bits: the same greedy and expected-greedy
    bits as with the natural table."""
    c = _permuted_pair(D, True)
    natural = _permuted_pair(D, False)
    assert not np.array_equal(c["p"]["bits"], natural["p"]["bits"]) and np.array_equal(c["p"]["policy"], natural["p"]["policy"])
    starts = _starts(c, 257, 10 + D)
    for kind in POLICY_KINDS:
        device, twin, handles = _controller(kind, c, cuda_device)
        IC.assert_same_rollout(device(starts, 5, 1), _twin_quiet(twin, starts, 5, 1), f"{kind} {D}-D permuted corners")
        for h in handles:
            h.close()
    a_g, a_e = _queries_and_resample(c, cuda_device, starts, f"{D}-D permuted corners", bits=c["p"]["bits"])
    b_g, b_e = _queries_and_resample(natural, cuda_device, starts, f"{D}-D natural corners")
    for a, b, name in ((a_g, b_g, "greedy"), (a_e, b_e, "expected-greedy")):
        for x, y in zip(a, b):
            IC.assert_bits_equal_but_nan(x, y, f"{D}-D {name}: the lookahead ignores corner_bits")


# ── e. one-cell and ragged grids ──────────────────────────────────────────────────────────────────────────────────────────
SHAPES = [("pendulum", (2, 2)), ("cartpole", (2, 2, 2, 2)), ("double_cartpole", (2,) * 6), ("pendulum", (2, 2047)),
          ("pendulum", (2047, 2)), ("cartpole", (257, 2, 3, 2))]


@pytest.mark.parametrize("env,shape", SHAPES, ids=["x".join(map(str, s)) for _, s in SHAPES])
def test_every_kernel_on_one_cell_and_ragged_grids(env, shape, cuda_device):
    """2 bins in every dimension (one cell: base index 0 everywhere) and ragged shapes; the hybrids' partner is the
    one-cell grid of the same D.  Starts include points outside the box on both sides."""
    D = len(shape)
    g = GRIDS[D]
    c = _pair(env, shape, (2,) * D, g["acts2"], g["enter"], g["leave"], seed=20 + D)
    starts = _starts(c, 257, 30 + D)
    p = c["p"]
    _, idx = B.get_barycentric_weights_and_indices(starts, *p["grid"], p["bits"])
    if set(shape) == {2}:
        assert (idx.min(axis=1) == 0).all() and (idx.max(axis=1) == len(p["policy"]) - 1).all()
    else:
        assert idx.max() == len(p["policy"]) - 1 and idx.min() == 0
    _queries_and_resample(c, cuda_device, starts, f"{shape}")
    for kind in ALL_KINDS:
        device, twin, handles = _controller(kind, c, cuda_device)
        IC.assert_same_rollout(device(starts, 5, 1), _twin_quiet(twin, starts, 5, 1), f"{kind} {shape}")
        for h in handles:
            h.close()
