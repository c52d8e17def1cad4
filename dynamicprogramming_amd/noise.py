"""
Noise-aware solving: disturbance sets and the numpy twins of the expectation and the worst-case sweeps.

The solvers back up the single deterministic successor, ``Q(s, a) = r + gamma * E[V](f(s, a))``.  With a
``Disturbances`` set installed (``solver.set_disturbances``) every sweep takes the expectation over K points instead,

    ``Q(s, a) = sum_k p_k * [ r_k + gamma * E[V](f(s, a (+) da_k) + dx_k) ]``

on the device (csrc/pi_expect_kernels.hip; include/pi_mi355.h at ``pi_set_disturbances`` is the definition).  The
functions below restate that definition in numpy, bit for bit, on any batched ``step`` callable — the one
``utils.barycentric.rollout`` takes: ``step(states (m, D), actions (m,)) -> (next (m, D), reward (m,), done (m,))``.

With ``risk="worst"`` the same functions restate the worst-case sweeps (``solver.set_disturbances(d, risk="worst")``,
``pi_robust_*``): ``Q(s, a) = min_k [...]`` over the points of weight != 0, folded with comparisons.

Expected-value greedy control closes the loop: ``expected_greedy_action`` is the one-step lookahead ``argmax_a Q(s, a)``
with that expectation inside it at arbitrary continuous states, ``expected_greedy_rollout`` the closed loop under it with
the noise of the stochastic rollouts — the twins of ``DevicePolicy.expected_greedy`` and
``DevicePolicy.rollout(controller="expected")`` (csrc/pi_expect_greedy_kernels.hip), same bits.
"""
from __future__ import annotations

import numpy as np

from utils.barycentric import _expected_value, _fmaf, _noisy_closed_loop

MAX_POINTS = 64


class Disturbances:
    """K disturbance points: ``action_offsets`` (K,) or None = zeros, ``state_offsets`` (K, D) in the order of
    ``step_dynamics``' arguments, ``weights`` (K,).  float32 throughout.  Validated as the library validates them:
    1 <= K <= 64, every value finite, weights >= 0 and ``|sum - 1| <= 1e-4`` with the sum in float64."""

    def __init__(self, action_offsets, state_offsets, weights):
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        K = len(w)
        if not 1 <= K <= MAX_POINTS:
            raise ValueError(f"a disturbance set holds 1 to {MAX_POINTS} points, not {K}")
        dx = np.ascontiguousarray(state_offsets, dtype=np.float32)
        if dx.ndim != 2 or len(dx) != K:
            raise ValueError(f"state_offsets must be (K, D) = ({K}, D), not {dx.shape}")
        da = np.zeros(K, np.float32) if action_offsets is None else np.ascontiguousarray(action_offsets, dtype=np.float32).ravel()
        if len(da) != K:
            raise ValueError(f"action_offsets must hold K = {K} values, not {len(da)}")
        if not (np.isfinite(w).all() and np.isfinite(dx).all() and np.isfinite(da).all()):
            raise ValueError("disturbance offsets and weights must be finite")
        if (w < 0).any():
            raise ValueError("disturbance weights must be >= 0")
        total = float(w.astype(np.float64).sum())
        if not abs(total - 1.0) <= 1e-4:
            raise ValueError(f"disturbance weights must sum to 1 within 1e-4, not to {total!r}")
        self.action_offsets, self.state_offsets, self.weights = da, dx, w

    @property
    def K(self) -> int:
        return len(self.weights)

    @property
    def D(self) -> int:
        return self.state_offsets.shape[1]

    def table(self) -> np.ndarray:
        """(K, D + 2) float32: columns da, dx_0 .. dx_{D-1}, p — the form ``save()`` archives."""
        return np.ascontiguousarray(np.column_stack([self.action_offsets, self.state_offsets, self.weights]), dtype=np.float32)

    @classmethod
    def from_table(cls, table) -> "Disturbances":
        t = np.asarray(table, dtype=np.float32)
        return cls(t[:, 0], t[:, 1:-1], t[:, -1])

    @classmethod
    def none(cls, D: int) -> "Disturbances":
        """The one-point zero set: the expectation sweeps then compute the deterministic backup, bit for bit."""
        return cls(None, np.zeros((1, int(D)), np.float32), [1.0])

    @classmethod
    def uniform(cls, D: int, state_noise=None, action_noise: float = 0.0, points: int = 3) -> "Disturbances":
        """The tensor Gauss-Legendre rule for the noise model of the stochastic rollouts — ``X * u``, u uniform on
        [-1, 1), per noisy dimension and for the action: ``points`` nodes ``X * x_i`` (ascending) with weights
        ``w_i / 2`` per noisy quantity.  ``state_noise``: None, one value for every dimension, or D values; a zero takes no
        part.  The action is the slowest index and the last noisy dimension the fastest, so points with equal action
        offsets are contiguous (the kernels step the dynamics once for them).  Weights are float32 of the float64
        product.  ValueError when the rule has more than 64 points."""
        D, points = int(D), int(points)
        if points < 1:
            raise ValueError("points must be >= 1")
        noise = np.zeros(1) if state_noise is None else np.asarray(state_noise, np.float64).ravel()
        if len(noise) not in (1, D):
            raise ValueError(f"state_noise must hold one value or D = {D} values")
        noise = np.broadcast_to(noise, (D,))
        A = float(action_noise)
        if not (np.isfinite(noise).all() and (noise >= 0).all() and np.isfinite(A) and A >= 0):
            raise ValueError("noise amplitudes must be finite and >= 0")
        axes = ([("a", A)] if A != 0.0 else []) + [(d, float(noise[d])) for d in range(D) if noise[d] != 0.0]
        K = points ** len(axes)
        if K > MAX_POINTS:
            raise ValueError(f"{points} points over {len(axes)} noisy quantities are {K} disturbance points: more than {MAX_POINTS}")
        x, w = np.polynomial.legendre.leggauss(points)
        da, dx, p = np.zeros(K, np.float64), np.zeros((K, D), np.float64), np.ones(K, np.float64)
        idx = np.indices((points,) * len(axes)).reshape(len(axes), K) if axes else np.zeros((0, 1), int)
        for j, (which, amp) in enumerate(axes):
            if which == "a":
                da = amp * x[idx[j]]
            else:
                dx[:, which] = amp * x[idx[j]]
            p = p * (w[idx[j]] / 2.0)
        return cls(da.astype(np.float32), dx.astype(np.float32), p.astype(np.float32))


def _tables(action_space, bounds_low, bounds_high, grid_shape, strides):
    acts = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
    return acts, (np.asarray(bounds_low, np.float32), np.asarray(bounds_high, np.float32),
                  np.asarray(grid_shape, np.int32), np.asarray(strides, np.int32))


RISKS = ("expected", "worst")


def _check_risk(risk):
    if risk not in RISKS:
        raise ValueError(f"risk must be 'expected' or 'worst', not {risk!r}")
    return risk == "worst"


def expected_q(step, states, actions, disturbances, value_function, action_space, bounds_low, bounds_high, grid_shape,
               strides, gamma, risk="expected", worst_point=False):
    """``Q(s, a)`` of the module docstring for ``states`` (m, D) and action VALUES ``actions`` (m,) or a scalar; float32
    (m,).  Per point in ascending k: ``a_k = a`` when ``da_k == 0``, else ``fmin(fmax(a + da_k, a_min), a_max)`` with
    the extremes of ``action_space``; ``(s', r, done) = step(s, a_k)`` (a point with the ``da`` of the one before it keeps
    that point's step, as on the device); ``E = 0`` where done, elsewhere ``dx_k`` is added
    to ``s'`` in every dimension where it is not zero and ``E`` is ``utils.barycentric._expected_value`` there;
    ``q = r + gamma * E``; ``Q = p_0 * q_0``, then ``Q = fmaf(p_k, q_k, Q)``.

    ``risk="worst"``: the WORST-CASE fold of ``pi_robust_eval_sweeps`` instead of the last step.  A point of weight 0 takes
    no part, as if it were not in the set (it neither starts nor breaks a run of equal ``da``); the first participating
    point gives ``Q = q_k`` and ``k* = k``, every later one replaces both where ``q_k < Q`` or ``q_k`` is NaN — strict, so
    the first of equal points stays and -0 does not replace +0, and only a NaN replaces a NaN.  ``worst_point=True``
    (that mode only) returns ``(Q, k*)``, ``k*`` int32 (m,) an index into the set."""
    worst = _check_risk(risk)
    if worst_point and not worst:
        raise ValueError("worst_point=True belongs to risk='worst'")
    pts = np.ascontiguousarray(np.atleast_2d(states), dtype=np.float32)
    m = len(pts)
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(actions, np.float32), (m,)))
    acts, grid = _tables(action_space, bounds_low, bounds_high, grid_shape, strides)
    a_min, a_max = acts.min(), acts.max()
    g32 = np.float32(gamma)
    Q = np.zeros(m, np.float32)
    k_star = np.zeros(m, np.int32)
    da_prev = None                                                   # no participating point yet
    for k in range(disturbances.K):
        if worst and disturbances.weights[k] == 0:
            continue
        da = disturbances.action_offsets[k]
        if da_prev is None or da != da_prev:                         # equal consecutive offsets share the step, as on the device
            ak = a if da == 0 else np.fmin(np.fmax(a + da, a_min), a_max)
            nxt, rew, done = step(pts, ak)
            nxt, done = np.asarray(nxt, np.float32), np.asarray(done, bool)
        e = np.zeros(m, np.float32)
        if not done.all():
            p = nxt[~done].copy()
            for d in range(pts.shape[1]):
                dx = disturbances.state_offsets[k, d]
                if dx != 0:
                    p[:, d] = p[:, d] + dx
            e[~done] = _expected_value(p, value_function, *grid)
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.asarray(rew, np.float32) + g32 * e
            if worst:
                take = np.ones(m, bool) if da_prev is None else (q < Q) | (q != q)
                Q = np.where(take, q, Q)
                k_star = np.where(take, np.int32(k), k_star)
            else:
                Q = disturbances.weights[k] * q if k == 0 else _fmaf(disturbances.weights[k], q, Q)
        da_prev = da
    return (Q, k_star) if worst_point else Q


def _range(n, s_begin, s_end, term):
    s_end = n if s_end is None else int(s_end)
    live = np.arange(int(s_begin), s_end)
    return live if term is None else live[~np.asarray(term, bool)[live]], s_end


def _residual(new, old):
    """max |new - old| as the kernels fold it: from 0, a NaN never raises it; a difference beyond float32 is inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(new - old)
    return np.float32(np.fmax.reduce(d, initial=np.float32(0.0))) if len(d) else np.float32(0.0)


def expected_eval(step, states, policy, value_function, term, disturbances, action_space, bounds_low, bounds_high,
                  grid_shape, strides, gamma, s_begin=0, s_end=None, out=None, risk="expected"):
    """One expectation evaluation sweep over the grid nodes ``states`` (n, D) in [s_begin, s_end):
    ``V'(s) = Q(s, action_space[policy[s]])``, terminal states (``term``, or None for none) copy their value.  Returns
    ``(V', residual)``: V' is ``out`` (or a copy of V) with the range written, the residual ``max |V' - V|`` over it.
    ``risk="worst"``: Q is the minimum over the set (``expected_q``), the sweep of ``pi_robust_eval_sweeps``."""
    _check_risk(risk)
    V = np.asarray(value_function, np.float32).ravel()
    new = V.copy() if out is None else out
    live, s_end = _range(len(V), s_begin, s_end, term)
    acts = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
    new[s_begin:s_end] = V[s_begin:s_end]
    if len(live):
        new[live] = expected_q(step, states[live], acts[np.asarray(policy)[live]], disturbances, V, acts, bounds_low,
                               bounds_high, grid_shape, strides, gamma, risk=risk)
    return new, _residual(new[s_begin:s_end], V[s_begin:s_end])


def _argmax(step, states, live, disturbances, V, acts, grid, gamma, risk="expected"):
    best = np.zeros(len(live), np.int32)
    best_q = np.full(len(live), np.float32(-1.0e30), np.float32)
    for a, u in enumerate(acts):
        q = expected_q(step, states[live], u, disturbances, V, acts, *grid, gamma, risk=risk)
        with np.errstate(invalid="ignore"):
            wins = q > best_q
        best_q = np.where(wins, q, best_q)
        best = np.where(wins, np.int32(a), best)
    return best, best_q


def expected_improve(step, states, policy, value_function, term, disturbances, action_space, bounds_low, bounds_high,
                     grid_shape, strides, gamma, s_begin=0, s_end=None, risk="expected"):
    """One expectation improvement sweep over [s_begin, s_end): ``policy[s] = argmax_a Q(s, a)``, strict ``>`` from
    -1e30 over ascending action indices; terminal states keep their entry.  Returns ``(policy', entries changed)``.
    ``risk="worst"``: the max-min improvement of ``pi_robust_improve_sweep``."""
    _check_risk(risk)
    V = np.asarray(value_function, np.float32).ravel()
    new = np.array(policy, dtype=np.int32, copy=True)
    live, _ = _range(len(V), s_begin, s_end, term)
    acts, grid = _tables(action_space, bounds_low, bounds_high, grid_shape, strides)
    if len(live):
        new[live], _ = _argmax(step, states, live, disturbances, V, acts, grid, gamma, risk)
    return new, int((new != np.asarray(policy)).sum())


def expected_value_sweep(step, states, policy, value_function, term, disturbances, action_space, bounds_low, bounds_high,
                         grid_shape, strides, gamma, s_begin=0, s_end=None, out=None, risk="expected"):
    """One expectation value-iteration sweep over [s_begin, s_end): ``expected_improve`` and ``V'(s) = max_a Q(s, a)`` at
    once (terminal states copy their value and keep their entry).  Returns ``(V', policy', residual, entries changed)``.
    ``risk="worst"``: the max-min backup of ``pi_robust_value_sweep``."""
    _check_risk(risk)
    V = np.asarray(value_function, np.float32).ravel()
    new_v = V.copy() if out is None else out
    new_p = np.array(policy, dtype=np.int32, copy=True)
    live, s_end = _range(len(V), s_begin, s_end, term)
    acts, grid = _tables(action_space, bounds_low, bounds_high, grid_shape, strides)
    new_v[s_begin:s_end] = V[s_begin:s_end]
    if len(live):
        new_p[live], new_v[live] = _argmax(step, states, live, disturbances, V, acts, grid, gamma, risk)
    return new_v, new_p, _residual(new_v[s_begin:s_end], V[s_begin:s_end]), int((new_p != np.asarray(policy)).sum())


def expected_greedy_action(step, points, disturbances, value_function, action_space, bounds_low, bounds_high, grid_shape,
                           strides, gamma, q_values=False):
    """The greedy one-step lookahead with the expectation over ``disturbances`` inside it, at ``points`` (m, D) (numpy):
    the twin of ``DevicePolicy.expected_greedy``, same bits.  For every action of ``action_space`` in ascending order
    ``Q = expected_q(points, action)``; the argmax is ``utils.barycentric.greedy_action``'s — strict ``>`` from -1e30, the
    lowest index wins ties, NaN never wins, index 0 with Q = -1e30 when nothing wins.  With ``Disturbances.none(D)`` it is
    ``greedy_action``, bit for bit.  Returns ``(best_index int32, action float32, q_best float32)`` and, with
    ``q_values=True``, ``Q (m, n_actions)`` float32."""
    pts = np.ascontiguousarray(np.atleast_2d(points), dtype=np.float32)
    acts, grid = _tables(action_space, bounds_low, bounds_high, grid_shape, strides)
    m = len(pts)
    best = np.zeros(m, np.int32)
    best_q = np.full(m, np.float32(-1.0e30), np.float32)
    Q = np.empty((m, len(acts)), np.float32)
    for a, u in enumerate(acts):
        q = expected_q(step, pts, u, disturbances, value_function, acts, *grid, gamma) if m else np.zeros(0, np.float32)
        with np.errstate(invalid="ignore"):
            wins = q > best_q
        Q[:, a] = q
        best_q = np.where(wins, q, best_q)
        best = np.where(wins, np.int32(a), best)
    out = (best, acts[best], best_q)
    return out + (Q,) if q_values else out


def expected_greedy_rollout(step, states, steps, disturbances, value_function, action_space, bounds_low, bounds_high,
                            grid_shape, strides, lookahead_gamma, gamma=1.0, record_every=0, epsilon=0.0, action_noise=0.0,
                            state_noise=None, seed=0, first_episode=0):
    """Closed-loop episodes under the expected-value greedy controller on the CPU (numpy): the twin of
    ``DevicePolicy.rollout(controller="expected")``, same bits.  It is ``utils.barycentric.stochastic_rollout`` with the
    action value ``expected_greedy_action`` returns for the state (discount ``lookahead_gamma``) in place of the
    interpolated one.  Per step of a running episode, in this order: the lookahead; an exploring step (block 0 of the
    episode's stream: ``(x0 >> 8) < explore_threshold(epsilon)``) takes ``action_space[random_action_index(x1)]``
    instead; ``action_noise != 0`` adds ``action_noise * sym(x2)`` and clamps to the extremes of ``action_space``;
    ``step`` with the action finally taken; then, unless the step was `done`, every dimension with ``state_noise[d] !=
    0`` of the successor gains ``state_noise[d] * sym(word d)`` (block 1 for d < 4, block 2 for d = 4, 5).  The draws are
    ``stochastic_rollout``'s — the same counters — so both controllers can be run under common random numbers.  The
    bookkeeping, ``gamma`` and ``record_every`` are ``rollout``'s.  Returns a ``RolloutResult`` of numpy arrays."""
    acts = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
    tables = (disturbances, value_function, acts, bounds_low, bounds_high, grid_shape, strides, lookahead_gamma)

    def controller(pts, wanted):                      # an exploring episode is not looked ahead for
        a = np.zeros(len(pts), np.float32)
        if wanted.any():
            a[wanted] = expected_greedy_action(step, pts[wanted], *tables)[1]
        return a
    return _noisy_closed_loop(step, states, steps, controller, acts, epsilon, action_noise, state_noise, seed,
                              first_episode, gamma, record_every)


# ── the robust lookahead and the adversary in the closed loop (csrc/pi_adversary_kernels.hip), same bits ────────────────
def _adversary_fold(step, pts, a, disturbances, value_function, acts, grid, gamma):
    """The worst-case fold of ``expected_q(risk="worst")`` at ``pts`` under the action values ``a`` that also keeps what the
    adversary's point does to the episode: ``(Q, k*, successor, reward, done)`` — the successor disturbed by ``dx_{k*}``
    unless the step is done."""
    m = len(pts)
    a_min, a_max = acts.min(), acts.max()
    g32 = np.float32(gamma)
    Q = np.zeros(m, np.float32)
    k_star = np.full(m, -1, np.int32)
    w_n, w_r, w_done = pts.copy(), np.zeros(m, np.float32), np.zeros(m, bool)
    da_prev = None
    for k in range(disturbances.K):
        if disturbances.weights[k] == 0:
            continue
        da = disturbances.action_offsets[k]
        if da_prev is None or da != da_prev:
            ak = a if da == 0 else np.fmin(np.fmax(a + da, a_min), a_max)
            nxt, rew, done = step(pts, ak)
            nxt, rew, done = np.asarray(nxt, np.float32), np.asarray(rew, np.float32), np.asarray(done, bool)
        p = nxt.copy()
        e = np.zeros(m, np.float32)
        if not done.all():
            live = p[~done]
            for d in range(pts.shape[1]):
                dx = disturbances.state_offsets[k, d]
                if dx != 0:
                    live[:, d] = live[:, d] + dx
            p[~done] = live
            e[~done] = _expected_value(live, value_function, *grid)
        with np.errstate(over="ignore", invalid="ignore"):
            q = rew + g32 * e
            take = np.ones(m, bool) if da_prev is None else (q < Q) | (q != q)
        Q = np.where(take, q, Q)
        k_star = np.where(take, np.int32(k), k_star)
        w_n = np.where(take[:, None], p, w_n)
        w_r = np.where(take, rew, w_r)
        w_done = np.where(take, done, w_done)
        da_prev = da
    return Q, k_star, w_n, w_r, w_done


def _robust_lookahead(step, pts, disturbances, value_function, acts, grid, gamma):
    """One pass over (action, point): ``(best, best_q, worst, Q (m, n_actions), successor, reward, done)`` — what is kept
    of the step is action 0's until an action wins."""
    m = len(pts)
    best = np.zeros(m, np.int32)
    best_q = np.full(m, np.float32(-1.0e30), np.float32)
    worst = np.full(m, -1, np.int32)
    Q = np.empty((m, len(acts)), np.float32)
    b_n, b_r, b_done = pts.copy(), np.zeros(m, np.float32), np.zeros(m, bool)
    for i, u in enumerate(acts):
        q, k, n, r, done = _adversary_fold(step, pts, np.full(m, u, np.float32), disturbances, value_function, acts, grid, gamma)
        with np.errstate(invalid="ignore"):
            wins = q > best_q
        Q[:, i] = q
        best_q = np.where(wins, q, best_q)
        best = np.where(wins, np.int32(i), best)
        worst = np.where(wins, k, worst)
        keep = wins | (i == 0)
        b_n = np.where(keep[:, None], n, b_n)
        b_r = np.where(keep, r, b_r)
        b_done = np.where(keep, done, b_done)
    return best, best_q, worst, Q, b_n, b_r, b_done


def robust_action(step, points, disturbances, value_function, action_space, bounds_low, bounds_high, grid_shape, strides,
                  gamma, q_values=False):
    """The robust one-step lookahead at ``points`` (m, D) (numpy): the twin of ``DevicePolicy.robust``, same bits.
    ``best = argmax_a Q_worst(points, action_space[a])`` with the worst-case fold of ``expected_q(risk="worst")`` — strict
    ``>`` from -1e30 over ascending indices, NaN never wins, index 0 with Q = -1e30 when nothing wins — and ``worst``, the
    point the adversary answers the winner with (an index into the set; -1 when no action won).  Returns ``(best int32,
    action float32, q_best float32, worst int32)`` and, with ``q_values=True``, ``Q (m, n_actions)``."""
    pts = np.ascontiguousarray(np.atleast_2d(points), dtype=np.float32)
    acts, grid = _tables(action_space, bounds_low, bounds_high, grid_shape, strides)
    best, best_q, worst, Q = _robust_lookahead(step, pts, disturbances, value_function, acts, grid, gamma)[:4]
    out = (best, acts[best], best_q, worst)
    return out + (Q,) if q_values else out


def adversary_rollout(step, states, steps, disturbances, value_function, action_space, bounds_low, bounds_high, grid_shape,
                      strides, controller="policy", policy=None, gamma=1.0, lookahead_gamma=None, record_every=0):
    """Closed-loop episodes in which the disturbance is chosen AGAINST the controller, on the CPU (numpy): the twin of
    ``DevicePolicy.adversary_rollout``, same bits.  ``controller="policy"``: the action of the interpolated policy table —
    ``policy`` is the tuple ``utils.barycentric.rollout`` takes after ``steps``: ``(policy, action_space, bounds_low,
    bounds_high, grid_shape, strides, corner_bits)`` — then the adversary step: the worst point of the fold
    (``expected_q(risk="worst")``, discount ``lookahead_gamma``) moves the episode to ``f(s, a (+) da_k*) + dx_k*`` (no dx
    on a done step) and gives its reward and flag.  ``controller="robust"``: the robust lookahead (``robust_action``) and
    the adversary's answer to the winner; what is kept is action 0's until an action wins.  No random numbers.  The
    bookkeeping, ``gamma`` and ``record_every`` are ``rollout``'s.  Returns a ``RolloutResult`` of numpy arrays."""
    from utils.barycentric import RolloutResult, _closed_loop, _interpolated_actions
    if controller not in ("policy", "robust"):
        raise ValueError(f"controller must be 'policy' or 'robust', not {controller!r}")
    if controller == "policy" and policy is None:
        raise ValueError("controller='policy' needs policy=(policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits)")
    acts, grid = _tables(action_space, bounds_low, bounds_high, grid_shape, strides)
    lg = gamma if lookahead_gamma is None else lookahead_gamma

    def act(live, pts):
        return _interpolated_actions(pts, *policy) if controller == "policy" else np.zeros(len(pts), np.float32)

    def adversary_step(pts, a):
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        if controller == "policy":
            return _adversary_fold(step, pts, np.asarray(a, np.float32), disturbances, value_function, acts, grid, lg)[2:]
        return _robust_lookahead(step, pts, disturbances, value_function, acts, grid, lg)[4:]
    return RolloutResult(*_closed_loop(adversary_step, states, steps, gamma, record_every, act))
