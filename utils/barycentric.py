"""
utils/barycentric.py — inference-time interpolation on the solver's grids (numpy, no numba).

Same module path and call signatures as the reference's CPU helper
(/root/reference/utils/barycentric.py): ``get_barycentric_weights_and_indices`` (:12-73)
and ``get_optimal_action`` (:76-108), so rollout code written against the reference
(``from utils.barycentric import get_optimal_action``) runs unchanged on policies trained
here or there.  Vectorised over the batch instead of JIT-compiled loops.

Batched GPU path (keyword opt-in): ``device="cuda:0"`` on either function —
or a ``DevicePolicy`` object that keeps the policy table on the GPU — runs the same arithmetic as
ONE hand-written HIP kernel over the whole batch (libpi_mi355.so, ``pi_infer_query``): indices and
weights bit-identical to the functions below, the action summed in float32 in ascending corner order.
Without the keyword nothing here touches the GPU or the native library.

Grid continuation (no reference counterpart): ``resample`` interpolates a solution — value function and policy on one
grid — onto the nodes of another grid of the same D; ``DevicePolicy.set_values`` + ``DevicePolicy.resample`` are its
device twin, one HIP kernel launch (``pi_infer_resample``), same bits.  ``action_map`` translates action indices
between two action tables.

Semantics kept from the reference helper (they differ slightly from the training kernels):
the POINT is clamped to the bounds (not the cell coordinate), cell widths are float64
``(hi - lo) / (shape - 1)``, corners follow the rows of ``corner_bits`` (MSB-first
``itertools.product``), weights are float64 products stored as float32, indices int32.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# What a closed-loop rollout returns (``DevicePolicy.rollout``, ``rollout``): final states (m, D) float32, returns (m)
# float32 = sum_t gamma^t r_t, lengths (m) int32 = steps taken, terminated (m) bool = ended by the env's `done`,
# trajectory (rows, m, D) float32 or None.
RolloutResult = namedtuple("RolloutResult", "states returns lengths terminated trajectory")
# ... and a rollout that switches between two policies (``HybridPolicy.rollout``, ``hybrid_rollout``): the same fields plus
# secondary_steps (m) int32 = steps taken on the secondary policy, last_mode (m) uint8 = the mode (0 primary, 1 secondary)
# of the last step taken, 0 for an episode of length 0.
HybridRolloutResult = namedtuple("HybridRolloutResult", RolloutResult._fields + ("secondary_steps", "last_mode"))


class DevicePolicy:
    """A trained policy resident on the GPU for batched queries: ``DevicePolicy(policy, action_space,
    bounds_low, bounds_high, grid_shape, strides, corner_bits, device="cuda:0")``; calling it with
    states (m, D) returns the m interpolated actions (float32 numpy array); ``weights_and_indices``
    returns what ``get_barycentric_weights_and_indices`` returns.  ``policy`` may be None when only
    weights and indices are wanted.  Raises if the native library or a GPU is missing (no fallback)."""

    def __init__(self, policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits,
                 device="cuda:0"):
        import torch
        from dynamicprogramming_amd import _native
        if not torch.cuda.is_available():
            raise RuntimeError("DevicePolicy needs a ROCm GPU (torch.cuda.is_available() is False)")
        self._torch = torch
        self.device = torch.device(device)
        self.D = len(np.asarray(grid_shape))
        self.n_corners = len(np.asarray(corner_bits))
        self._engine = _native.InferenceEngine(bounds_low, bounds_high, grid_shape, strides, corner_bits,
                                               device=self.device.index or 0)
        self._has_policy = policy is not None
        self._n_actions = 0
        if self._has_policy:
            self._engine.set_policy(policy, action_space)
            self._n_actions = len(np.asarray(action_space))

    def _points(self, states):
        pts = np.ascontiguousarray(np.atleast_2d(states), dtype=np.float32)
        assert pts.shape[1] == self.D, f"states must be (m, {self.D})"
        return self._torch.from_numpy(pts).to(self.device), len(pts)

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def __call__(self, states):
        """states (m, D): a numpy array -> numpy actions (m,), or a float32 torch tensor already on this
        device -> a torch tensor on the device (no host round trip: closed-loop rollouts on the GPU)."""
        if not self._has_policy:
            raise RuntimeError("this DevicePolicy was built without a policy table")
        on_device = self._torch.is_tensor(states)
        if on_device:
            if states.device != self.device or states.dtype != self._torch.float32 or states.dim() != 2 \
                    or states.shape[1] != self.D:
                raise ValueError(f"device states must be a float32 (m, {self.D}) tensor on {self.device}")
            d_pts, m = states.contiguous(), states.shape[0]
        else:
            d_pts, m = self._points(states)
        out = self._torch.empty(m, dtype=self._torch.float32, device=self.device)
        self._engine.query(d_pts.data_ptr(), m, d_actions=out.data_ptr(), stream=self._stream())
        return out if on_device else out.cpu().numpy()

    def weights_and_indices(self, states):
        d_pts, m = self._points(states)
        w = self._torch.empty((m, self.n_corners), dtype=self._torch.float32, device=self.device)
        idx = self._torch.empty((m, self.n_corners), dtype=self._torch.int32, device=self.device)
        self._engine.query(d_pts.data_ptr(), m, d_weights=w.data_ptr(), d_indices=idx.data_ptr(), stream=self._stream())
        return w.cpu().numpy(), idx.cpu().numpy()

    def set_dynamics(self, dynamics_src: str) -> str:
        """The env plugin (the ``step_dynamics`` C string the solver compiles) the rollouts of this policy step
        through; returns the compiler's log.  Calling it again replaces the plugin."""
        log = self._engine.set_dynamics(dynamics_src)
        self._has_dynamics = True
        self._dynamics_serial = getattr(self, "_dynamics_serial", 0) + 1      # HybridPolicy rebuilds its module after this
        return log

    def _rollout_buffers(self, states, steps, record_every):
        """Checked arguments and the output tensors every rollout fills: (on_device, d_start, m, steps, every, final,
        returns, lengths, terminated (uint8), trajectory or None)."""
        torch = self._torch
        if not self._has_policy:
            raise RuntimeError("this DevicePolicy was built without a policy table")
        if not getattr(self, "_has_dynamics", False):
            raise RuntimeError("rollout needs the env's dynamics: call set_dynamics(dynamics_src) first")
        steps, every = int(steps), int(record_every)
        if steps < 0 or every < 0 or (steps > 0 and every > steps):
            raise ValueError("rollout needs steps >= 0 and 0 <= record_every <= steps")
        on_device = torch.is_tensor(states)
        if on_device:
            if states.device != self.device or states.dtype != torch.float32 or states.dim() != 2 \
                    or states.shape[1] != self.D:
                raise ValueError(f"device states must be a float32 (m, {self.D}) tensor on {self.device}")
            d_start, m = states.contiguous(), states.shape[0]
        else:
            d_start, m = self._points(states)
        final = torch.empty((m, self.D), dtype=torch.float32, device=self.device)
        ret = torch.empty(m, dtype=torch.float32, device=self.device)
        length = torch.empty(m, dtype=torch.int32, device=self.device)
        term = torch.empty(m, dtype=torch.uint8, device=self.device)
        traj = torch.empty((steps // every + 1, m, self.D), dtype=torch.float32, device=self.device) if every else None
        return on_device, d_start, m, steps, every, final, ret, length, term, traj

    def rollout(self, states, steps, gamma=1.0, record_every=0):
        """Closed-loop episodes from ``states`` (m, D) in ONE kernel launch: per step the interpolated action (what
        calling this object returns for the state, same bits) and the plugin's ``step_dynamics``; an episode whose
        step reports `done` keeps the state it reached.  ``returns`` accumulates ``ret + disc * r`` in float32,
        ``disc`` running through ``gamma``.  ``record_every = k > 0``: ``trajectory[j]`` holds all states after
        ``j * k`` steps (row 0 the start, ended episodes repeat their last state), ``steps // k + 1`` rows.
        A float32 tensor on this device in -> torch tensors on the device out; a numpy array in -> numpy out."""
        on_device, d_start, m, steps, every, final, ret, length, term, traj = self._rollout_buffers(states, steps, record_every)
        self._engine.rollout(d_start.data_ptr(), m, steps, gamma, d_final=final.data_ptr(), d_return=ret.data_ptr(),
                             d_length=length.data_ptr(), d_terminated=term.data_ptr(),
                             d_traj=traj.data_ptr() if every else 0, traj_every=every, stream=self._stream())
        term = term != 0
        if on_device:
            return RolloutResult(final, ret, length, term, traj)
        return RolloutResult(final.cpu().numpy(), ret.cpu().numpy(), length.cpu().numpy(), term.cpu().numpy(),
                             traj.cpu().numpy() if every else None)

    def set_values(self, V) -> str:
        """The value function that goes with this policy's grid (n_states float32, the user's order), for ``resample``;
        returns the compiler's log of the resample kernel.  Calling it again replaces the values."""
        log = self._engine.set_values(V)
        self._has_values = True
        return log

    def resample(self, bins, strides, term, out_values, out_policy, action_map=None, n_actions=None):
        """This solution interpolated onto the nodes of another grid in ONE kernel launch — the device twin of the
        module's ``resample``, same bits.  ``bins``: the destination's D bin tables; ``strides``: the element strides of
        its dense device arrays, one per dimension in the user's order (any memory order of the dimensions); ``term``:
        its terminal mask, a uint8 tensor on this device in that memory layout, or None — masked nodes are not written;
        ``out_values`` (float32) and ``out_policy`` (int32): tensors on this device with at least one entry per node,
        either may be None.  ``action_map`` (see ``action_map``) and ``n_actions`` describe the destination's action
        table; by default the destination shares the source's.  Asynchronous on torch's current stream."""
        torch = self._torch
        tables = [np.ascontiguousarray(b, dtype=np.float32).ravel() for b in bins]
        n = int(np.prod([len(t) for t in tables], dtype=np.int64))
        if out_values is None and out_policy is None:
            raise ValueError("resample needs out_values or out_policy")
        if out_values is not None and not getattr(self, "_has_values", False):
            raise RuntimeError("resample of values needs the value function: call set_values(V) first")
        if out_policy is not None and not self._has_policy:
            raise RuntimeError("this DevicePolicy was built without a policy table")
        for t, dtype, what in ((term, torch.uint8, "term"), (out_values, torch.float32, "out_values"),
                               (out_policy, torch.int32, "out_policy")):
            if t is not None and (not torch.is_tensor(t) or t.device != self.device or t.dtype != dtype
                                  or not t.is_contiguous() or t.numel() < n):
                raise ValueError(f"{what} must be a contiguous {dtype} tensor on {self.device} with at least {n} entries")
        ptr = lambda t: 0 if t is None else t.data_ptr()     # noqa: E731
        self._engine.resample([len(t) for t in tables], strides, tables, d_term=ptr(term), d_values=ptr(out_values),
                              d_policy=ptr(out_policy), action_map=action_map,
                              n_actions=self._n_actions if n_actions is None else int(n_actions), stream=self._stream())

    def close(self) -> None:
        self._engine.close()


class HybridPolicy:
    """Two trained policies on the GPU and the rule that switches between them: ``HybridPolicy(primary, secondary,
    enter, leave)`` — two ``DevicePolicy`` objects of the same D on the same device, each on its own grid with its own
    action table, and two vectors of D float32 thresholds.  Every episode starts on the primary policy (mode 0); per
    step it moves to the secondary (mode 1) iff ``|s[d]| < enter[d]`` in every dimension and back iff ``|s[d]| >
    leave[d]`` in some dimension (float32, strict; ``inf`` in both: the dimension takes no part) — the reference's
    runners/hybrid_double_cartpole.py with ``enter = (inf, inf, 0.32, 4, 0.32, 4)``, ``leave = (inf, inf, 0.38, 5, 0.38,
    5)``.  The env plugin is the primary's: ``primary.set_dynamics(...)`` first."""

    def __init__(self, primary: DevicePolicy, secondary: DevicePolicy, enter, leave):
        if primary.D != secondary.D or primary.device != secondary.device:
            raise ValueError("both policies of a HybridPolicy need the same D and the same device")
        self.primary, self.secondary = primary, secondary
        self.enter = np.ascontiguousarray(enter, dtype=np.float32)
        self.leave = np.ascontiguousarray(leave, dtype=np.float32)
        if self.enter.shape != (primary.D,) or self.leave.shape != (primary.D,):
            raise ValueError(f"enter and leave must hold {primary.D} thresholds each")
        self._built_for = None                     # the primary's set_dynamics call the hybrid module was built after

    def rollout(self, states, steps, gamma=1.0, record_every=0):
        """Closed-loop episodes from ``states`` (m, D) in ONE kernel launch, in/out conventions of ``DevicePolicy.rollout``;
        returns a ``HybridRolloutResult``.  The hybrid kernel is built on first use and again after a new
        ``primary.set_dynamics``."""
        a, b = self.primary, self.secondary
        if not b._has_policy:
            raise RuntimeError("the secondary DevicePolicy was built without a policy table")
        on_device, d_start, m, steps, every, final, ret, length, term, traj = a._rollout_buffers(states, steps, record_every)
        if self._built_for != a._dynamics_serial:
            a._engine.set_partner(b._engine)
            self._built_for = a._dynamics_serial
        torch = a._torch
        second = torch.empty(m, dtype=torch.int32, device=a.device)
        mode = torch.empty(m, dtype=torch.uint8, device=a.device)
        a._engine.rollout_hybrid(b._engine, d_start.data_ptr(), m, steps, self.enter, self.leave, gamma,
                                 d_final=final.data_ptr(), d_return=ret.data_ptr(), d_length=length.data_ptr(),
                                 d_terminated=term.data_ptr(), d_secondary_steps=second.data_ptr(),
                                 d_last_mode=mode.data_ptr(), d_traj=traj.data_ptr() if every else 0, traj_every=every,
                                 stream=a._stream())
        term = term != 0
        if on_device:
            return HybridRolloutResult(final, ret, length, term, traj, second, mode)
        return HybridRolloutResult(final.cpu().numpy(), ret.cpu().numpy(), length.cpu().numpy(), term.cpu().numpy(),
                                   traj.cpu().numpy() if every else None, second.cpu().numpy(), mode.cpu().numpy())


def get_barycentric_weights_and_indices(points, bounds_low, bounds_high, grid_shape, strides,
                                        corner_bits, *, device=None):
    """
    points (n, D) float32 -> (weights (n, 2^D) float32 summing to 1, indices (n, 2^D) int32).
    ``device="cuda:0"``: the whole batch in one HIP kernel (same bits).
    """
    if device is not None:
        dp = DevicePolicy(None, None, bounds_low, bounds_high, grid_shape, strides, corner_bits, device=device)
        try:
            return dp.weights_and_indices(points)
        finally:
            dp.close()
    pts = np.asarray(points)
    lo = np.asarray(bounds_low)
    hi = np.asarray(bounds_high)
    shape = np.asarray(grid_shape)
    st = np.asarray(strides).astype(np.int64)
    bits = np.asarray(corner_bits).astype(np.int64)           # (C, D)
    step = (hi - lo) / (shape - 1)                             # float64, like the reference
    p = np.maximum(lo, np.minimum(pts, hi))                    # clamp the point
    cell = (p - lo) / step
    idx = cell.astype(np.int64)                                # truncation, cell >= 0
    idx = np.where(idx >= shape - 1, shape - 2, idx)
    t = ((p - (lo + idx * step)) / step).astype(np.float32)    # (n, D)
    t64 = t.astype(np.float64)
    # w[c] = prod_d (t_d if bit else 1 - t_d), multiplied in dimension order
    w = np.ones((pts.shape[0], bits.shape[0]), dtype=np.float64)
    for d in range(pts.shape[1]):
        w = w * np.where(bits[None, :, d] == 1, t64[:, None, d], 1.0 - t64[:, None, d])
    flat = ((idx[:, None, :] + bits[None, :, :]) * st[None, None, :]).sum(axis=2)
    return w.astype(np.float32), flat.astype(np.int32)


def get_optimal_action(state, policy, action_space, bounds_low, bounds_high, grid_shape, strides,
                       corner_bits, *, device=None):
    """Interpolated action at a continuous state: weights @ action VALUES of the surrounding
    grid nodes' greedy actions (reference :96-108).  ``device="cuda:0"``: ``state`` may be a batch
    (m, D) and the m actions come from one HIP kernel launch (for repeated queries keep a
    ``DevicePolicy`` instead: it uploads the policy table once)."""
    if device is not None:
        dp = DevicePolicy(policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits,
                          device=device)
        try:
            out = dp(state)
        finally:
            dp.close()
        return out[0] if np.ndim(state) == 1 else out
    state_2d = np.atleast_2d(state).astype(np.float32)
    lambdas, flat = get_barycentric_weights_and_indices(state_2d, bounds_low, bounds_high,
                                                        grid_shape, strides, corner_bits)
    lambdas = lambdas.flatten()
    flat = flat.flatten()
    return lambdas @ np.asarray(action_space)[np.asarray(policy)[flat]]


def action_map(source_actions, destination_actions):
    """For every source action the index of the nearest destination action VALUE — float32 absolute difference, the
    lowest index on ties — as an int32 array; None (the identity) when the two tables are equal."""
    src = np.ascontiguousarray(source_actions, dtype=np.float32).ravel()
    dst = np.ascontiguousarray(destination_actions, dtype=np.float32).ravel()
    if np.array_equal(src, dst):
        return None
    return np.abs(src[:, None] - dst[None, :]).argmin(axis=1).astype(np.int32)


def resample(value_function, policy, bounds_low, bounds_high, grid_shape, strides, corner_bits, bins, *,
             action_map=None, at=None, chunk=1 << 18):
    """A solution on one grid — ``value_function`` and ``policy`` (either may be None) with the grid description
    ``get_barycentric_weights_and_indices`` takes — interpolated onto the nodes of the grid spanned by the D bin tables
    ``bins`` (numpy): the twin of ``DevicePolicy.resample``, same definition.  For the node with coordinates
    ``x_d = bins[d][i_d]``: weights and indices from ``get_barycentric_weights_and_indices`` (the point clamped to the
    source's bounds); ``V = V + w[c] * value_function[idx[c]]`` in float32 from 0 over ascending corners (multiply,
    then add); ``policy[idx[c*]]`` at the corner c* of largest weight, the first one on ties, sent through
    ``action_map`` when one is given.  ``at``: flat indices of the nodes wanted, in the destination's row-major user
    order (default: every node, in that order).  Returns (V float32 or None, policy int32 or None).  What happens to the
    destination's terminal nodes is the caller's business: the device leaves them unwritten."""
    tables = [np.ascontiguousarray(b, dtype=np.float32).ravel() for b in bins]
    shape = [len(t) for t in tables]
    at = np.arange(int(np.prod(shape, dtype=np.int64)), dtype=np.int64) if at is None else np.asarray(at, dtype=np.int64)
    val = None if value_function is None else np.asarray(value_function, dtype=np.float32).ravel()
    pol = None if policy is None else np.asarray(policy).ravel()
    V = None if val is None else np.empty(len(at), np.float32)
    P = None if pol is None else np.empty(len(at), np.int32)
    for k in range(0, len(at), int(chunk)):
        node = np.unravel_index(at[k:k + chunk], shape)
        pts = np.stack([t[i] for t, i in zip(tables, node)], axis=1)
        w, idx = get_barycentric_weights_and_indices(pts, bounds_low, bounds_high, grid_shape, strides, corner_bits)
        if val is not None:
            v = np.zeros(len(pts), np.float32)
            for c in range(w.shape[1]):
                v = v + w[:, c] * val[idx[:, c]]
            V[k:k + chunk] = v
        if pol is not None:
            a = pol[idx[np.arange(len(pts)), w.argmax(axis=1)]]
            P[k:k + chunk] = a if action_map is None else np.asarray(action_map)[a]
    return V, P


def _interpolated_actions(points, policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits):
    """The rollouts' action: weights and indices from ``get_barycentric_weights_and_indices``, summed in float32 over
    ascending corners (multiply, then add)."""
    pol = np.asarray(policy)
    acts = np.asarray(action_space, dtype=np.float32)
    w, idx = get_barycentric_weights_and_indices(points, bounds_low, bounds_high, grid_shape, strides, corner_bits)
    a = np.zeros(len(points), np.float32)
    for c in range(w.shape[1]):
        a = a + w[:, c] * acts[pol[idx[:, c]]]
    return a


def _closed_loop(step, states, steps, gamma, record_every, act):
    """The loop ``rollout`` and ``hybrid_rollout`` share.  ``act(live, states (k, D)) -> actions (k,) float32`` is asked
    for the episodes still running (``live``: their indices).  Returns the fields of a ``RolloutResult``."""
    steps, every = int(steps), int(record_every)
    if steps < 0 or every < 0 or (steps > 0 and every > steps):
        raise ValueError("rollout needs steps >= 0 and 0 <= record_every <= steps")
    s = np.array(np.atleast_2d(states), dtype=np.float32)
    m = len(s)
    ret = np.zeros(m, np.float32)
    length = np.zeros(m, np.int32)
    terminated = np.zeros(m, bool)
    running = np.ones(m, bool)
    disc, g = np.float32(1.0), np.float32(gamma)
    rows = [s.copy()] if every else None
    for t in range(steps):
        live = np.flatnonzero(running)
        if len(live) == 0 and not every:
            break
        if len(live):
            a = act(live, s[live])
            nxt, rew, done = step(s[live], a)
            ret[live] = ret[live] + disc * np.asarray(rew, np.float32)
            s[live] = np.asarray(nxt, np.float32)
            length[live] = t + 1
            ended = live[np.asarray(done, bool)]
            terminated[ended] = True
            running[ended] = False
        disc = np.float32(disc * g)
        if every and (t + 1) % every == 0:
            rows.append(s.copy())
    return s, ret, length, terminated, np.stack(rows) if every else None


def rollout(step, states, steps, policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits,
            gamma=1.0, record_every=0):
    """Closed-loop episodes on the CPU (numpy): the twin of ``DevicePolicy.rollout``, same definition.
    ``step(states (k, D) float32, actions (k,) float32) -> (next (k, D), reward (k,), done (k,))`` is any batched
    env step; it is only handed the episodes still running.  Per step: weights and indices from
    ``get_barycentric_weights_and_indices``, the action summed in float32 over ascending corners (multiply, then
    add), ``ret = ret + disc * r`` and ``disc = disc * gamma`` in float32, state = successor, length = t + 1; `done`
    freezes the episode at the state it reached.  Returns a ``RolloutResult`` of numpy arrays."""
    tables = (policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits)
    return RolloutResult(*_closed_loop(step, states, steps, gamma, record_every,
                                       lambda live, pts: _interpolated_actions(pts, *tables)))


def switch_mode(mode, states, enter, leave):
    """One application of the hybrid rule: ``mode`` (k,) bool (True: secondary) and ``states`` (k, D) -> the new modes.
    A secondary episode stays unless ``|s[d]| > leave[d]`` for some d; a primary one moves over iff ``|s[d]| < enter[d]``
    for every d.  float32, strict comparisons."""
    mag = np.abs(np.asarray(states, dtype=np.float32))
    inside = (mag < np.asarray(enter, dtype=np.float32)).all(axis=1)
    outside = (mag > np.asarray(leave, dtype=np.float32)).any(axis=1)
    return np.where(np.asarray(mode, bool), ~outside, inside)


def hybrid_rollout(step, states, steps, primary, secondary, enter, leave, gamma=1.0, record_every=0):
    """Closed-loop episodes that switch between two policies, on the CPU (numpy): the twin of ``HybridPolicy.rollout``.
    ``primary`` and ``secondary`` are the tuples of tables ``rollout`` takes — ``(policy, action_space, bounds_low,
    bounds_high, grid_shape, strides, corner_bits)`` — and ``step`` its batched env step.  Every episode starts in
    mode 0; per step ``switch_mode`` first, then the action of the mode's policy on its own grid, ``secondary_steps``
    counts the steps in mode 1, and the step's bookkeeping is ``rollout``'s.  Returns a ``HybridRolloutResult``."""
    m = len(np.atleast_2d(states))
    mode = np.zeros(m, bool)
    second = np.zeros(m, np.int32)

    def act(live, pts):
        now = switch_mode(mode[live], pts, enter, leave)
        mode[live] = now
        second[live] += now
        a = np.empty(len(live), np.float32)
        for which, tables in ((~now, primary), (now, secondary)):
            if which.any():
                a[which] = _interpolated_actions(pts[which], *tables)
        return a
    return HybridRolloutResult(*_closed_loop(step, states, steps, gamma, record_every, act), second, mode.astype(np.uint8))
