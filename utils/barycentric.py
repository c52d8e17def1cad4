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
        if self._has_policy:
            self._engine.set_policy(policy, action_space)

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
        return log

    def rollout(self, states, steps, gamma=1.0, record_every=0):
        """Closed-loop episodes from ``states`` (m, D) in ONE kernel launch: per step the interpolated action (what
        calling this object returns for the state, same bits) and the plugin's ``step_dynamics``; an episode whose
        step reports `done` keeps the state it reached.  ``returns`` accumulates ``ret + disc * r`` in float32,
        ``disc`` running through ``gamma``.  ``record_every = k > 0``: ``trajectory[j]`` holds all states after
        ``j * k`` steps (row 0 the start, ended episodes repeat their last state), ``steps // k + 1`` rows.
        A float32 tensor on this device in -> torch tensors on the device out; a numpy array in -> numpy out."""
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
        self._engine.rollout(d_start.data_ptr(), m, steps, gamma, d_final=final.data_ptr(), d_return=ret.data_ptr(),
                             d_length=length.data_ptr(), d_terminated=term.data_ptr(),
                             d_traj=traj.data_ptr() if every else 0, traj_every=every, stream=self._stream())
        term = term != 0
        if on_device:
            return RolloutResult(final, ret, length, term, traj)
        return RolloutResult(final.cpu().numpy(), ret.cpu().numpy(), length.cpu().numpy(), term.cpu().numpy(),
                             traj.cpu().numpy() if every else None)

    def close(self) -> None:
        self._engine.close()


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


def rollout(step, states, steps, policy, action_space, bounds_low, bounds_high, grid_shape, strides, corner_bits,
            gamma=1.0, record_every=0):
    """Closed-loop episodes on the CPU (numpy): the twin of ``DevicePolicy.rollout``, same definition.
    ``step(states (k, D) float32, actions (k,) float32) -> (next (k, D), reward (k,), done (k,))`` is any batched
    env step; it is only handed the episodes still running.  Per step: weights and indices from
    ``get_barycentric_weights_and_indices``, the action summed in float32 over ascending corners (multiply, then
    add), ``ret = ret + disc * r`` and ``disc = disc * gamma`` in float32, state = successor, length = t + 1; `done`
    freezes the episode at the state it reached.  Returns a ``RolloutResult`` of numpy arrays."""
    steps, every = int(steps), int(record_every)
    if steps < 0 or every < 0 or (steps > 0 and every > steps):
        raise ValueError("rollout needs steps >= 0 and 0 <= record_every <= steps")
    s = np.array(np.atleast_2d(states), dtype=np.float32)
    m = len(s)
    pol = np.asarray(policy)
    acts = np.asarray(action_space, dtype=np.float32)
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
            w, idx = get_barycentric_weights_and_indices(s[live], bounds_low, bounds_high, grid_shape, strides,
                                                         corner_bits)
            a = np.zeros(len(live), np.float32)
            for c in range(w.shape[1]):
                a = a + w[:, c] * acts[pol[idx[:, c]]]
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
    return RolloutResult(s, ret, length, terminated, np.stack(rows) if every else None)
