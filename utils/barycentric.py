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

Value-greedy control (no reference counterpart): ``greedy_action`` is the one-step lookahead on the interpolated VALUE
function, ``a*(s) = argmax_a [r(s, a) + gamma * E[V](s')]`` — the improvement backup of the training kernels at an
arbitrary continuous state, in their arithmetic, not this helper's — and ``greedy_rollout`` the closed loop under it;
``DevicePolicy.set_greedy`` + ``DevicePolicy.greedy`` / ``DevicePolicy.rollout(controller="greedy")`` are their device
twins, one HIP kernel launch each (``pi_infer_greedy``, ``pi_infer_rollout_greedy``), same bits.  It needs only V.

Stochastic rollouts (the reference's ``evaluate_random()`` baseline, and beyond it): ``stochastic_rollout`` is the closed
loop with epsilon-random actions, action noise and state noise drawn from Philox4x32-10 (``philox4x32``) keyed by
(seed; episode, step, draw block) — ``random_words`` — so the draws need no state and do not depend on how a batch is
cut; ``DevicePolicy.set_stochastic`` + ``DevicePolicy.rollout(epsilon=..., action_noise=..., state_noise=..., seed=...,
first_episode=...)`` / ``rollout(controller="random")`` / ``DevicePolicy.random_words`` are the device twins, one HIP
kernel launch each (``pi_infer_rollout_stochastic``, ``pi_infer_random_words``), same bits.

Expected-value greedy control (no reference counterpart): the greedy lookahead with the expectation of noise-aware
solving inside it, ``argmax_a sum_k p_k [r_k + gamma * E[V](f(s, a (+) da_k) + dx_k)]`` over a
``dynamicprogramming_amd.noise.Disturbances`` set, and closed loops under it that draw the stochastic rollouts' noise from
the same counters: ``DevicePolicy.set_expected_greedy`` + ``set_disturbances`` + ``expected_greedy`` /
``rollout(controller="expected")``, one HIP kernel launch each (``pi_infer_expect_greedy``,
``pi_infer_rollout_expect_greedy``); the numpy twins live beside the set, ``noise.expected_greedy_action`` /
``noise.expected_greedy_rollout``, same bits.

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
# ... and one that does so under noise (``HybridPolicy.rollout(epsilon=..., ...)``, ``stochastic_hybrid_rollout``): the same
# fields plus switches (m) int32 = the steps whose mode differs from that of the step taken before (mode 0 before step 0).
StochasticHybridRolloutResult = namedtuple("StochasticHybridRolloutResult", HybridRolloutResult._fields + ("switches",))


def check_controller(controller) -> None:
    if controller not in ("policy", "greedy", "random", "expected"):
        raise ValueError(f"controller must be 'policy', 'greedy', 'random' or 'expected', not {controller!r}")


def is_stochastic(controller, epsilon=0.0, action_noise=0.0, state_noise=None) -> bool:
    """Whether a rollout with these arguments runs a stochastic kernel: the random controller, or an epsilon, an action
    noise or a state noise that is not zero — the noises as the float32 values the kernel is given.  It judges, it does
    not check: a value out of range counts as noise and is refused where the keywords are parsed."""
    return controller == "random" or float(epsilon) != 0.0 or (action_noise != 0 and np.float32(action_noise) != 0) or \
        (state_noise is not None and bool(np.asarray(state_noise, dtype=np.float32).any()))


def refuse_noisy_greedy(controller, stochastic) -> None:
    if controller == "greedy" and stochastic:
        raise ValueError("controller='greedy' takes no epsilon, action_noise or state_noise: a stochastic greedy "
                         "controller does not exist")


def _u64(x) -> int:
    """A seed or an episode number as the uint64 the kernels count in (wrapping at 2^64)."""
    return int(x) & (2 ** 64 - 1)


def _table(action_space, default=None):
    """An action table as flat float32; None: `default`."""
    return default if action_space is None else np.ascontiguousarray(action_space, dtype=np.float32).ravel()


def _noise_keywords(policy, epsilon, action_noise, state_noise) -> dict:
    """The noise keywords of a ``rollout``, checked in this order, as the keywords the engine's noisy rollouts take;
    ``state_noise`` None stays None (no vector, and ``policy.D`` is not read)."""
    explore_threshold(epsilon)                      # raises outside [0, 1]
    a_noise = float(_checked_action_noise(action_noise))
    s_noise = None if state_noise is None else _noise_vector(state_noise, policy.D)
    return dict(epsilon=epsilon, action_noise=a_noise, state_noise=s_noise)


def _result(kind, on_device, fields):
    """The output tensors of a rollout (``terminated``, the fourth, still uint8) as the result namedtuple `kind`: as they
    are for a caller that gave device states, numpy otherwise."""
    fields[3] = fields[3] != 0
    return kind(*fields) if on_device else kind(*(None if x is None else x.cpu().numpy() for x in fields))


class DevicePolicy:
    """A trained policy resident on the GPU for batched queries: ``DevicePolicy(policy, action_space,
    bounds_low, bounds_high, grid_shape, strides, corner_bits, device="cuda:0")``; calling it with
    states (m, D) returns the m interpolated actions (float32 numpy array); ``weights_and_indices``
    returns what ``get_barycentric_weights_and_indices`` returns.  ``policy`` may be None when only
    weights and indices, or the value-greedy controller (``set_values``, ``set_dynamics``, ``set_greedy``: it acts on
    the value function and ``action_space``), are wanted.  Raises if the native library or a GPU is missing (no fallback)."""

    # what the setters below record, at its value before any of them was called
    _has_dynamics = False                      # set_dynamics was called
    _has_values = False                        # set_values was called
    _dynamics_serial = 0                       # the number of set_dynamics calls: HybridPolicy rebuilds its modules after one
    _greedy_actions = None                     # the table of the last set_greedy; None: no greedy module
    _stochastic_actions = None                 # the table of the last set_stochastic; None: no stochastic module
    _expected_actions = None                   # the table of the last set_expected_greedy; None: no such module
    _robust_actions = None                     # the table of the last set_robust; None: no such module
    _disturbances = None                       # the set of the last set_disturbances
    _partner_stochastic = None                 # (serial, secondary, table) HybridPolicy built this handle's noisy module for

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
        # the action table on its own: the value-greedy controller needs no policy (set_greedy)
        self._action_space = _table(action_space)
        if self._has_policy:
            self._engine.set_policy(policy, action_space)
            self._n_actions = len(np.asarray(action_space))

    def _points(self, states):
        pts = np.ascontiguousarray(np.atleast_2d(states), dtype=np.float32)
        assert pts.shape[1] == self.D, f"states must be (m, {self.D})"
        return self._torch.from_numpy(pts).to(self.device), len(pts)

    def _device_states(self, states):
        """(on_device, float32 (m, D) tensor on this device, m) of states given as numpy or as such a tensor."""
        if not self._torch.is_tensor(states):
            return (False, *self._points(states))
        if states.device != self.device or states.dtype != self._torch.float32 or states.dim() != 2 \
                or states.shape[1] != self.D:
            raise ValueError(f"device states must be a float32 (m, {self.D}) tensor on {self.device}")
        return True, states.contiguous(), states.shape[0]

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def __call__(self, states):
        """states (m, D): a numpy array -> numpy actions (m,), or a float32 torch tensor already on this
        device -> a torch tensor on the device (no host round trip: closed-loop rollouts on the GPU)."""
        if not self._has_policy:
            raise RuntimeError("this DevicePolicy was built without a policy table")
        on_device, d_pts, m = self._device_states(states)
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
        self._dynamics_serial += 1                                            # HybridPolicy rebuilds its module after this
        self._greedy_actions = None                                           # the library dropped the greedy module
        self._stochastic_actions = None                                       # ... and the stochastic one
        self._expected_actions = None                                         # ... and the expected-greedy one
        self._robust_actions = None                                           # ... and the adversary one
        return log

    def _rollout_buffers(self, states, steps, record_every, need_policy=True):
        """Checked arguments and the output tensors every rollout fills: (on_device, d_start, m, steps, [final, returns,
        lengths, terminated (uint8), trajectory or None], the keywords that hand those to the engine's rollouts)."""
        torch = self._torch
        if need_policy and not self._has_policy:
            raise RuntimeError("this DevicePolicy was built without a policy table")
        if not self._has_dynamics:
            raise RuntimeError("rollout needs the env's dynamics: call set_dynamics(dynamics_src) first")
        steps, every = int(steps), int(record_every)
        if steps < 0 or every < 0 or (steps > 0 and every > steps):
            raise ValueError("rollout needs steps >= 0 and 0 <= record_every <= steps")
        on_device, d_start, m = self._device_states(states)
        final = torch.empty((m, self.D), dtype=torch.float32, device=self.device)
        ret = torch.empty(m, dtype=torch.float32, device=self.device)
        length = torch.empty(m, dtype=torch.int32, device=self.device)
        term = torch.empty(m, dtype=torch.uint8, device=self.device)
        traj = torch.empty((steps // every + 1, m, self.D), dtype=torch.float32, device=self.device) if every else None
        outs = dict(d_final=final.data_ptr(), d_return=ret.data_ptr(), d_length=length.data_ptr(),
                    d_terminated=term.data_ptr(), d_traj=traj.data_ptr() if every else 0, traj_every=every,
                    stream=self._stream())
        return on_device, d_start, m, steps, [final, ret, length, term, traj], outs

    def rollout(self, states, steps, gamma=1.0, record_every=0, controller="policy", lookahead_gamma=None, *,
                epsilon=0.0, action_noise=0.0, state_noise=None, seed=0, first_episode=0):
        """Closed-loop episodes from ``states`` (m, D) in ONE kernel launch: per step the interpolated action (what
        calling this object returns for the state, same bits) and the plugin's ``step_dynamics``; an episode whose
        step reports `done` keeps the state it reached.  ``returns`` accumulates ``ret + disc * r`` in float32,
        ``disc`` running through ``gamma``.  ``record_every = k > 0``: ``trajectory[j]`` holds all states after
        ``j * k`` steps (row 0 the start, ended episodes repeat their last state), ``steps // k + 1`` rows.
        A float32 tensor on this device in -> torch tensors on the device out; a numpy array in -> numpy out.
        ``controller="greedy"``: per step the action ``greedy`` returns for the state with the discount
        ``lookahead_gamma`` (required; a property of the solution, not the ``gamma`` the return is summed with) instead
        of the interpolated one — after ``set_greedy``, no policy table needed; everything else is the same.
        Stochastic rollouts (after ``set_stochastic``; the device twin of the module's ``stochastic_rollout``, same bits):
        ``epsilon`` in [0, 1] is the probability that a step takes a uniformly random action of the table instead of the
        policy's; ``action_noise >= 0`` adds ``action_noise * u``, u in [-1, 1), to the action and clamps it to the
        table's extremes; ``state_noise`` (one value or D, >= 0) adds ``state_noise[d] * u_d`` to the successor of every
        step that is not `done`.  The draws are a function of (``seed``, ``first_episode`` + the episode's row, step)
        alone: the same arguments give the same bits, and a batch cut into several calls with the matching
        ``first_episode`` gives the results of one.  ``controller="random"`` is ``epsilon = 1``, the random-policy
        baseline; it needs no policy table.  With all five at their defaults this is the deterministic rollout.
        ``controller="expected"`` (after ``set_expected_greedy`` and ``set_disturbances``; the device twin of
        ``dynamicprogramming_amd.noise.expected_greedy_rollout``, same bits): per step the action ``expected_greedy``
        returns for the state with the discount ``lookahead_gamma`` (required) — the lookahead with the expectation over
        the disturbance set inside it.  It accepts the five stochastic keywords, drawn from the same counters as the
        policy-table controller's (an exploring step takes its random action instead of the lookahead's), so the two can
        be compared under common random numbers; with ``Disturbances.none(D)`` it is the greedy lookahead under noise."""
        check_controller(controller)
        greedy = controller == "greedy"
        expected = controller == "expected"
        if controller == "random":
            if float(epsilon) not in (0.0, 1.0):
                raise ValueError("controller='random' is epsilon = 1: give no other epsilon with it")
            epsilon = 1.0
        noise = _noise_keywords(self, epsilon, action_noise, state_noise)
        stochastic = is_stochastic(controller, **noise)
        refuse_noisy_greedy(controller, stochastic)
        if (greedy or expected) and lookahead_gamma is None:
            raise ValueError(f"controller={controller!r} needs lookahead_gamma, the discount the value function was solved with")
        if expected:
            self._need_expected_greedy()
        elif greedy:
            self._need_greedy()
        elif stochastic:
            self._need_stochastic("a stochastic rollout")
        on_device, d_start, m, steps, out, outs = \
            self._rollout_buffers(states, steps, record_every, need_policy=not greedy and not expected and float(epsilon) != 1.0)
        if expected or stochastic:
            noise.update(seed=_u64(seed), first_episode=_u64(first_episode))
        if greedy:
            self._engine.rollout_greedy(d_start.data_ptr(), m, steps, lookahead_gamma, gamma, **outs)
        elif expected:
            self._engine.rollout_expect_greedy(d_start.data_ptr(), m, steps, lookahead_gamma, gamma, **noise, **outs)
        elif stochastic:
            self._engine.rollout_stochastic(d_start.data_ptr(), m, steps, gamma, **noise, **outs)
        else:
            self._engine.rollout(d_start.data_ptr(), m, steps, gamma, **outs)
        return _result(RolloutResult, on_device, out)

    def set_values(self, V) -> str:
        """The value function that goes with this policy's grid (n_states float32, the user's order), for ``resample``;
        returns the compiler's log of the resample kernel.  Calling it again replaces the values."""
        log = self._engine.set_values(V)
        self._has_values = True
        return log

    def set_greedy(self, action_space=None) -> str:
        """Build the value-greedy controller — the one-step lookahead on the value function of ``set_values`` through
        the plugin of ``set_dynamics`` — over ``action_space`` (default: the table the constructor was given); returns
        the compiler's log.  Needs no policy table.  ``set_dynamics`` drops it again; ``set_values`` only replaces the
        values it reads."""
        return self._build_module("set_greedy", "the greedy controller", action_space, self._engine.set_greedy,
                                  "_greedy_actions")

    def set_stochastic(self, action_space=None) -> str:
        """Build the stochastic rollout kernels — ``rollout(epsilon=..., action_noise=..., state_noise=...)`` and
        ``controller="random"`` — through the plugin of ``set_dynamics``; exploring steps draw from ``action_space``
        (default: the table the constructor was given), whose extremes clamp a noisy action.  Returns the compiler's
        log.  Needs neither a policy table nor values.  ``set_dynamics`` drops it again."""
        return self._build_module("set_stochastic", "a stochastic rollout", action_space, self._engine.set_stochastic,
                                  "_stochastic_actions", needs_values=False)

    def set_expected_greedy(self, action_space=None) -> str:
        """Build the expected-value greedy controller — the one-step lookahead on the value function of ``set_values``
        through the plugin of ``set_dynamics`` with the expectation over the set of ``set_disturbances`` inside it — over
        ``action_space`` (default: the table the constructor was given; finite values: its extremes clamp ``a + da_k`` and
        a noisy action); returns the compiler's log.  Needs no policy table.  ``set_dynamics`` drops it again;
        ``set_values`` and ``set_disturbances`` only replace what it reads."""
        return self._build_module("set_expected_greedy", "the expected controller", action_space,
                                  self._engine.set_expect_greedy, "_expected_actions")

    def set_robust(self, action_space=None) -> str:
        """Build the robust lookahead and the adversary rollout — the worst case over the set of ``set_disturbances`` on
        the value function of ``set_values`` through the plugin of ``set_dynamics`` — over ``action_space`` (default: the
        table the constructor was given; its extremes clamp ``a + da_k``); returns the compiler's log.  ``set_dynamics``
        drops it again; ``set_values`` and ``set_disturbances`` only replace what it reads."""
        return self._build_module("set_robust", "the robust controller", action_space, self._engine.set_robust,
                                  "_robust_actions")

    def _need_robust(self) -> None:
        if self._robust_actions is None:
            raise RuntimeError("the robust controller needs set_robust() (again after every set_dynamics)")
        if self._disturbances is None:
            raise RuntimeError("the robust controller needs a disturbance set: call set_disturbances(...) first")

    def robust(self, states, gamma, q_values=False):
        """The robust one-step lookahead at ``states`` (m, D) in ONE kernel launch — the device twin of
        ``dynamicprogramming_amd.noise.robust_action``, same bits: ``(best_index int32, action, q_best, worst int32)`` and,
        with ``q_values=True``, ``Q (m, n_actions)``; ``worst`` is the point of the set the adversary answers the winner
        with, -1 when no action won.  In/out conventions of ``greedy``.  After ``set_robust`` and ``set_disturbances``."""
        self._need_robust()
        torch = self._torch
        on_device, d_pts, m = self._device_states(states)
        best = torch.empty(m, dtype=torch.int32, device=self.device)
        act = torch.empty(m, dtype=torch.float32, device=self.device)
        qb = torch.empty(m, dtype=torch.float32, device=self.device)
        worst = torch.empty(m, dtype=torch.int32, device=self.device)
        out = [best, act, qb, worst]
        if q_values:
            out.append(torch.empty((m, len(self._robust_actions)), dtype=torch.float32, device=self.device))
        self._engine.robust(d_pts.data_ptr(), m, gamma, d_best=best.data_ptr(), d_action=act.data_ptr(),
                            d_q_best=qb.data_ptr(), d_q_all=out[4].data_ptr() if q_values else 0,
                            d_worst=worst.data_ptr(), stream=self._stream())
        return tuple(out) if on_device else tuple(x.cpu().numpy() for x in out)

    def adversary_rollout(self, states, steps, gamma=1.0, record_every=0, controller="policy", lookahead_gamma=None):
        """Closed-loop episodes in which the disturbance is chosen AGAINST the controller, in ONE kernel launch — the
        device twin of ``dynamicprogramming_amd.noise.adversary_rollout``, same bits.  ``controller="policy"``: the
        interpolated action of the policy table, then the worst point of the set for it (the fold of the worst-case
        sweeps on the value function, discount ``lookahead_gamma``, required) moves the episode and gives its reward and
        flag.  ``controller="robust"``: the robust lookahead and the adversary's answer to its winner; no policy table
        needed.  No random numbers.  The outputs and in/out conventions are ``rollout``'s.  After ``set_robust`` and
        ``set_disturbances``."""
        if controller not in ("policy", "robust"):
            raise ValueError(f"controller must be 'policy' or 'robust', not {controller!r}")
        if lookahead_gamma is None:
            raise ValueError("adversary_rollout needs lookahead_gamma, the discount the value function was solved with")
        self._need_robust()
        on_device, d_start, m, steps, out, outs = \
            self._rollout_buffers(states, steps, record_every, need_policy=controller == "policy")
        self._engine.rollout_adversary(d_start.data_ptr(), m, steps, lookahead_gamma, int(controller == "robust"), gamma, **outs)
        return _result(RolloutResult, on_device, out)

    def _build_module(self, setter, who, action_space, build, record, needs_values=True) -> str:
        """What set_greedy, set_stochastic and set_expected_greedy do: the table (default: the constructor's), the
        refusals in `setter`'s and `who`'s name, the engine's `build`, and the table noted in the attribute `record`."""
        acts = _table(action_space, self._action_space)
        if acts is None:
            raise ValueError(f"{setter} needs an action table: this DevicePolicy was built without one")
        if needs_values and not self._has_values:
            raise RuntimeError(f"{who} needs the value function: call set_values(V) first")
        if not self._has_dynamics:
            raise RuntimeError(f"{who} needs the env's dynamics: call set_dynamics(dynamics_src) first")
        log = build(acts)
        setattr(self, record, acts)
        return log

    # the modules a rollout or a query needs, refused in one place each
    def _need_greedy(self) -> None:
        if self._greedy_actions is None:
            raise RuntimeError("the greedy controller needs set_greedy() (again after every set_dynamics)")

    def _need_expected_greedy(self) -> None:
        if self._expected_actions is None:
            raise RuntimeError("the expected controller needs set_expected_greedy() (again after every set_dynamics)")
        if self._disturbances is None:
            raise RuntimeError("the expected controller needs a disturbance set: call set_disturbances(...) first")

    def _need_stochastic(self, who) -> None:
        if self._stochastic_actions is None:
            raise RuntimeError(f"{who} needs set_stochastic() (again after every set_dynamics)")

    def set_disturbances(self, disturbances) -> None:
        """The ``dynamicprogramming_amd.noise.Disturbances`` set the expected controller takes its expectation over
        (``Disturbances.none(D)``: the deterministic lookahead); ``None`` drops it.  Run-time data: an upload, never a
        build, before or after ``set_expected_greedy``."""
        if disturbances is None:
            self._engine.set_disturbances(None, None, None)
        else:
            if disturbances.D != self.D:
                raise ValueError(f"the disturbance set is {disturbances.D}-D, this policy's grid {self.D}-D")
            self._engine.set_disturbances(disturbances.action_offsets, disturbances.state_offsets, disturbances.weights)
        self._disturbances = disturbances

    def expected_greedy(self, states, gamma, q_values=False):
        """``greedy`` with the expectation over the disturbance set inside Q, in ONE kernel launch — the device twin of
        ``dynamicprogramming_amd.noise.expected_greedy_action``, same bits; the same outputs and in/out conventions.
        After ``set_expected_greedy`` and ``set_disturbances``."""
        self._need_expected_greedy()
        return self._lookahead(self._engine.expect_greedy, self._expected_actions, states, gamma, q_values)

    def random_words(self, seed, first_episode, m, step, block):
        """The random stream the stochastic rollouts draw from, read on the device: the (m, 4) uint32 words of draw
        block ``block`` at step ``step`` of the episodes ``first_episode + 0 .. m`` under ``seed`` (numpy) — the device
        twin of the module's ``random_words``, same bits.  After ``set_stochastic``."""
        self._need_stochastic("random_words")
        torch = self._torch
        m = int(m)
        out = torch.empty((m, 4), dtype=torch.int32, device=self.device)
        self._engine.random_words(_u64(seed), _u64(first_episode), m, step, block, out.data_ptr(), stream=self._stream())
        return out.cpu().numpy().view(np.uint32)

    def greedy(self, states, gamma, q_values=False):
        """The greedy one-step lookahead at ``states`` (m, D) in ONE kernel launch — the device twin of the module's
        ``greedy_action``, same bits: ``(best_index (m,) int32, action (m,) float32, q_best (m,) float32)`` and, with
        ``q_values=True``, the matrix ``Q (m, n_actions)`` float32 behind them.  A numpy array in -> numpy out, a float32
        tensor on this device in -> torch tensors on the device out, like calling this object."""
        self._need_greedy()
        return self._lookahead(self._engine.greedy, self._greedy_actions, states, gamma, q_values)

    def _lookahead(self, launch, actions, states, gamma, q_values):
        """A lookahead query (``greedy``, ``expected_greedy``): the checked points, the output tensors, one launch."""
        torch = self._torch
        on_device, d_pts, m = self._device_states(states)
        best = torch.empty(m, dtype=torch.int32, device=self.device)
        act = torch.empty(m, dtype=torch.float32, device=self.device)
        qb = torch.empty(m, dtype=torch.float32, device=self.device)
        out = [best, act, qb]
        if q_values:
            out.append(torch.empty((m, len(actions)), dtype=torch.float32, device=self.device))
        launch(d_pts.data_ptr(), m, gamma, d_best=best.data_ptr(), d_action=act.data_ptr(), d_q_best=qb.data_ptr(),
               d_q_all=out[3].data_ptr() if q_values else 0, stream=self._stream())
        return tuple(out) if on_device else tuple(x.cpu().numpy() for x in out)

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
        if out_values is not None and not self._has_values:
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

    def rollout(self, states, steps, gamma=1.0, record_every=0, *, epsilon=None, action_noise=None, state_noise=None,
                seed=None, first_episode=None, action_space=None):
        """Closed-loop episodes from ``states`` (m, D) in ONE kernel launch, in/out conventions of ``DevicePolicy.rollout``;
        returns a ``HybridRolloutResult``.  The hybrid kernel is built on first use and again after a new
        ``primary.set_dynamics``.
        With any of the keywords given (the others default to 0) the episodes run in a noisy world — the device twin of
        ``stochastic_hybrid_rollout``, same bits: ``epsilon``, ``action_noise``, ``state_noise``, ``seed`` and
        ``first_episode`` mean what they mean in ``DevicePolicy.rollout`` and draw from the same counters, so the pair and
        a single policy are compared under common random numbers.  The mode rule sees the disturbed state and is applied
        on every step, exploring or not.  An exploring step takes its action from ``action_space``, ONE table for the pair
        (default: the primary's), whose extremes clamp a noisy action.  Returns a ``StochasticHybridRolloutResult``: the
        same fields plus ``switches``, how often each episode changed its mode.  That kernel is built on first use, and
        again after a new ``primary.set_dynamics`` or for another ``action_space``."""
        a, b = self.primary, self.secondary
        if not b._has_policy:
            raise RuntimeError("the secondary DevicePolicy was built without a policy table")
        noisy = any(v is not None for v in (epsilon, action_noise, state_noise, seed, first_episode, action_space))
        if noisy:                                   # a keyword that was not given is 0: no such noise
            noise = _noise_keywords(a, epsilon or 0.0, action_noise or 0.0, state_noise)
            if state_noise is None:
                noise["state_noise"] = np.zeros(a.D, np.float32)
            table = _table(action_space, a._action_space)
            if table is None:
                raise ValueError("a stochastic hybrid rollout needs an exploration table: give action_space")
        on_device, d_start, m, steps, out, outs = a._rollout_buffers(states, steps, record_every)
        torch = a._torch
        second = torch.empty(m, dtype=torch.int32, device=a.device)
        mode = torch.empty(m, dtype=torch.uint8, device=a.device)
        outs.update(d_secondary_steps=second.data_ptr(), d_last_mode=mode.data_ptr())
        out += [second, mode]
        # _built_for (this object) and _partner_stochastic (the primary) rebuild at different times: merging them changes behaviour
        if noisy:
            # the module lives on the primary's handle, and so does the note of what it was built for: HybridPolicy
            # objects that share a primary replace each other's module
            built = a._partner_stochastic
            if built is None or built[0] != a._dynamics_serial or built[1] is not b or not np.array_equal(built[2], table):
                a._engine.set_partner_stochastic(b._engine, table)
                a._partner_stochastic = (a._dynamics_serial, b, table.copy())
            switches = torch.empty(m, dtype=torch.int32, device=a.device)
            a._engine.rollout_hybrid_stochastic(b._engine, d_start.data_ptr(), m, steps, self.enter, self.leave, gamma,
                                                seed=_u64(seed or 0), first_episode=_u64(first_episode or 0),
                                                d_switches=switches.data_ptr(), **noise, **outs)
            return _result(StochasticHybridRolloutResult, on_device, out + [switches])
        if self._built_for != a._dynamics_serial:
            a._engine.set_partner(b._engine)
            self._built_for = a._dynamics_serial
        a._engine.rollout_hybrid(b._engine, d_start.data_ptr(), m, steps, self.enter, self.leave, gamma, **outs)
        return _result(HybridRolloutResult, on_device, out)


def _clamp_point(pts, lo, hi):
    """The reference's ``max(lo, min(x, hi))`` as Python's min / max compare — ``m = hi if hi < x else x``, ``p = m if
    m > lo else lo`` — not ``np.maximum(lo, np.minimum(x, hi))``: a NaN coordinate fails both comparisons and lands on
    ``lo`` (cell 0, t = +0, finite weights), +-inf lands on the bounds, and when ``x`` and a bound are zeros of opposite
    sign the result is ``lo``'s zero on the low side and ``x``'s on the high side.  Every other input: the same value.
    (CPython semantics, from the reference's text run in memory; that numba lowers min / max to the same comparisons is
    read from its source, not from a numba run.)  The device kernels use the same two selects."""
    m = np.where(hi < pts, hi, pts)
    return np.where(m > lo, m, lo)


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
    p = _clamp_point(pts, lo, hi)
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


def _fmaf(a, b, c):
    """``fmaf(a, b, c)`` on float32 arrays, exactly: numpy has no fused multiply-add.  The product of two float32 is
    exact in float64; the sum with c is rounded to ODD there — TwoSum recovers the rounding error, and an inexact sum
    with an even last bit moves to its odd neighbour on the error's side — so the one final rounding to float32 sees
    a sticky bit and cannot round twice."""
    a, b, c = (np.asarray(x, dtype=np.float32) for x in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        s, err = np.atleast_1d(s).ravel(), np.atleast_1d(err).ravel()
        # an overflowed sum leaves a NaN error term: nothing to fix there
        fix = np.flatnonzero(np.isfinite(err) & (err != 0.0) & ((s.view(np.int64) & 1) == 0))
        if len(fix):
            s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0.0, np.inf, -np.inf))
        return s.astype(np.float32).reshape(p.shape)


def _expected_value(points, value_function, bounds_low, bounds_high, grid_shape, strides):
    """E[V] at ``points`` (k, D) in the arithmetic of the training kernels' backup: per dimension
    ``n = (x - lo) / (hi - lo) * (g - 1)`` in float32 (divide, then multiply), clamped to [0, g - 1] (a NaN lands on the
    top border), ``i = min(int(n), g - 2)``, ``frac = n - i``; corner c takes bit d of c for dimension d (2-D: dimension
    1 toggles fastest), its weight the left-to-right float32 product from 1, its index ``sum (i_d + bit) * stride_d``
    in int32; one fmaf chain over ascending corners from 0."""
    pts = np.asarray(points, dtype=np.float32)
    V = np.asarray(value_function, dtype=np.float32).ravel()
    lo, hi = np.asarray(bounds_low, dtype=np.float32), np.asarray(bounds_high, dtype=np.float32)
    g, st = np.asarray(grid_shape, dtype=np.int32), np.asarray(strides, dtype=np.int32)
    k, D = pts.shape
    corners = np.arange(1 << D)
    w = np.ones((k, 1 << D), np.float32)                       # all corners at once: one multiply per dimension, in order
    idx = np.zeros((k, 1 << D), np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(D):
            top = np.float32(g[d] - 1)
            n = (pts[:, d] - lo[d]) / np.float32(hi[d] - lo[d]) * top
            n = np.fmax(np.float32(0.0), np.fmin(n, top))
            i = np.minimum(n.astype(np.int32), np.int32(g[d] - 2))
            frac = n - i.astype(np.float32)
            bit = ((corners >> (1 - d if D == 2 else d)) & 1).astype(np.int32)
            w = w * np.where(bit[None, :] == 1, frac[:, None], (np.float32(1.0) - frac)[:, None])
            idx = idx + (i[:, None] + bit[None, :]) * st[d]
        values = V[idx]
        e = np.zeros(k, np.float32)
        for c in corners:
            e = _fmaf(w[:, c], values[:, c], e)
    return e


def greedy_action(step, points, value_function, action_space, bounds_low, bounds_high, grid_shape, strides, gamma,
                  q_values=False):
    """Greedy one-step lookahead on the interpolated value function at ``points`` (m, D) (numpy): the twin of
    ``DevicePolicy.greedy``, same definition.  ``step`` is the batched env step ``rollout`` takes.  For every action
    ``a`` of ``action_space`` in ascending order: ``(s', r, done) = step(points, a)``, ``E = 0`` where done and the
    interpolation of ``_expected_value`` elsewhere, ``Q = r + gamma * E`` in float32 (multiply, then add); the greedy
    action is the strict ``>`` argmax from -1e30: the lowest index wins ties, NaN never wins, index 0 with Q = -1e30
    when nothing wins.  Returns ``(best_index int32, action float32, q_best float32)`` and, with ``q_values=True``,
    ``Q (m, n_actions)`` float32."""
    pts = np.ascontiguousarray(np.atleast_2d(points), dtype=np.float32)
    acts = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
    m = len(pts)
    g32 = np.float32(gamma)
    best = np.zeros(m, np.int32)
    best_q = np.full(m, np.float32(-1.0e30), np.float32)
    Q = np.empty((m, len(acts)), np.float32)
    for a, u in enumerate(acts):
        nxt, rew, done = step(pts, np.full(m, u, np.float32))
        nxt, done = np.asarray(nxt, np.float32), np.asarray(done, bool)
        e = np.zeros(m, np.float32)
        if not done.all():
            e[~done] = _expected_value(nxt[~done], value_function, bounds_low, bounds_high, grid_shape, strides)
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.asarray(rew, np.float32) + g32 * e
            wins = q > best_q
        Q[:, a] = q
        best_q = np.where(wins, q, best_q)
        best = np.where(wins, np.int32(a), best)
    out = (best, acts[best], best_q)
    return out + (Q,) if q_values else out


def greedy_rollout(step, states, steps, value_function, action_space, bounds_low, bounds_high, grid_shape, strides,
                   lookahead_gamma, gamma=1.0, record_every=0):
    """Closed-loop episodes under the value-greedy controller on the CPU (numpy): the twin of
    ``DevicePolicy.rollout(controller="greedy")``.  Per step the action value ``greedy_action`` returns for the state
    with the discount ``lookahead_gamma``; the step's bookkeeping, ``gamma`` and ``record_every`` are ``rollout``'s.
    Returns a ``RolloutResult`` of numpy arrays."""
    tables = (value_function, action_space, bounds_low, bounds_high, grid_shape, strides, lookahead_gamma)
    return RolloutResult(*_closed_loop(step, states, steps, gamma, record_every,
                                       lambda live, pts: greedy_action(step, pts, *tables)[1]))


# ── the random stream of the stochastic rollouts (csrc/pi_stochastic_kernels.hip), same bits ──────────────────────────
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 as published (Salmon et al., SC'11), vectorised: ``counter`` (..., 4) and ``key`` (..., 2) uint32
    words (broadcast against each other) -> (..., 4) uint32 words."""
    c = np.asarray(counter, dtype=np.uint32)
    k = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).astype(np.uint64) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).astype(np.uint64) for i in range(2))
    for r in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2             # 32 x 32 -> 64 bits: exact in uint64
        kr0 = (k0 + np.uint64((_PHILOX_W0 * r) & 0xFFFFFFFF)) & _U32
        kr1 = (k1 + np.uint64((_PHILOX_W1 * r) & 0xFFFFFFFF)) & _U32
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ kr0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ kr1, p0 & _U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def random_words(seed, first_episode, m, step, block):
    """The stream of the stochastic rollouts: the (m, 4) uint32 words of draw block ``block`` at step ``step`` for the
    episodes ``first_episode + 0 .. m`` under ``seed`` — key = (low, high 32 bits of the uint64 seed), counter = (low,
    high 32 bits of the uint64 episode number, step, block).  The twin of ``DevicePolicy.random_words``."""
    return _episode_words(seed, _episode_numbers(first_episode, np.arange(int(m))), step, block)


def _episode_numbers(first_episode, rows):
    """first_episode + rows as uint64 (wrapping at 2^64, as the kernel's addition does)."""
    with np.errstate(over="ignore"):
        return np.uint64(_u64(first_episode)) + np.asarray(rows).astype(np.uint64)


def _episode_words(seed, episodes, step, block):
    seed = _u64(seed)
    e = np.asarray(episodes, dtype=np.uint64)
    counter = np.empty(e.shape + (4,), np.uint32)
    counter[..., 0] = (e & _U32).astype(np.uint32)
    counter[..., 1] = (e >> np.uint64(32)).astype(np.uint32)
    counter[..., 2] = np.uint32(int(step) & 0xFFFFFFFF)
    counter[..., 3] = np.uint32(int(block) & 0xFFFFFFFF)
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32))


def sym(words):
    """A uint32 word as a float32 in [-1, 1): ``(float)((int)(x >> 8) - 8388608) * 2^-23``, every value exact."""
    x = np.asarray(words, dtype=np.uint32)
    return ((x >> np.uint32(8)).astype(np.int32) - np.int32(8388608)).astype(np.float32) * np.float32(2.0 ** -23)


def explore_threshold(epsilon) -> int:
    """eps24 of the exploration coin — a step explores iff ``(x0 >> 8) < eps24`` — from the float32 ``epsilon`` as the
    library computes it: ``llrint((double)epsilon * 2^24)``.  0 never explores, 2^24 always does."""
    eps = float(np.float32(epsilon))
    if not 0.0 <= eps <= 1.0:
        raise ValueError("epsilon must lie in [0, 1]")
    return round(eps * 16777216.0)                 # exact in double, ties to even: llrint


def random_action_index(words, n_actions):
    """The exploring step's action index: ``(uint32)(((uint64)x1 * n_actions) >> 32)``."""
    return ((np.asarray(words, dtype=np.uint32).astype(np.uint64) * np.uint64(int(n_actions))) >> np.uint64(32)).astype(np.int64)


def _noise_vector(state_noise, D):
    """state_noise as D float32 values: None = none, one value = every dimension, or D values; finite, not negative."""
    if state_noise is None:
        return np.zeros(D, np.float32)
    v = np.atleast_1d(np.asarray(state_noise, dtype=np.float32)).ravel()
    if len(v) == 1:
        v = np.repeat(v, D)
    if len(v) != D:
        raise ValueError(f"state_noise must hold one value or {D}")
    if not (np.isfinite(v).all() and (v >= 0).all()):
        raise ValueError("state_noise must be finite and not negative")
    return np.ascontiguousarray(v)


def _checked_action_noise(action_noise) -> np.float32:
    a = np.float32(action_noise)
    if not 0 <= a < np.inf:
        raise ValueError("action_noise must be finite and not negative")
    return a


def stochastic_rollout(step, states, steps, policy, action_space, bounds_low, bounds_high, grid_shape, strides,
                       corner_bits, epsilon, action_noise, state_noise, seed, first_episode=0, gamma=1.0, record_every=0):
    """Closed-loop episodes with epsilon-random actions, action noise and state noise on the CPU (numpy): the twin of
    ``DevicePolicy.rollout(epsilon=..., action_noise=..., state_noise=..., seed=..., first_episode=...)``, same bits.
    Episode ``i`` of the batch draws from the stream of episode number ``first_episode + i`` (``random_words``), so a
    batch cut into several calls gives the results of one.  Per step of a running episode, in this order: the
    interpolated action of ``rollout`` (``policy`` may be None when ``epsilon == 1``, the random-policy baseline); an
    exploring step (block 0: ``(x0 >> 8) < explore_threshold(epsilon)``) takes ``action_space[random_action_index(x1)]``
    instead; ``action_noise != 0`` adds ``action_noise * sym(x2)`` (multiply, then add) and clamps to the extremes of
    ``action_space`` (no clamp otherwise); ``step``; then, unless the step was `done`, every dimension d with
    ``state_noise[d] != 0`` of the successor gains ``state_noise[d] * sym(word d)`` (block 1 for d < 4, block 2 for
    d = 4, 5) — not clamped, not wrapped, and it is the state the next step starts from and the trajectory records.
    The bookkeeping, ``gamma`` and ``record_every`` are ``rollout``'s.  Returns a ``RolloutResult`` of numpy arrays."""
    acts = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
    if policy is None and explore_threshold(epsilon) != 1 << 24:
        raise ValueError("epsilon < 1 acts on the policy: a rollout without one needs epsilon = 1")
    tables = (policy, acts, bounds_low, bounds_high, grid_shape, strides, corner_bits)

    def controller(pts, wanted):
        return np.zeros(len(pts), np.float32) if policy is None else _interpolated_actions(pts, *tables)
    return _noisy_closed_loop(step, states, steps, controller, acts, epsilon, action_noise, state_noise, seed,
                              first_episode, gamma, record_every)


def stochastic_hybrid_rollout(step, states, steps, primary, secondary, enter, leave, action_space, epsilon, action_noise,
                              state_noise, seed, first_episode=0, gamma=1.0, record_every=0):
    """Closed-loop episodes that switch between two policies under epsilon-random actions, action noise and state noise,
    on the CPU (numpy): the twin of ``HybridPolicy.rollout(epsilon=..., action_noise=..., state_noise=..., seed=...,
    first_episode=..., action_space=...)``, same bits.  ``hybrid_rollout`` inside the loop of ``stochastic_rollout``: per
    step of a running episode ``switch_mode`` on the state the step starts from — disturbed or not, exploring or not —,
    ``secondary_steps`` counts the steps in mode 1 and ``switches`` those whose mode differs from that of the step taken
    before (mode 0 before step 0); an exploring step takes its action from ``action_space``, the ONE exploration table of
    the pair, any other the interpolated action of the mode's policy on its own grid; action noise (clamped to the
    extremes of ``action_space``), ``step`` and state noise as in ``stochastic_rollout``, from the same words.  Returns a
    ``StochasticHybridRolloutResult``."""
    m = len(np.atleast_2d(states))
    mode = np.zeros(m, bool)
    second = np.zeros(m, np.int32)
    switches = np.zeros(m, np.int32)

    def controller(pts, wanted, live):
        now = switch_mode(mode[live], pts, enter, leave)
        switches[live] += now != mode[live]
        mode[live] = now
        second[live] += now
        a = np.zeros(len(live), np.float32)
        for which, tables in ((~now & wanted, primary), (now & wanted, secondary)):
            if which.any():
                a[which] = _interpolated_actions(pts[which], *tables)
        return a
    res = _noisy_closed_loop(step, states, steps, controller, action_space, epsilon, action_noise, state_noise, seed,
                             first_episode, gamma, record_every, with_live=True)
    return StochasticHybridRolloutResult(*res, second, mode.astype(np.uint8), switches)


def _noisy_closed_loop(step, states, steps, controller, action_space, epsilon, action_noise, state_noise, seed,
                       first_episode, gamma, record_every, with_live=False):
    """The loop ``stochastic_rollout`` documents, for any controller: ``controller(states (k, D), wanted (k,) bool) ->
    actions (k,) float32`` is asked for the running episodes; only the entries where ``wanted`` (the episode does not
    explore this step) are used.  ``with_live``: the controller keeps state per episode and is handed the indices of the
    running episodes as a third argument.  Returns a ``RolloutResult``."""
    acts = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
    if len(acts) < 1 or not np.isfinite(acts).all():
        raise ValueError("action_space needs at least one action, all finite")
    eps24 = explore_threshold(epsilon)
    a_noise = _checked_action_noise(action_noise)
    D = np.atleast_2d(states).shape[1]
    s_noise = _noise_vector(state_noise, D)
    a_min, a_max = acts.min(), acts.max()
    now = {"t": -1, "episodes": None}                 # _closed_loop asks act() once per step, then steps those episodes

    def act(live, pts):
        now["t"] += 1
        now["episodes"] = _episode_numbers(first_episode, live)
        w = _episode_words(seed, now["episodes"], now["t"], 0)
        explore = (w[:, 0] >> np.uint32(8)) < eps24
        a = np.asarray(controller(pts, ~explore, live) if with_live else controller(pts, ~explore), np.float32)
        a = np.where(explore, acts[random_action_index(w[:, 1], len(acts))], a).astype(np.float32)
        if a_noise != 0:
            with np.errstate(invalid="ignore"):
                a = a + a_noise * sym(w[:, 2])
                a = np.fmin(np.fmax(a, a_min), a_max)
        return a

    def noisy_step(pts, a):
        nxt, rew, done = step(pts, a)
        nxt, done = np.array(nxt, dtype=np.float32), np.asarray(done, bool)
        if s_noise.any():
            words = _episode_words(seed, now["episodes"], now["t"], 1)
            if D > 4:
                words = np.concatenate([words, _episode_words(seed, now["episodes"], now["t"], 2)], axis=1)
            go = ~done
            for d in range(D):
                if s_noise[d] != 0:
                    nxt[go, d] = nxt[go, d] + s_noise[d] * sym(words[go, d])
        return nxt, rew, done
    return RolloutResult(*_closed_loop(noisy_step, states, steps, gamma, record_every, act))
