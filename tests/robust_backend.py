"""CPU stand-in for the worst-case sweeps of HipSweepBackend, for HOST-LOGIC tests and as the reference of the GPU solver
test: tests.noise_backend.NoiseSweepBackend with ``robust_*`` computed by the numpy twins of dynamicprogramming_amd.noise
with ``risk="worst"`` on the checker's ``step``.  Lives under tests/ so the product can never pick it up."""
from __future__ import annotations

import numpy as np

from dynamicprogramming_amd import noise
from tests.noise_backend import NoiseSweepBackend


class RobustSweepBackend(NoiseSweepBackend):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.calls.update({"robust_eval": 0, "robust_improve": 0, "robust_value": 0})

    def robust_eval_sweeps(self, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta):
        self._whole(s_begin, s_end)
        for i in range(n_sweeps):
            src, dst = (Vb, Va) if (i & 1) else (Va, Vb)
            out = np.ascontiguousarray(self._u(dst)).copy()
            _, delta = noise.expected_eval(self.lib.step, self.states, self._u(policy), np.ascontiguousarray(self._u(src)),
                                           self._term(term), *self._tables(), gamma, s_begin, s_end, out=out, risk="worst")
            dst.numpy()[:self.n] = self.to_memory(out)
            self.calls["robust_eval"] += 1
            if d_delta is not None and i == n_sweeps - 1:
                d_delta[0] = float(delta)

    def robust_improve_sweep(self, V, policy, term, s_begin, s_end, gamma, d_changed):
        self._whole(s_begin, s_end)
        new_pol, changed = noise.expected_improve(self.lib.step, self.states, self._u(policy), self._u(V), self._term(term),
                                                  *self._tables(), gamma, s_begin, s_end, risk="worst")
        self._store_policy(policy, new_pol, s_begin, s_end)
        self.calls["robust_improve"] += 1
        if d_changed is not None:
            d_changed[0] = changed

    def robust_value_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta, d_changed):
        self._whole(s_begin, s_end)
        out = np.ascontiguousarray(self._u(Vnew)).copy()
        _, new_pol, delta, changed = noise.expected_value_sweep(self.lib.step, self.states, self._u(policy), self._u(V),
                                                                self._term(term), *self._tables(), gamma, s_begin, s_end,
                                                                out=out, risk="worst")
        Vnew.numpy()[:self.n] = self.to_memory(out)
        self._store_policy(policy, new_pol, s_begin, s_end)
        self.calls["robust_value"] += 1
        if d_delta is not None:
            d_delta[0] = float(delta)
        if d_changed is not None:
            d_changed[0] = changed


def with_robust_backend(cls):
    """tests.helpers.with_checker_backend with the backend above."""
    def __init__(self, *args, **kwargs):
        from dynamicprogramming_amd import solver as S
        saved = (S.HipSweepBackend, S.GPU_AVAILABLE)
        S.HipSweepBackend, S.GPU_AVAILABLE = RobustSweepBackend, True
        try:
            cls.__init__(self, *args, **kwargs)
        finally:
            S.HipSweepBackend, S.GPU_AVAILABLE = saved
    return type(cls.__name__ + "OnRobustChecker", (cls,), {"__init__": __init__})
