"""CPU stand-in for the expectation sweeps of HipSweepBackend, for HOST-LOGIC tests and as the reference of the GPU
solver test: tests.helpers.OracleSweepBackend with ``expect_*`` computed by the numpy twins of
dynamicprogramming_amd.noise on the checker's ``step``.  Lives under tests/ so the product can never pick it up."""
from __future__ import annotations

import numpy as np

from dynamicprogramming_amd import noise
from tests import helpers as H


class NoiseSweepBackend(H.OracleSweepBackend):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.disturbances = None
        self.calls.update({"expect_eval": 0, "expect_improve": 0, "expect_value": 0, "value": 0})

    def set_disturbances(self, disturbances) -> int:
        self.disturbances = disturbances
        return 0 if disturbances is None else disturbances.K

    def value_sweep(self, *args, **kwargs):
        self.calls["value"] += 1
        return super().value_sweep(*args, **kwargs)

    def _tables(self):
        assert self.disturbances is not None, "expect_* without a disturbance set"
        return (self.disturbances, self.actions, self.lo, self.hi, self.shape, self.strides)

    def _term(self, term):
        return None if term is None else self._u(term).astype(bool)

    def expect_eval_sweeps(self, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta):
        self._whole(s_begin, s_end)
        for i in range(n_sweeps):
            src, dst = (Vb, Va) if (i & 1) else (Va, Vb)
            out = np.ascontiguousarray(self._u(dst)).copy()
            _, delta = noise.expected_eval(self.lib.step, self.states, self._u(policy), np.ascontiguousarray(self._u(src)),
                                           self._term(term), *self._tables(), gamma, s_begin, s_end, out=out)
            dst.numpy()[:self.n] = self.to_memory(out)
            self.calls["expect_eval"] += 1
            if d_delta is not None and i == n_sweeps - 1:
                d_delta[0] = float(delta)

    def _store_policy(self, policy, new_pol, s_begin, s_end):
        if self.order is None:
            policy.numpy()[:self.n][s_begin:s_end] = new_pol[s_begin:s_end]
        else:
            policy.numpy()[:self.n] = self.to_memory(new_pol)

    def expect_improve_sweep(self, V, policy, term, s_begin, s_end, gamma, d_changed):
        self._whole(s_begin, s_end)
        new_pol, changed = noise.expected_improve(self.lib.step, self.states, self._u(policy), self._u(V), self._term(term),
                                                  *self._tables(), gamma, s_begin, s_end)
        self._store_policy(policy, new_pol, s_begin, s_end)
        self.calls["expect_improve"] += 1
        if d_changed is not None:
            d_changed[0] = changed

    def expect_value_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta, d_changed):
        self._whole(s_begin, s_end)
        out = np.ascontiguousarray(self._u(Vnew)).copy()
        _, new_pol, delta, changed = noise.expected_value_sweep(self.lib.step, self.states, self._u(policy), self._u(V),
                                                                self._term(term), *self._tables(), gamma, s_begin, s_end,
                                                                out=out)
        Vnew.numpy()[:self.n] = self.to_memory(out)
        self._store_policy(policy, new_pol, s_begin, s_end)
        self.calls["expect_value"] += 1
        if d_delta is not None:
            d_delta[0] = float(delta)
        if d_changed is not None:
            d_changed[0] = changed


def with_noise_backend(cls):
    """tests.helpers.with_checker_backend with the backend above."""
    def __init__(self, *args, **kwargs):
        from dynamicprogramming_amd import solver as S
        saved = (S.HipSweepBackend, S.GPU_AVAILABLE)
        S.HipSweepBackend, S.GPU_AVAILABLE = NoiseSweepBackend, True
        try:
            cls.__init__(self, *args, **kwargs)
        finally:
            S.HipSweepBackend, S.GPU_AVAILABLE = saved
    return type(cls.__name__ + "OnNoiseChecker", (cls,), {"__init__": __init__})
