"""CPU stand-in for the acceleration entry points of HipSweepBackend, for HOST-LOGIC tests and as the reference of the GPU
solver tests: tests.noise_backend.NoiseSweepBackend (the oracle's sweeps, the expectation sweeps' numpy twins) with
``accel_update`` / ``accel_combine`` computed by the numpy twin of dynamicprogramming_amd.accel on the tensors' own
memory — memory order, as the device kernels see them.  Lives under tests/ so the product can never pick it up."""
from __future__ import annotations

from dynamicprogramming_amd import accel
from tests.noise_backend import NoiseSweepBackend


class AccelSweepBackend(NoiseSweepBackend):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.calls.update({"accel_update": 0, "accel_combine": 0})

    def accel_update(self, x, g, f_prev, g_prev, dF, dG, slot, k_used, first, n, d_dots):
        values = accel.dots(x.numpy()[:n], g.numpy()[:n], f_prev.numpy()[:n], g_prev.numpy()[:n], dF.numpy()[:, :n],
                            dG.numpy()[:, :n], slot, k_used, bool(first))
        d_dots.numpy()[:len(values)] = values
        self.calls["accel_update"] += 1

    def accel_combine(self, g, dG, coeffs, k_used, n, out):
        accel.combine(g.numpy()[:n], dG.numpy()[:, :n], coeffs, k_used, out=out.numpy()[:n])
        self.calls["accel_combine"] += 1


def with_accel_backend(cls):
    """tests.helpers.with_checker_backend with the backend above."""
    def __init__(self, *args, **kwargs):
        from dynamicprogramming_amd import solver as S
        saved = (S.HipSweepBackend, S.GPU_AVAILABLE)
        S.HipSweepBackend, S.GPU_AVAILABLE = AccelSweepBackend, True
        try:
            cls.__init__(self, *args, **kwargs)
        finally:
            S.HipSweepBackend, S.GPU_AVAILABLE = saved
    return type(cls.__name__ + "OnAccelChecker", (cls,), {"__init__": __init__})
