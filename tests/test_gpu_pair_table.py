"""
The improvement sweep on the pair table (PI_OPTION_PAIR_TABLE; csrc/pi_sweep_kernels.hip, PI_PAIR_TABLE) against the plain
sweep and the CPU checker, bit for bit, over ALL states of grids small enough to take a moment: policy and changed count
of three runs per case — option 1, option 0, the checker.

What the table could get wrong, and the case that shows it: which component of a 16-byte quad is which corner (V ~ 30 N(0, 1):
every one of the 16 values of a cell decides the argmax somewhere), the stride of the second-to-last MEMORY dimension
(memory orders other than the env's), the top row and column (successors clamped onto the border by the cell search), the
branch without corner reuse (5 actions), the live-list kernel (a terminal mask), a state count that is no multiple of 256.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info, Option
from tests import helpers as H

pytestmark = pytest.mark.gpu

# (env, shape, memory order or None, keep a live-state list)
CASES = [
    ("double_pendulum_swingup", (6, 6, 6, 6), None, False),
    ("double_pendulum_swingup", (6, 6, 6, 6), (0, 2, 1, 3), False),
    ("double_pendulum_swingup", (9, 9, 9, 9), None, False),
    ("double_pendulum_swingup", (9, 9, 9, 9), (0, 2, 1, 3), False),
    ("double_pendulum_swingup", (9, 9, 9, 9), (3, 1, 0, 2), False),
    ("cartpole_swingup", (7, 7, 7, 7), None, False),           # 5 actions: the branch without corner reuse
    ("cartpole", (8, 9, 8, 9), None, True),                    # terminal mask + live list: pi_improve_live_kernel
    ("overhead_crane", (6, 6, 6, 6), None, False),
]
IDS = [f"{name}-{'x'.join(map(str, shape))}-{'env' if order is None else ''.join(map(str, order))}" for name, shape, order, _ in CASES]


def _torch():
    import torch
    return torch


class _Case:
    """Grid, seeded (V, policy, mask) in the user's order, and the checker's improvement sweep on them — computed once."""

    def __init__(self, name, shape):
        cls = envs.ENVS[name]
        self.name, self.shape, self.cls = name, tuple(shape), cls
        self.bins = H.env_bins(name, shape)
        self.acts = np.asarray(cls.ACTIONS, dtype=np.float32)
        self.meta = oracle.grid_metadata(self.bins)
        self.states = oracle.states_from_bins(self.bins)
        self.n = len(self.states)
        assert self.n % 256 != 0
        self.term, tval = H.terminal_mask(name, self.states)
        rng = np.random.default_rng(1109)
        self.V = (rng.standard_normal(self.n) * 30.0).astype(np.float32)
        self.V[self.term] = np.float32(tval)
        self.V2 = (rng.standard_normal(self.n) * 30.0).astype(np.float32)      # what a caller writes into V between two calls
        self.V2[self.term] = np.float32(tval)
        self.pol = rng.integers(0, len(self.acts), size=self.n).astype(np.int32)
        self.pol[self.term] = 0
        self.gamma = float(np.float32(cls.CONFIG["gamma"]))
        chk = H.oracle_for(name)
        self.ref = {0: chk.improve_sweep(self.states, self.acts, self.pol, self.V, self.term, *self.meta, self.gamma),
                    1: chk.improve_sweep(self.states, self.acts, self.pol, self.V2, self.term, *self.meta, self.gamma)}

    def engine(self, dev, order, option):
        """An engine of this grid whose unit was built with the option as given (None: left alone)."""
        eng = _native.Engine(self.cls._D, [len(b) for b in self.bins], [b.min() for b in self.bins],
                             [b.max() for b in self.bins], self.bins, self.acts, device=dev.index or 0, order=order)
        if option is not None:
            eng.set_option(Option.PAIR_TABLE, option)
        eng.compile(envs.dynamics_source(self.name))
        return eng


_cases: dict = {}


def _case(name, shape) -> _Case:
    key = (name, tuple(shape))
    if key not in _cases:
        _cases[key] = _Case(name, shape)
    return _cases[key]


def _improve(c, eng, dev, V, live=False, s_begin=0, s_end=None, d_V=None):
    """One improvement sweep of `eng` from the seeded policy: (policy in the user's order, changed, info selector)."""
    torch = _torch()
    if d_V is None:
        d_V = torch.from_numpy(np.ascontiguousarray(eng.to_memory(V))).to(dev)
    d_pol = torch.from_numpy(np.ascontiguousarray(eng.to_memory(c.pol))).to(dev)
    d_term = torch.from_numpy(np.ascontiguousarray(eng.to_memory(c.term.astype(np.uint8)))).to(dev)
    d_changed = torch.full((1,), 77, dtype=torch.int32, device=dev)
    if live:
        eng.set_option(Option.KEEP_LIVE_LIST, 1)
        assert eng.prepare_mask(d_term.data_ptr()) == int((~c.term).sum())
    eng.improve_sweep(d_V.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), s_begin, c.n if s_end is None else s_end, c.gamma,
                      d_changed.data_ptr())
    torch.cuda.synchronize()
    return eng.to_user(d_pol.cpu().numpy()), int(d_changed.item()), eng.info(Info.PAIR_TABLE)


@pytest.mark.parametrize("name,shape,order,live", CASES, ids=IDS)
def test_table_sweep_equals_plain_sweep_and_checker(name, shape, order, live, cuda_device, monkeypatch):
    if live:
        monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")             # the list is kept from 2^20 states on by default
    c = _case(name, shape)
    o_pol, o_changed = c.ref[0]
    results = {}
    eng = c.engine(cuda_device, order, 1)            # one unit holds the table kernels and the plain ones: the option picks
    for option in (1, 0):
        eng.set_option(Option.PAIR_TABLE, option)
        pol, changed, used = _improve(c, eng, cuda_device, c.V, live)
        if live:
            assert eng.info(Info.LIVE_STATES) > 0
        assert used == option, f"option {option}: PI_INFO_PAIR_TABLE says {used}"
        results[option] = (pol, changed)
    eng.close()
    for option, (pol, changed) in results.items():
        assert np.array_equal(pol, o_pol), f"{name} {shape} {order}: policy of option {option} against the checker"
        assert changed == o_changed, (option, changed, o_changed)
    assert np.array_equal(results[0][0], results[1][0]) and results[0][1] == results[1][1]


def test_partial_range_takes_the_plain_path(cuda_device):
    c = _case("double_pendulum_swingup", (9, 9, 9, 9))
    a, b = 700, 5003
    on = c.engine(cuda_device, None, 1)
    pol1, changed1, used1 = _improve(c, on, cuda_device, c.V, s_begin=a, s_end=b)
    on.close()
    off = c.engine(cuda_device, None, 0)
    pol0, changed0, used0 = _improve(c, off, cuda_device, c.V, s_begin=a, s_end=b)
    off.close()
    assert used1 == 0 and used0 == 0
    assert np.array_equal(pol1, pol0) and changed1 == changed0
    o_pol = c.ref[0][0]
    assert np.array_equal(pol1[a:b], o_pol[a:b])
    assert np.array_equal(pol1[:a], c.pol[:a]) and np.array_equal(pol1[b:], c.pol[b:])        # outside the range: untouched


def test_the_table_is_packed_again_on_every_call(cuda_device):
    """Callers write V behind the library's back: a second call on the same buffer with new values sees the new values."""
    torch = _torch()
    c = _case("double_pendulum_swingup", (9, 9, 9, 9))
    eng = c.engine(cuda_device, (0, 2, 1, 3), 1)
    d_V = torch.from_numpy(np.ascontiguousarray(eng.to_memory(c.V))).to(cuda_device)
    pol, changed, used = _improve(c, eng, cuda_device, None, d_V=d_V)
    assert used == 1 and np.array_equal(pol, c.ref[0][0]) and changed == c.ref[0][1]
    d_V.copy_(torch.from_numpy(np.ascontiguousarray(eng.to_memory(c.V2))).to(cuda_device))
    pol, changed, used = _improve(c, eng, cuda_device, None, d_V=d_V)
    eng.close()
    assert used == 1 and np.array_equal(pol, c.ref[1][0]) and changed == c.ref[1][1]
    off = c.engine(cuda_device, (0, 2, 1, 3), 0)
    pol0, changed0, used0 = _improve(c, off, cuda_device, c.V2)
    off.close()
    assert used0 == 0 and np.array_equal(pol, pol0) and changed == changed0


def test_auto_leaves_small_grids_on_the_plain_path_and_on_needs_the_kernels(cuda_device):
    c = _case("cartpole_swingup", (7, 7, 7, 7))
    eng = c.engine(cuda_device, None, None)
    pol, changed, used = _improve(c, eng, cuda_device, c.V)
    assert used == 0 and np.array_equal(pol, c.ref[0][0]) and changed == c.ref[0][1]
    # the unit was built without the table kernels: switching on now is refused, off and auto are accepted
    with pytest.raises(_native.NativeError, match="before pi_compile"):
        eng.set_option(Option.PAIR_TABLE, 1)
    eng.set_option(Option.PAIR_TABLE, 0)
    eng.set_option(Option.PAIR_TABLE, -1)
    eng.close()
    # a unit built with them can be switched off and on again at any time
    on = c.engine(cuda_device, None, 1)
    on.set_option(Option.PAIR_TABLE, 0)
    assert _improve(c, on, cuda_device, c.V)[2] == 0
    on.set_option(Option.PAIR_TABLE, -1)                      # the library's choice for 2 401 states, kernels or not
    assert _improve(c, on, cuda_device, c.V)[2] == 0
    on.set_option(Option.PAIR_TABLE, 1)
    pol, changed, used = _improve(c, on, cuda_device, c.V)
    on.close()
    assert used == 1 and np.array_equal(pol, c.ref[0][0]) and changed == c.ref[0][1]
