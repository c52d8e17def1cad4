"""
The top half of the 32-bit byte-offset range: grids between the sizes the suite ran (n <= 2^24 at the dispatch edges, about
4 x 10^7 states at full size) and the 64-bit addressing form of tests/test_gpu_addr64.py (n >= 2^30).

pi_request_corners addresses V with `base * 4u + far * 4u` while 4 n < 2^32, pi_request_corners_pairs the pair table with
`base * 8u + far * 8u` while 8 n < 2^32 (csrc/pi_sweep_kernels.hip): V offsets reach 2^31 bytes from n >= 2^29, pair-table
offsets from n >= 2^28 — where a signed/unsigned slip in either expression, or in how the compiler folds it into the
load's offset operand, would first show, and where the pair table is on by default (n >= 2^24).

* double_pendulum_swingup (152, 152, 151, 153), n = 533 771 712 in [2^28, 2^29): the pair table, default options, the
  env's order and (0, 2, 1, 3); table against plain sweep on the whole grid, against the oracle at the samples.
* double_pendulum_swingup (160, 161, 159, 162), n = 663 526 080 in [2^29, 2^30): V in the 32-bit form, the table refused
  whatever the option says (8 n >= 2^32: PI_PAIR_OFF32 == false is unreachable); evaluation, improvement, value sweep.
* double_cartpole (27, 28, 29, 30, 31, 32), n = 652 458 240, the class's MEMORY_ORDER, its terminal mask, no list kernels.

Bar: bit for bit against the CPU oracle's point-list entries at 2^20 states scattered over the table, 2^18 in its last
2^24 states, and the states (at least 10 000) whose successor cell lies in the top 1/64 of the table, where 8 * base or
4 * base >= 2^31 certainly holds; residuals and changed counts against torch reductions over the whole grid.  Helpers are
those of tests/test_gpu_addr64.py.  Every test closes its engine and frees its tensors.

Measured on an MI355X in one `pytest -m gpu --durations=0` run of the whole suite (521 s): pair table 2.24 s (env order)
and 2.20 s ((0, 2, 1, 3)), V 4-D 2.70 s, V 6-D 2.90 s — the existing 4-D test of tests/test_gpu_addr64.py took 4.13 and
3.74 s in that run.  Peak device memory as torch counts it (the library's 4.3 GB pair table is not in the figure): pair
table 10.4 GiB per order, V 4-D 15.5 GiB, V 6-D 15.8 GiB.  States found with their successor cell in the top 1/64 of the
table (of ~1.0 M candidates): 136 337 / 161 575, 138 233, 166 413.

Not run, judged from the code: `.y` and `.z` swapped in pi_request_corners_pairs changes the argmax wherever two corner
values differ (tests/test_gpu_pair_table.py shows that on small grids; here the table-against-plain comparison over the
whole grid would); `base * 8u` as a signed int product widened to 64 bits is negative from base >= 2^28 on, an address
in front of the table — every state of the top-1/64 sample reads there.
"""
from __future__ import annotations

import numpy as np
import pytest

from dynamicprogramming_amd import envs
from dynamicprogramming_amd._native import Info, Option
from tests.test_gpu_addr64 import (_check_at, _free, _grid, _report_peak, _seeded_state, _single_sweeps_and_samples,
                                   _tail_sample, _top_successor_sample, _torch)
from tests.test_gpu_fullsize import _term_c5

pytestmark = pytest.mark.gpu

DEFINE = "#define PI_PAIR_TABLE"
SHAPE_PAIRS = (152, 152, 151, 153)              # n = 533 771 712: 8 n in [2^31, 2^32)
SHAPE_V_4D = (160, 161, 159, 162)               # n = 663 526 080: 4 n in [2^31, 2^32), 8 n >= 2^32
SHAPE_V_6D = (27, 28, 29, 30, 31, 32)           # n = 652 458 240


def _ragged(shape):
    strides = np.cumprod((shape[1:] + (1,))[::-1])[::-1]
    return int(np.prod(shape, dtype=np.int64)) % 256 != 0 and all(int(s) & (int(s) - 1) for s in strides[:-1])


@pytest.mark.parametrize("order", [None, (0, 2, 1, 3)], ids=["env-order", "permuted-order"])
def test_pair_table_byte_offsets_beyond_2_pow_31(order, cuda_device):
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    name = "double_pendulum_swingup"
    g = _grid(name, SHAPE_PAIRS, order, cuda_device, form64=False)
    try:
        n, eng = g.n, g.eng
        assert n == 533_771_712 and 1 << 28 <= n < 1 << 29 and _ragged(tuple(g.mem_shape))
        assert DEFINE + " 1\n" in eng.kernel_source(envs.dynamics_source(name))        # the library's own choice
        # V ~ 30 N(0, 1): every one of the 16 values of a cell decides the argmax somewhere (tests/test_gpu_pair_table.py)
        Vh, polh, _, d_V, d_pol, _ = _seeded_state(g, 13, None, cuda_device, scale=30.0)
        d_changed = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        d_p1 = d_pol.clone()
        eng.improve_sweep(d_V.data_ptr(), d_p1.data_ptr(), 0, 0, n, g.gamma, d_changed.data_ptr())
        torch.cuda.synchronize()
        assert eng.info(Info.PAIR_TABLE) == 1
        changed1 = int(d_changed.item())
        assert changed1 == int(torch.count_nonzero(d_p1 != d_pol).item()) > 0
        what = f"{name} {g.shape} order {g.ordr}, pair table"
        scattered = np.unique(np.random.default_rng(2013).integers(0, n, size=1 << 20, dtype=np.int64))
        tail = _tail_sample(g, 3013)
        assert len(scattered) > 600_000 and len(tail) > 150_000 and tail.min() >= n - (1 << 24)
        top = _top_successor_sample(g, polh, None, 4013)                               # asserts at least 10 000
        for idx, where in ((scattered, "scattered"), (tail, "the last 2^24 states"), (top, "successor cell in the top 1/64")):
            _check_at(f"{what}, {where}", g, idx, Vh, polh, None, d_pol_new=d_p1)
        # the same engine on the plain kernels: the same policy on the whole grid
        eng.set_option(Option.PAIR_TABLE, 0)
        d_p0 = d_pol.clone()
        d_changed.zero_()
        eng.improve_sweep(d_V.data_ptr(), d_p0.data_ptr(), 0, 0, n, g.gamma, d_changed.data_ptr())
        torch.cuda.synchronize()
        assert eng.info(Info.PAIR_TABLE) == 0
        assert torch.equal(d_p0, d_p1) and int(d_changed.item()) == changed1
        del d_V, d_pol, d_p0, d_p1, Vh, polh
    finally:
        g.eng.close()
        _report_peak(f"pair table, order {g.ordr}")
        _free()


def test_v_byte_offsets_beyond_2_pow_31_on_a_4d_grid(cuda_device):
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    name = "double_pendulum_swingup"
    g = _grid(name, SHAPE_V_4D, None, cuda_device, form64=False)
    try:
        n, eng = g.n, g.eng
        assert n == 663_526_080 and 1 << 29 <= n < 1 << 30 and _ragged(tuple(g.mem_shape))
        assert DEFINE not in eng.kernel_source(envs.dynamics_source(name))
        s = _single_sweeps_and_samples(g, 17, None, cuda_device)       # evaluation with residual, improvement, the samples
        assert eng.info(Info.PAIR_TABLE) == 0
        what = f"{name} {g.shape}"
        # the value sweep: V' = max_a Q and the greedy policy at the samples, residual and changed count over the whole grid
        d_Vm = s.d_Vn
        d_Vm.fill_(float("nan"))
        d_p3 = s.d_pol.clone()
        d_changed = torch.zeros(1, dtype=torch.int32, device=cuda_device)
        eng.value_sweep(s.d_V.data_ptr(), d_Vm.data_ptr(), d_p3.data_ptr(), 0, 0, n, g.gamma, s.d_delta.data_ptr(),
                        d_changed.data_ptr())
        torch.cuda.synchronize()
        assert not bool(torch.isnan(d_Vm).any())
        assert int(d_changed.item()) == int(torch.count_nonzero(d_p3 != s.d_pol).item()) > 0
        scattered = np.unique(np.random.default_rng(2017).integers(0, n, size=1 << 20, dtype=np.int64))
        for idx, where in ((scattered, "scattered"), (s.tail, "the last 2^24 states"), (s.top, "successor cell in the top 1/64")):
            _check_at(f"{what}, value sweep, {where}", g, idx, s.Vh, s.polh, None, d_pol_new=d_p3, d_Vmax=d_Vm)
        d_Vm -= s.d_V
        assert float(s.d_delta.item()) == float(d_Vm.abs_().max().item())
        del d_Vm
        # Option.PAIR_TABLE = 1 before pi_compile changes nothing: no table kernels, the sweep reads V, the same policy
        on = _grid(name, SHAPE_V_4D, None, cuda_device, form64=False, options=((Option.PAIR_TABLE, 1),))
        try:
            assert DEFINE not in on.eng.kernel_source(envs.dynamics_source(name))
            d_p4 = s.d_pol.clone()
            on.eng.improve_sweep(s.d_V.data_ptr(), d_p4.data_ptr(), 0, 0, n, g.gamma, d_changed.data_ptr())
            torch.cuda.synchronize()
            assert on.eng.info(Info.PAIR_TABLE) == 0
            assert torch.equal(d_p4, d_p3)                               # the value sweep's policy is the improvement sweep's
        finally:
            on.eng.close()
        del s, d_p3, d_p4
    finally:
        g.eng.close()
        _report_peak("V in the 32-bit form, 4-D")
        _free()


def test_v_byte_offsets_beyond_2_pow_31_on_a_6d_grid(cuda_device):
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    name = "double_cartpole"
    order = envs.ENVS[name].MEMORY_ORDER
    assert isinstance(order, tuple) and order != tuple(range(6))
    g = _grid(name, SHAPE_V_6D, order, cuda_device, form64=False)
    try:
        assert g.n == 652_458_240 and 1 << 29 <= g.n < 1 << 30
        assert g.eng.info(Info.LIVE_STATES) == 0                         # no list: the state-order kernels and the mask
        s = _single_sweeps_and_samples(g, 19, _term_c5, cuda_device)
        assert g.eng.info(Info.PAIR_TABLE) == 0 and g.eng.info(Info.LIVE_STATES) == 0
        del s
    finally:
        g.eng.close()
        _report_peak("V in the 32-bit form, 6-D")
        _free()
