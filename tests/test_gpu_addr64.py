"""
The 64-bit addressing form of EVERY kernel a real run uses, on grids of 2^30 <= n < 2^31 states.

At 4 n >= 2^32 bytes a value table no longer fits 32-bit byte offsets: PI_OFF32 in csrc/pi_sweep_kernels.hip is false and
every kernel compiled for the grid is another translation unit than the one the several hundred tests at n < 2^30 run
(pi_request_corners' 64-bit branch, int32 live lists indexing 4-byte tables beyond 4 GiB, the packed block counters of
the list builders, the strip schedule's group arithmetic).  tests/test_gpu_endtoend.py::
test_64_bit_addressing_path_at_2_pow_30_states pins single state-order sweeps in the identity order at four windows; this
module runs what a real run of such a grid takes besides: the class's memory order, the 4-D form, the device-built
live-state list and the list kernels, batches, the per-evaluation list, the fused value sweep and the solver path itself.
Bar everywhere: bit for bit against the CPU oracle, asked through its point-list entries at states scattered over the
whole table, at its very end, and at states whose successor cell reaches into the top 1/64 of the table (where byte
offsets need their 33rd bit).  The oracle's point-list entries are themselves checked against its sweep entries at this
size first (`oracle_points_equal_oracle_sweeps`, host only).

One 2^30 grid at a time: every test frees its tensors and closes its engine.  Peak device memory as torch counts it
(torch.cuda.max_memory_allocated, printed by every test; the library's own hipMallocs — the live-state list and the
per-evaluation list, 2.7 GB each at 32^6, and the list builders' bitmap and counters — are NOT in these figures),
measured on an MI355X: 6-D sweeps 26.0 GiB, 4-D sweeps 25.1 GiB per order, list kernels 26.0 GiB, solver run + replay
30.0 GiB.  States found with their successor cell in the top 1/64 of the table (of ~1.04 M candidates; at least 10 000
are required): 6-D memory order 165 583, 6-D identity order 63 717, 4-D 176 546 / 166 026, after run() 162 639.

Wall time on an MI355X: the module alone 71 s; in one `pytest -m gpu --durations=20` run of the whole suite (372 s)
its five tests took 46.1 + 8.7 + 5.2 + 3.6 + 3.6 = 67 s, the solver test's share being run() itself (two 4 GiB
transposes on the host).  The existing 2^30 test of tests/test_gpu_endtoend.py took less than 4.2 s in that same run
(it is not among its 20 slowest).  The oracle's point-list entries against its sweep entries at this size
(`oracle_points_equal_oracle_sweeps`) also ran on a CPU-only machine: equal, about a second.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info
from tests import helpers as H
from tests.test_gpu_fullsize import _check_scattered_sample, _term_c5

pytestmark = pytest.mark.gpu

SHAPE_6D = (32,) * 6
SHAPE_4D = (181, 183, 179, 182)                 # n = 1 079 081 094: n % 256 != 0, no stride a power of two


def _torch():
    import torch
    return torch


def _free():
    import gc
    torch = _torch()
    gc.collect()
    torch.cuda.empty_cache()


def _report_peak(what):
    gib = _torch().cuda.max_memory_allocated() / 2 ** 30
    print(f"[addr64] {what}: peak device memory (torch's allocations only) {gib:.1f} GiB")


def _assert_64_bit_form(eng, name):
    n = eng.n_states
    assert 4 * n >= 1 << 32 and n < 1 << 31, f"{n} states do not take the 64-bit addressing form"
    assert "PI_OFF32" in eng.kernel_source(envs.dynamics_source(name))


def _grid(name, shape, order, cuda_device, form64=True, options=()):
    """Engine + what the oracle needs of the grid.  `order` None: the env's own (identity) order.  `form64`: the grid
    must take the 64-bit addressing form (this module's grids; tests/test_gpu_offsets32.py passes False and states its
    own band).  `options`: (selector, value) pairs set before pi_compile."""
    cls = envs.ENVS[name]
    D = cls._D
    bins = H.env_bins(name, shape)
    acts = np.asarray(cls.ACTIONS, np.float32)
    eng = _native.Engine(D, list(shape), [b.min() for b in bins], [b.max() for b in bins], bins, acts,
                         device=cuda_device.index or 0, order=order)
    for what, value in options:
        eng.set_option(what, value)
    eng.compile(envs.dynamics_source(name))
    ordr = tuple(range(D)) if order is None else tuple(order)
    assert eng.order == ordr
    if form64:
        _assert_64_bit_form(eng, name)
    return SimpleNamespace(name=name, shape=tuple(shape), D=D, n=int(np.prod(shape, dtype=np.int64)), bins=bins, acts=acts,
                           eng=eng, order=order, ordr=ordr, mem_shape=[shape[d] for d in ordr],
                           gamma=float(np.float32(cls.CONFIG["gamma"])), chk=H.oracle_for(name), meta=oracle.grid_metadata(bins))


def _seeded_state(g, seed, term_fn, cuda_device, scale=1.0):
    """Seeded (V, policy, terminal mask): host copies in the USER's order (what the oracle sees), device tensors in the
    engine's memory order.  Drawn on the device; the mask per dimension from the bin tables."""
    torch = _torch()
    gen = torch.Generator(device=cuda_device).manual_seed(seed)
    u = torch.randn(g.n, generator=gen, dtype=torch.float32, device=cuda_device) * scale
    Vh = u.cpu().numpy()
    d_V = g.eng.to_memory(u)
    del u
    u = torch.randint(0, len(g.acts), (g.n,), generator=gen, dtype=torch.int32, device=cuda_device)
    polh = u.cpu().numpy()
    d_pol = g.eng.to_memory(u)
    del u
    termh = d_term = None
    if term_fn is not None:
        t = term_fn(g.bins, g.shape).to(torch.uint8)
        termh = t.numpy()
        d_term = g.eng.to_memory(t.to(cuda_device))
        del t
    return Vh, polh, termh, d_V, d_pol, d_term


def _points(g, idx_mem):
    """MEMORY-order flat indices -> (USER flat indices, coordinates (m, D)) from the bin tables."""
    im = np.stack(np.unravel_index(idx_mem, g.mem_shape), axis=1)
    iu = np.empty_like(im)
    for k, d in enumerate(g.ordr):
        iu[:, d] = im[:, k]
    flat_user = np.ravel_multi_index(tuple(iu.T), g.shape)
    coords = np.stack([g.bins[d][iu[:, d]] for d in range(g.D)], axis=1).astype(np.float32)
    return flat_user, coords


def _check_at(what, g, idx_mem, V_user, pol_user, term_user, d_Vn=None, d_pol_new=None, d_Vmax=None):
    """The device's results at the memory-order indices `idx_mem` against the oracle's point-list entries, bit for bit:
    `d_Vn` one evaluation sweep of (V_user, pol_user), `d_pol_new` one improvement sweep of V_user, `d_Vmax` the value
    sweep's V' = max_a Q (terminal states: values copied, entries kept).  Device arrays in memory order."""
    torch = _torch()
    lo, hi, gshape, strides = g.meta
    flat_user, coords = _points(g, idx_mem)
    t = np.zeros(len(idx_mem), dtype=bool) if term_user is None else term_user[flat_user].astype(bool)
    d_idx = torch.from_numpy(idx_mem).to(torch.device("cuda", g.eng.device))
    if d_Vn is not None:
        want = g.chk.eval_points(coords, g.acts[pol_user[flat_user]], V_user, lo, hi, gshape, strides, g.gamma)
        want[t] = V_user[flat_user][t]
        H.assert_bits_equal(d_Vn[d_idx].cpu().numpy(), want, f"{what}: evaluation at {len(idx_mem)} states")
    if d_pol_new is not None or d_Vmax is not None:
        best, best_q = g.chk.improve_points(coords, g.acts, V_user, lo, hi, gshape, strides, g.gamma)
        best[t] = pol_user[flat_user][t]
        best_q[t] = V_user[flat_user][t]
        if d_pol_new is not None:
            assert np.array_equal(d_pol_new[d_idx].cpu().numpy(), best), f"{what}: improvement at {len(idx_mem)} states"
        if d_Vmax is not None:
            H.assert_bits_equal(d_Vmax[d_idx].cpu().numpy(), best_q, f"{what}: max-backup at {len(idx_mem)} states")
    return len(idx_mem)


def _tail_sample(g, seed, m=1 << 18):
    """`m` seeded memory-order indices from the last 2^24 states of the table."""
    return np.unique(np.random.default_rng(seed).integers(g.n - (1 << 24), g.n, size=m, dtype=np.int64))


def _top_successor_sample(g, pol_user, term_user, seed, candidates=1 << 20):
    """Live states whose successor under their policy entry bootstraps from a cell that reaches into the top 1/64 of
    the table in MEMORY order (the cell's highest corner has flat index >= n - n/64: the loads whose byte offsets need
    bit 32).  Picked on the host: seeded candidates from the last three planes of the slowest memory dimension, the
    oracle's step and interp at them."""
    lo, hi, gshape, strides = g.meta
    plane = g.n // g.mem_shape[0]
    cand = np.unique(np.random.default_rng(seed).integers(g.n - 3 * plane, g.n, size=candidates, dtype=np.int64))
    flat_user, coords = _points(g, cand)
    live = np.ones(len(cand), dtype=bool) if term_user is None else ~term_user[flat_user].astype(bool)
    nxt, _, done = g.chk.step(coords, g.acts[pol_user[flat_user]])
    idxs, _ = g.chk.interp(nxt, lo, hi, gshape, strides)
    base = np.stack(np.unravel_index(idxs[:, 0].astype(np.int64), g.shape), axis=1)      # lowest corner, USER indices
    del idxs
    top_mem = np.ravel_multi_index(tuple(base[:, d] + 1 for d in g.ordr), g.mem_shape)   # highest corner, MEMORY index
    found = cand[live & ~done & (top_mem >= g.n - g.n // 64)]
    print(f"[addr64] {g.name} {g.shape} order {g.ordr}: {len(found)} of {len(cand)} candidate states have their successor "
          f"cell in the top 1/64 of the table")
    assert len(found) >= 10_000
    return found


def _windows(n):
    """The windows of tests/test_gpu_endtoend.py::test_64_bit_addressing_path_at_2_pow_30_states."""
    return [(0, 1536), (n // 2 - 1000, n // 2 + 1000), (n - (1 << 29) - 700, n - (1 << 29) + 700), (n - 1536, n)]


def oracle_points_equal_oracle_sweeps(chk, bins, acts, Vh, polh, termh, gamma):
    """Host only.  The oracle's point-list entries (eval_points / improve_points), never called with a table of 2^30
    floats before, against its sweep entries (the ones the existing 2^30 test exercises) on that test's windows of the
    reference's flat order: values, greedy entries and their values, bit for bit."""
    shape = tuple(len(b) for b in bins)
    D, n = len(shape), len(Vh)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    for a, b in _windows(n):
        idx = np.stack(np.unravel_index(np.arange(a, b), shape), axis=1)
        coords = np.stack([bins[d][idx[:, d]] for d in range(D)], axis=1).astype(np.float32)
        pad_states = np.zeros((b, D), dtype=np.float32)          # calloc: only rows [a, b) are ever touched
        pad_states[a:b] = coords
        t = termh[a:b].astype(bool)
        o_Vn = np.zeros(b, dtype=np.float32)
        chk.eval_sweep(pad_states, acts, polh[:b], Vh, termh[:b], lo, hi, gshape, strides, gamma, a, b, out=o_Vn)
        p_Vn = chk.eval_points(coords, acts[polh[a:b]], Vh, lo, hi, gshape, strides, gamma)
        p_Vn[t] = Vh[a:b][t]
        H.assert_bits_equal(p_Vn, o_Vn[a:b], f"oracle eval_points against eval_sweep on [{a},{b})")
        o_pol, _, o_q, _ = chk.improve_sweep(pad_states, acts, polh[:b], Vh, termh[:b], lo, hi, gshape, strides, gamma,
                                             a, b, want_q=True)
        best, best_q = chk.improve_points(coords, acts, Vh, lo, hi, gshape, strides, gamma)
        best[t] = polh[a:b][t]
        assert np.array_equal(best, o_pol[a:b]), f"oracle improve_points against improve_sweep on [{a},{b})"
        H.assert_bits_equal(best_q[~t], o_q[a:b][~t], f"oracle improve_points' values on [{a},{b})")
        del pad_states, o_Vn, o_pol, o_q


def _single_sweeps_and_samples(g, seed, term_fn, cuda_device, host_check=False):
    """Sections 1 and 2 of the module: one evaluation sweep with residual over [0, n), one whole-grid improvement sweep
    and the three samples against the oracle.  Returns what the caller goes on with (the engine stays open)."""
    torch = _torch()
    n, eng = g.n, g.eng
    Vh, polh, termh, d_V, d_pol, d_term = _seeded_state(g, seed, term_fn, cuda_device)
    if host_check:
        oracle_points_equal_oracle_sweeps(g.chk, g.bins, g.acts, Vh, polh, termh, g.gamma)
    tptr = 0 if d_term is None else d_term.data_ptr()
    d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=cuda_device)
    d_delta = torch.zeros(1, dtype=torch.float32, device=cuda_device)
    eng.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), tptr, 0, n, g.gamma, d_delta.data_ptr())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(d_Vn).any())                                   # every state written
    diff = d_Vn - d_V
    assert float(d_delta.item()) == float(diff.abs_().max().item())
    del diff
    if d_term is not None:
        tmask = d_term.bool()
        assert int(tmask.sum()) > 0 and torch.equal(d_Vn[tmask], d_V[tmask])   # terminal states copy their value
        del tmask
    d_p2 = d_pol.clone()
    d_changed = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    eng.improve_sweep(d_V.data_ptr(), d_p2.data_ptr(), tptr, 0, n, g.gamma, d_changed.data_ptr())
    torch.cuda.synchronize()
    assert int(d_changed.item()) == int(torch.count_nonzero(d_p2 != d_pol).item()) > 0
    what = f"{g.name} {g.shape} order {g.ordr}"
    m = _check_scattered_sample(what, g.chk, g.bins, g.acts, g.shape, g.order, g.gamma, Vh, polh, termh, d_Vn, d_p2,
                                seed=2000 + seed)
    assert m > 600_000
    tail = _tail_sample(g, 3000 + seed)
    assert len(tail) > 150_000
    _check_at(what + ", the last 2^24 states", g, tail, Vh, polh, termh, d_Vn=d_Vn, d_pol_new=d_p2)
    top = _top_successor_sample(g, polh, termh, 4000 + seed)
    _check_at(what + ", successor cell in the top 1/64", g, top, Vh, polh, termh, d_Vn=d_Vn, d_pol_new=d_p2)
    del d_p2
    return SimpleNamespace(Vh=Vh, polh=polh, termh=termh, d_V=d_V, d_pol=d_pol, d_term=d_term, d_Vn=d_Vn, d_delta=d_delta,
                           tail=tail, top=top)


# ---- 1. 6-D, the order a real run uses -------------------------------------------------------------------------------
def test_6d_sweeps_at_2_pow_30_states_in_the_order_a_real_run_uses(cuda_device):
    """double_cartpole 32^6 in the class's MEMORY_ORDER (what envs.make("double_cartpole", 32) resolves to): the oracle's
    own point-list entries at high indices first (host), then one evaluation sweep with residual and one whole-grid
    improvement sweep against torch reductions and against the oracle at 2^20 states scattered over the whole table, 2^18
    in its last 2^24 states and the states whose successor cell lies in the top 1/64 of the table."""
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    order = envs.ENVS["double_cartpole"].MEMORY_ORDER
    assert isinstance(order, tuple) and order[0] != 0 and order != tuple(range(6))
    g = _grid("double_cartpole", SHAPE_6D, order, cuda_device)
    assert g.n == 1 << 30
    s = _single_sweeps_and_samples(g, 3, _term_c5, cuda_device, host_check=True)
    del s
    g.eng.close()
    _report_peak("6-D sweeps, memory order")
    _free()


# ---- 2. 4-D ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [None, (0, 2, 1, 3)], ids=["env-order", "permuted-order"])
def test_4d_sweeps_beyond_2_pow_30_states_on_a_ragged_grid(order, cuda_device):
    """double_pendulum_swingup (181, 183, 179, 182): the 4-D form (8 pair loads, another stride mix), no terminal states
    (no mask stream).  The checks of the 6-D test, a 3-sweep batch whose first two sweeps stream no old values, and the
    chunk walk over the ragged tail of the range (pi_probe_coords)."""
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    g = _grid("double_pendulum_swingup", SHAPE_4D, order, cuda_device)
    n, eng = g.n, g.eng
    assert n == 1_079_081_094 and n % 256 != 0
    s = _single_sweeps_and_samples(g, 7, None, cuda_device)
    # 8 n >= 2^32: the whole-grid improvement sweep above read V, and the unit holds no table kernels to read anything else
    assert eng.info(Info.PAIR_TABLE) == 0
    assert "#define PI_PAIR_TABLE" not in eng.kernel_source(envs.dynamics_source(g.name))
    what = f"{g.name} {g.shape} order {g.ordr}"
    # a batch of 3 sweeps, residual asked of the last one only: sweeps 0 and 1 read no old value (need_old == false)
    d_A, d_B = s.d_V, s.d_Vn
    d_B.fill_(float("nan"))
    eng.eval_sweeps(d_A.data_ptr(), d_B.data_ptr(), s.d_pol.data_ptr(), 0, 0, n, g.gamma, 3, s.d_delta.data_ptr())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(d_B).any()) and not bool(torch.isnan(d_A).any())
    diff = d_B - d_A
    assert float(s.d_delta.item()) == float(diff.abs_().max().item())
    del diff
    prev = eng.to_user(d_A).cpu().numpy()                        # the iterate before the newest: the oracle's input V
    assert not np.array_equal(prev[-4096:], s.Vh[-4096:])        # ... which the batch has written (sweep 1)
    for idx, where in ((np.unique(np.random.default_rng(11).integers(0, n, size=1 << 20, dtype=np.int64)), "scattered"),
                       (s.tail, "the last 2^24 states"), (s.top, "successor cell in the top 1/64")):
        _check_at(f"{what}, third sweep of a batch, {where}", g, idx, prev, s.polh, None, d_Vn=d_B)
    del prev, d_A, d_B
    # the chunk walk at s close to 2^30: coordinates of the last 70 000 states, one and three chunks per workgroup
    a = n - 70_000
    _, coords = _points(g, np.arange(a, n, dtype=np.int64))
    out = torch.empty((n - a) * 4, dtype=torch.float32, device=cuda_device)
    for cpw in (1, 3):
        out.fill_(float("nan"))
        eng.probe_coords(a, n, out.data_ptr(), cpw)
        torch.cuda.synchronize()
        H.assert_bits_equal(out.cpu().numpy().reshape(-1, 4), coords, f"{what}: state coordinates of [{a},{n}), cpw {cpw}")
    del s, out
    eng.close()
    _report_peak(f"4-D sweeps, order {g.ordr}")
    _free()


# ---- 3. the list kernels ---------------------------------------------------------------------------------------------
def test_list_kernels_at_2_pow_30_states(cuda_device, monkeypatch):
    """double_cartpole 32^6, identity order: the device-built live-state list (pi_mask_list_kernel, pi_scan_slots_kernel),
    the sweeps over it (pi_eval_live_kernel, pi_improve_live_kernel), the per-evaluation list (pi_policy_list_kernel)
    and the fused value sweep — with the list against without it on the whole grid, and against the oracle at the
    samples."""
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    monkeypatch.setenv("PI_MI355_GRAPHS", "0")
    monkeypatch.setenv("PI_MI355_RESIDENT", "0")
    g = _grid("double_cartpole", SHAPE_6D, None, cuda_device)
    n, eng, gamma = g.n, g.eng, g.gamma
    Vh, polh, termh, d_V0, d_pol, d_term = _seeded_state(g, 5, _term_c5, cuda_device)
    tptr = d_term.data_ptr()
    what = "double_cartpole 32^6 lists"
    rng = np.random.default_rng(2005)
    scattered = np.unique(rng.integers(0, n, size=1 << 20, dtype=np.int64))
    assert len(scattered) > 600_000
    tail = _tail_sample(g, 3005)
    top = _top_successor_sample(g, polh, termh, 4005)
    samples = ((scattered, "scattered"), (tail, "the last 2^24 states"), (top, "successor cell in the top 1/64"))

    # the list itself: all 2^30 bits of the mask, compared on the device
    n_live = int((d_term == 0).sum().item())
    assert 0 < n_live < n
    assert eng.prepare_mask(tptr) == n_live and eng.info(Info.LIVE_STATES) == n_live
    d_list = torch.full((n_live,), -1, dtype=torch.int32, device=cuda_device)
    assert eng.live_list(d_list.data_ptr(), n_live) == n_live
    torch.cuda.synchronize()
    want_list = torch.nonzero(d_term == 0).reshape(-1)
    assert want_list.numel() == n_live and int(want_list[-1].item()) >= 1 << 29
    assert torch.equal(d_list.to(torch.int64), want_list)
    del d_list, want_list

    def use_list(on):
        if on:
            assert eng.prepare_mask(tptr) == n_live and eng.info(Info.LIVE_STATES) == n_live
        else:
            assert eng.prepare_mask(0) == 0 and eng.info(Info.LIVE_STATES) == 0

    def same_bits(a, b):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))

    # batches of k sweeps with residual: both buffers and the residual, with the list and without it
    d_delta = torch.zeros(1, dtype=torch.float32, device=cuda_device)
    for k in (1, 2, 5):
        res = []
        for on in (True, False):
            use_list(on)
            d_A = d_V0.clone()
            d_B = torch.full((n,), float("nan"), dtype=torch.float32, device=cuda_device)
            d_delta.zero_()
            eng.eval_sweeps(d_A.data_ptr(), d_B.data_ptr(), d_pol.data_ptr(), tptr, 0, n, gamma, k, d_delta.data_ptr())
            torch.cuda.synchronize()
            res.append((d_A, d_B, float(d_delta.item())))
        (A1, B1, r1), (A2, B2, r2) = res
        assert not bool(torch.isnan(B2).any())
        assert same_bits(A1, A2) and same_bits(B1, B2) and r1 == r2 > 0.0, f"batch of {k} sweeps: list against no list"
        if k == 5:                                               # newest iterate B, its input A: against the oracle
            prev = A1.cpu().numpy()
            for idx, where in samples:
                _check_at(f"{what}, fifth sweep of a batch, {where}", g, idx, prev, polh, termh, d_Vn=B1)
            del prev
        del res, A1, B1, A2, B2, d_A, d_B

    # improvement through the list: whole grid and a ragged range, with the list against without it and the oracle
    d_changed = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    for a, b in ((0, n), (7, n - 9)):
        res = []
        for on in (True, False):
            use_list(on)
            d_p = d_pol.clone()
            d_changed.zero_()
            eng.improve_sweep(d_V0.data_ptr(), d_p.data_ptr(), tptr, a, b, gamma, d_changed.data_ptr())
            torch.cuda.synchronize()
            res.append((d_p, int(d_changed.item())))
        (P1, c1), (P2, c2) = res
        assert torch.equal(P1, P2) and c1 == c2 > 0, f"improvement over [{a},{b}): list against no list"
        assert c1 == int(torch.count_nonzero(P1 != d_pol).item())
        assert torch.equal(P1[:a], d_pol[:a]) and torch.equal(P1[b:], d_pol[b:])           # nothing outside the range
        for idx, where in samples:
            idx = idx[(idx >= a) & (idx < b)]
            _check_at(f"{what}, improvement over [{a},{b}) through the list, {where}", g, idx, Vh, polh, termh, d_pol_new=P1)
        del res, P1, P2, d_p

    # the per-evaluation list: the solver's 1 + 25 + 25 batches with the bracket and without it
    use_list(True)
    res = []
    for bracket in (True, False):
        d_A = d_V0.clone()
        d_B = d_V0.clone()
        residuals = []
        if bracket:
            listed = eng.eval_begin(d_pol.data_ptr(), tptr)
            assert 0 < listed < n_live and eng.info(Info.EVAL_LIST_ENTRIES) == listed
        for k in (1, 25, 25):
            eng.eval_sweeps(d_A.data_ptr(), d_B.data_ptr(), d_pol.data_ptr(), tptr, 0, n, gamma, k, d_delta.data_ptr())
            if k & 1:
                d_A, d_B = d_B, d_A
            residuals.append(float(d_delta.item()))
        if bracket:
            eng.eval_end()
        res.append((d_A, d_B, residuals))
    (A1, B1, r1), (A2, B2, r2) = res
    assert same_bits(A1, A2) and same_bits(B1, B2) and r1 == r2, "1 + 25 + 25 sweeps: per-evaluation list against none"
    assert not same_bits(A1, d_V0)
    del res, A1, B1, A2, B2, d_A, d_B

    # the fused value sweep over a ragged range
    a, b = 3, n - 5
    d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=cuda_device)
    d_p = d_pol.clone()
    eng.value_sweep(d_V0.data_ptr(), d_Vn.data_ptr(), d_p.data_ptr(), tptr, a, b, gamma, d_delta.data_ptr(), d_changed.data_ptr())
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_Vn[:a]).all()) and bool(torch.isnan(d_Vn[b:]).all()) and not bool(torch.isnan(d_Vn[a:b]).any())
    assert torch.equal(d_p[:a], d_pol[:a]) and torch.equal(d_p[b:], d_pol[b:])
    diff = d_Vn[a:b] - d_V0[a:b]
    assert float(d_delta.item()) == float(diff.abs_().max().item())
    del diff
    assert int(d_changed.item()) == int(torch.count_nonzero(d_p != d_pol).item()) > 0
    for idx, where in samples:
        idx = idx[(idx >= a) & (idx < b)]
        _check_at(f"{what}, value sweep over [{a},{b}), {where}", g, idx, Vh, polh, termh, d_pol_new=d_p, d_Vmax=d_Vn)
    del d_Vn, d_p, d_V0, d_pol, d_term
    eng.close()
    _report_peak("6-D list kernels")
    _free()


# ---- 4. the solver path ----------------------------------------------------------------------------------------------
def test_solver_run_at_2_pow_30_states(cuda_device):
    """envs.make("double_cartpole", 32) with two rounds of 30 evaluation sweeps: the run took the live-state list and the
    strip schedule; its (V, policy) equal a replay of the same sweeps by the plain state-order kernels (one launch per
    sweep, no list) over the whole grid, bit for bit; and one further evaluation sweep and improvement sweep of that
    policy-iteration state equal the oracle at 2^20 scattered states."""
    torch = _torch()
    torch.cuda.reset_peak_memory_stats()
    name = "double_cartpole"
    cls = envs.ENVS[name]
    solver = envs.make(name, 32, config=envs.CudaPIConfig(**{**cls.CONFIG, "max_pi_iter": 2, "max_eval_iter": 30}),
                       device=cuda_device)
    n = solver.n_states
    order = solver._order
    assert order == tuple(cls.MEMORY_ORDER) and solver._backend.engine.order == order
    _assert_64_bit_form(solver._backend.engine, name)
    n_live = solver._backend.engine.info(Info.LIVE_STATES)
    assert 0 < n_live < n                                          # the list paths ...
    assert solver._backend.engine.info(Info.STRIP_STATES) > 0      # ... and the strip schedule
    solver.run()
    assert solver.stats["sweeps_per_iter"] == [30, 30] and solver.stats["improve_sweeps"] == 2
    V_user = np.ascontiguousarray(solver.value_function, dtype=np.float32)
    pol_user = np.ascontiguousarray(solver.policy, dtype=np.int32)
    del solver
    _free()
    # run() has released the device: a fresh engine in the solver's order, without any list
    g = _grid(name, SHAPE_6D, order, cuda_device)
    eng, gamma = g.eng, g.gamma
    assert eng.info(Info.LIVE_STATES) == 0
    term = _term_c5(g.bins, g.shape).to(torch.uint8)
    term_user = term.numpy()
    d_term = eng.to_memory(term.to(cuda_device))
    tptr = d_term.data_ptr()
    assert int((d_term == 0).sum().item()) == n_live
    # the replay: V = 0, policy = 0, two rounds of 30 single state-order sweeps and one state-order improvement sweep
    d_A = torch.zeros(n, dtype=torch.float32, device=cuda_device)
    d_B = torch.zeros(n, dtype=torch.float32, device=cuda_device)
    d_P = torch.zeros(n, dtype=torch.int32, device=cuda_device)
    for _ in range(2):
        for _ in range(30):
            eng.eval_sweep(d_A.data_ptr(), d_B.data_ptr(), d_P.data_ptr(), tptr, 0, n, gamma, 0)
            d_A, d_B = d_B, d_A
        eng.improve_sweep(d_A.data_ptr(), d_P.data_ptr(), tptr, 0, n, gamma, 0)
    torch.cuda.synchronize()
    d_V = eng.to_memory(torch.from_numpy(V_user).to(cuda_device))
    d_pol = eng.to_memory(torch.from_numpy(pol_user).to(cuda_device))
    assert torch.equal(d_V.view(torch.int32), d_A.view(torch.int32)), "run(): V differs from the replay by the plain kernels"
    assert torch.equal(d_pol, d_P), "run(): policy differs from the replay by the plain kernels"
    assert int(torch.count_nonzero(d_pol).item()) > 0 and float(d_V.abs().max().item()) > 1.0
    del d_A, d_P
    # one more evaluation sweep and improvement sweep of the run's final state against the oracle
    d_Vn = d_B
    d_Vn.fill_(float("nan"))
    d_p2 = d_pol.clone()
    eng.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), tptr, 0, n, gamma, 0)
    eng.improve_sweep(d_V.data_ptr(), d_p2.data_ptr(), tptr, 0, n, gamma, 0)
    torch.cuda.synchronize()
    m = _check_scattered_sample("double_cartpole 32^6 after run()", g.chk, g.bins, g.acts, g.shape, order, gamma, V_user,
                                pol_user, term_user, d_Vn, d_p2, seed=78)
    assert m > 600_000
    top = _top_successor_sample(g, pol_user, term_user, 4078)
    _check_at("double_cartpole 32^6 after run(), successor cell in the top 1/64", g, top, V_user, pol_user, term_user,
              d_Vn=d_Vn, d_pol_new=d_p2)
    del d_V, d_pol, d_Vn, d_B, d_p2, d_term
    eng.close()
    _report_peak("solver run + replay")
    _free()
