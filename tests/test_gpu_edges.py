"""
The sweep kernels at every threshold of pi_create's dispatch and on degenerate grids, against the CPU oracle, bit for bit
and over ALL states of every grid (the host half: tests/test_edge_dispatch.py, which also pins the oracle on the
degenerate grids against float64 numpy).

The kernels are specialised at run time on grid shape, action count, workgroup size, chunks per workgroup and schedule,
and pi_create picks the kernel family by comparing the state count with fixed numbers.  The shapes below sit ON those
numbers and one step beyond.  When a constant of choose_dispatch (csrc/pi_api.cpp) moves, update `helpers.DISPATCH_TABLE` and this list:

  threshold                                   shapes (env)
  table floats 8 * 256 = 2048 (staging)       2 x 2025 = 2048, 2 x 2026 = 2049; strided branch also: 2 x 3000, 3000 x 2,
                                              2 x 15337 (pendulum / mountain_car, 21 / 3 actions)
  table floats 15 360 (pi_create's limit)     2 x 15337 with 21 actions
  resident 2-D, n <= 12 288                   96 x 128 | 97 x 127 (mountain_car)
  XCD_MIN 4 096                               64 x 64 | 64 x 65 (pendulum)
  XCD_MAX 2^16                                256 x 256 | 256 x 257 (pendulum)
  dataflow, n <= 2^17                         256 x 512 | 363 x 362 (mountain_car); 16.16.16.32 | 16.16.16.33 (cartpole_swingup)
  dataflow 4-D as placed on 256 CUs (2^16)    16^4 | 16.16.16.17 (cartpole_swingup): beyond one workgroup per CU the kernel is
                                              refused when it is loaded, 16.16.16.32 included (helpers.DISPATCH_TABLE, `placed`)
  resident 4-D, n <= 4 096                    8^4 | 8.8.8.9 (cartpole)
  resident 6-D, n <= 1 024                    2.2.4.4.4.4 | 2.2.4.4.4.5 (double_cartpole)
  2^20 (evaluation cpw 2, live lists)         32.32.32.31 | 32^4 (cartpole), 8.8.8.8.16.15 | 8.8.8.8.16.16 (double_cartpole): a
                                              list from 2^20 on; 32^4 (cartpole_swingup): cpw 2, no mixed waves, no list
  2^22 (memory order)                         64.64.32.31 | 64.64.32.32 (double_pendulum_swingup)
  2^24 4-D (1024 / 512 threads)               64.64.64.63 | 64^4 (double_pendulum_swingup)
  2^24 6-D (cpw 4 / 3)                        16^5.15 | 16^6 (double_cartpole)
  degenerate                                  all dimensions 2 bins (2^2, 2^4 twice, 2^6); one 2-bin dimension slowest /
                                              fastest / in 4-D (2.2.2.1500 register-staged, 2.2.2.2100 strided); n = 63, 255, 256, 258, 259, 513, 1025 (257 is prime);
                                              1, 2, 64, 257 actions (pendulum torques beyond the plugin's clamp: ties)
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info, Option
from tests import helpers as H

pytestmark = pytest.mark.gpu

EXPECTED = {cid: row for row, (cid, _, _, _) in zip(H.DISPATCH_TABLE + H.EDGE_ROWS, H.THRESHOLD_CASES + H.EDGE_CASES)}
ORDERS = {(name, tuple(shape)): order for name, shape, order in H.SOLVER_ORDER_TABLE}


def _torch():
    import torch
    return torch


def _dev(a, dev):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(dev)


class _Case:
    """Engine, grid, seeded (V, policy, mask) and the oracle of one specialisation."""

    def __init__(self, name, shape, actions, dev, seed=41):
        cls = envs.ENVS[name]
        self.name, self.shape, self.dev, self.cls = name, tuple(shape), dev, cls
        self.bins = H.env_bins(name, shape)
        self.acts = H.edge_actions(name, actions)
        self.eng = _native.Engine(cls._D, [len(b) for b in self.bins], [b.min() for b in self.bins],
                                  [b.max() for b in self.bins], self.bins, self.acts, device=dev.index or 0)
        self.eng.compile(envs.dynamics_source(name))
        self.meta = oracle.grid_metadata(self.bins)
        self.states = oracle.states_from_bins(self.bins)
        self.n = len(self.states)
        self.term, tval = H.terminal_mask(name, self.states)
        rng = np.random.default_rng(seed)
        self.V = (rng.standard_normal(self.n) * 3.0).astype(np.float32)
        self.V[self.term] = np.float32(tval)
        self.pol = rng.integers(0, len(self.acts), size=self.n).astype(np.int32)
        self.pol[self.term] = 0
        self.gamma = float(np.float32(cls.CONFIG["gamma"]))
        self.chk = H.oracle_for(name)
        self.d_V, self.d_pol = _dev(self.V, dev), _dev(self.pol, dev)
        self.d_term = _dev(self.term.astype(np.uint8), dev)

    def o_eval(self, V, a=0, b=None, out=None):
        return self.chk.eval_sweep(self.states, self.acts, self.pol, V, self.term, *self.meta, self.gamma, a, b, out=out)

    def o_improve(self, pol, a=0, b=None):
        return self.chk.improve_sweep(self.states, self.acts, pol, self.V, self.term, *self.meta, self.gamma, a, b)

    def o_value(self, a=0, b=None, out=None):
        return self.chk.value_sweep(self.states, self.acts, self.pol, self.V, self.term, *self.meta, self.gamma, a, b, out=out)


def _assert_dispatch(c, row):
    """On the device the info codes answer in full: the row of helpers.DISPATCH_TABLE / EDGE_DISPATCH, exactly.  The
    dataflow kernel is there with all its ceil(n / 256) workgroups wherever pi_create wants it, except on the rows that
    pin a refusal at load time (`placed` False: 4-D grids beyond one workgroup per CU)."""
    eng = c.eng
    assert eng.info(Info.COMPUTE_UNITS) == 256
    assert eng.info(Info.RESIDENT_STATES_PER_THREAD) == row["k"] and eng.info(Info.RESIDENT_ENABLED) == 1
    placed = row["flow"] and row.get("placed", True)
    assert eng.info(Info.FLOW_WORKGROUPS) == (-(-c.n // 256) if placed else 0)
    assert eng.info(Info.XCD_ENABLED) == (0 if row["xcd_s"] is None else 1)
    assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == (row["eb"], row["ib"])
    assert (eng.info(Info.EVAL_CPW), eng.info(Info.IMPROVE_CPW)) == (row["ecpw"], row["icpw"])
    return row["k"] > 0 or placed


def _single_sweeps(c):
    """One evaluation sweep with residual, one improvement sweep, one value sweep: every state against the oracle."""
    torch = _torch()
    eng, n, dev = c.eng, c.n, c.dev
    d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    d_delta = torch.full((1,), 123.0, dtype=torch.float32, device=dev)
    d_changed = torch.full((1,), 77, dtype=torch.int32, device=dev)
    eng.eval_sweep(c.d_V.data_ptr(), d_Vn.data_ptr(), c.d_pol.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, d_delta.data_ptr())
    o_Vn, o_delta = c.o_eval(c.V)
    H.assert_bits_equal(d_Vn.cpu().numpy(), o_Vn, f"{c.name} {c.shape}: V' of one evaluation sweep")
    H.assert_bits_equal(np.float32(d_delta.item()), np.float32(o_delta), "its residual")
    d_p2 = c.d_pol.clone()
    eng.improve_sweep(c.d_V.data_ptr(), d_p2.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, d_changed.data_ptr())
    o_pol, o_changed = c.o_improve(c.pol)
    assert np.array_equal(d_p2.cpu().numpy(), o_pol), f"{c.name} {c.shape}: improved policy"
    assert int(d_changed.item()) == o_changed
    if len(c.acts) == 1:                                   # a single action: nothing to choose, nothing changes
        d_p0 = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.improve_sweep(c.d_V.data_ptr(), d_p0.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, d_changed.data_ptr())
        assert int(torch.count_nonzero(d_p0).item()) == 0 and int(d_changed.item()) == 0
    d_p3 = c.d_pol.clone()
    d_Vm = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    eng.value_sweep(c.d_V.data_ptr(), d_Vm.data_ptr(), d_p3.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma,
                    d_delta.data_ptr(), d_changed.data_ptr())
    o_Vm, o_pol3, o_delta3, o_changed3 = c.o_value()
    H.assert_bits_equal(d_Vm.cpu().numpy(), o_Vm, f"{c.name} {c.shape}: V' of the value sweep")
    assert np.array_equal(d_p3.cpu().numpy(), o_pol3) and np.array_equal(o_pol3, o_pol)
    H.assert_bits_equal(np.float32(d_delta.item()), np.float32(o_delta3), "the value sweep's residual")
    assert int(d_changed.item()) == o_changed3
    return o_Vn, o_pol, o_Vm


def _batches(c):
    """eval_sweeps of 3 and of 26, graphs on and off: BOTH buffers and the residual equal as many oracle sweeps.  Vb
    starts as NaN: the first sweep has to put the terminal states' values there."""
    torch = _torch()
    eng, n, dev = c.eng, c.n, c.dev
    keep, cur = {0: c.V}, c.V
    for i in range(1, 27):
        cur, delta = c.o_eval(cur)
        if i in (2, 3, 25, 26):
            keep[i] = (cur, delta)
    d_delta = torch.zeros(1, dtype=torch.float32, device=dev)
    for graphs in (1, 0):
        eng.set_option(Option.GRAPHS, graphs)
        for k in (3, 26):
            d_A, d_B = c.d_V.clone(), torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            d_delta.fill_(-1.0)
            eng.eval_sweeps(d_A.data_ptr(), d_B.data_ptr(), c.d_pol.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, k,
                            d_delta.data_ptr())
            last, other = (d_B, d_A) if k & 1 else (d_A, d_B)
            what = f"{c.name} {c.shape}: batch of {k}, graphs {graphs}"
            H.assert_bits_equal(last.cpu().numpy(), keep[k][0], what + ", newest iterate")
            H.assert_bits_equal(other.cpu().numpy(), keep[k - 1][0], what + ", the iterate before (other buffer)")
            H.assert_bits_equal(np.float32(d_delta.item()), np.float32(keep[k][1]), what + ", residual")
    eng.set_option(Option.GRAPHS, 1)


def _sub_ranges(c, o_Vn, o_pol, o_Vm):
    """[0, 1), [n-1, n), an empty range and a ragged one: results inside equal the whole sweep's, NaN / the old entries
    stay outside, residual and changed count are the range's own."""
    torch = _torch()
    eng, n, dev = c.eng, c.n, c.dev
    a0 = n // 3
    d_delta = torch.zeros(1, dtype=torch.float32, device=dev)
    d_changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for a, b in ((0, 1), (n - 1, n), (n // 2, n // 2), (a0, max(a0 + 1, n - n // 5 - 1))):
        assert 0 <= a <= b <= n
        what = f"{c.name} {c.shape} [{a},{b})"
        inside = np.zeros(n, dtype=bool)
        inside[a:b] = True
        d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        d_delta.fill_(123.0)
        eng.eval_sweep(c.d_V.data_ptr(), d_Vn.data_ptr(), c.d_pol.data_ptr(), c.d_term.data_ptr(), a, b, c.gamma, d_delta.data_ptr())
        got = d_Vn.cpu().numpy()
        assert np.isnan(got[~inside]).all(), what + ": evaluation wrote outside its range"
        H.assert_bits_equal(got[a:b], o_Vn[a:b], what + ": evaluation")
        _, o_delta = c.o_eval(c.V, a, b)
        H.assert_bits_equal(np.float32(d_delta.item()), np.float32(o_delta), what + ": residual")
        d_p2 = c.d_pol.clone()
        d_changed.fill_(77)
        eng.improve_sweep(c.d_V.data_ptr(), d_p2.data_ptr(), c.d_term.data_ptr(), a, b, c.gamma, d_changed.data_ptr())
        got = d_p2.cpu().numpy()
        assert np.array_equal(got[~inside], c.pol[~inside]) and np.array_equal(got[a:b], o_pol[a:b]), what + ": improvement"
        assert int(d_changed.item()) == int((o_pol[a:b] != c.pol[a:b]).sum())
        d_p3 = c.d_pol.clone()
        d_Vm = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        eng.value_sweep(c.d_V.data_ptr(), d_Vm.data_ptr(), d_p3.data_ptr(), c.d_term.data_ptr(), a, b, c.gamma,
                        d_delta.data_ptr(), d_changed.data_ptr())
        got, got_p = d_Vm.cpu().numpy(), d_p3.cpu().numpy()
        assert np.isnan(got[~inside]).all(), what + ": value sweep wrote outside its range"
        H.assert_bits_equal(got[a:b], o_Vm[a:b], what + ": value sweep")
        assert np.array_equal(got_p[~inside], c.pol[~inside]) and np.array_equal(got_p[a:b], o_pol[a:b])
        _, _, o_delta3, o_changed3 = c.o_value(a, b)
        H.assert_bits_equal(np.float32(d_delta.item()), np.float32(o_delta3), what + ": value sweep residual")
        assert int(d_changed.item()) == o_changed3 == int((o_pol[a:b] != c.pol[a:b]).sum())


def _solver(c, resident, monkeypatch, **cfg):
    monkeypatch.setenv("PI_MI355_RESIDENT", resident)
    s = c.cls(H.env_bins_space(c.name, c.shape), c.acts, envs.CudaPIConfig(**dict(c.cls.CONFIG, **cfg)), device=c.dev)
    n = s.n_states
    s.d_value_function[:n] = s._to_memory(_dev(c.V, c.dev))
    s.d_new_value_function.copy_(s.d_value_function)
    s.d_policy[:n] = s._to_memory(_dev(c.pol, c.dev))
    return s


def _one_launch_families(c, monkeypatch):
    """Where the handle has a one-launch family (LDS-resident, dataflow, XCD-local): pi_policy_evaluation with at most 60
    sweeps and the whole run() with 3 rounds, from the seeded (V, policy), against the same solver with the one-launch
    kernels off — V, policy, sweep counts, the residuals looked at, the stable flag; no XCD fallback."""
    torch = _torch()
    eng = c.eng
    if not (eng.info(Info.RESIDENT_STATES_PER_THREAD) > 0 or eng.info(Info.FLOW_WORKGROUPS) > 0 or eng.info(Info.XCD_ENABLED) > 0):
        return False
    a = _solver(c, "1", monkeypatch, max_eval_iter=60, max_pi_iter=3)
    b = _solver(c, "0", monkeypatch, max_eval_iter=60, max_pi_iter=3)
    ea, eb = a._backend.engine, b._backend.engine
    assert a._backend.resident and not b._backend.resident
    for code in (Info.RESIDENT_STATES_PER_THREAD, Info.FLOW_WORKGROUPS, Info.XCD_ENABLED):
        assert ea.info(code) == eng.info(code) and eb.info(code) == 0
    n, term = a.n_states, a._mask_arg()
    theta = float(c.cls.CONFIG["theta"])
    V1 = a.d_value_function[:n].clone()
    sweeps, looked = a._backend.policy_evaluation(V1, a.d_policy, term, c.gamma, theta, 60, 25)
    d_delta = torch.zeros(1, dtype=torch.float32, device=c.dev)
    src, dst = b.d_value_function[:n].clone(), torch.zeros(n, dtype=torch.float32, device=c.dev)
    host_looked, i = [], 0
    while i < 60:
        check = min(i if i % 25 == 0 else (i // 25 + 1) * 25, 59)
        k = check - i + 1
        eb.eval_sweeps(src.data_ptr(), dst.data_ptr(), b.d_policy.data_ptr(), b._backend._ptr(b._mask_arg()), 0, n, c.gamma, k,
                       d_delta.data_ptr())
        if k & 1:
            src, dst = dst, src
        i = check + 1
        host_looked.append(np.float32(d_delta.item()))
        if host_looked[-1] < theta:
            break
    what = f"{c.name} {c.shape}"
    assert sweeps == i, what
    H.assert_bits_equal(np.asarray(looked, np.float32), np.asarray(host_looked, np.float32), what + ": residuals looked at")
    H.assert_bits_equal(V1.cpu().numpy(), src.cpu().numpy(), what + ": V of pi_policy_evaluation")
    for s in (a, b):
        s.run()
    assert a.stats["sweeps_per_iter"] == b.stats["sweeps_per_iter"] and a.stats["pi_iterations"] == b.stats["pi_iterations"]
    assert a.stats["stable"] == b.stats["stable"] and a.stats["eval_sweeps"] == b.stats["eval_sweeps"]
    H.assert_bits_equal(a.value_function, b.value_function, what + ": V after run()")
    assert np.array_equal(a.policy, b.policy), what + ": policy after run()"
    assert a._backend.xcd_fallbacks == 0 and a._backend.one_launch_failures == 0
    if eng.info(Info.XCD_ENABLED) > 0 or eng.info(Info.RESIDENT_STATES_PER_THREAD) > 0:
        assert a._backend.whole_runs == 1                    # run() was one launch
    return True


def _solver_path(c, live, monkeypatch):
    """One evaluation sweep and one improvement sweep through the solver's own path — its memory order, its live-state
    list (`live`: whether there must be one), its per-evaluation list — from the seeded (V, policy), every state
    against the oracle."""
    monkeypatch.delenv("PI_MI355_ORDER", raising=False)
    s = _solver(c, "1", monkeypatch, max_eval_iter=1, max_pi_iter=1)
    if (c.name, c.shape) in ORDERS:
        assert s._order == ORDERS[(c.name, c.shape)] and s._backend.engine.order == (s._order or tuple(range(len(c.shape))))
    # the rule of the table, restated on this grid's mask in the solver's memory order: 2^20 states or more, and at least
    # 3 % of the lanes of the 64-state waves that hold a live state are dead
    mem = np.asarray(s._to_memory(c.term))
    waves = np.concatenate([mem, np.ones(-len(mem) % 64, dtype=bool)]).reshape(-1, 64)
    idle = (int((~waves).any(axis=1).sum()) * 64 - int((~mem).sum())) / c.n
    assert live == (c.n >= 1 << 20 and bool(c.term.any()) and idle >= 0.03), (c.n, idle)
    assert s._backend.engine.info(Info.LIVE_STATES) == (int((~c.term).sum()) if live else 0)
    assert not live or 0 < int((~c.term).sum()) < c.n
    s.policy_evaluation()
    assert s.stats["sweeps_per_iter"] == [1]
    n = s.n_states
    o_Vn, o_delta = c.o_eval(c.V)
    H.assert_bits_equal(s._to_user(s.d_value_function[:n]).cpu().numpy(), o_Vn, f"{c.name} {c.shape}: solver evaluation sweep")
    H.assert_bits_equal(np.float32(s._d_delta.item()), np.float32(o_delta), "its residual")
    # the improvement the solver makes is against ITS V (the sweep above): the oracle's entry for that
    o_pol, o_changed = c.chk.improve_sweep(c.states, c.acts, c.pol, o_Vn, c.term, *c.meta, c.gamma)
    s.policy_improvement()
    assert np.array_equal(s._to_user(s.d_policy[:n]).cpu().numpy(), o_pol), f"{c.name} {c.shape}: solver improvement sweep"
    assert s.stats["last_changed"] == o_changed
    s._backend.close()


ALL_CASES = H.edge_case_params()


@pytest.mark.parametrize("cid,name,shape,actions", ALL_CASES)
def test_edge_case_against_the_oracle(cid, name, shape, actions, cuda_device, monkeypatch):
    """The core check of the module on one specialisation: single sweeps, batches, sub-ranges, and — where they apply —
    the one-launch families and the solver's own path."""
    monkeypatch.delenv("PI_MI355_RESIDENT", raising=False)
    c = _Case(name, shape, actions, cuda_device)
    assert c.n == int(np.prod(shape, dtype=np.int64))
    row = EXPECTED[cid]
    assert (row["name"], tuple(row["shape"])) == (name, tuple(shape))
    expect_one_launch = _assert_dispatch(c, row)
    o_Vn, o_pol, o_Vm = _single_sweeps(c)
    _batches(c)
    _sub_ranges(c, o_Vn, o_pol, o_Vm)
    assert _one_launch_families(c, monkeypatch) == expect_one_launch
    assert ("live" in row) == (c.n >= 1 << 20 or tuple(shape) in ((32, 32, 32, 31), (8, 8, 8, 8, 16, 15)))
    if "live" in row:
        _solver_path(c, row["live"], monkeypatch)
    c.eng.close()
    _torch().cuda.empty_cache()


def test_ties_between_clamped_actions_go_to_the_first_index(cuda_device):
    """Pendulum torques beyond the plugin's clamp of +-2 give exactly the same Q: wherever the greedy torque is a clamped
    one the kernel must return the FIRST index of the tie, as the oracle's strict '>' does (64 and 257 actions)."""
    for cid in ("act64", "act257"):
        _, name, shape, actions = next(case for case in H.EDGE_CASES if case[0] == cid)
        c = _Case(name, shape, actions, cuda_device, seed=5)
        d_p = c.d_pol.clone()
        c.eng.improve_sweep(c.d_V.data_ptr(), d_p.data_ptr(), c.d_term.data_ptr(), 0, c.n, c.gamma, 0)
        got = d_p.cpu().numpy()
        o_pol, _ = c.o_improve(c.pol)
        assert np.array_equal(got, o_pol)
        low, high = int((c.acts <= -2.0).sum()), int((c.acts < 2.0).sum())
        # no entry ever lands INSIDE a run of tied torques: index 0 stands for all of [0, low), `high` for [high, A)
        assert not ((got > 0) & (got < low)).any() and not (got > high).any()
        assert (got == 0).any() and (got == high).any(), "the seeded V never made a clamped torque greedy"
        c.eng.close()
