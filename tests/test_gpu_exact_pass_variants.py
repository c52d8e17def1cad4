"""The sweeps' exact pass (csrc/pi_sweep_kernels.hip, "common paths first") in the variants tests/test_gpu_fallback_paths.py
leaves out, on that module's synthetic plugins and grids, bit for bit against the oracle built from the same string (a NaN
matches any NaN):

* with the pair table: pi_argmax<false, true>, the exact instantiation gathering 16-byte quads, in the redo loops of
  pi_improve_body and pi_improve_live_body (Option.PAIR_TABLE = 1 set before compile; a plugin that leaves its common path
  on an 80^4 grid takes this path by default);
* with more than one chunk per workgroup (Option.IMPROVE_CPW / EVAL_CPW 2, 3 and 64): a flagged lane walks ALL its chunks
  again, so an unflagged state of that lane is visited twice — `changed` and the value sweep's residual must not count it
  twice, in the PI_FAST_FIRST form (lane re-derived behind a barrier, old action re-read) and in the live-list form;
* in memory orders other than the identity: pi_dynamics_common, pi_exact_coords and pi_state_coords work in memory order;
* the 6-D grid as the control: the single-instantiation form, `rare` constant 0, the redo loop folded away.

`test_the_cases_test_what_they_claim` computes on the host, from _flagged, Info.IMPROVE_BLOCK and the slab schedule, that
the inputs do reach those paths: lanes with a flagged state in one chunk and an unflagged live state whose action changes
in another (lanes with both kinds of state, unmasked, [0, n) / [3, n - 5): 24x17 cpw 2 and 3 106 / 100; 9x7x11x5 702 and 948;
5x4x6x4x5x4 1 024 and 1 408), a ragged last chunk (tid != lane), and at cpw 64 one workgroup for the whole range.

Ranges and lists are in MEMORY order, the oracle works in the user's: its whole-grid results go through Engine.to_memory
and a range's `changed` and residual are taken from them as the oracle takes them (count of entries that differ; maximum
of |V' - V| in float32, a NaN never wins) — in the identity order the oracle's own ranged calls are asked as well.

One engine per (grid, memory order), five in all; the pair table and the chunks per workgroup are switched at run time.
`test_ranged_expectations_are_the_oracles_own` needs no device and carries no gpu mark.

Wall time on an MI355X, from one `pytest -m gpu --durations=0` run of the whole suite (521 s): building the five engines
(the setup of the first test of each) 0.54 + 0.97 + 1.05 + 1.03 + 0.56 s, every one of the 26 test bodies under 5 ms —
4.2 s for the module, against 0.4 to 1.05 s for each case of tests/test_gpu_fallback_paths.py in the same run.

That the tests bite, tried on a scratch build: without `rare == 0u` at the hot passes' stores 18 of these cases fail (and
4 of tests/test_gpu_fallback_paths.py); with the redo loops calling pi_argmax<false, false> on the table pointer, the
three pair-table cases and the twelve 4-D cpw cases fail; with the hot pass not storing once its lane is flagged
(a double count at cpw > 1 only), the three 24x17 cpw cases fail as well, `changed` 366 for the oracle's 324 — and nothing
else in tests/test_gpu_fallback_paths.py, tests/test_gpu_pair_table.py or the cpw test of tests/test_gpu_parity.py does.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native
from dynamicprogramming_amd._native import Info, Option
from tests import helpers as H
from tests.test_gpu_fallback_paths import ACTIONS, GAMMA, GRIDS, _bins, _flagged, _plugin, _same

gpu = pytest.mark.gpu               # every test but the host-only one at the oracle's ranged calls

SHAPE_4D = GRIDS[1]
ORDERS_4D = [None, (0, 2, 1, 3), (3, 1, 0, 2)]
UNITS = [(GRIDS[0], None)] + [(SHAPE_4D, o) for o in ORDERS_4D] + [(GRIDS[2], None)]
UNIT_IDS = ["x".join(map(str, s)) + ("" if o is None else "-" + "".join(map(str, o))) for s, o in UNITS]
CPWS = (2, 3, 64)


def _to_mem(a, shape, order):
    """numpy restatement of Engine.to_memory (checked against it where an engine exists)."""
    return a if order is None else np.ascontiguousarray(a.reshape(shape).transpose(order)).reshape(-1)


def _fmax_abs_diff(a, b):
    """max |a - b| in float32 the way the oracle and the kernels fold it: from 0, a NaN never wins."""
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float32) - b.astype(np.float32))
    d = d[~np.isnan(d)]
    return np.float32(d.max()) if len(d) else np.float32(0.0)


class _Inputs:
    """Seeded (V, policy, mask) of one (grid, order, masked or not) and the oracle's whole-grid sweeps of them; host
    arrays in MEMORY order."""

    def __init__(self, host, masked, seed):
        rng = np.random.default_rng(seed)
        n = host.n
        V = (rng.standard_normal(n) * 3.0).astype(np.float32)
        pol = rng.integers(0, len(ACTIONS), size=n).astype(np.int32)
        term = (rng.random(n) < 0.4) if masked else np.zeros(n, bool)
        V[term] = np.float32(-7.0)
        pol[term] = 0
        self.masked = masked
        self.user = (V, pol, term)
        args = (host.states, ACTIONS, pol, V, term, *host.meta, GAMMA)
        o_Vn, self.o_delta = host.chk.eval_sweep(*args)
        o_pol, self.o_changed = host.chk.improve_sweep(*args)
        o_Vm, o_pol3, self.o_delta3, o_changed3 = host.chk.value_sweep(*args)
        assert np.array_equal(o_pol, o_pol3) and o_changed3 == self.o_changed > 0
        m = lambda a: _to_mem(a, host.shape, host.order)
        self.V, self.pol, self.term = m(V), m(pol), m(term)
        self.o_Vn, self.o_pol, self.o_Vm = m(o_Vn), m(o_pol), m(o_Vm)
        self.n_live = int((~term).sum())

    # what a sweep over [a, b) of the memory order must leave, from the whole-grid results
    def want_eval(self, a, b):
        Vn = self.V.copy()
        Vn[a:b] = self.o_Vn[a:b]
        return Vn, _fmax_abs_diff(self.o_Vn[a:b], self.V[a:b])

    def want_improve(self, a, b):
        pol = self.pol.copy()
        pol[a:b] = self.o_pol[a:b]
        return pol, int(np.count_nonzero(self.o_pol[a:b] != self.pol[a:b]))

    def want_value(self, a, b):
        Vm = self.V.copy()
        Vm[a:b] = self.o_Vm[a:b]
        live = ~self.term[a:b]
        return Vm, _fmax_abs_diff(self.o_Vm[a:b][live], self.V[a:b][live])


class _Host:
    """Grid, plugin, oracle and both sets of inputs of one unit — nothing here needs a device."""

    def __init__(self, shape, order):
        self.shape, self.order, self.D = tuple(shape), order, len(shape)
        self.src = _plugin(self.D)
        self.bins = _bins(shape)
        self.chk = oracle.build(self.D, self.src)
        self.meta = oracle.grid_metadata(self.bins)
        self.states = oracle.states_from_bins(self.bins)
        self.n = len(self.states)
        self.flag = _to_mem(_flagged(self.states)[0], self.shape, order)          # per state of the memory order
        seed = 4100 + 10 * UNITS.index((self.shape, order))
        self.plain, self.masked = _Inputs(self, False, seed), _Inputs(self, True, seed + 1)
        self.ranges = ((0, self.n), (3, self.n - 5))


_hosts: dict = {}
_units: dict = {}


def _host(shape, order) -> _Host:
    key = (tuple(shape), order)
    if key not in _hosts:
        _hosts[key] = _Host(shape, order)
    return _hosts[key]


class _Unit:
    """The engine of one (grid, order) — 4-D: built with the table kernels — and its inputs on the device."""

    def __init__(self, host, dev):
        import torch
        self.torch, self.dev, self.h = torch, dev, host
        b = host.bins
        self.eng = eng = _native.Engine(host.D, list(host.shape), [x.min() for x in b], [x.max() for x in b], b, ACTIONS,
                                        device=dev.index or 0, order=host.order)
        self.tables = host.D == 4
        if self.tables:
            eng.set_option(Option.PAIR_TABLE, 1)
        eng.compile(host.src)
        assert ("#define PI_PAIR_TABLE 1\n" in eng.kernel_source(host.src)) == self.tables
        assert ("#define PI_FAST_FIRST 1\n" in eng.kernel_source(host.src)) == (host.D <= 4)
        self.d = {}
        for c in (host.plain, host.masked):
            V, pol, term = c.user
            for got, kept in ((eng.to_memory(V), c.V), (eng.to_memory(pol), c.pol), (eng.to_memory(term), c.term)):
                assert np.array_equal(got, kept)
            self.d[c.masked] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (c.V, c.pol, c.term.astype(np.uint8)))
        self.d_delta = torch.zeros(1, dtype=torch.float32, device=dev)
        self.d_changed = torch.zeros(1, dtype=torch.int32, device=dev)

    def use_list(self, c, on):
        """The live-state list of the mask of `c` (kept whatever it saves), or none: the state-order kernels."""
        eng = self.eng
        if on:
            eng.set_option(Option.KEEP_LIVE_LIST, 1)
            assert eng.prepare_mask(self.d[True][2].data_ptr()) == c.n_live and eng.info(Info.LIVE_STATES) == c.n_live > 0
        else:
            assert eng.prepare_mask(0) == 0 and eng.info(Info.LIVE_STATES) == 0

    def improve(self, c, a, b, what):
        """One improvement sweep over [a, b) against the oracle; returns (policy, changed, Info.PAIR_TABLE)."""
        d_V, d_pol, d_term = self.d[c.masked]
        d_p = d_pol.clone()
        self.d_changed.fill_(77)
        self.eng.improve_sweep(d_V.data_ptr(), d_p.data_ptr(), d_term.data_ptr(), a, b, GAMMA, self.d_changed.data_ptr())
        got, changed = d_p.cpu().numpy(), int(self.d_changed.item())
        want, want_changed = c.want_improve(a, b)
        _same(got, want, f"{what}: improved policy over [{a},{b})")
        assert changed == want_changed > 0, f"{what}: changed over [{a},{b}) {changed}, the oracle {want_changed}"
        return got, changed, self.eng.info(Info.PAIR_TABLE)

    def value(self, c, a, b, what):
        d_V, d_pol, d_term = self.d[c.masked]
        d_p, d_Vm = d_pol.clone(), d_V.clone()
        self.d_changed.fill_(77)
        self.d_delta.fill_(123.0)
        self.eng.value_sweep(d_V.data_ptr(), d_Vm.data_ptr(), d_p.data_ptr(), d_term.data_ptr(), a, b, GAMMA,
                             self.d_delta.data_ptr(), self.d_changed.data_ptr())
        want_V, want_delta = c.want_value(a, b)
        want_pol, want_changed = c.want_improve(a, b)
        _same(d_Vm.cpu().numpy(), want_V, f"{what}: V' of the value sweep over [{a},{b})")
        _same(d_p.cpu().numpy(), want_pol, f"{what}: policy of the value sweep over [{a},{b})")
        _same(np.float32(self.d_delta.item()), want_delta, f"{what}: the value sweep's residual over [{a},{b})")
        assert int(self.d_changed.item()) == want_changed, f"{what}: the value sweep's changed over [{a},{b})"

    def evaluate(self, c, a, b, what):
        d_V, d_pol, d_term = self.d[c.masked]
        d_Vn = d_V.clone()
        self.d_delta.fill_(123.0)
        self.eng.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), a, b, GAMMA, self.d_delta.data_ptr())
        want_V, want_delta = c.want_eval(a, b)
        _same(d_Vn.cpu().numpy(), want_V, f"{what}: V' of the evaluation sweep over [{a},{b})")
        _same(np.float32(self.d_delta.item()), want_delta, f"{what}: the evaluation sweep's residual over [{a},{b})")

    def set_cpw(self, cpw):
        self.eng.set_option(Option.IMPROVE_CPW, cpw)
        self.eng.set_option(Option.EVAL_CPW, cpw)
        assert self.eng.info(Info.IMPROVE_CPW) == cpw and self.eng.info(Info.EVAL_CPW) == cpw


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for u in _units.values():
        u.eng.close()
    _units.clear()


@pytest.fixture
def unit(request, cuda_device, monkeypatch):
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")                  # the live list on grids this small
    key = request.param
    if key not in _units:
        _units[key] = _Unit(_host(*key), cuda_device)
    u = _units[key]
    yield u
    u.set_cpw(1)
    u.eng.prepare_mask(0)
    if u.tables:
        u.eng.set_option(Option.PAIR_TABLE, 1)


def _per_unit(units=UNITS):
    return pytest.mark.parametrize("unit", units, ids=[UNIT_IDS[UNITS.index(k)] for k in units], indirect=True)


# ---- the guard ------------------------------------------------------------------------------------------------------
def mixed_lanes(flag, live, moves, block, cpw):
    """Of the launch that walks the units `flag` / `live` / `moves` describe (states of a range, entries of a list) with
    `cpw` consecutive chunks of `block` units per workgroup: (lanes that hold a flagged live unit in one chunk and an
    unflagged live one in another, those of them in which such an unflagged unit's action changes).  Only the lanes that
    store (tid == lane) are looked at."""
    m = len(flag)
    chunks = -(-m // block)
    groups = -(-chunks // cpw)
    idx = np.full(groups * cpw * block, -1, dtype=np.int64)
    idx[:m] = np.arange(m)
    idx = idx.reshape(groups, cpw, block)
    ok = idx >= 0
    f = ok & flag[idx] & live[idx]
    u = ok & ~flag[idx] & live[idx]
    both = f.any(axis=1) & u.any(axis=1)                          # a cell is one or the other: two different chunks
    twice = f.any(axis=1) & (u & moves[idx]).any(axis=1)
    return int(both.sum()), int(twice.sum())


def guard(host, c, a, b, block, cpw, listed=False):
    """mixed_lanes of one sweep of the tests below: over the states [a, b), or over their live-list entries."""
    flag, live, moves = host.flag[a:b], ~c.term[a:b], (c.o_pol != c.pol)[a:b]
    if listed:
        flag, moves, live = flag[live], moves[live], live[live]
    return mixed_lanes(flag, live, moves, block, cpw) + (len(flag),)


@gpu
@_per_unit()
def test_the_cases_test_what_they_claim(unit):
    h, eng = unit.h, unit.eng
    block = eng.info(Info.IMPROVE_BLOCK)
    assert block == eng.info(Info.EVAL_BLOCK) == 256
    assert 0.05 <= h.flag.mean() <= 0.60
    for a, b in h.ranges:
        for c, listed in ((h.plain, False), (h.masked, False), (h.masked, True)):
            for cpw in (2, 3):
                both, twice, m = guard(h, c, a, b, block, cpw, listed)
                print(f"{h.shape} {h.order} [{a},{b}) masked {c.masked} listed {listed} cpw {cpw}: {both} lanes hold a "
                      f"flagged and an unflagged live state, in {twice} of them the unflagged one's action changes")
                if not listed or h.D > 2:                            # 24x17 lists ~245 live states: one chunk, no claim made
                    assert both >= 1 and twice >= 1
                    assert m % block != 0 and -(-m // block) >= 2    # a ragged last chunk: tid != lane there
                # the slab schedule with consecutive chunks per workgroup is what these launches take
                s = eng.plan_schedule(block, 0 if listed else a, m, total=m if listed else None, chunks_per_workgroup=cpw)
                assert s["period"] == 0 and s["cpw"] == cpw
                g = H.schedule_groups(s, -(-m // block))[:, 0]
                assert sorted(g[g >= 0]) == list(range(-(-(-(-m // block)) // cpw)))
            m = guard(h, c, a, b, block, 64, listed)[2]
            s = eng.plan_schedule(block, 0 if listed else a, m, total=m if listed else None, chunks_per_workgroup=64)
            g = H.schedule_groups(s, -(-m // block))[:, 0]
            assert -(-m // block) <= 64 and s["period"] == 0 and list(g[g >= 0]) == [0]         # one workgroup takes it all
            assert -(-m // block) >= 2 or (listed and h.D == 2)


def test_ranged_expectations_are_the_oracles_own():
    """Identity order: `changed` and the residuals taken from the whole-grid results equal the oracle's ranged calls."""
    for shape in GRIDS:
        h = _host(shape, None)
        for c in (h.plain, h.masked):
            V, pol, term = c.user
            for a, b in h.ranges:
                args = (h.states, ACTIONS, pol, V, term, *h.meta, GAMMA, a, b)
                o_Vn, o_delta = h.chk.eval_sweep(*args)
                _same(o_Vn, c.want_eval(a, b)[0], "V'")
                _same(np.float32(o_delta), c.want_eval(a, b)[1], "residual")
                o_pol, o_changed = h.chk.improve_sweep(*args)
                _same(o_pol, c.want_improve(a, b)[0], "policy")
                assert o_changed == c.want_improve(a, b)[1]
                o_Vm, o_pol3, o_delta3, o_changed3 = h.chk.value_sweep(*args)
                _same(o_Vm, c.want_value(a, b)[0], "V' of the value sweep")
                _same(np.float32(o_delta3), c.want_value(a, b)[1], "its residual")
                assert o_changed3 == o_changed and np.array_equal(o_pol3, o_pol)


# ---- the exact pass on the pair table, in three memory orders -----------------------------------------------------------
@gpu
@_per_unit(UNITS[1:4])
def test_exact_pass_on_the_pair_table(unit):
    h, eng = unit.h, unit.eng
    n = h.n
    assert n > 256 and n % 256 != 0
    res = {}
    for option in (1, 0):
        eng.set_option(Option.PAIR_TABLE, option)
        for c, listed in ((h.plain, False), (h.masked, False), (h.masked, True)):
            unit.use_list(c, listed)
            pol, changed, used = unit.improve(c, 0, n, f"option {option}, masked {c.masked}, list {listed}")
            assert used == option, f"option {option}: Info.PAIR_TABLE says {used}"
            if listed:
                assert eng.info(Info.LIVE_STATES) > 0
            res[option, c.masked, listed] = (pol, changed)
    for (option, masked, listed), (pol, changed) in res.items():
        if option == 1:
            pol0, changed0 = res[0, masked, listed]
            assert np.array_equal(pol, pol0) and changed == changed0
    # a sub-range of the engine with the option on reads V
    eng.set_option(Option.PAIR_TABLE, 1)
    for c, listed in ((h.plain, False), (h.masked, False), (h.masked, True)):
        unit.use_list(c, listed)
        assert unit.improve(c, 3, n - 5, f"option 1, masked {c.masked}, list {listed}")[2] == 0


@gpu
@_per_unit(UNITS[1:4])
def test_plain_kernels_in_memory_orders(unit):
    h = unit.h
    unit.eng.set_option(Option.PAIR_TABLE, 0)
    for c, listed in ((h.plain, False), (h.masked, False), (h.masked, True)):
        unit.use_list(c, listed)
        for a, b in h.ranges:
            what = f"order {h.order}, masked {c.masked}, list {listed}"
            unit.evaluate(c, a, b, what)
            assert unit.improve(c, a, b, what)[2] == 0
            unit.value(c, a, b, what)


# ---- more than one chunk per workgroup -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cpw", CPWS)
@_per_unit()
def test_exact_pass_with_several_chunks_per_workgroup(unit, cpw):
    h, eng = unit.h, unit.eng
    unit.set_cpw(cpw)
    for option in ((1, 0) if unit.tables else (None,)):
        if option is not None:
            eng.set_option(Option.PAIR_TABLE, option)
        for c, listed in ((h.plain, False), (h.masked, False), (h.masked, True)):
            unit.use_list(c, listed)
            for a, b in h.ranges:
                what = f"cpw {cpw}, option {option}, masked {c.masked}, list {listed}"
                used = unit.improve(c, a, b, what)[2]
                assert used == (1 if option == 1 and (a, b) == (0, h.n) else 0), what
                if option != 1:                                  # neither sweep below looks at the option
                    unit.value(c, a, b, what)
                    unit.evaluate(c, a, b, what)
