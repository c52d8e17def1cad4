"""The sweep kernels at the workgroup sizes PI_MI355_EVAL_BLOCK / PI_MI355_IMPROVE_BLOCK accept beyond the default 256 —
sizes that are no power of two (320, 448, 576, 704, 768, 960: what an occupancy experiment reaches for) and the product's
own 1024 / 512 of big 4-D grids, which otherwise runs on grids of 2^24 states only — against the oracle, bit for bit,
over ALL states of grids small enough to take a moment (tests/test_block_sizes_host.py builds every accepted size without
a device).  A chunk is as many states as the workgroup has threads, so the size moves every chunk boundary, the ragged
tail, the number of waves whose residual and changed count are folded, the groups of the strip schedule and which lanes
share a wave in the exact pass.

The knobs are read by pi_create: every engine here is made after monkeypatch.setenv and says Info.EVAL_BLOCK /
Info.IMPROVE_BLOCK back.  Grids: the smallest that give every kernel two workgroups and a ragged last chunk — pendulum
67 x 61 = 4 087, cartpole 9.7.11.5 = 3 465 = 3 * 1024 + 393, double_cartpole 5.4.6.4.5.4 = 9 600 (exactly 10 chunks of 960
and 30 of 320: a tail that is NOT ragged; ragged at every other size).  The one-launch kernels are switched off
(Option.RESIDENT 0) so that batches stay with the sweep kernels.  The oracle's sweeps of a grid do not depend on the size:
they are computed once per grid (`_REF`) and shared by every pair.

The strip schedule needs a period of at least 16 groups that is shorter than the range (plan_launch, csrc/pi_api.cpp): on
13.19.17.23 = 96 577 states a plane (7 429 states) is 16 groups of 448 and fewer of anything larger, and 16 * block states
are 16 groups at one chunk per workgroup and 8 at two.  Those launches are planned as slabs and run as such (the test
pins the planner's decision with the rule written out); 16 * block * cpw states are run as well, which is 16 groups in
every case, so that every size and both cpw do take strips.
"""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info, Option
from tests import helpers as H
from tests.test_gpu_edges import _Case, _batches, _single_sweeps, _sub_ranges

pytestmark = pytest.mark.gpu

PAIRS = [(320, 448), (768, 320), (960, 704), (576, 576), (1024, 512), (512, 1024)]        # (evaluation, improvement)
GRIDS = [("pendulum", (67, 61)), ("cartpole", (9, 7, 11, 5)), ("double_cartpole", (5, 4, 6, 4, 5, 4))]
TABLE_PAIRS = [(320, 448), (1024, 512)]
STRIP_PAIRS = [(960, 448), (1024, 512)]


def _torch():
    import torch
    return torch


def set_blocks(monkeypatch, pair):
    monkeypatch.setenv("PI_MI355_EVAL_BLOCK", str(pair[0]))
    monkeypatch.setenv("PI_MI355_IMPROVE_BLOCK", str(pair[1]))


_REF: dict = {}          # (env, shape, sweep kind, digest of its input, range) -> the oracle's result, never written to


def _digest(a) -> bytes:
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).digest()


class _Sized(_Case):
    """tests.test_gpu_edges._Case at a pair of workgroup sizes; `pair_table`: the unit is built with the table kernels.
    The oracle's answers are kept per grid, whatever the sizes."""

    def __init__(self, name, shape, dev, pair, monkeypatch, pair_table=False):
        set_blocks(monkeypatch, pair)
        monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")             # live-state lists on grids this small
        if not pair_table:
            super().__init__(name, shape, None, dev)
        else:                                                    # the same construction with the option set before pi_compile
            cls = envs.ENVS[name]
            self.name, self.shape, self.dev, self.cls = name, tuple(shape), dev, cls
            self.bins = H.env_bins(name, shape)
            self.acts = H.edge_actions(name)
            self.eng = _native.Engine(cls._D, [len(b) for b in self.bins], [b.min() for b in self.bins],
                                      [b.max() for b in self.bins], self.bins, self.acts, device=dev.index or 0)
            self.eng.set_option(Option.PAIR_TABLE, 1)
            self.eng.compile(envs.dynamics_source(name))
            plain = _cached(name, shape, dev, pair, monkeypatch)
            for k in ("meta", "states", "n", "term", "V", "pol", "gamma", "chk", "d_V", "d_pol", "d_term"):
                setattr(self, k, getattr(plain, k))
        self.pair = pair
        assert (self.eng.info(Info.EVAL_BLOCK), self.eng.info(Info.IMPROVE_BLOCK)) == tuple(pair)
        self.eng.set_option(Option.RESIDENT, 0)

    def _kept(self, kind, what, a, b, compute):
        key = (self.name, self.shape, kind, _digest(what), a, b)
        if key not in _REF:
            _REF[key] = compute()
        return _REF[key]

    def o_eval(self, V, a=0, b=None, out=None):
        assert out is None
        return self._kept("eval", V, a, b, lambda: _Case.o_eval(self, V, a, b))

    def o_improve(self, pol, a=0, b=None):
        return self._kept("improve", pol, a, b, lambda: _Case.o_improve(self, pol, a, b))

    def o_value(self, a=0, b=None, out=None):
        assert out is None
        return self._kept("value", self.pol, a, b, lambda: _Case.o_value(self, a, b))

    def set_cpw(self, cpw):
        self.eng.set_option(Option.EVAL_CPW, cpw)
        self.eng.set_option(Option.IMPROVE_CPW, cpw)
        assert (self.eng.info(Info.EVAL_CPW), self.eng.info(Info.IMPROVE_CPW)) == (cpw, cpw)


_cases: dict = {}


def _cached(name, shape, dev, pair, monkeypatch) -> _Sized:
    key = (name, tuple(shape), tuple(pair))
    if key not in _cases:
        _cases[key] = _Sized(name, shape, dev, pair, monkeypatch)
    return _cases[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c.eng.close()
    _cases.clear()
    _REF.clear()


@pytest.fixture
def case(request, cuda_device, monkeypatch):
    (name, shape), pair = request.param
    c = _cached(name, shape, cuda_device, pair, monkeypatch)
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")                 # read by pi_prepare_mask, not by pi_create
    yield c
    c.set_cpw(1)
    c.eng.prepare_mask(0)
    c.eng.set_option(Option.KEEP_LIVE_LIST, 0)
    c.eng.set_option(Option.STRIP_STATES, 0)
    c.eng.set_option(Option.GRAPHS, 1)


def _per_case(grids=GRIDS, pairs=PAIRS):
    params = [(g, p) for g in grids for p in pairs]
    return pytest.mark.parametrize("case", params, indirect=True,
                                   ids=[f"{g[0]}-{p[0]}-{p[1]}" for g, p in params])


@_per_case()
def test_the_grids_give_every_kernel_two_workgroups_and_both_kinds_of_tail(case):
    n = case.n
    assert n == int(np.prod(case.shape))
    for block in case.pair:
        assert block % 64 == 0 and -(-n // block) >= 2
        assert (n % block == 0) == (case.name == "double_cartpole" and block in (320, 960))


@pytest.mark.parametrize("cpw", [1, 3])
@_per_case()
def test_single_sweeps_and_sub_ranges(case, cpw):
    """All three sweep kinds on the whole grid and on [0, 1), [n - 1, n), an empty and a ragged range: V', policy, the
    residual and the changed count (their slots folded once: both outputs are pre-filled with other numbers), nothing
    written outside the range."""
    case.set_cpw(cpw)
    o_Vn, o_pol, o_Vm = _single_sweeps(case)
    _sub_ranges(case, o_Vn, o_pol, o_Vm)


@_per_case()
def test_batches(case):
    """Batches of 3 and of 26 evaluation sweeps, as a replayed graph and as plain launches."""
    _batches(case)


@_per_case(GRIDS[1:2])
def test_live_list_and_per_evaluation_list(case):
    """cartpole has terminal states: the live-state list (built by 256-thread kernels, consumed at the knob's size) serves
    the improvement sweep and every sweep of a batch but the first, the per-evaluation list (pi_eval_begin) the sweeps from
    the third on."""
    torch = _torch()
    c, eng, n, dev = case, case.eng, case.n, case.dev
    live = int((~c.term).sum())
    assert 0 < live < n
    eng.set_option(Option.KEEP_LIVE_LIST, 1)
    assert eng.prepare_mask(c.d_term.data_ptr()) == live == eng.info(Info.LIVE_STATES)
    for block in c.pair:
        assert -(-live // block) >= 2 and live % block != 0       # two workgroups and a ragged tail over the list as well
    # one evaluation sweep (state order: it copies the terminal values) and the improvement sweep over the list
    d_delta = torch.full((1,), 123.0, dtype=torch.float32, device=dev)
    d_changed = torch.full((1,), 77, dtype=torch.int32, device=dev)
    d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    eng.eval_sweep(c.d_V.data_ptr(), d_Vn.data_ptr(), c.d_pol.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, d_delta.data_ptr())
    o_Vn, o_delta = c.o_eval(c.V)
    H.assert_bits_equal(d_Vn.cpu().numpy(), o_Vn, "evaluation sweep with a live list kept")
    H.assert_bits_equal(np.float32(d_delta.item()), np.float32(o_delta), "its residual")
    d_p = c.d_pol.clone()
    eng.improve_sweep(c.d_V.data_ptr(), d_p.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, d_changed.data_ptr())
    o_pol, o_changed = c.o_improve(c.pol)
    assert np.array_equal(d_p.cpu().numpy(), o_pol), "improvement sweep over the live list"
    assert int(d_changed.item()) == o_changed
    # a 7-sweep batch over the list, and once more inside the bracket of one policy evaluation
    keep, cur = {}, c.V
    for i in range(1, 8):
        cur, delta = c.o_eval(cur)
        keep[i] = (cur, delta)
    nxt, _, done = c.chk.step(c.states, c.acts[c.pol])
    bootstraps = int((~c.term & ~done).sum())                     # live states whose successor under the policy is not terminal
    for bracket in (False, True):
        for graphs in (1, 0):
            eng.set_option(Option.GRAPHS, graphs)
            if bracket:
                assert eng.eval_begin(c.d_pol.data_ptr(), c.d_term.data_ptr()) == bootstraps == eng.info(Info.EVAL_LIST_ENTRIES)
                assert 0 < bootstraps <= live
            d_A, d_B = c.d_V.clone(), torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            d_delta.fill_(-1.0)
            eng.eval_sweeps(d_A.data_ptr(), d_B.data_ptr(), c.d_pol.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, 7, d_delta.data_ptr())
            what = f"7-sweep batch over the list, bracket {bracket}, graphs {graphs}"
            H.assert_bits_equal(d_B.cpu().numpy(), keep[7][0], what + ": newest iterate")
            H.assert_bits_equal(d_A.cpu().numpy(), keep[6][0], what + ": the iterate before")
            H.assert_bits_equal(np.float32(d_delta.item()), np.float32(keep[7][1]), what + ": residual")
            if bracket:
                eng.eval_end()
    assert eng.info(Info.LIVE_STATES) == live


@pytest.mark.parametrize("pair", TABLE_PAIRS, ids=[f"{e}-{i}" for e, i in TABLE_PAIRS])
def test_improvement_on_the_pair_table(pair, cuda_device, monkeypatch):
    """Option.PAIR_TABLE = 1: pi_improve_sweep_pairs_kernel and, with a list, pi_improve_live_pairs_kernel."""
    torch = _torch()
    name, shape = GRIDS[1]
    c = _Sized(name, shape, cuda_device, pair, monkeypatch, pair_table=True)
    eng, n = c.eng, c.n
    try:
        o_pol, o_changed = c.o_improve(c.pol)
        d_changed = torch.full((1,), 77, dtype=torch.int32, device=cuda_device)
        for listed in (False, True):
            if listed:
                eng.set_option(Option.KEEP_LIVE_LIST, 1)
                assert eng.prepare_mask(c.d_term.data_ptr()) == int((~c.term).sum()) == eng.info(Info.LIVE_STATES) > 0
            d_p = c.d_pol.clone()
            d_changed.fill_(77)
            eng.improve_sweep(c.d_V.data_ptr(), d_p.data_ptr(), c.d_term.data_ptr(), 0, n, c.gamma, d_changed.data_ptr())
            assert eng.info(Info.PAIR_TABLE) == 1
            assert np.array_equal(d_p.cpu().numpy(), o_pol), f"pair table, list {listed}"
            assert int(d_changed.item()) == o_changed
    finally:
        eng.close()


# ---- strip schedule -----------------------------------------------------------------------------------------------------
STRIP_GRID = ("double_pendulum_swingup", (13, 19, 17, 23))


def _strips_expected(period_states, block, cpw, count):
    """plan_launch's rule, written out: the period rounded to whole groups must be at least 16 groups and shorter than
    the range."""
    T = int(period_states / (block * cpw) + 0.5)
    groups = -(-(-(-count // block)) // cpw)
    return T if 16 <= T < groups else 0


@pytest.mark.parametrize("pair", STRIP_PAIRS, ids=[f"{e}-{i}" for e, i in STRIP_PAIRS])
def test_strip_schedule(pair, cuda_device, monkeypatch):
    torch = _torch()
    name, shape = STRIP_GRID
    c = _Sized(name, shape, cuda_device, pair, monkeypatch)
    eng, n, dev = c.eng, c.n, cuda_device
    eb, ib = pair
    plane = n // shape[0]
    d_delta = torch.zeros(1, dtype=torch.float32, device=dev)
    d_changed = torch.zeros(1, dtype=torch.int32, device=dev)
    taken = {"eval": set(), "improve": set()}
    try:
        for a, b in ((0, n), (n // 9 + 5, n - n // 7)):           # the whole grid; a ragged range that starts inside a period
            o_Vn, o_delta = c.o_eval(c.V, a, b)
            o_pol, o_changed = c.o_improve(c.pol, a, b)
            for cpw in (1, 2):
                c.set_cpw(cpw)
                for kind, block in (("eval", eb), ("improve", ib)):
                    for period in (plane, 16 * block, 16 * block * cpw):
                        eng.set_option(Option.STRIP_STATES, period)
                        s = eng.plan_schedule(block, a, b - a, chunks_per_workgroup=cpw)
                        assert s["period"] == _strips_expected(period, block, cpw, b - a), (kind, block, cpw, period)
                        assert period != 16 * block * cpw or s["period"] == 16
                        if s["period"]:
                            taken[kind].add(cpw)
                            assert s["grid_y"] >= 2 and (a == 0) == (s["phase"] == 0)
                            g = H.schedule_groups(s, -(-(b - a) // block))[:, 0]
                            assert sorted(g[g >= 0]) == list(range(-(-(-(-(b - a) // block)) // cpw)))
                        what = f"{kind} block {block} cpw {cpw} period {period} [{a},{b})"
                        if kind == "eval":
                            d_Vn = c.d_V.clone()
                            d_delta.fill_(123.0)
                            eng.eval_sweep(c.d_V.data_ptr(), d_Vn.data_ptr(), c.d_pol.data_ptr(), c.d_term.data_ptr(), a, b, c.gamma,
                                           d_delta.data_ptr())
                            got = d_Vn.cpu().numpy()
                            H.assert_bits_equal(got[a:b], o_Vn[a:b], what)
                            assert np.array_equal(got[:a], c.V[:a]) and np.array_equal(got[b:], c.V[b:]), what
                            H.assert_bits_equal(np.float32(d_delta.item()), np.float32(o_delta), what + ": residual")
                        else:
                            d_p = c.d_pol.clone()
                            d_changed.fill_(77)
                            eng.improve_sweep(c.d_V.data_ptr(), d_p.data_ptr(), c.d_term.data_ptr(), a, b, c.gamma, d_changed.data_ptr())
                            got = d_p.cpu().numpy()
                            assert np.array_equal(got[a:b], o_pol[a:b]), what
                            assert np.array_equal(got[:a], c.pol[:a]) and np.array_equal(got[b:], c.pol[b:]), what
                            assert int(d_changed.item()) == o_changed, what
        assert taken == {"eval": {1, 2}, "improve": {1, 2}}       # the strip schedule was really taken, by both kernels at both cpw
    finally:
        eng.close()


# ---- exact pass ---------------------------------------------------------------------------------------------------------
def mixed_waves(flag, block, cpw):
    """Of the launch that walks the units `flag` describes (states of a range, entries of a list) in chunks of `block`:
    how many waves — 64 consecutive lanes of one chunk — hold a flagged and an unflagged unit.  Lanes past the end shadow
    the last unit and store nothing; they are not counted."""
    m = len(flag)
    chunks = -(-m // block)
    groups = -(-chunks // cpw)
    idx = np.full(groups * cpw * block, -1, dtype=np.int64)
    idx[:m] = np.arange(m)
    idx = idx.reshape(groups * cpw * (block // 64), 64)
    ok = idx >= 0
    f = ok & flag[np.maximum(idx, 0)]
    u = ok & ~flag[np.maximum(idx, 0)]
    return int((f.any(axis=1) & u.any(axis=1)).sum())


@pytest.mark.parametrize("pair", TABLE_PAIRS, ids=[f"{e}-{i}" for e, i in TABLE_PAIRS])
@pytest.mark.parametrize("shape", [(24, 17), (9, 7, 11, 5)], ids=["24x17", "9x7x11x5"])
def test_exact_pass(shape, pair, monkeypatch):
    """The synthetic plugin of tests/test_gpu_fallback_paths.py, whose calls leave their common path on some lanes of a
    wave: evaluation, improvement and value sweep over [3, n - 5), in state order and over a live list, at one and three
    chunks per workgroup, against the oracle built from the same text."""
    torch = _torch()
    from tests import test_gpu_fallback_paths as F
    set_blocks(monkeypatch, pair)
    syn = F._Syn(shape, torch.device("cuda:0"))
    eng = syn.eng
    try:
        assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == tuple(pair)
        eng.set_option(Option.RESIDENT, 0)
        flag = F._flagged(syn.states)[0]
        lo, hi = 3, syn.n - 5
        for masked in (False, True):
            rng_state = syn.rng.bit_generator.state               # the mask test_sweeps_match_the_oracle... is about to draw
            term = (syn.rng.random(syn.n) < 0.4) if masked else np.zeros(syn.n, bool)
            syn.rng.bit_generator.state = rng_state
            units = flag[lo:hi][~term[lo:hi]] if masked else flag[lo:hi]
            for cpw in (1, 3):
                for block in pair:
                    assert mixed_waves(units, block, cpw) >= 1, (shape, block, cpw, masked)
                eng.set_option(Option.EVAL_CPW, cpw)
                eng.set_option(Option.IMPROVE_CPW, cpw)
                syn.rng.bit_generator.state = rng_state
                F.test_sweeps_match_the_oracle_bit_for_bit(syn, masked, monkeypatch)
    finally:
        eng.close()


# ---- whole runs -----------------------------------------------------------------------------------------------------------
def test_whole_run_against_the_oracle(cuda_device, monkeypatch):
    name, shape = GRIDS[1]
    set_blocks(monkeypatch, (320, 448))
    monkeypatch.setenv("PI_MI355_RESIDENT", "0")
    cls = envs.ENVS[name]
    cfg = envs.CudaPIConfig(**dict(cls.CONFIG, max_pi_iter=3, max_eval_iter=60))
    s = cls(H.env_bins_space(name, shape), cls.ACTIONS, cfg, device=cuda_device)
    eng = s._backend.engine
    assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == (320, 448) and not s._backend.resident
    s.run()
    bins = H.env_bins(name, shape)
    states = oracle.states_from_bins(bins)
    term, tval = H.terminal_mask(name, states)
    ref = H.oracle_for(name).run(states, cls.ACTIONS, term, *oracle.grid_metadata(bins), gamma=cfg.gamma, theta=cfg.theta,
                                 max_eval_iter=cfg.max_eval_iter, max_pi_iter=cfg.max_pi_iter, terminal_value=tval)
    assert s.stats["sweeps_per_iter"] == list(ref["sweeps_per_iter"]) and len(ref["sweeps_per_iter"]) >= 2
    assert np.array_equal(s.policy, ref["policy"])
    H.assert_bits_equal(s.value_function, ref["value_function"], "V of run() at 320 / 448 threads")


def test_sharded_run_equals_the_single_rank_run(cuda_device, monkeypatch):
    """World 3 over the in-process transport, halo exchange (the case and the harness of
    tests/test_gpu_parity.py::test_sharded_driver_local_transport): a rank's sub-ranges start and end anywhere in a
    320- or 448-state chunk."""
    import threading
    import uuid
    from dynamicprogramming_amd import transport as T
    torch = _torch()
    world, name, shape = 3, "double_pendulum_swingup", (14, 9, 11, 8)
    set_blocks(monkeypatch, (320, 448))
    monkeypatch.setenv("PI_MI355_RESIDENT", "0")
    monkeypatch.setenv("PI_MI355_EXCHANGE", "halo")
    cls = envs.ENVS[name]
    cfg_kw = {**cls.CONFIG, "max_pi_iter": 3, "max_eval_iter": 60}
    single = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg_kw), device=cuda_device)
    eng = single._backend.engine
    assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == (320, 448)      # before run() releases the device
    single.run()
    group = f"test-{uuid.uuid4().hex}"
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            stream = torch.cuda.Stream(device=cuda_device)
            with torch.cuda.stream(stream):
                s = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cfg_kw), device=cuda_device,
                        transport=T.NativeTransport.local(r, world, group))
                eng = s._backend.engine
                blocks = (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK))
                info = dict(s._comm.info)
                s.run()
            out[r] = (s.value_function, s.policy, list(s.stats["sweeps_per_iter"]), info, blocks)
        except Exception as exc:  # noqa: BLE001
            errors.append((r, repr(exc)))

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    assert all(o is not None for o in out), "a rank did not finish"
    for r in range(world):
        V, pol, sweeps, info, blocks = out[r]
        assert blocks == (320, 448) and info["mode"] == "halo"
        H.assert_bits_equal(V, single.value_function, f"rank {r} V")
        assert np.array_equal(pol, single.policy)
        assert sweeps == single.stats["sweeps_per_iter"]
