"""
GPU: the worst-case sweeps (pi_robust_eval_kernel, pi_robust_improve_kernel, pi_robust_value_kernel of
csrc/pi_expect_kernels.hip) where the expectation sweeps have their edge coverage: sections 0 and a - e of
tests/test_gpu_expect_edges.py with the minimum fold, plus the inputs that exist for the fold alone.  The case tables and
helpers are that file's, the device arrays are `_Sweeps` of tests/test_gpu_robust.py (its `sweep` launches pi_robust_*),
the twin is `test_gpu_robust._twin_of` (dynamicprogramming_amd/noise.py with risk="worst" on the checker's step).

Bar everywhere: V' and policy bit for bit against the twin (a NaN matches a NaN of any payload in section d1 only),
residual and changed count exactly, states outside a launched range keep their sentinel, the source buffer is untouched.
Every GPU step runs once.  What a sub-range launch leaves behind follows from ONE whole-grid twin per (case, set), kept in
`_TWINS`.  What makes a comparison worth something is asserted from twin arrays alone, never from GPU output: the per-point
q of tests/robust_cases.point_q folded on the host by the strict rule and by three wrong ones (robust_cases.fold):
"fmin" (a NaN is dropped, -0 is below +0), "last-of-equals" (`<=`), "zero-weight-rows-participate".

Which wrong fold a case can tell from the right one follows from the values it folds.  Two q that compare equal and are
not zeros have the same bits, so "last-of-equals" changes a SWEEP's output only where +0 meets -0 (the adversary query
returns k*: tests/test_gpu_adversary_edges.py); "fmin" differs only where a NaN or a zero of the other sign is folded;
the third only where a row of weight 0 is in the set.  So: the signed-zero case separates all three, the non-finite
cases "fmin" (and the third under their zero-weight set), the sets of d2 with a weight-0 row the third.  A finite V
without zeros cannot separate the first two, so the sets of d2 run once more on a non-finite V and on the signed-zero V,
where each of them separates every rule its rows can show (D2_SEPARATES says which and why).

What would have to be wrong in the kernel for a section to fail.  OBSERVED: failed in the mutation run (pi_expect_q's
`if (!started || q < Q || q != q) Q = q;` replaced by `Q = started ? fminf(Q, q) : q;`, run once, not committed);
JUDGED: written from the code, not run.

0. checked handle.  JUDGED: the pi_robust_* kernels are in the expectation module and add to its copy of pi_debug_words;
   a report that read the sweeps' module only would say 0 violations; pi_checked_action not reached from the second
   instantiation of PI_EXPECT_EVAL_KERNEL would read lds_tab past the action table.
a. degenerate grids / staging.  JUDGED: as section a of the expectation file — pi_stage_table<256>, lds_noise beside a
   15 360-float lds_tab with 64 rows installed, 2-bin dimensions, 4 and 63 states under `lane = min(tid, count - 1)`,
   PI_NA = 1 and 257 actions with exact ties — in the improve / value body, which is instantiated a second time with WORST
   and keeps its own `held` cache across the action loop: a weight-0 `continue` that skipped the cache's invalidation,
   or `started` kept across actions, would show on act257 and act1.
b. chunk boundaries.  JUDGED: pi_expect_chunk's tail bound, a workgroup without a chunk reaching the barrier, span = 2 at
   nine chunks, shadow lanes of a tail adding to the changed count or the residual, a tail whose last valid state is
   terminal (its shadows skip the point loop, the readfirstlane of a row is then taken from another lane), an unaligned
   s_begin — in pi_expect_improve_body<*, true> as well as in the evaluation macro's second instantiation.
c. build forms.  JUDGED: PI_BLOCK_EVAL / PI_BLOCK_IMPROVE of 320, 448, 1024, 512, the IEEE and the mixed pi_locate, the
   checked pi_locate / pi_checked_action, PI_PAIR_TABLE 1 and three chunks per workgroup leaking into the robust kernels.
d1. non-finite values and signed zeros.  OBSERVED: test_non_finite_values (3), test_every_q_of_a_state_nan (3),
   test_signed_zeros and both cases of test_sets_with_edge_entries_on_non_finite_and_signed_zero_values fail under the
   fminf mutation (a NaN point is dropped; -0 replaces +0); the other 52 tests of this file pass under it, as a finite V
   without zeros has to.  Of the earlier tests, tests/test_gpu_robust.py::test_a_nan_under_one_point_makes_q_nan (3) fails
   too and nothing else does.  JUDGED: `q != q` lost (a NaN never taken: same outputs as fminf where the NaN is not
   first), `q <= Q` (-0 replaces +0: the signed-zero case), best_q = -1.0e30f / best = 0 where every Q is NaN with the
   changed count counting that state, `dlt > dmax` letting a NaN through.
d2. sets at their edges.  JUDGED: `started` set before the weight test (a weight-0 first row would give Q), a weight-0 row
   updating da_prev (A, 0, A would step twice: same bits, not visible) or NOT updating it while stepping (A, B, A sharing
   A's step: visible, asserted from the twin), `== 0.0f` replaced by a bit test (-0.0 would take part) or evaluated
   with denormals flushed (1e-40 would not), K = 64 with one participating row reading row 63's words from the wrong
   offset, the clamp one ulp inside and beyond a_max / a_min.
e. large handles.  JUDGED: as section e of the expectation file; only the launch differs.

Measured on an MI355X (this module alone, `pytest -m gpu --durations=0`, code objects in the cache): 61 tests in 25.2 s;
the expectation file on the same machine in the same call: 55 tests in 29.1 s, its slowest test 3.66 s (64^4).  Slowest
calls here: the 2^29 grid 3.2 s, 64^4 3.0 s (both with a quarter of the expectation file's sample states: sample_shift=2),
act257 1.8 s, sets 6d 1.7 s, one2-4d-strided 1.2 s, one2-4d 1.1 s, tab15360 1.0 s, non-finite 6d 0.9 s, everything else 0.8 s
or less.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import noise
from dynamicprogramming_amd._native import Info
from dynamicprogramming_amd.noise import Disturbances
from tests import helpers as H
from tests import robust_cases as RC
from tests import test_gpu_expect_edges as E
from tests.test_gpu_expect import _case, _check, _engine, _expected, _make_set, _residual
from tests.test_gpu_expect_edges import (EDGE_BY_ID, FORM_GRIDS, FORMS, SMALL, _all_kinds, _check_nan, _install,
                                         _same_or_both_nan, _sub)
from tests.test_gpu_robust import _Sweeps, _twin, _twin_of

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = E.KINDS
_TWINS = {}


def _twin_once(key, c, d, **kw):
    """The whole-grid worst-case twin of (case, set) under `key`, computed once per process."""
    if key not in _TWINS:
        _TWINS[key] = _twin_of(c, d, **kw)
    return _TWINS[key]


def _policy_q(c, d, V=None):
    """Per-point q (K, live states) of the set under the policy's action, and the live states' indices."""
    live = np.flatnonzero(~c["term"])
    V = c["V"] if V is None else V
    q = RC.point_q(c["chk"].step, c["states"][live], c["acts"][c["pol"][live]], d, V, c["acts"], c["grid"], c["gamma"])
    return q, live


def _assert_separates(c, d, twin, wrong, what, V=None):
    """From the twin alone: the host fold of the per-point q under the strict rule IS the evaluation twin, and under each
    rule of `wrong` it differs from it in bits on at least one live state.  Returns the number of such states per rule."""
    q, live = _policy_q(c, d, V)
    assert len(live)
    strict, _ = RC.fold(q, d.weights)
    assert not RC.differs(strict, twin[1][live]).any(), f"{what}: the host fold is not the twin's"
    counts = {}
    for rule in wrong:
        counts[rule] = int(RC.differs(RC.fold(q, d.weights, rule)[0], strict).sum())
        assert counts[rule] >= 1, f"{what}: the fold '{rule}' gives the twin's bits on every live state"
    return counts


# ---- 0. the checked handle's report ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", FORM_GRIDS)
def test_checked_handle_reports_what_the_robust_sweeps_met(grid, cuda_device, monkeypatch):
    """Section 0 of the expectation file with pi_robust_* in place of pi_expect_*: clean sweeps of the three kinds report
    nothing and give the unchecked handle's bits; the three corrupt policy entries met by robust_eval_sweeps are reported
    (3 violations) and contained; a second report is clean; the deterministic sweep's 3 and both modules' 6 as there."""
    E.test_checked_handle_reports_what_the_expectation_sweeps_met(grid, cuda_device, monkeypatch, fold="robust")


# ---- a. degenerate grids and the thresholds of staging ------------------------------------------------------------------
WINDOWED_FROM = 4096          # states: from here on the K = 64 twin is evaluated on three windows only, and only they are launched


def _windows(n):
    """An aligned head, an unaligned window in the middle and an unaligned tail that ends on the last state."""
    return ((0, 300), (n // 2 - 129, n // 2 + 400), (n - 777, n))


def _twin_on(c, d, ranges):
    """`_twin_of` evaluated on the states of `ranges` only (every state's backup is independent of the others); the
    entries outside them hold V and the policy and stand for nothing."""
    V_eval, V_val, pol_val = np.array(c["V"]), np.array(c["V"]), np.array(c["pol"])
    args = (c["chk"].step, c["states"], c["pol"], c["V"], c["term"], d, c["acts"], *c["grid"], c["gamma"])
    for a, b in ranges:
        noise.expected_eval(*args, s_begin=a, s_end=b, out=V_eval, risk="worst")
        pol_val[a:b] = noise.expected_value_sweep(*args, s_begin=a, s_end=b, out=V_val, risk="worst")[1][a:b]
    for x in (V_eval, V_val, pol_val):
        x.setflags(write=False)
    return d, V_eval, V_val, pol_val


def _windowed(n, which):
    return which == "S3" and n >= WINDOWED_FROM


def _edge_ranges(n, which):
    return _windows(n) if _windowed(n, which) else ((0, n), _sub(n))


@lru_cache(maxsize=None)
def _edge(cid):
    """Case and the twins of S1, S2, S3 of one row of helpers.EDGE_CASES, computed once: over the whole grid, but for S3
    (64 points: the host's cost) on grids of WINDOWED_FROM states and more over `_windows` alone."""
    name, shape, acts = EDGE_BY_ID[cid]
    c = _case((name, tuple(shape)), actions=acts)
    twins = {}
    for w in E.EDGE_SETS:
        d = _make_set(w, c["D"], c["cell"], c["acts"])
        twins[w] = _twin_on(c, d, _windows(c["n"])) if _windowed(c["n"], w) else _twin_of(c, d)
    return c, twins


def _assert_edge_case_not_vacuous(cid, c, twins):
    """From the twin arrays alone: the minimum over S2 and over S3 is not the undisturbed backup on most live states (a
    minimum over points that differ is below the one point of S1 unless that point is the smallest: measured minimum over
    the 21 cases with live states 0.833 (act1-4d, S2 and S3 alike), 0.97 and more elsewhere)."""
    live = ~c["term"]
    if cid in E.ALL_TERMINAL:
        assert not live.any()
        return
    assert live.any()
    for which in ("S2", "S3"):
        seen = np.zeros(c["n"], bool)
        for a, b in _edge_ranges(c["n"], which):
            seen[a:b] = True
        assert (seen & live).sum() >= min(live.sum(), 256)
        for j in (1, 2):
            share = float(RC.differs(twins[which][j][seen & live], twins["S1"][j][seen & live]).mean())
            assert share >= 0.5, f"{cid} {which}: only {share:.4f} of the live states change"


@pytest.mark.parametrize("cid", list(EDGE_BY_ID))
def test_degenerate_grids_and_staging_thresholds(cid, cuda_device):
    """Every row of helpers.EDGE_CASES with its own action table: S1, S2, S3 (K = 64) installed one after the other on ONE
    handle, the three kinds on the whole grid and on one unaligned sub-range (S3 on the five grids of 4 096 states and more:
    on three windows, `_edge`).  The two all-terminal grids copy through with
    residual 0 and changed 0."""
    assert len(EDGE_BY_ID) == 23
    name, shape, _ = EDGE_BY_ID[cid]
    c, twins = _edge(cid)
    n = c["n"]
    floats = {"tab2048": 2048, "tab2049": 2049, "tab15360": 15360}
    if cid in floats:
        assert H.table_floats(name, shape, c["acts"]) == floats[cid] and twins["S3"][0].K == 64
    _assert_edge_case_not_vacuous(cid, c, twins)
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    for which in E.EDGE_SETS:
        _install(eng, twins[which][0])
        _all_kinds(dv, c, twins[which], f"{cid} {which}", _edge_ranges(n, which))
        if cid in E.ALL_TERMINAL:
            for kind in KINDS:
                Va, Vb, pol, delta, changed = dv.sweep(kind, 0, n)
                assert delta in (None, f32(0.0)) and changed in (None, 0) and np.array_equal(pol, c["pol"])
                if kind != "improve":
                    H.assert_bits_equal(Vb, c["V"], f"{cid} {which} {kind}: terminal values copied")
    eng.close()


# ---- b. every chunk boundary of a range --------------------------------------------------------------------------------
def _workgroups(count):
    """Workgroups of a launch over `count` states as the design has them (the slab schedule: chunks of 256
    states, one per workgroup, dealt to the 8 XCDs in equal runs): a multiple of 8, at least 8."""
    chunks = -(-count // 256)
    return max(-(-chunks // 8) * 8, 8)


def _assert_boundaries_occur(size, n, term, ranges):
    """Each boundary condition of section b really occurs among the ranges of this grid."""
    chunks = {-(-(b - a) // 256) for a, b in ranges}
    assert any(_workgroups(b - a) > -(-(b - a) // 256) for a, b in ranges), "no workgroup without a chunk"
    assert any((b - a) % 256 == 1 for a, b in ranges), "no one-state tail"
    assert any(a % 256 and (b - a) > 256 for a, b in ranges), "no unaligned s_begin over more than one chunk"
    assert any(b < n and a > 0 for a, b in ranges), "no range with states on both sides"
    if n >= 2049:
        assert {7, 8, 9} <= chunks
        assert any(_workgroups(b - a) == 8 and -(-(b - a) // 256) == 7 for a, b in ranges), "7 chunks on 8 workgroups"
        assert any(_workgroups(b - a) == 16 and -(-(b - a) // 256) == 9 for a, b in ranges), "9 chunks: span = 2"
    if term.any():
        tails = [(a, b) for a, b in ranges if (b - a) % 256 and term[b - 1]]
        assert tails, "no tail ends on a terminal state"
        assert any(not term[a:b].all() for a, b in tails), "such a tail has no live state in front of it"
    else:
        assert size == "2d"


@pytest.mark.parametrize("size", list(SMALL))
def test_every_chunk_boundary_of_a_range(size, cuda_device):
    """S2; the value sweep, the improvement sweep and two evaluation sweeps over every range the expectation file
    enumerates (`_ranges`: counts 1 .. 2049 from begin 0, 1, 255, 256 and n - count): 7 chunks on 8 workgroups, exactly 8,
    9, one-state tails, tails whose last valid state is terminal, unaligned s_begin.  The second evaluation sweep reads the
    first one's output with the sentinel around it: its twin is noise.expected_eval(risk="worst") over the range."""
    c = _case(SMALL[size])
    n, term = c["n"], c["term"]
    d = _make_set("S2", c["D"], c["cell"], c["acts"])
    twin = _twin_once((size, "S2"), c, d)
    ranges = E._ranges(n)
    _assert_boundaries_occur(size, n, term, ranges)
    eng = _engine(c, cuda_device)
    _install(eng, d)
    dv = _Sweeps(eng, c, cuda_device)
    targs = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    for a, b in ranges:
        what = f"{size} [{a}, {b})"
        for kind in ("value", "improve"):
            got = dv.sweep(kind, a, b)
            H.assert_bits_equal(got[0], c["V"], f"{what} {kind}: the source buffer")
            _check(got, _expected(c, twin, kind, a, b), kind, what)
        e_Vb = _expected(c, twin, "eval", a, b)[0]
        e_Va, e_delta = noise.expected_eval(c["chk"].step, c["states"], c["pol"], e_Vb, *targs, s_begin=a, s_end=b,
                                            out=np.array(c["V"]), risk="worst")
        Va, Vb, pol, delta, _ = dv.sweep("eval", a, b, n_sweeps=2)
        H.assert_bits_equal(Vb, e_Vb, f"{what}: first of two evaluation sweeps")
        H.assert_bits_equal(Va, e_Va, f"{what}: second of two evaluation sweeps")
        assert delta == f32(e_delta) and np.array_equal(pol, c["pol"])
    eng.close()


# ---- c. every build form of the unit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form,grid", [(f, g) for f, spec in FORMS.items() for g in spec[3]])
def test_build_forms_of_the_unit(form, grid, cuda_device, monkeypatch):
    """Every entry of FORMS on its grids: S2 and S3, the three kinds, whole grid and a sub-range; the handle says from
    Info / its source that it has the form, before and after.  The checked form gives the same bits and a clean report."""
    env, options, has_form, _ = FORMS[form]
    for k in E.FORM_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device, options=options)
    has_form(eng, c)
    dv = _Sweeps(eng, c, cuda_device)
    for which in ("S2", "S3"):
        twin = _twin(grid, which)
        _install(eng, twin[0])
        _all_kinds(dv, c, twin, f"{form} {grid} {which}", ((0, n), _sub(n)))
    has_form(eng, c)
    if form == "checked":
        assert eng.debug_report() == {"violations": 0, "kind": 0, "where": 0, "value": 0}
    if form == "pair-table":
        assert eng.info(Info.PAIR_TABLE) == 0
    eng.close()


@pytest.mark.parametrize("D", [2, 4])
def test_mixed_division_grids_with_the_linear_plugin(D, cuda_device, monkeypatch):
    """The mixed form of pi_locate under the robust point loop, on the grids and the linear plugin of the expectation
    file's test (which asserts the share of disturbed successors inside the grid for these very sets: it does not depend
    on the fold).  From the twin: V decides the action, and the minimum is not the first point's q."""
    from tests.test_gpu_division_paths import MIXED_VERDICT
    for k in E.FORM_KNOBS:
        monkeypatch.delenv(k, raising=False)
    c = E._mixed(D)[0]
    n = c["n"]
    twins = {w: _twin_once((f"mixed-{D}", w), c, _make_set(w, D, c["cell"], c["acts"])) for w in ("S2", "S3")}
    first = _twin_once((f"mixed-{D}", "S1"), c, Disturbances.none(D))
    for which, twin in twins.items():
        assert len(np.unique(twin[3])) > 1
        assert RC.differs(twin[1], first[1]).mean() > 0.5, f"mixed {D}-D {which}"
    eng = _engine(c, cuda_device)
    assert [eng.info(Info.RECIPROCAL_DIV + k) for k in range(D)] == MIXED_VERDICT[D]
    dv = _Sweeps(eng, c, cuda_device)
    for which, twin in twins.items():
        _install(eng, twin[0])
        _all_kinds(dv, c, twin, f"mixed {D}-D {which}", ((0, n), _sub(n)))
    eng.close()


# ---- d1. non-finite values and signed zeros -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SMALL))
def test_non_finite_values(size, cuda_device):
    """V with NaN, +-inf and +-3e38 at scattered nodes (`_poisoned` of the expectation file): inf - inf and 0 * inf inside
    reward + gamma * e, a NaN q taken by the fold and replaced only by another NaN, -inf the minimum wherever a point
    reaches it.  Sets S2, S3 and the point of weight exactly 0 whose successor value is non-finite at a share of the states.
    From the twin: the evaluation V' under S2 is mixed on the live states (at least 5 % NaN, 5 % infinite, 30 % finite),
    fminf would give other bits under S2 and S3 (it drops the NaN), and a participating weight-0 row other bits under the
    third set."""
    c = E._poisoned(size)
    n, live = c["n"], ~c["term"]
    sets = {"S2": _make_set("S2", c["D"], c["cell"], c["acts"]), "S3": _make_set("S3", c["D"], c["cell"], c["acts"]),
            "zero-weight": E._zero_weight_set(c)}
    twins = {w: _twin_once((size, "poisoned", w), c, d) for w, d in sets.items()}
    v = twins["S2"][1][live]
    mix = (float(np.isnan(v).mean()), float(np.isinf(v).mean()), float(np.isfinite(v).mean()))
    print(f"[robust edges] {size} non-finite mix of the evaluation twin under S2 (NaN, infinite, finite): "
          + " ".join(f"{x:.4f}" for x in mix))
    assert mix[0] >= 0.05 and mix[1] >= 0.05 and mix[2] >= 0.30, mix
    for which, wrong in (("S2", ("fmin",)), ("S3", ("fmin",)), ("zero-weight", ("zero-weight-rows-participate",))):
        print(f"[robust edges] {size} {which}: live states a wrong fold changes:",
              _assert_separates(c, sets[which], twins[which], wrong, f"{size} non-finite {which}"))
    assert any((np.isnan(t[2][live]) | (t[2][live] == f32(-1.0e30))).any() for t in twins.values())
    assert any(np.isinf(_residual(t[j], c["V"])) for t in twins.values() for j in (1, 2))
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    for which, twin in twins.items():
        _install(eng, twin[0])
        _all_kinds(dv, c, twin, f"{size} non-finite {which}", ((0, n), _sub(n)), check=_check_nan, same=_same_or_both_nan)
    eng.close()


@lru_cache(maxsize=None)
def _half_nan(size):
    """The case with NaN at every node of the lower planes of dimension 0 (12 of 25, 4 of 9, 2 of 5), finite elsewhere."""
    c = _case(SMALL[size])
    first = np.unravel_index(np.arange(c["n"]), c["shape"])[0]
    V = np.array(c["V"])
    V[first < c["shape"][0] // 2] = np.nan
    V.setflags(write=False)
    return {**c, "V": V}


@pytest.mark.parametrize("size", list(SMALL))
def test_every_q_of_a_state_nan(size, cuda_device):
    """Half of V is NaN: deep inside that half every point of every action interpolates a NaN, so every Q of the state is
    NaN, no action wins and the sweeps leave best_q = -1.0e30f and policy 0 — the improvement sweep included, whose
    changed count counts such a state where its entry was not 0.  At the border of the halves some points are NaN and
    some are not: the fold takes the NaN (fminf would not).  From the twin: states of all three sorts exist."""
    c = _half_nan(size)
    n, live = c["n"], ~c["term"]
    sets = {"S2": _make_set("S2", c["D"], c["cell"], c["acts"]), "zero-weight": E._zero_weight_set(c)}
    twins = {w: _twin_once((size, "half-nan", w), c, d) for w, d in sets.items()}
    for which, twin in twins.items():
        nothing = live & (twin[2] == f32(-1.0e30))
        assert nothing.any() and (twin[3][nothing] == 0).all(), f"{size} {which}: no state whose every Q is NaN"
        assert (c["pol"][nothing] != 0).any(), f"{size} {which}: the changed count does not see such a state"
        assert (live & np.isfinite(twin[2]) & (twin[2] != f32(-1.0e30))).any() and np.isnan(twin[1][live]).any()
    _assert_separates(c, sets["S2"], twins["S2"], ("fmin",), f"{size} half-NaN S2")
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    for which, twin in twins.items():
        _install(eng, twin[0])
        _all_kinds(dv, c, twin, f"{size} half-NaN {which}", ((0, n), _sub(n)), check=_check_nan, same=_same_or_both_nan)
    eng.close()


ZERO_SHAPE, ZERO_SPANS, ZERO_GAMMA = (24, 17), (2.4, 1.6), 0.25
ZERO_ACTIONS = np.array([-1.0, 0.0, 1.0], f32)
# x0 moves by a quarter of a cell per unit of action, x1 stays; the reward is -0.0f, so that q = -0 + gamma * e keeps the
# sign of a zero gamma * e (+0 + -0 would be +0); never terminates
ZERO_PLUGIN = ("__device__ void step_dynamics(float x0, float x1, float action, float* n_x0, float* n_x1, float* reward, "
               "bool* terminated) {\n    *n_x0 = x0 + 0.025f * action;\n    *n_x1 = x1;\n    *reward = -0.0f;\n"
               "    *terminated = false;\n}\n")
TINY = f32(-2.0 ** -149)                     # the negative float32 next to zero


@lru_cache(maxsize=None)
def _zeros_case():
    """V is -2^-149 on columns 0 .. 5 and 12 .. 17 of dimension 0 and +0.0 on columns 6 .. 11 and 18 .. 23, gamma 0.25.
    A V of -0.0 nodes cannot make a q of -0: the interpolation's fmaf chain starts from +0, and w * -0 + +0 is +0.  With
    -2^-149 at all four corners of a cell the chain gives e = -0 or -2^-149 (each product is rounded to a multiple of
    2^-149 with its sign kept), gamma * e = 0.25 * e underflows to -0 either way, and q = -0 + -0 = -0; where the corners
    are +0, q = -0 + +0 = +0."""
    from tests.test_gpu_division_paths import centred_bins
    c = _case(("signed-zeros", ZERO_SHAPE), actions=ZERO_ACTIONS, chk=oracle.build(2, ZERO_PLUGIN), plugin=ZERO_PLUGIN,
              bins=centred_bins(ZERO_SPANS, ZERO_SHAPE), gamma=ZERO_GAMMA)
    col = np.unravel_index(np.arange(c["n"]), c["shape"])[0]
    V = np.where((col // 6) % 2 == 0, TINY, f32(0.0)).astype(f32)
    assert (V[V != 0] == TINY).all() and (V != 0).sum() == c["n"] // 2
    V.setflags(write=False)
    return {**c, "V": V}


def test_signed_zeros(cuda_device):
    """A plugin with reward -0.0f and a V whose bands, six columns wide, make q = -0 and q = +0 (`_zeros_case`); the set is
    a weight-0 row six cells up dimension 0, the undisturbed point, and the first row again with weight 1/2.  A state inside a -0 band folds
    (-0, +0): the strict rule keeps -0, `<=` takes +0, a participating first row starts from +0 and keeps it.  A state
    inside a +0 band folds (+0, -0): the strict rule keeps +0, fminf and `<=` take -0.  From the twin: both orders occur,
    and each of the three wrong folds gives other bits."""
    c = _zeros_case()
    n = c["n"]
    dx = np.zeros((3, 2), f32)
    dx[0, 0] = dx[2, 0] = f32(6.0 * c["cell"][0])
    d = Disturbances(None, dx, [0.0, 0.5, 0.5])
    twin = _twin_once(("signed-zeros", "0-a-b"), c, d)
    q, live = _policy_q(c, d)
    assert len(live) == n and (q == 0).all()
    neg = np.signbit(q)
    assert (neg[1] & ~neg[2]).sum() > n // 8 and (~neg[1] & neg[2]).sum() > n // 8, "both orders of (+0, -0)"
    counts = _assert_separates(c, d, twin, RC.FOLDS[1:], "signed zeros")
    print(f"[robust edges] signed zeros: states a wrong fold changes, of {n}: {counts}")
    assert np.signbit(twin[1]).any() and (~np.signbit(twin[1])).any() and (twin[1] == 0).all()
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    _install(eng, d)
    _all_kinds(dv, c, twin, "signed zeros", ((0, n), _sub(n)))
    eng.close()


# ---- d2. sets at their edges --------------------------------------------------------------------------------------------
ZERO_WEIGHT_SETS = ("last-row-only", "a-zero-a", "negative-zero-and-denormal-weights")


@pytest.mark.parametrize("size", list(SMALL))
def test_sets_with_edge_entries(size, cuda_device):
    """The sets of the expectation file's section d (-0.0 offsets, a + da on a_max / a_min and one ulp to either side, a
    swallowed da, A, B, A, one point, K = 64 dense) and the fold's own (tests/robust_cases.fold_sets): K = 64 with only
    row 63 taking part = that row alone; A, 0-weight B, A = A, A; A, B, A with three steps; weights -0.0 and 1e-40; two
    bit-identical rows — then all of them on a handle with a single action.  Partner sets are compared twin against twin
    on the host and both run on the device against the one twin."""
    for actions in (None, E.ONE_ACTION[size]):
        c = _case(SMALL[size], actions=None if actions is None else np.array(actions, f32))
        n, live = c["n"], ~c["term"]
        sets = {**E._edge_sets(c), **RC.fold_sets(c["acts"], c["cell"], c["D"])}
        assert ("action-bounds" in sets) == (actions is None)
        tag = (size, "one-action" if actions else "actions")
        base = _twin_once((*tag, "none"), c, Disturbances.none(c["D"]))
        eng = _engine(c, cuda_device)
        dv = _Sweeps(eng, c, cuda_device)
        for which, entry in sets.items():
            group = entry if isinstance(entry, tuple) else (entry,)
            d = group[0]
            twin = _twin_once((*tag, which), c, d)
            for other in group[1:]:
                t = _twin_of(c, other)
                for x, y in zip(twin[1:], t[1:]):
                    assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{size} {which}: the partner set's twin"
            if which in ("negative-zeros", "tiny-da"):       # two points with the undisturbed q: its bits exactly
                H.assert_bits_equal(twin[1], base[1], f"{size} {which}: the twin against the undisturbed backup")
                H.assert_bits_equal(twin[2], base[2], f"{size} {which}: the twin's value sweep likewise")
            else:
                assert RC.differs(twin[1][live], base[1][live]).mean() > 0.5, f"{size} {which} changes too little"
            if which in ZERO_WEIGHT_SETS:
                _assert_separates(c, d, twin, ("zero-weight-rows-participate",), f"{size} {tag[1]} {which}")
            if which == "a-b-a" and actions is None:
                # the third row keeping the SECOND row's step (da compared with the row two back) would show
                shared = Disturbances(d.action_offsets[[0, 1, 1]], d.state_offsets, d.weights)
                wrong, _ = noise.expected_eval(c["chk"].step, c["states"], c["pol"], c["V"], c["term"], shared, c["acts"],
                                               *c["grid"], c["gamma"], risk="worst")
                assert RC.differs(wrong[live], twin[1][live]).any(), f"{size} a-b-a: sharing a step would not show"
            for dd in group:
                _install(eng, dd)
                _all_kinds(dv, c, twin, f"{size} actions={actions} {which} K={dd.K}", ((0, n), _sub(n)))
        eng.close()


# What a set of d2 can tell apart, by its rows: "last-row-only" folds ONE point (no rule but the weight-0 one applies);
# the two outer rows of "identical-rows" are equal, so the last of equals IS the first; only a set with a weight-0 row
# can show that such a row took part.
D2_ON_OTHER_VALUES = ("a-b-a", "action-bounds", "k64-dense", "last-row-only", "a-zero-a",
                      "negative-zero-and-denormal-weights", "identical-rows")
D2_SEPARATES = {
    "non-finite": lambda w: (("fmin",) if w != "last-row-only" else ()) + (("zero-weight-rows-participate",) if w in ZERO_WEIGHT_SETS else ()),
    "signed-zeros": lambda w: () if w == "last-row-only" else ("fmin",) if w == "identical-rows" else ("fmin", "last-of-equals"),
}


@pytest.mark.parametrize("values", list(D2_SEPARATES))
def test_sets_with_edge_entries_on_non_finite_and_signed_zero_values(values, cuda_device):
    """The sets of d2 once more where the folds differ: on the 2-D grid with NaN, +-inf and +-3e38 nodes (a NaN matches a
    NaN) and on the signed-zero grid (bit for bit).  From the twin, per set: fminf gives other bits on both, `<=` on the
    signed zeros, a participating weight-0 row on the non-finite V — every rule the set's rows can show (D2_SEPARATES)."""
    c = E._poisoned("2d") if values == "non-finite" else _zeros_case()
    n = c["n"]
    every = {**E._edge_sets(c), **RC.fold_sets(c["acts"], c["cell"], c["D"])}
    eng = _engine(c, cuda_device)
    dv = _Sweeps(eng, c, cuda_device)
    loose = dict(check=_check_nan, same=_same_or_both_nan) if values == "non-finite" else {}
    for which in D2_ON_OTHER_VALUES:
        d = every[which][0] if isinstance(every[which], tuple) else every[which]
        twin = _twin_once((values, "d2", which), c, d)
        counts = _assert_separates(c, d, twin, D2_SEPARATES[values](which), f"{values} {which}")
        print(f"[robust edges] {values} {which}: live states a wrong fold changes: {counts}")
        _install(eng, d)
        _all_kinds(dv, c, twin, f"{values} {which}", ((0, n), _sub(n)), **loose)
    eng.close()


# ---- e. large handles --------------------------------------------------------------------------------------------------
def test_large_default_handle_64_4(cuda_device):
    """double_pendulum_swingup 64^4 with pi_robust_eval_sweeps and pi_robust_value_sweep over the whole grid (65 536
    workgroups): the expectation file's test with the worst-case fold, the twin evaluated at its sample states only."""
    E.test_large_default_handle_64_4(cuda_device, fold="robust", sample_shift=2)


def test_large_handle_with_v_byte_offsets_beyond_2_pow_31(cuda_device):
    """(160, 161, 159, 162): the three robust kinds on the three windows of the expectation file's test, chunk bases and
    V byte offsets beyond 2^31; the twin at the sample states of each window."""
    E.test_large_handle_with_v_byte_offsets_beyond_2_pow_31(cuda_device, fold="robust", sample_shift=2)
