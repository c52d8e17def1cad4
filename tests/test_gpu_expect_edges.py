"""
GPU: the expectation sweeps (csrc/pi_expect_kernels.hip) where the deterministic sweeps have their edge coverage: degenerate
grids and the staging thresholds, every chunk boundary of a range, every build form of the unit they are appended to,
non-finite values, disturbance sets with edge entries, and the large handles.  tests/test_gpu_expect.py has the nine
friendly grids; its helpers (`_case`, `_twin_of`, `_Device`, `_expected`, `_check`, `_make_set`) are the ones used here.

Bar everywhere: V' and policy bit for bit against the numpy twins of dynamicprogramming_amd/noise.py (a NaN matches a NaN
where the values are not finite, section d), residual and changed count exactly, states outside a launched range keep
their sentinel, the source buffer is untouched.  Every GPU step runs once.  What a sub-range launch leaves behind follows
from ONE whole-grid twin per (case, set): every state's backup is independent of the others.  The conditions that make a
comparison worth something (a set moves the values, the non-finite mix, successors inside the mixed grids) are asserted
from the twin arrays alone, never from GPU output.

What would have to be wrong in the kernel for a section to fail — written from the code; nothing below was observed
failing, every item is JUDGED, NOT RUN (no kernel was broken on purpose):

0. checked handle (test_checked_handle_reports_...).  Not the kernel: pi_debug_report read the tally of the sweeps' module
   only, and the expectation module has its own copy of pi_debug_words.  Before the fix the three corrupt entries were
   contained (V' was right) and reported as 0 violations.
a. degenerate grids / staging (test_degenerate_grids_...).  pi_stage_table<256> staging the table for another block size
   than the launch's 256 threads (the unit's PI_BLOCK_EVAL): entries of the table beyond 256 * kPer missing at 2049 and
   15 360 floats; lds_noise overlapping lds_tab when both are at their largest (15 360 + 64 * 4 floats: 62 464 bytes);
   pi_state_coords on a dimension of 2 bins; a single chunk of 4 or 63 states where lane = min(tid, count - 1) shadows from
   lane 4 on; PI_NA = 1 (the action loop runs once, a_min == a_max) and 257 actions with exact ties (strict '>' keeps
   the lowest index); an all-terminal grid has to copy V and leave residual and changed count at 0 although every lane
   skips the backup.
b. chunk boundaries (test_every_chunk_boundary_...).  pi_expect_chunk: `min(s_end - sb, 256) - 1` off by one (the last
   state of a tail chunk not stored, or a shadow lane storing past s_end); a workgroup without a chunk (7 chunks on 8
   workgroups) going on to the barrier or to pi_wave_max_to; span = gridDim.x / 8 = 2 at nine chunks dealing chunk 8 to
   the wrong workgroup; shadow lanes of a tail adding to the changed count or the residual (`live` / threadIdx.x == lane);
   a tail whose last valid state is terminal making its shadows skip the point loop (the readfirstlane of a row word is
   then taken from another lane: same word); s_begin not a multiple of 256 (chunk base addresses are unaligned).
c. build forms (test_build_forms_..., test_mixed_division_grids_...).  PI_BLOCK_EVAL / PI_BLOCK_IMPROVE of 320, 448, 1024,
   512 leaking into the expectation kernels (launch bounds, the slot index of pi_wave_max_to, pi_stage_table's stride);
   pi_locate's IEEE form and its mixed form (the `else` arm inside the fast branch) under the point loop; the checked
   pi_locate / pi_checked_action changing a clean result; a unit built with PI_PAIR_TABLE 1 making pi_request_corners
   read the pair table (the expectation sweeps never pack one); chunks per workgroup of 3 being honoured by the host's
   launch geometry (the kernels take exactly one chunk: two thirds of the range would stay unswept).
d. values and sets at their edges (test_non_finite_values_..., test_sets_with_edge_entries_...).  `Q = -0.0f` and fmaf
   in place of multiply-then-fmaf differing for 0 * inf and inf - inf; `dlt > dmax` replaced by fmaxf (same) or by a
   comparison that lets a NaN through; best_q = -1.0e30f / best = 0 when every Q is NaN; `da == 0.0f` and `dx != 0.0f`
   treating -0.0 as non-zero (a clamp that rounds, an add that turns -0 + s' into something else: it cannot, but a
   `signbit` test would); the clamp at a_max / a_min one ulp inside and beyond; `da != da_prev` comparing with the row
   two back (A, B, A would share a step); the `held` corner cache not invalidated when K = 64 points all leave the cell;
   a_min == a_max.
e. large handles (test_large_...).  Only the launch differs: 65 536 and more workgroups (gridDim.x beyond 2^16 at n =
   2^24), `(unsigned int)sb + lane` and the 32-bit byte offsets of pi_request_corners at 4 * base >= 2^31, chunk bases
   sb * 4 beyond 2^31 in pi_load_state / pi_store_lane (64-bit pointer + 32-bit lane offset), a unit whose own sweeps
   run 1024 / 512 threads and the pair table, neither of which the expectation launch may pick up.

Measured on an MI355X (this module alone, `pytest -m gpu --durations=0`, code objects already in the cache): 55 tests in
29 s.  Slowest calls: one2-4d-strided 3.1 s, the 2^29 grid 3.0 s, 64^4 3.7 s, tab15360 3.2 s, one2-4d 2.3 s, act257 1.9 s
(each mostly its twins on the host), everything else 1.1 s or less.  Without the cache every handle here compiles its
unit and its expectation module first: 2 to 5 s per handle, 130 s for all of them on one CPU core.
"""
from __future__ import annotations

import time
from functools import lru_cache

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs, noise
from dynamicprogramming_amd._native import Info, Option
from dynamicprogramming_amd.noise import Disturbances
from tests import helpers as H
from tests.test_gpu_expect import SENTINEL, _Device, _case, _check, _engine, _expected, _make_set, _residual, _twin, _twin_of

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = ("eval", "improve", "value")
SMALL = {"2d": ("pendulum", (25, 41)), "4d": ("cartpole_swingup", (9, 7, 11, 5)), "6d": ("double_cartpole", (5, 4, 6, 4, 5, 4))}
FORM_GRIDS = ("ragged-2d", "ragged-4d", "ragged-6d")        # of tests/test_gpu_expect.py: their twins are shared with it


def _sub(n):
    return (37, n - 53) if n > 128 else (1, n - 1)


def _install(eng, d):
    assert eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights) == d.K == eng.info(Info.DISTURBANCES)


def _same_or_both_nan(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, what
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} differ, first at {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"


def _check_nan(got, want, kind, what):
    """`_check` of tests/test_gpu_expect.py with a NaN matching a NaN of any payload."""
    Va, Vb, pol, delta, changed = got
    e_Vb, e_pol, e_delta, e_changed = want
    _same_or_both_nan(Vb, e_Vb, f"{what} {kind}: V'")
    assert np.array_equal(pol, e_pol), f"{what} {kind}: policy"
    if delta is not None:
        assert delta == e_delta, f"{what} {kind}: residual {delta} vs {e_delta}"
    if changed is not None:
        assert changed == e_changed, f"{what} {kind}: changed {changed} vs {e_changed}"


def _all_kinds(dv, c, twin, what, ranges, check=_check, same=H.assert_bits_equal):
    for kind in KINDS:
        for a, b in ranges:
            got = dv.sweep(kind, a, b)
            same(got[0], c["V"], f"{what} {kind} [{a}, {b}): the source buffer")
            check(got, _expected(c, twin, kind, a, b), kind, f"{what} [{a}, {b})")


FOLD_NAMES = {"expect": "expectation", "robust": "worst-case"}


def _fold(fold):
    """(device class, whole-grid twin of (grid, set), risk of the twins) of the expectation sweeps ("expect") or of the
    worst-case sweeps ("robust": tests/test_gpu_robust_edges.py runs section 0 and section e of this file with it)."""
    if fold == "expect":
        return _Device, _twin, "expected"
    from tests import test_gpu_robust as R
    assert fold == "robust"
    return R._Sweeps, R._twin, "worst"


# ---- 0. the checked handle's report ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", FORM_GRIDS)
def test_checked_handle_reports_what_the_expectation_sweeps_met(grid, cuda_device, monkeypatch, fold="expect"):
    """PI_MI355_DEBUG=1 with a set installed: clean expectation sweeps of the three kinds report nothing and give the
    unchecked handle's bits; three corrupt policy entries (one past the end, -1, 2^30) met by expect_eval_sweeps are
    reported — 3 violations, kind 1, `where` one of the three states — and contained: V' is that of the policy with 0 at
    those states; a second report is clean; the deterministic sweep with the same array still reports its own 3, and both
    together 6.  The handle's push module is loaded as well (Option.BUILD_PUSH), so the report walks all three modules;
    no kernel of the push module runs on one device: that third of the report is covered for a clean tally only."""
    monkeypatch.delenv("PI_MI355_DEBUG", raising=False)
    Device, twin_of, risk = _fold(fold)
    c = _case(grid)
    n = c["n"]
    twin = twin_of(grid, "S2")
    d = twin[0]
    plain = _engine(c, cuda_device)
    assert plain.info(Info.DEBUG_CHECKS) == 0
    _install(plain, d)
    dv = Device(plain, c, cuda_device)
    want = {kind: dv.sweep(kind, 0, n) for kind in KINDS}
    plain.close()
    monkeypatch.setenv("PI_MI355_DEBUG", "1")
    chk = _engine(c, cuda_device)
    assert chk.info(Info.DEBUG_CHECKS) == 1 and "#define PI_DEBUG_BOUNDS 1" in chk.kernel_source(c["src"])
    _install(chk, d)
    chk.set_option(Option.BUILD_PUSH, 1)
    dv = Device(chk, c, cuda_device)
    clean = {"violations": 0, "kind": 0, "where": 0, "value": 0}
    for kind in KINDS:
        got = dv.sweep(kind, 0, n)
        _check(got, _expected(c, twin, kind, 0, n), kind, f"{grid} checked")
        for x, y in zip(got, want[kind]):
            assert x is y is None or np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8))
    assert chk.debug_report() == clean
    # bad indices go to the checked handle only, at live states (a terminal state's entry is never looked at)
    live = np.flatnonzero(~c["term"])
    where = [int(live[5]), int(live[len(live) // 2]), int(live[-3])]
    values = (len(c["acts"]), -1, 1 << 30)
    bad = c["pol"].copy()
    bad[where] = values
    fixed = c["pol"].copy()
    fixed[where] = 0                                        # what the checked kernel substitutes
    e_Vb = np.array(twin[1])
    e_Vb[where] = noise.expected_q(c["chk"].step, c["states"][where], c["acts"][0], d, c["V"], c["acts"], *c["grid"], c["gamma"],
                                   risk=risk)
    got = dv.sweep("eval", 0, n, pol=bad)
    rep = chk.debug_report()
    assert rep["violations"] == 3 and rep["kind"] == 1 and rep["where"] in where, rep
    assert rep["value"] == values[where.index(rep["where"])] & 0xffffffff
    H.assert_bits_equal(got[1], e_Vb, f"{grid}: V' with action 0 substituted at the three states")
    assert got[3] == _residual(e_Vb, c["V"]) and np.array_equal(got[2], bad)
    assert chk.debug_report() == clean                      # cleared by the report before
    # the deterministic sweep of the same handle (pi_eval_sweep, as tests/test_gpu_endtoend.py runs it) still reports its own
    d_V, d_bad = dv.put(c["V"]), dv.put(bad)
    d_Vn = dv.torch.full_like(d_V, float(SENTINEL))

    def deterministic():
        chk.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_bad.data_ptr(), dv.term.data_ptr(), 0, n, c["gamma"], 0)

    deterministic()
    rep = chk.debug_report()
    assert rep["violations"] == 3 and rep["kind"] == 1 and rep["where"] in where, rep
    e_det, _ = c["chk"].eval_sweep(c["states"], c["acts"], fixed, c["V"], c["term"], *c["grid"], c["gamma"])
    H.assert_bits_equal(dv.get(d_Vn), e_det, f"{grid}: the deterministic sweep with action 0 substituted")
    deterministic()                                         # both modules' tallies in one report: the sum
    dv.sweep("eval", 0, n, pol=bad)
    rep = chk.debug_report()
    assert rep["violations"] == 6 and rep["kind"] == 1 and rep["where"] in where, rep
    assert chk.debug_report() == clean
    chk.close()


# ---- a. degenerate grids and the thresholds of staging ------------------------------------------------------------------
EDGE_BY_ID = {cid: (name, shape, acts) for cid, name, shape, acts in H.EDGE_CASES}
ALL_TERMINAL = ("all2-4d-terminal", "all2-6d")
EDGE_SETS = ("S1", "S2", "S3")


@lru_cache(maxsize=None)
def _edge(cid):
    """Case and the whole-grid twins of S1, S2, S3 of one row of helpers.EDGE_CASES, computed once."""
    name, shape, acts = EDGE_BY_ID[cid]
    c = _case((name, tuple(shape)), actions=acts)
    return c, {w: _twin_of(c, _make_set(w, c["D"], c["cell"], c["acts"])) for w in EDGE_SETS}


def _assert_edge_case_not_vacuous(cid, c, twins):
    """From the twin arrays alone.  Measured minima over the 21 cases with live states: S2 changes V' against S1 on
    0.9896 of the live states (act1; 1.0 elsewhere), S3 on 0.833 (act1-4d), S2 moves 0.068 of the argmaxes (act2)."""
    live = ~c["term"]
    if cid in ALL_TERMINAL:
        assert not live.any()
        return
    assert live.any()
    base = twins["S1"]
    for which, least in (("S2", 0.95), ("S3", 0.8)):
        for j in (1, 2):                                     # V' of the evaluation sweep, V' of the value sweep
            share = float((twins[which][j][live].view(np.uint32) != base[j][live].view(np.uint32)).mean())
            assert share >= least, f"{cid} {which}: only {share:.4f} of the live states change"
    if len(c["acts"]) > 1:
        share = float((twins["S2"][3][live] != base[3][live]).mean())
        assert share >= 0.05, f"{cid} S2: only {share:.4f} of the argmaxes move"


@pytest.mark.parametrize("cid", list(EDGE_BY_ID))
def test_degenerate_grids_and_staging_thresholds(cid, cuda_device):
    """Every row of helpers.EDGE_CASES with its own action table: S1, S2, S3 installed one after the other on ONE handle,
    the three kinds on the whole grid and on one unaligned sub-range.  The two all-terminal grids copy through with
    residual 0 and changed 0."""
    assert len(EDGE_BY_ID) == 23
    name, shape, _ = EDGE_BY_ID[cid]
    c, twins = _edge(cid)
    n = c["n"]
    floats = {"tab2048": 2048, "tab2049": 2049, "tab15360": 15360}
    if cid in floats:
        assert H.table_floats(name, shape, c["acts"]) == floats[cid]
    _assert_edge_case_not_vacuous(cid, c, twins)
    eng = _engine(c, cuda_device)
    dv = _Device(eng, c, cuda_device)
    for which in EDGE_SETS:
        _install(eng, twins[which][0])
        _all_kinds(dv, c, twins[which], f"{cid} {which}", ((0, n), _sub(n)))
        if cid in ALL_TERMINAL:
            for kind in KINDS:
                Va, Vb, pol, delta, changed = dv.sweep(kind, 0, n)
                assert delta in (None, f32(0.0)) and changed in (None, 0) and np.array_equal(pol, c["pol"])
                if kind != "improve":
                    H.assert_bits_equal(Vb, c["V"], f"{cid} {which} {kind}: terminal values copied")
    eng.close()


# ---- b. every chunk boundary of a range --------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1792, 2047, 2048, 2049)


def _ranges(n):
    out = []
    for count in COUNTS:
        for begin in (0, 1, 255, 256, n - count):
            r = (begin, begin + count)
            if count <= n and begin >= 0 and r[1] <= n and r not in out:
                out.append(r)
    return out


@pytest.mark.parametrize("size", list(SMALL))
def test_every_chunk_boundary_of_a_range(size, cuda_device):
    """S2, the value sweep and two evaluation sweeps over [begin, begin + count) for count in COUNTS (as far as the grid
    holds them: 1 025, 3 465 and 9 600 states) from begin 0, 1, 255, 256 and n - count: 7 chunks on 8 workgroups (one leaves
    before the barrier), exactly 8, 9 (two chunks per XCD run), one-lane tails (count = 1, 65, 257, 513, 2049) and, on the
    grids with terminal states, tails whose last valid state is terminal (every range that ends at n).  The second
    evaluation sweep reads the first one's output with the sentinel around it: its twin is noise.expected_eval over the
    range."""
    c = _case(SMALL[size])
    n, term = c["n"], c["term"]
    d = _make_set("S2", c["D"], c["cell"], c["acts"])
    twin = _twin_of(c, d)
    ranges = _ranges(n)
    assert any((b - a) % 256 == 1 for a, b in ranges)
    if n >= 2049:
        assert {7, 8, 9} <= {-(-(b - a) // 256) for a, b in ranges}
    if term.any():
        assert any(term[b - 1] and (b - a) % 256 for a, b in ranges), "no tail ends on a terminal state"
    eng = _engine(c, cuda_device)
    _install(eng, d)
    dv = _Device(eng, c, cuda_device)
    targs = (c["term"], d, c["acts"], *c["grid"], c["gamma"])
    for a, b in ranges:
        what = f"{size} [{a}, {b})"
        got = dv.sweep("value", a, b)
        H.assert_bits_equal(got[0], c["V"], f"{what}: the source buffer")
        _check(got, _expected(c, twin, "value", a, b), "value", what)
        e_Vb = _expected(c, twin, "eval", a, b)[0]
        e_Va, e_delta = noise.expected_eval(c["chk"].step, c["states"], c["pol"], e_Vb, *targs, s_begin=a, s_end=b,
                                            out=np.array(c["V"]))
        Va, Vb, pol, delta, _ = dv.sweep("eval", a, b, n_sweeps=2)
        H.assert_bits_equal(Vb, e_Vb, f"{what}: first of two evaluation sweeps")
        H.assert_bits_equal(Va, e_Va, f"{what}: second of two evaluation sweeps")
        assert delta == f32(e_delta) and np.array_equal(pol, c["pol"])
    eng.close()


# ---- c. every build form of the unit -----------------------------------------------------------------------------------
def _form_ieee(eng, c):
    assert [eng.info(Info.RECIPROCAL_DIV + k) for k in range(c["D"])] == [0] * c["D"]


def _form_checked(eng, c):
    assert eng.info(Info.DEBUG_CHECKS) == 1


def _form_blocks(pair):
    def check(eng, c):
        assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == pair
        src = eng.kernel_source(c["src"])
        assert f"#define PI_BLOCK_EVAL {pair[0]}\n" in src and f"#define PI_BLOCK_IMPROVE {pair[1]}\n" in src
    return check


def _form_cpw(eng, c):
    assert (eng.info(Info.EVAL_CPW), eng.info(Info.IMPROVE_CPW)) == (3, 3)


def _form_pairs(eng, c):
    assert "#define PI_PAIR_TABLE 1\n" in eng.kernel_source(c["src"])


# form -> (environment, options before pi_compile, the assertion that the handle has the form, grids)
FORMS = {
    "ieee-div": ({"PI_MI355_IEEE_DIV": "1"}, (), _form_ieee, FORM_GRIDS),
    "checked": ({"PI_MI355_DEBUG": "1"}, (), _form_checked, FORM_GRIDS),
    "blocks-320-448": ({"PI_MI355_EVAL_BLOCK": "320", "PI_MI355_IMPROVE_BLOCK": "448"}, (), _form_blocks((320, 448)), FORM_GRIDS),
    "blocks-1024-512": ({"PI_MI355_EVAL_BLOCK": "1024", "PI_MI355_IMPROVE_BLOCK": "512"}, (), _form_blocks((1024, 512)), FORM_GRIDS),
    "cpw-3": ({}, ((Option.EVAL_CPW, 3), (Option.IMPROVE_CPW, 3)), _form_cpw, FORM_GRIDS),
    "pair-table": ({}, ((Option.PAIR_TABLE, 1),), _form_pairs, ("ragged-4d",)),      # the table is for 4-D grids only
}
FORM_KNOBS = ("PI_MI355_IEEE_DIV", "PI_MI355_DEBUG", "PI_MI355_EVAL_BLOCK", "PI_MI355_IMPROVE_BLOCK")


@pytest.mark.parametrize("form,grid", [(f, g) for f, spec in FORMS.items() for g in spec[3]])
def test_build_forms_of_the_unit(form, grid, cuda_device, monkeypatch):
    """The expectation module is build_source(h) + pi_expect_kernels.hip: every define and option that shapes the unit
    shapes it as well, while its kernels keep their 256-thread block and one chunk per workgroup.  S2 and S3, the three
    kinds, whole grid and a sub-range; the handle says from Info / its source that it has the form.  The checked form
    gives the same bits (the same twin) and a clean report; a unit with the pair table kernels still reads V itself
    (Info.PAIR_TABLE stays 0: no improvement sweep of the handle read the table)."""
    env, options, has_form, _ = FORMS[form]
    for k in FORM_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _case(grid)
    n = c["n"]
    eng = _engine(c, cuda_device, options=options)
    has_form(eng, c)
    dv = _Device(eng, c, cuda_device)
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


MIXED_INSIDE = {2: 0.879, 4: 0.544}         # share of UNDISTURBED successors strictly inside (tests/test_block_sizes_host.py)


@lru_cache(maxsize=None)
def _mixed(D):
    from tests import test_gpu_division_paths as DP
    spans = DP.MIXED_SPANS[D]
    src = DP.linear_plugin(spans)
    c = _case(("mixed-division", DP.MIXED_SHAPES[D]), actions=DP.MIXED_ACTIONS, chk=oracle.build(D, src), plugin=src,
              bins=DP.centred_bins(spans, DP.MIXED_SHAPES[D]), gamma=DP.MIXED_GAMMA)
    return c, {w: _twin_of(c, _make_set(w, D, c["cell"], c["acts"])) for w in ("S2", "S3")}


def _inside_share(c, d):
    """Share of the disturbed successors f(s, a (+) da_k) + dx_k, over every state, action and point, that lie strictly
    inside the grid in every dimension — on the CPU, from the twin's step."""
    lo, hi = c["grid"][0], c["grid"][1]
    a_min, a_max = c["acts"].min(), c["acts"].max()
    inside = []
    for a in c["acts"]:
        for k in range(d.K):
            da = d.action_offsets[k]
            ak = a if da == 0 else np.fmin(np.fmax(f32(a + da), a_min), a_max)
            nxt, _, done = c["chk"].step(c["states"], f32(ak))
            assert not done.any()
            p = (np.asarray(nxt, f32) + d.state_offsets[k]).astype(f32)
            inside.append(((p > lo) & (p < hi)).all(axis=1))
    return float(np.mean(inside))


@pytest.mark.parametrize("D", [2, 4])
def test_mixed_division_grids_with_the_linear_plugin(D, cuda_device, monkeypatch):
    """The mixed form of pi_locate (spans 5e-10 and 3e9 beside ordinary ones: tests/test_gpu_division_paths.py) under the
    point loop, the twin's step being the oracle's of the same plugin.  State offsets are in cell widths of their own
    dimension (_make_set), so the 5e-10 and the 3e9 dimensions are disturbed in proportion.  Share of disturbed successors
    strictly inside the grid, measured on the CPU: S2 0.8749 (2-D) and 0.5520 (4-D), S3 0.8054 and 0.2976 — asserted to
    be at least half of the undisturbed share of that file (0.879 / 2, 0.544 / 2)."""
    from tests.test_gpu_division_paths import MIXED_VERDICT
    for k in FORM_KNOBS:
        monkeypatch.delenv(k, raising=False)
    c, twins = _mixed(D)
    n = c["n"]
    for which, twin in twins.items():
        share = _inside_share(c, twin[0])
        print(f"[expect edges] mixed {D}-D {which}: {share:.4f} of the disturbed successors strictly inside the grid")
        assert share >= 0.5 * MIXED_INSIDE[D], f"mixed {D}-D {which}: {share:.4f}"
        assert len(np.unique(twin[3])) > 1                   # V decides the action, not the grid's border
    eng = _engine(c, cuda_device)
    assert [eng.info(Info.RECIPROCAL_DIV + k) for k in range(D)] == MIXED_VERDICT[D]
    dv = _Device(eng, c, cuda_device)
    for which, twin in twins.items():
        _install(eng, twin[0])
        _all_kinds(dv, c, twin, f"mixed {D}-D {which}", ((0, n), _sub(n)))
    eng.close()


# ---- d. values and sets at their edges ---------------------------------------------------------------------------------
# nodes holding NaN, +inf, -inf, +3e38, -3e38 (of 1 025, 3 465 and 9 600), tuned on the CPU: about one node in 100, 500 and
# 2 000 per kind, fewer NaN than infinities in 6-D, where a NaN reaches 2^6 cells and swallows the infinities beside it
POISON_NODES = {2: (10, 10, 10, 10, 10), 4: (7, 7, 7, 7, 7), 6: (3, 6, 6, 4, 4)}       # nodes per kind (NaN, +inf, -inf, +3e38, -3e38), tuned on the CPU


@lru_cache(maxsize=None)
def _poisoned(size):
    """The case with NaN, +inf, -inf and +-3e38 at scattered nodes of V (live and terminal alike), finite elsewhere."""
    c = _case(SMALL[size])
    rng = np.random.default_rng(1913)
    V = np.array(c["V"])
    counts = POISON_NODES[c["D"]]
    at = rng.choice(c["n"], size=sum(counts), replace=False)
    for v, m in zip((np.nan, np.inf, -np.inf, 3e38, -3e38), counts):
        V[at[:m]] = f32(v)
        at = at[m:]
    V.setflags(write=False)
    return {**c, "V": V}


def _zero_weight_set(c):
    """Two points: half a cell away in every dimension with a weight of exactly 0, and the undisturbed one with 1."""
    dx = np.zeros((2, c["D"]), f32)
    dx[0] = 0.5 * c["cell"]
    return Disturbances(None, dx, np.array([0.0, 1.0], f32))


@pytest.mark.parametrize("size", list(SMALL))
def test_non_finite_values(size, cuda_device):
    """V with NaN, +-inf and +-3e38 at scattered nodes: 0 * inf, inf - inf in the residual (a NaN never raises it), a
    residual of inf, best_q = -1.0e30f with index 0 where no Q wins.  The number of poisoned nodes (POISON_NODES) is
    chosen so that the evaluation twin's V' under S2 is mixed on the live states — at least 5 % NaN, 5 % infinite and 30 %
    finite, asserted here from the twin; measured NaN / infinite / finite: 2-D 0.084 / 0.134 / 0.782, 4-D
    0.123 / 0.101 / 0.776, 6-D 0.087 / 0.096 / 0.817 (under S3, whose 64 points reach three cells far, 0.38 / 0.32 / 0.31,
    0.90 / 0.06 / 0.04 and 0.96 / 0.02 / 0.02: compared all the same, not asserted).  Sets: S2, S3, and a point of weight
    exactly 0 whose successor value is infinite or NaN at a share of the states (44, 141 and 133 live states are NaN under
    it and finite without it)."""
    c = _poisoned(size)
    n, live = c["n"], ~c["term"]
    sets = {"S2": _make_set("S2", c["D"], c["cell"], c["acts"]), "S3": _make_set("S3", c["D"], c["cell"], c["acts"]),
            "zero-weight": _zero_weight_set(c)}
    twins = {w: _twin_of(c, d) for w, d in sets.items()}
    v = twins["S2"][1][live]
    mix = (float(np.isnan(v).mean()), float(np.isinf(v).mean()), float(np.isfinite(v).mean()))
    print(f"[expect edges] {size} non-finite mix of the evaluation twin under S2 (NaN, infinite, finite): "
          + " ".join(f"{x:.4f}" for x in mix))
    assert mix[0] >= 0.05 and mix[1] >= 0.05 and mix[2] >= 0.30, mix
    # the weight of 0 makes NaN where the undisturbed backup is finite; nothing wins somewhere; a residual is inf
    alone = _twin_of(c, Disturbances.none(c["D"]))
    assert (np.isnan(twins["zero-weight"][1][live]) & np.isfinite(alone[1][live])).any()
    assert any((np.isnan(t[2][live]) | (t[2][live] == f32(-1.0e30))).any() for t in twins.values())
    assert any(np.isinf(_residual(t[j], c["V"])) for t in twins.values() for j in (1, 2))
    eng = _engine(c, cuda_device)
    dv = _Device(eng, c, cuda_device)
    for which, twin in twins.items():
        _install(eng, twin[0])
        _all_kinds(dv, c, twin, f"{size} non-finite {which}", ((0, n), _sub(n)), check=_check_nan, same=_same_or_both_nan)
    eng.close()


def _landing(acts, target):
    """A float32 da != 0 with float32(a + da) == target exactly for an action a of the table, the nearest one that has
    such an offset (from -2 no float32 offset reaches the float below 2: the sum is rounded to an even neighbour)."""
    target = f32(target)
    for a in sorted((f32(a) for a in acts if a != target), key=lambda a: abs(float(a) - float(target))):
        da = f32(target - a)
        for _ in range(4):
            got = f32(a + da)
            if got == target and da != 0:
                return da
            da = np.nextafter(da, f32(np.inf) if got < target else f32(-np.inf))
    raise AssertionError(f"no float32 offset takes an action of {acts} to {target}")


def _edge_sets(c):
    """The sets of section d for the case's action table and cell widths."""
    D, cell = c["D"], c["cell"]
    a_min, a_max = c["acts"].min(), c["acts"].max()
    arange = float(a_max - a_min) or 1.0
    rng = np.random.default_rng(29)
    third = np.full(3, 1.0 / 3.0)
    sets = {}
    # -0.0 counts as zero: no clamp, no add, and the point shares the step of the +0.0 one before it
    dx = np.zeros((2, D), f32)
    dx[1] = f32(-0.0)
    sets["negative-zeros"] = Disturbances(np.array([0.0, -0.0], f32), dx, np.array([0.5, 0.5], f32))
    if a_max > a_min:
        # an action of the table lands exactly on a_max, one ulp inside, one ulp beyond (clamped back); on a_min likewise;
        # the other actions clamp or land inside under the same offsets
        ups = [_landing(c["acts"], t) for t in (a_max, np.nextafter(a_max, f32(-np.inf)), np.nextafter(a_max, f32(np.inf)))]
        downs = [_landing(c["acts"], t) for t in (a_min, np.nextafter(a_min, f32(np.inf)), np.nextafter(a_min, f32(-np.inf)))]
        sets["action-bounds"] = Disturbances(np.array(ups + downs, f32), rng.uniform(-0.4, 0.4, size=(6, D)) * cell,
                                             np.full(6, 1.0 / 6.0))
    # a + da == a for every action that is not 0 (da != 0: the clamp runs and changes nothing)
    tiny = f32(1e-30)
    assert all(f32(a + tiny) == a for a in c["acts"] if a != 0)
    sets["tiny-da"] = Disturbances(np.array([tiny, 0.0], f32), np.zeros((2, D), f32), np.array([0.5, 0.5], f32))
    # equal offsets in rows that are not adjacent: three dynamics steps
    A, B = 0.21 * arange, -0.17 * arange
    sets["a-b-a"] = Disturbances(np.array([A, B, A], f32), rng.uniform(-0.7, 0.7, size=(3, D)) * cell, third)
    sets["one-point"] = Disturbances(np.array([0.13 * arange], f32), (rng.uniform(0.2, 0.8, size=(1, D)) * cell), [1.0])
    # K = 64, every dx non-zero, offsets of up to two cells: the corner cache is refilled again and again
    dx = rng.uniform(0.05, 2.0, size=(64, D)) * rng.choice([-1.0, 1.0], size=(64, D)) * cell
    p = rng.random(64) + 0.05
    sets["k64-dense"] = Disturbances(np.repeat(rng.uniform(-0.5, 0.5, size=16) * arange, 4).astype(f32), dx.astype(f32),
                                     (p / p.sum()).astype(f32))
    assert (sets["k64-dense"].state_offsets != 0).all()
    return sets


ONE_ACTION = {"2d": [0.5], "4d": [10.0], "6d": [10.0]}


@pytest.mark.parametrize("size", list(SMALL))
def test_sets_with_edge_entries(size, cuda_device):
    """-0.0 offsets, offsets that put a + da exactly on a_max / a_min and one ulp to either side, a da that a + da
    swallows, equal offsets in non-adjacent rows, one point with p = 1, K = 64 with every dx non-zero; then the same sets
    on a handle with a single action (a_min == a_max: every non-zero da clamps back onto the action)."""
    for actions in (None, ONE_ACTION[size]):
        c = _case(SMALL[size], actions=None if actions is None else np.array(actions, f32))
        n, live = c["n"], ~c["term"]
        sets = _edge_sets(c)
        assert ("action-bounds" in sets) == (actions is None)
        base = _twin_of(c, Disturbances.none(c["D"]))
        eng = _engine(c, cuda_device)
        dv = _Device(eng, c, cuda_device)
        for which, d in sets.items():
            twin = _twin_of(c, d)
            if which in ("negative-zeros", "tiny-da"):       # 0.5 q + 0.5 q of the undisturbed backup: its bits exactly
                H.assert_bits_equal(twin[1], base[1], f"{size} {which}: the twin against the undisturbed backup")
                H.assert_bits_equal(twin[2], base[2], f"{size} {which}: the twin's value sweep likewise")
            else:                                            # measured: every live state changes, on every grid
                assert (twin[1][live] != base[1][live]).mean() > 0.95, f"{size} {which} changes too little"
            _install(eng, d)
            _all_kinds(dv, c, twin, f"{size} actions={actions} {which}", ((0, n), _sub(n)))
        eng.close()


# ---- e. large handles --------------------------------------------------------------------------------------------------
def _large_twin(g, d, coords, pol_at, V_user, risk="expected"):
    """The twin at sample points (node coordinates): evaluation under the policy's action; argmax and maximum."""
    grid = g.meta
    V_eval = noise.expected_q(g.chk.step, coords, g.acts[pol_at], d, V_user, g.acts, *grid, g.gamma, risk=risk)
    if risk == "worst":                                      # the argmax of the worst-case sweeps' twins
        best, best_q = noise._argmax(g.chk.step, coords, np.arange(len(coords)), d, V_user, g.acts, grid, g.gamma, risk)
    else:
        best, _, best_q = noise.expected_greedy_action(g.chk.step, coords, d, V_user, g.acts, *grid, g.gamma)
    return V_eval, best, best_q


def _large_set(g):
    lo, hi, gshape, _ = g.meta
    cell = (hi.astype(np.float64) - lo.astype(np.float64)) / (np.asarray(gshape, np.float64) - 1)
    return _make_set("S2", g.D, cell, g.acts)


def test_large_default_handle_64_4(cuda_device, fold="expect", sample_shift=0):
    """double_pendulum_swingup 64^4 (2^24 states): the unit's own sweeps run 1024 / 512 threads and the pair table by
    default (the strip schedule is the library's choice for 6-D grids of this size only: Info.STRIP_STATES is 0 here, and
    is asserted to be); the expectation kernels keep 256 threads, one chunk, the slab schedule and V itself.  S2,
    whole-grid evaluation and value sweep: bit for bit against the twin at 2^16 scattered states and the last 2^12;
    residual and changed count against torch reductions over the device arrays.
    Measured on an MI355X: 3.4 s (3.7 s as pytest counts the call), most of it the twin at the about 69 500 samples on the host;
    peak device memory as torch counts it 0.4 GiB."""
    from tests.test_gpu_addr64 import _free, _grid, _points, _report_peak, _seeded_state, _torch
    torch = _torch()
    risk = _fold(fold)[2]
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    name = "double_pendulum_swingup"
    g = _grid(name, (64, 64, 64, 64), None, cuda_device, form64=False)
    try:
        n, eng = g.n, g.eng
        assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == (1024, 512)
        assert "#define PI_PAIR_TABLE 1\n" in eng.kernel_source(envs.dynamics_source(name))
        assert eng.info(Info.STRIP_STATES) == 0                 # resolve_strip: the library's choice for 4-D grids is the slab schedule
        d = _large_set(g)
        _install(eng, d)
        Vh, polh, _, d_V, d_pol, _ = _seeded_state(g, 23, None, cuda_device, scale=30.0)
        idx = np.unique(np.concatenate([np.random.default_rng(2023).integers(0, n, size=(1 << 16) >> sample_shift, dtype=np.int64),
                                        np.arange(n - (1 << 12), n, dtype=np.int64)]))
        flat_user, coords = _points(g, idx)
        e_eval, e_best, e_best_q = _large_twin(g, d, coords, polh[flat_user], Vh, risk)
        d_idx = torch.from_numpy(idx).to(cuda_device)
        d_Vn = torch.full((n,), float("nan"), dtype=torch.float32, device=cuda_device)
        d_delta = torch.full((1,), 123.0, dtype=torch.float32, device=cuda_device)
        d_changed = torch.full((1,), 77, dtype=torch.int32, device=cuda_device)
        getattr(eng, f"{fold}_eval_sweeps")(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), 0, 0, n, g.gamma, 1, d_delta.data_ptr())
        torch.cuda.synchronize()
        assert not bool(torch.isnan(d_Vn).any())
        H.assert_bits_equal(d_Vn[d_idx].cpu().numpy(), e_eval, f"64^4 evaluation at {len(idx)} states")
        assert float(d_delta.item()) == float((d_Vn - d_V).abs_().max().item())
        d_Vn.fill_(float("nan"))
        d_p = d_pol.clone()
        getattr(eng, f"{fold}_value_sweep")(d_V.data_ptr(), d_Vn.data_ptr(), d_p.data_ptr(), 0, 0, n, g.gamma, d_delta.data_ptr(),
                                            d_changed.data_ptr())
        torch.cuda.synchronize()
        assert not bool(torch.isnan(d_Vn).any())
        H.assert_bits_equal(d_Vn[d_idx].cpu().numpy(), e_best_q, f"64^4 value sweep at {len(idx)} states")
        assert np.array_equal(d_p[d_idx].cpu().numpy(), e_best)
        assert float(d_delta.item()) == float((d_Vn - d_V).abs_().max().item())
        assert int(d_changed.item()) == int(torch.count_nonzero(d_p != d_pol).item()) > 0
        assert eng.info(Info.PAIR_TABLE) == 0
        del d_V, d_pol, d_Vn, d_p, Vh, polh
    finally:
        g.eng.close()
        _report_peak(f"{FOLD_NAMES[fold]} sweeps, 64^4")
        print(f"[{fold} edges] 64^4: {time.perf_counter() - t0:.2f} s")
        _free()


def test_large_handle_with_v_byte_offsets_beyond_2_pow_31(cuda_device, fold="expect", sample_shift=0):
    """double_pendulum_swingup (160, 161, 159, 162), n = 663 526 080 in [2^29, 2^30): the three kinds on sub-ranges only —
    the last 2^20 states, an unaligned window in the middle, and 2^19 states of the last theta1 plane with small negative
    th1_dot — compared at the states of that third window whose (undisturbed) successor cell lies in the top 1/64 of the
    table (at least 10 000; 4 * base >= 2^31 there; no state of the last 2^20 has such a successor: theta1 wraps) and at
    scattered states of every window; states outside a window keep their sentinel / their entry.
    Measured on an MI355X: 2.9 s (3.0 s as pytest counts the call; the deterministic test of this grid in
    tests/test_gpu_offsets32.py: 2.7 s); peak device memory as torch counts it 15.5 GiB; 31 234 of the 31 806 candidates
    have their successor cell in the top 1/64 of the table."""
    from tests.test_gpu_addr64 import _free, _grid, _points, _report_peak, _seeded_state, _torch
    from tests.test_gpu_offsets32 import SHAPE_V_4D
    torch = _torch()
    risk = _fold(fold)[2]
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    name = "double_pendulum_swingup"
    g = _grid(name, SHAPE_V_4D, None, cuda_device, form64=False)
    try:
        n, eng = g.n, g.eng
        assert n == 663_526_080 and 1 << 29 <= n < 1 << 30
        d = _large_set(g)
        _install(eng, d)
        Vh, polh, _, d_V, d_pol, _ = _seeded_state(g, 29, None, cuda_device, scale=30.0)
        lo, hi, gshape, strides = g.meta
        # the last plane of theta1 where th1_dot is small and negative (rows 60 .. 80 of 161): a step moves theta1 by less
        # than two cells there, so the successor cell keeps a corner in the last two planes (from the last 2^20 states, rows
        # 120 and up, theta1 wraps round to the other end of the table)
        top_a = n - n // g.shape[0] + 60 * int(strides[1]) + 11
        windows = {"the last 2^20 states": (n - (1 << 20), n), "the middle": (n // 2 - 300_007, n // 2 + 700_001),
                   "below the top": (top_a, top_a + (1 << 19))}
        rng = np.random.default_rng(2029)
        # the top-1/64 sample, picked on the host from that window with the checker's step and cell search
        a, b = windows["below the top"]
        cand = np.unique(rng.integers(a, b, size=(1 << 15) >> sample_shift, dtype=np.int64))
        flat_user, coords = _points(g, cand)
        nxt, _, done = g.chk.step(coords, g.acts[polh[flat_user]])
        cells, _ = g.chk.interp(nxt, lo, hi, gshape, strides)
        top = cand[~done & (cells.astype(np.int64).max(axis=1) >= n - n // 64)]
        print(f"[expect edges] {len(top)} of {len(cand)} candidates have their successor cell in the top 1/64 of the table")
        assert len(top) >= 10_000 >> sample_shift and 4 * int(cells.astype(np.int64).max()) >= 1 << 31
        d_Vb = torch.full((n,), float(SENTINEL), dtype=torch.float32, device=cuda_device)
        d_p = d_pol.clone()
        d_delta = torch.full((1,), 123.0, dtype=torch.float32, device=cuda_device)
        d_changed = torch.full((1,), 77, dtype=torch.int32, device=cuda_device)
        for where, (a, b) in windows.items():
            idx = np.unique(rng.integers(a, b, size=(1 << 13) >> sample_shift, dtype=np.int64))
            if where == "below the top":
                idx = np.unique(np.concatenate([idx, top]))
            if b == n:
                idx = np.unique(np.concatenate([idx, np.arange(n - 256, n, dtype=np.int64)]))
            flat_user, coords = _points(g, idx)
            e_eval, e_best, e_best_q = _large_twin(g, d, coords, polh[flat_user], Vh, risk)
            d_idx = torch.from_numpy(idx).to(cuda_device)
            what = f"{g.shape} {where} [{a}, {b})"

            def outside_untouched():
                assert int(torch.count_nonzero(d_Vb[:a] != float(SENTINEL)).item()) == 0
                assert int(torch.count_nonzero(d_Vb[b:] != float(SENTINEL)).item()) == 0
                assert torch.equal(d_p[:a], d_pol[:a]) and torch.equal(d_p[b:], d_pol[b:])

            getattr(eng, f"{fold}_eval_sweeps")(d_V.data_ptr(), d_Vb.data_ptr(), d_pol.data_ptr(), 0, a, b, g.gamma, 1, d_delta.data_ptr())
            torch.cuda.synchronize()
            H.assert_bits_equal(d_Vb[d_idx].cpu().numpy(), e_eval, f"{what}: evaluation at {len(idx)} states")
            assert float(d_delta.item()) == float((d_Vb[a:b] - d_V[a:b]).abs_().max().item())
            assert int(torch.count_nonzero(d_Vb[a:b] == float(SENTINEL)).item()) == 0
            outside_untouched()
            d_Vb[a:b] = float(SENTINEL)
            getattr(eng, f"{fold}_improve_sweep")(d_V.data_ptr(), d_p.data_ptr(), 0, a, b, g.gamma, d_changed.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(d_p[d_idx].cpu().numpy(), e_best), f"{what}: improvement at {len(idx)} states"
            assert int(d_changed.item()) == int(torch.count_nonzero(d_p[a:b] != d_pol[a:b]).item()) > 0
            assert int(torch.count_nonzero(d_Vb != float(SENTINEL)).item()) == 0
            outside_untouched()
            d_p[a:b] = d_pol[a:b]
            getattr(eng, f"{fold}_value_sweep")(d_V.data_ptr(), d_Vb.data_ptr(), d_p.data_ptr(), 0, a, b, g.gamma, d_delta.data_ptr(),
                                                d_changed.data_ptr())
            torch.cuda.synchronize()
            H.assert_bits_equal(d_Vb[d_idx].cpu().numpy(), e_best_q, f"{what}: value sweep at {len(idx)} states")
            assert np.array_equal(d_p[d_idx].cpu().numpy(), e_best)
            assert float(d_delta.item()) == float((d_Vb[a:b] - d_V[a:b]).abs_().max().item())
            assert int(d_changed.item()) == int(torch.count_nonzero(d_p[a:b] != d_pol[a:b]).item()) > 0
            outside_untouched()
            d_Vb[a:b] = float(SENTINEL)
            d_p[a:b] = d_pol[a:b]
        del d_V, d_pol, d_Vb, d_p, Vh, polh
    finally:
        g.eng.close()
        _report_peak(f"{FOLD_NAMES[fold]} sweeps, 32-bit V offsets beyond 2^31")
        print(f"[{fold} edges] (160, 161, 159, 162): {time.perf_counter() - t0:.2f} s")
        _free()
