"""Host-only half of tests/test_gpu_block_sizes.py and tests/test_gpu_division_paths.py: every workgroup size the knobs
PI_MI355_EVAL_BLOCK / PI_MI355_IMPROVE_BLOCK accept ("a multiple of 64 in 256..1024") and every division-path
specialisation those files run is built for gfx950 on a handle without a device, and the claims the GPU tests rest on
that a CPU can check are checked here: the verdicts of pi_create's division proof on the synthetic grids, the float32
numpy restatement of the cell search against the oracle, and that most successors of the mixed grids lie strictly inside
the grid.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info
from tests import helpers as H
from tests import test_gpu_division_paths as DP

SIZES = list(range(256, 1025, 64))
GRID = {2: ("pendulum", (24, 17)), 4: ("cartpole", (9, 7, 11, 5)), 6: ("double_cartpole", (5, 4, 6, 4, 5, 4))}
# (dimensions, evaluation size, improvement size, checked build)
BUILDS = ([(4, b, b, 0) for b in SIZES] + [(D, b, b, 0) for D in (2, 6) for b in (320, 768, 960, 1024)]
          + [(D, 960, 448, 0) for D in (2, 4, 6)] + [(D, b, b, 1) for D in (2, 4, 6) for b in (320, 960)])


def _define(src: str, macro: str):
    m = re.search(rf"^#define {macro} (\S+)$", src, flags=re.M)
    return None if m is None else m.group(1)


def test_the_list_of_sizes_is_the_knobs_range(monkeypatch):
    assert len(SIZES) == 13 and SIZES[0] == 256 and SIZES[-1] == 1024
    for knob, what in (("PI_MI355_EVAL_BLOCK", Info.EVAL_BLOCK), ("PI_MI355_IMPROVE_BLOCK", Info.IMPROVE_BLOCK)):
        for value in SIZES + [192, 300, 1088]:
            monkeypatch.setenv(knob, str(value))
            eng = H.host_engine(*GRID[2])
            assert eng.info(what) == (value if value in SIZES else 256), (knob, value)
            eng.close()
        monkeypatch.delenv(knob)


@pytest.mark.parametrize("D,eb,ib,debug", BUILDS, ids=[f"{D}d-{eb}-{ib}" + ("-checked" if dbg else "") for D, eb, ib, dbg in BUILDS])
def test_every_accepted_workgroup_size_builds(D, eb, ib, debug, tmp_path, monkeypatch):
    """pi_compile of the env's own dynamics at every size the knobs accept, default and checked build.  FAILS ON THE PARENT
    of the commit that added this file, for every size but 256, 512 and 1024: pi_create accepted the size, pi_first_chunk
    refused it with `static assertion failed ... chunk size must be a power of two (shift, not divide)`."""
    name, shape = GRID[D]
    monkeypatch.setenv("PI_MI355_EVAL_BLOCK", str(eb))
    monkeypatch.setenv("PI_MI355_IMPROVE_BLOCK", str(ib))
    if debug:
        monkeypatch.setenv("PI_MI355_DEBUG", "1")
    else:
        monkeypatch.delenv("PI_MI355_DEBUG", raising=False)
    eng = H.host_engine(name, shape)
    try:
        assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK), eng.info(Info.DEBUG_CHECKS)) == (eb, ib, debug)
        dyn = envs.dynamics_source(name)
        src = eng.kernel_source(dyn)
        assert (_define(src, "PI_BLOCK_EVAL"), _define(src, "PI_BLOCK_IMPROVE")) == (str(eb), str(ib))
        eng.compile(dyn, cache_dir=tmp_path)
        assert eng.info(Info.CACHE_HIT) == 0
        (obj,) = list(tmp_path.glob("pi_*.hsaco"))
        assert obj.read_bytes()[:4] == b"\x7fELF"
    finally:
        eng.close()


def test_plan_schedule_takes_every_whole_number_of_waves():
    """pi_plan_schedule answers for the sizes the sweeps can be launched with (it refused all but the powers of two), and
    the kernels' map covers a ragged range at each of them."""
    eng = H.host_engine(*GRID[6])
    n = eng.n_states
    for block in [64, 128, 192] + SIZES:
        for cpw in (1, 3):
            s = eng.plan_schedule(block, 5, n - 12, chunks_per_workgroup=cpw)
            chunks = -(-(n - 12) // block)
            g = H.schedule_groups(s, chunks)[:, 0]
            assert s["period"] == 0 and sorted(g[g >= 0]) == list(range(-(-chunks // cpw))), (block, cpw)
    for block in (0, 32, 300, 1000, 1088, 2048):
        with pytest.raises(_native.NativeError, match="bad launch shape"):
            eng.plan_schedule(block, 0, n)
    eng.close()


# ---- the division paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", DP.SMALL_GRIDS, ids=[n for n, _ in DP.SMALL_GRIDS])
def test_ieee_div_builds_report_no_proven_dimension(name, shape, tmp_path, monkeypatch):
    monkeypatch.setenv("PI_MI355_IEEE_DIV", "1")
    eng = H.host_engine(name, shape)
    D = len(shape)
    assert [eng.info(Info.RECIPROCAL_DIV + d) for d in range(D)] == [0] * D
    eng.compile(envs.dynamics_source(name), cache_dir=tmp_path)
    assert eng.info(Info.CACHE_HIT) == 0
    eng.close()


@pytest.mark.parametrize("build", ["default", "ieee", "checked"])
def test_the_grid_of_the_guards_edges_builds(build, tmp_path, monkeypatch):
    monkeypatch.delenv("PI_MI355_IEEE_DIV", raising=False)
    monkeypatch.delenv("PI_MI355_DEBUG", raising=False)
    if build != "default":
        monkeypatch.setenv({"ieee": "PI_MI355_IEEE_DIV", "checked": "PI_MI355_DEBUG"}[build], "1")
    bins, src = DP.guard_bins(), DP.guard_plugin()
    assert all(b[0] == 0.0 for b in bins)
    eng = DP.synthetic_engine(bins, src)
    assert [eng.info(Info.RECIPROCAL_DIV + d) for d in range(4)] == ([0] * 4 if build == "ieee" else [1] * 4)
    assert eng.info(Info.DEBUG_CHECKS) == (build == "checked")
    eng.compile(src, cache_dir=tmp_path)
    assert eng.info(Info.CACHE_HIT) == 0
    eng.close()


@pytest.mark.parametrize("D", [2, 4])
def test_mixed_grids_build_with_the_verdicts_they_are_about(D, tmp_path, monkeypatch):
    monkeypatch.delenv("PI_MI355_IEEE_DIV", raising=False)
    spans, shape = DP.MIXED_SPANS[D], DP.MIXED_SHAPES[D]
    assert spans[0] < 2.0 ** -30 and (D == 2 or spans[2] > 2.0 ** 30)
    bins, src = DP.centred_bins(spans, shape), DP.linear_plugin(spans)
    for b, span in zip(bins, spans):
        assert b.dtype == np.float32 and np.all(np.diff(b) > 0) and np.float32(b[-1] - b[0]) == np.float32(span)
    eng = DP.synthetic_engine(bins, src)
    assert [eng.info(Info.RECIPROCAL_DIV + d) for d in range(D)] == DP.MIXED_VERDICT[D] == [0, 1, 0, 1][:D]
    eng.compile(src, cache_dir=tmp_path)
    assert eng.info(Info.CACHE_HIT) == 0
    assert "PI_FASTDIV_INIT {" + ",".join(str(v) for v in DP.MIXED_VERDICT[D]) + "}" in eng.kernel_source(src)
    eng.close()


@pytest.mark.parametrize("D", [2, 4])
def test_most_successors_of_the_mixed_grids_lie_strictly_inside(D):
    """A sweep that only ever clamps proves nothing about the division: with the oracle's step, at least half of the (state,
    action) successors lie strictly inside the grid in every dimension (measured: 2-D 0.879, 4-D 0.544), and some do leave it
    on either side of every dimension, so that the clamp is run as well."""
    spans, shape = DP.MIXED_SPANS[D], DP.MIXED_SHAPES[D]
    bins, src = DP.centred_bins(spans, shape), DP.linear_plugin(spans)
    chk = oracle.build(D, src)
    states = oracle.states_from_bins(bins)
    lo, hi = np.array([b[0] for b in bins]), np.array([b[-1] for b in bins])
    inside, below, above = [], np.zeros(D, bool), np.zeros(D, bool)
    for a in DP.MIXED_ACTIONS:
        nxt, reward, done = chk.step(states, a)
        assert not done.any() and np.isfinite(nxt).all() and np.isfinite(reward).all()
        inside.append(((nxt > lo) & (nxt < hi)).all(axis=1))
        below |= (nxt < lo).any(axis=0)
        above |= (nxt > hi).any(axis=0)
    share = float(np.mean(inside))
    print(f"[mixed {D}-D] share of successors strictly inside the grid: {share:.4f}")
    assert share >= 0.5
    assert below.all() and above.all()


def test_numpy_restatement_of_the_cell_search_equals_the_oracle():
    """interp_float32 (tests/test_gpu_division_paths.py) against oracle.interp on the guard's edges, on sampled points of
    that grid, and on a mixed grid: cells equal, weights bit-equal, NaN matching NaN."""
    bins = DP.guard_bins()
    chk = oracle.build(4, DP.guard_plugin())
    rng = np.random.default_rng(3)
    pts = np.concatenate([DP.guard_points(bins), H.sample_states(rng, bins, 4096)])
    assert len(DP.guard_points(bins)) > 300
    pts[-3:] = np.array([np.nan, np.inf, -np.inf], np.float32)[:, None]
    o_idx, o_w = chk.interp(pts, *oracle.grid_metadata(bins))
    n_idx, n_w = DP.interp_float32(pts, bins)
    assert np.array_equal(o_idx, n_idx)
    DP._same(o_w, n_w, "weights on the guard grid")
    for D in (2, 4):
        mb = DP.centred_bins(DP.MIXED_SPANS[D], DP.MIXED_SHAPES[D])
        mp = H.sample_states(rng, mb, 4096)
        o_idx, o_w = oracle.build(D, DP.linear_plugin(DP.MIXED_SPANS[D])).interp(mp, *oracle.grid_metadata(mb))
        n_idx, n_w = DP.interp_float32(mp, mb)
        assert np.array_equal(o_idx, n_idx)
        DP._same(o_w, n_w, f"weights on the mixed {D}-D grid")
