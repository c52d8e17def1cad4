"""The parse rule of every PI_MI355_* knob that shows on a host-only handle or in the Python package, pinned value by
value (CPU only; the tables: csrc/pi_knobs.cpp, dynamicprogramming_amd/_knobs.py).  The expected values are facts of
the library's behaviour, the odd ones included — text that is no number reads as 0 (C's atoi), which an on/off knob
takes for "off" and a knob whose range excludes 0 refuses."""
from __future__ import annotations

import re
import types

import pytest

from dynamicprogramming_amd import envs
from dynamicprogramming_amd import solver as S
from dynamicprogramming_amd import transport as T
from dynamicprogramming_amd._native import Info, Plan
from tests import helpers as H

SMALL = ("pendulum", (24, 17))              # 408 states: one CU holds it
XCD_GRID = ("pendulum", (65, 64))           # 4 160 states: the smallest kind of grid the XCD-local kernel takes
GRID_4D = ("cartpole", (9, 8, 11, 7))


def _set(monkeypatch, knob, value):
    if value is None:
        monkeypatch.delenv(knob, raising=False)
    else:
        monkeypatch.setenv(knob, value)


def _info(monkeypatch, knob, value, what, grid=SMALL):
    _set(monkeypatch, knob, value)
    eng = H.host_engine(*grid)
    try:
        return eng.info(what)
    finally:
        eng.close()


def _define(monkeypatch, knob, value, macro, grid=SMALL):
    """The value the head of the generated translation unit defines `macro` as; None when it does not define it."""
    _set(monkeypatch, knob, value)
    eng = H.host_engine(*grid)
    try:
        defines = eng.kernel_source(envs.dynamics_source(grid[0])).split("// ---- env plugin", 1)[0]     # the handle's own
        m = re.search(rf"^#define {macro} (.*)$", defines, re.M)
        return m.group(1) if m else None
    finally:
        eng.close()


# knob, the info code it shows in, {value: expected}; None = unset
INT_KNOBS = [
    ("PI_MI355_EVAL_BLOCK", Info.EVAL_BLOCK,
     {None: 256, "512": 512, "1024": 1024, "320": 320, "300": 256, "128": 256, "2048": 256, "abc": 256, "": 256, "512x": 512}),
    ("PI_MI355_IMPROVE_BLOCK", Info.IMPROVE_BLOCK, {None: 256, "768": 768, "700": 256, "64": 256, "abc": 256}),
    ("PI_MI355_EVAL_CPW", Info.EVAL_CPW, {None: 1, "4": 4, "64": 64, "0": 1, "65": 1, "-3": 1, "abc": 1}),
    ("PI_MI355_IMPROVE_CPW", Info.IMPROVE_CPW, {None: 1, "3": 3, "0": 1, "65": 1, "abc": 1}),
    ("PI_MI355_GRAPHS", Info.GRAPHS_ENABLED, {None: 1, "0": 0, "1": 1, "2": 1, "-1": 1, "abc": 0}),
    ("PI_MI355_RESIDENT", Info.RESIDENT_STATES_PER_THREAD, {None: 1, "0": 0, "1": 1, "2": 1, "abc": 0}),
    ("PI_MI355_DEBUG", Info.DEBUG_CHECKS, {None: 0, "1": 1, "0": 0, "2": 0, "abc": 0}),
]


@pytest.mark.parametrize("knob,what,cases", INT_KNOBS, ids=[k[0] for k in INT_KNOBS])
def test_integer_knobs_take_values_in_range_and_nothing_else(knob, what, cases, monkeypatch):
    for value, expected in cases.items():
        assert _info(monkeypatch, knob, value, what) == expected, (knob, value)


def test_block_and_debug_knobs_reach_the_generated_source(monkeypatch):
    assert _define(monkeypatch, "PI_MI355_EVAL_BLOCK", "320", "PI_BLOCK_EVAL") == "320"
    assert _define(monkeypatch, "PI_MI355_EVAL_BLOCK", "300", "PI_BLOCK_EVAL") == "256"       # no multiple of 64
    monkeypatch.delenv("PI_MI355_EVAL_BLOCK")
    assert _define(monkeypatch, "PI_MI355_DEBUG", "1", "PI_DEBUG_BOUNDS") == "1"
    for value in (None, "0", "2", "abc"):
        assert _define(monkeypatch, "PI_MI355_DEBUG", value, "PI_DEBUG_BOUNDS") is None, value


def test_xcd_and_resident_knobs_decide_the_one_launch_kernels(monkeypatch):
    """PI_MI355_XCD takes the XCD-local kernel out and leaves the dataflow kernel; PI_MI355_RESIDENT = 0 takes out both."""
    for value, expected in {None: "1", "1": "1", "0": None, "2": "1", "abc": None}.items():
        assert _define(monkeypatch, "PI_MI355_XCD", value, "PI_XCD", XCD_GRID) == expected, value
        assert _define(monkeypatch, "PI_MI355_XCD", value, "PI_FLOW", XCD_GRID) == ("1" if expected else None), value
    # constants, not knobs: the ring depth, the first sleep (the kernel file's default), the sizes the kernel takes
    assert _define(monkeypatch, "PI_MI355_XCD", None, "PI_XCD_RING", XCD_GRID) == "64"
    assert _define(monkeypatch, "PI_MI355_XCD", None, "PI_XCD_FIRST_SLEEP", XCD_GRID) is None
    assert _define(monkeypatch, "PI_MI355_XCD", None, "PI_XCD", ("pendulum", (64, 64))) is None         # 4 096 states: one CU's
    assert _define(monkeypatch, "PI_MI355_XCD", None, "PI_XCD", ("pendulum", (256, 256))) == "1"        # 2^16: the last one
    assert _define(monkeypatch, "PI_MI355_XCD", None, "PI_XCD", ("pendulum", (257, 256))) is None
    assert _define(monkeypatch, "PI_MI355_XCD", None, "PI_FLOW", ("pendulum", (257, 256))) == "1"
    for value, expected in {"0": None, "1": "1", "2": "1"}.items():
        assert _define(monkeypatch, "PI_MI355_RESIDENT", value, "PI_XCD", XCD_GRID) == expected, value
        assert _define(monkeypatch, "PI_MI355_RESIDENT", value, "PI_FLOW", XCD_GRID) == expected, value


def test_ieee_div_is_on_whenever_the_variable_exists(monkeypatch):
    for grid, dims in ((SMALL, 2), (GRID_4D, 4)):
        assert _define(monkeypatch, "PI_MI355_IEEE_DIV", None, "PI_FASTDIV_INIT", grid) != "{" + ",".join("0" * dims) + "}"
        for value in ("1", "0", "", "no"):
            assert _define(monkeypatch, "PI_MI355_IEEE_DIV", value, "PI_FASTDIV_INIT", grid) == "{" + ",".join("0" * dims) + "}", value
            assert _info(monkeypatch, "PI_MI355_IEEE_DIV", value, Info.RECIPROCAL_DIV + dims - 1, grid) == 0


def test_strip_takes_a_whole_number_of_states_and_nothing_else(monkeypatch):
    """PI_MI355_STRIP shows in Info.STRIP_STATES once pi_compile has fixed the memory order; the knob is not in the
    source, so the handles share one code object.  The grid is pendulum 64 x 64 because build() puts that unit into the
    code-object cache: every compile here is then a hit and the test takes milliseconds; on a tree whose cache does
    not hold it the first compile takes a few seconds and fills it.  On grids below 2^24 states the library's own
    choice is the slab schedule (0)."""
    grid = ("pendulum", (64, 64))
    dyn = envs.dynamics_source(grid[0])
    cases = {None: 0, "0": 0, "100": 100, "4096": 4096, "4097": 0, "-1": 0, "auto": 0, "12x": 0, "": 0, " 12": 12, "12 ": 0}
    for value, expected in cases.items():
        _set(monkeypatch, "PI_MI355_STRIP", value)
        eng = H.host_engine(*grid)
        eng.compile(dyn)
        assert eng.info(Info.STRIP_STATES) == expected, value
        eng.close()


def test_knobs_are_read_per_handle_not_once(monkeypatch):
    assert _info(monkeypatch, "PI_MI355_EVAL_CPW", "8", Info.EVAL_CPW) == 8
    assert _info(monkeypatch, "PI_MI355_EVAL_CPW", "2", Info.EVAL_CPW) == 2
    assert _info(monkeypatch, "PI_MI355_EVAL_CPW", None, Info.EVAL_CPW) == 1


# ── the Python side ─────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("value,expected", [(None, True), ("1", True), ("0", False)])
def test_whole_run_overlap_and_p2p_fused_are_off_at_0_only(value, expected, monkeypatch):
    backend = types.SimpleNamespace(resident=True, engine=types.SimpleNamespace(info=lambda what: 1))
    _set(monkeypatch, "PI_MI355_WHOLE_RUN", value)
    assert S.HipSweepBackend.whole_run.fget(backend) is expected

    seen = {}
    def exchange_plan(term, shard_len, mode, overlap, stream):
        seen.update(mode=mode, overlap=overlap)
        return {"mode": "allgather", "recv_elems": 0}
    transport = types.SimpleNamespace(engine=types.SimpleNamespace(exchange_plan=exchange_plan), _stream=lambda: 0)
    solver = types.SimpleNamespace(_backend=types.SimpleNamespace(_ptr=lambda t: 0), _mask_arg=lambda: None, _shard_len=1)
    monkeypatch.delenv("PI_MI355_EXCHANGE", raising=False)
    _set(monkeypatch, "PI_MI355_OVERLAP", value)
    T.NativeTransport.plan(transport, solver)
    assert bool(seen["overlap"]) is expected and seen["mode"] == Plan.NONE

    # a sharded solver without a transport of its own: peer-to-peer and fused <=> it may take its sharded memory order
    chooser = types.SimpleNamespace(_transport_arg=None)
    _set(monkeypatch, "PI_MI355_P2P_FUSED", value)
    monkeypatch.setenv("PI_MI355_TRANSPORT", "P2P")                  # case-folded
    assert bool(S._CudaPolicyIterationBase._shards_over_p2p(chooser)) is expected
    monkeypatch.setenv("PI_MI355_TRANSPORT", "rccl")
    assert not S._CudaPolicyIterationBase._shards_over_p2p(chooser)
    monkeypatch.delenv("PI_MI355_TRANSPORT")
    assert not S._CudaPolicyIterationBase._shards_over_p2p(chooser)


def test_exchange_names_a_plan_mode_or_raises(monkeypatch):
    seen = []
    transport = types.SimpleNamespace(_stream=lambda: 0, engine=types.SimpleNamespace(
        exchange_plan=lambda term, shard_len, mode, overlap, stream: seen.append(mode) or {"mode": "allgather", "recv_elems": 0}))
    solver = types.SimpleNamespace(_backend=types.SimpleNamespace(_ptr=lambda t: 0), _mask_arg=lambda: None, _shard_len=1)
    for value, mode in (("auto", Plan.NONE), ("allgather", Plan.ALLGATHER), ("halo", Plan.HALO)):
        monkeypatch.setenv("PI_MI355_EXCHANGE", value)
        T.NativeTransport.plan(transport, solver)
        assert seen[-1] == mode
    for value in ("Halo", "ring", ""):
        monkeypatch.setenv("PI_MI355_EXCHANGE", value)
        with pytest.raises(KeyError):
            T.NativeTransport.plan(transport, solver)
