"""
Host-only half of the dispatch-threshold and degenerate-grid tests (the GPU half: tests/test_gpu_edges.py).

pi_create picks among six kernel families and several launch geometries by comparing the state count with fixed numbers.
`helpers.DISPATCH_TABLE` states, from the design, what it must decide on the nearest grid on each side of every one of
them; this module reads the decisions back from handles without a device (pi_info, and the generated source for the
two facts no info code reports there), pins pi_create's table limit, compiles every specialisation the GPU half runs —
default and checked build — and pins the CPU oracle on the degenerate grids where it becomes that half's reference.

Two facts cannot be read through pi_info on a handle without a device: Info.XCD_ENABLED answers whether pi_xcd_kernel
was LOADED and placed (always 0 here), and Info.FLOW_WORKGROUPS answers 1 instead of the workgroup count.  Both
decisions are in the translation unit pi_create specialises (`#define PI_XCD 1`, `PI_XCD_S`, `PI_FLOW`), which
Engine.kernel_source returns without a device; tests/test_gpu_edges.py asserts the info codes themselves on the device.

pi_stage_table's strided branch (tables of more than 8 * 256 = 2048 floats): the largest table of any shape the GPU
test files named before this module is 736 floats (181 x 183 x 179 x 182 with 11 actions; 200 x 200 with
21 actions: 421), so that branch was in no kernel any test ran.  `helpers.EDGE_CASES` has six shapes that take it (2 x 3000, 3000 x 2, 2 x 2026, 2 x 15337, 2.2.2.2100;
2.2.2.1500, which the issue lists among them, holds 1517 floats and does not).
"""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from dynamicprogramming_amd._native import Info
from tests import helpers as H

ROOT = Path(__file__).resolve().parents[1]


def _readelf():
    """llvm-readelf of the ROCm installation hipcc belongs to."""
    import __graft_entry__ as G
    return Path(G.HIPCC).resolve().parents[1] / "llvm" / "bin" / "llvm-readelf"


def _define(src: str, macro: str):
    m = re.search(rf"^#define {macro} (\S+)$", src, flags=re.M)
    return None if m is None else m.group(1)


def _row_id(row):
    acts = "" if row.get("actions") is None else f"-{len(row['actions'])}actions"
    return row["name"] + "-" + "x".join(str(g) for g in row["shape"]) + acts


@pytest.mark.parametrize("row", H.DISPATCH_TABLE + H.EDGE_ROWS, ids=_row_id)
def test_dispatch_table(row):
    """Every decision of pi_create at the thresholds of its dispatch, on both sides of each."""
    name, shape = row["name"], row["shape"]
    eng = H.host_engine(name, shape, row.get("actions"))
    n = int(np.prod(shape, dtype=np.int64))
    assert eng.n_states == n
    assert eng.info(Info.RESIDENT_STATES_PER_THREAD) == row["k"]
    assert eng.info(Info.RESIDENT_ENABLED) == 1
    assert eng.info(Info.FLOW_WORKGROUPS) == (1 if row["flow"] else 0)           # host-only handles answer 0 / 1
    assert eng.info(Info.XCD_ENABLED) == 0                                       # ... and never load pi_xcd_kernel
    assert (eng.info(Info.EVAL_BLOCK), eng.info(Info.IMPROVE_BLOCK)) == (row["eb"], row["ib"])
    assert (eng.info(Info.EVAL_CPW), eng.info(Info.IMPROVE_CPW)) == (row["ecpw"], row["icpw"])
    whole = eng.kernel_source(envs.dynamics_source(name))
    src = whole[:whole.index("#define PI_D ")]                                  # the lines pi_create's decisions write
    assert _define(src, "PI_RESIDENT_K") == str(row["k"])
    assert (_define(src, "PI_FLOW") == "1") == row["flow"]
    assert _define(src, "PI_XCD") == (None if row["xcd_s"] is None else "1")
    assert _define(src, "PI_XCD_S") == (None if row["xcd_s"] is None else str(row["xcd_s"]))
    if row["xcd_s"] is not None:                                                # 32 workgroups cover the grid
        assert row["xcd_s"] % 32 == 0 and 32 * row["xcd_s"] >= n > 32 * (row["xcd_s"] - 32)
    assert (_define(src, "PI_BLOCK_EVAL"), _define(src, "PI_BLOCK_IMPROVE")) == (str(row["eb"]), str(row["ib"]))
    # the one-launch kernels are part of the translation unit exactly where one of them is wanted
    assert ("// ---- one-launch kernels ----" in whole) == (row["k"] > 0 or row["flow"])
    eng.close()


def test_dispatch_table_covers_both_sides_of_every_threshold():
    """The table's own shape: every threshold has a grid of exactly that many states and a neighbour on the other side no
    further than a quarter of it away (6-D, 1024: the nearest grid of 2- and 4-bin dimensions beyond it has 1280)."""
    n = [int(np.prod(r["shape"], dtype=np.int64)) for r in H.DISPATCH_TABLE]
    sides = {(len(r["shape"]), m) for r, m in zip(H.DISPATCH_TABLE, n)}
    for D, limit in ((2, 12288), (2, 4096), (2, 1 << 16), (2, 1 << 17), (4, 1 << 17), (4, 4096), (6, 1024), (4, 1 << 20),
                     (4, 1 << 22), (4, 1 << 24), (6, 1 << 24)):
        assert (D, limit) in sides, (D, limit)
        near = [m for d, m in sides if d == D and m != limit and abs(m - limit) <= limit // 4]
        assert near, (D, limit)


@pytest.mark.parametrize("name,shape,order", H.SOLVER_ORDER_TABLE)
def test_solver_memory_order_threshold(name, shape, order, monkeypatch):
    """2^22 states: from there on a single-rank solver stores the grid in its class's MEMORY_ORDER; a plugin without one
    has its order measured (`_tune_memory_order`), below the limit nothing is measured and nothing permuted."""
    from dynamicprogramming_amd import solver as S
    monkeypatch.delenv("PI_MI355_ORDER", raising=False)
    cls = envs.ENVS[name]
    n = int(np.prod(shape, dtype=np.int64))
    assert S._CudaPolicyIterationBase._ORDER_MIN_STATES == 1 << 22 == cls._ORDER_MIN_STATES
    assert (n >= 1 << 22) == (order is not None)
    measured = []

    def fake_tune(self):
        measured.append(type(self).__name__)
        return tuple(reversed(range(self._D)))

    def bare(klass):
        s = object.__new__(klass)
        s.n_states, s._transport_arg, s._process_group = n, False, None
        return s
    monkeypatch.setattr(S._CudaPolicyIterationBase, "_tune_memory_order", fake_tune)
    assert bare(cls)._choose_memory_order() == order and measured == []
    untuned = type("Untuned", (cls,), {"MEMORY_ORDER": None})
    got = bare(untuned)._choose_memory_order()
    assert got == (None if order is None else tuple(reversed(range(cls._D))))
    assert measured == ([] if order is None else ["Untuned"])


def test_table_limit():
    """15 360 floats of actions + bin tables (60 KiB) are accepted, 15 361 refused."""
    for name, shape in (("pendulum", (2, 15337)), ("pendulum", (7669, 7670))):
        assert H.table_floats(name, shape) == 15360
        eng = H.host_engine(name, shape)
        assert eng.n_states == int(np.prod(shape, dtype=np.int64))
        eng.close()
    for name, shape in (("pendulum", (2, 15338)), ("pendulum", (7670, 7670))):
        assert H.table_floats(name, shape) == 15361
        with pytest.raises(_native.NativeError, match="bin tables \\+ actions exceed the 60 KiB LDS budget"):
            H.host_engine(name, shape)
    # the actions count: one torque more on the accepted shape is refused, one fewer on the refused one accepted
    acts = np.linspace(-2.0, 2.0, 22, dtype=np.float32)
    with pytest.raises(_native.NativeError, match="60 KiB LDS budget"):
        H.host_engine("pendulum", (2, 15337), acts)
    H.host_engine("pendulum", (2, 15338), acts[:20]).close()


def test_edge_case_list_is_what_it_says():
    """The sizes the case ids promise (table floats, state counts, ties in the clamped action sets)."""
    case = {cid: (name, shape, acts) for cid, name, shape, acts in H.EDGE_CASES}
    assert [H.table_floats(*case[c]) for c in ("tab2048", "tab2049", "tab15360")] == [2048, 2049, 15360]
    for cid in ("one2-slowest", "one2-fastest"):
        assert H.table_floats(*case[cid]) > 2048 and 2 in case[cid][1]
    assert H.table_floats(*case["one2-4d"]) == 1517 and case["one2-4d"][1] == (2, 2, 2, 1500)        # register-staged
    assert H.table_floats(*case["one2-4d-strided"]) == 2117
    for cid, n in (("n63", 63), ("n255", 255), ("n256", 256), ("n258", 258), ("n259", 259), ("n513-4d", 513), ("n1025", 1025),
                   ("all2-2d", 4), ("all2-4d", 16), ("all2-6d", 64)):
        assert int(np.prod(case[cid][1])) == n
    assert all(257 % k for k in range(2, 17))                                    # prime: no grid has 257 states
    assert [len(case[c][2]) for c in ("act1", "act2", "act64", "act257")] == [1, 2, 64, 257]
    for cid in ("act2", "act64", "act257"):                                      # several actions clamp to the same torque
        a = case[cid][2]
        assert (a <= -2.0).sum() + (a >= 2.0).sum() >= 2 and a.min() < -2.0 and a.max() > 2.0
    envs_used = {name for _, name, _, _ in H.EDGE_CASES + H.THRESHOLD_CASES}
    assert {"pendulum", "double_pendulum_swingup", "double_cartpole_swingup"} <= envs_used      # wrapped angles
    assert {"mountain_car", "cartpole", "double_cartpole"} <= envs_used                          # terminal states


def _kernel_scratch(hsaco: Path) -> dict:
    """{kernel: bytes of scratch per work-item} from the code object's metadata note."""
    out = subprocess.run([str(_readelf()), "--notes", str(hsaco)], capture_output=True, text=True, check=True).stdout
    usage, name = {}, None
    for key, value in re.findall(r"\.(name|private_segment_fixed_size):\s+(\S+)", out):
        if key == "name":
            name = value
        elif name is not None:
            usage[name] = int(value)
            name = None
    return usage


@pytest.mark.parametrize("cid,name,shape,actions", H.edge_case_params())
def test_edge_specialisations_compile(cid, name, shape, actions, tmp_path, monkeypatch):
    """Every specialisation tests/test_gpu_edges.py runs builds for gfx950, default and checked (PI_MI355_DEBUG=1), and
    the sweep kernels keep no scratch (what test_register_budgets_of_the_baseline_kernels asserts of them)."""
    dyn = envs.dynamics_source(name)
    for debug in (0, 1):
        if debug:
            monkeypatch.setenv("PI_MI355_DEBUG", "1")
        else:
            monkeypatch.delenv("PI_MI355_DEBUG", raising=False)
        cache = tmp_path / f"debug{debug}"
        eng = H.host_engine(name, shape, actions)
        assert eng.info(Info.DEBUG_CHECKS) == debug and eng.info(Info.N_ACTIONS) == len(H.edge_actions(name, actions))
        eng.compile(dyn, cache_dir=cache)
        assert eng.info(Info.CACHE_HIT) == 0
        (obj,) = list(cache.glob("pi_*.hsaco"))
        assert obj.read_bytes()[:4] == b"\x7fELF"
        scratch = _kernel_scratch(obj)
        for kernel in ("pi_eval_sweep_kernel", "pi_improve_sweep_kernel"):
            assert scratch[kernel] == 0, (cid, debug, kernel, scratch[kernel])
        eng.close()


# |dV| <= 1e-5 * max(1, |V|) against the float64 statement, policy equal wherever the top-two gap exceeds that: the
# tolerance of tests/test_gpu_parity.py for fp32 sweeps against another arithmetic.
ORACLE_TOL = 1e-5            # measured on the grids below: at most 1.9e-6 (values), no policy entry differs at any gap


@pytest.mark.parametrize("name,shape", [("pendulum", (2, 2)), ("mountain_car", (2, 2)), ("double_pendulum_swingup", (2, 2, 2, 2)),
                                         ("cartpole", (2, 2, 2, 2)), ("double_cartpole_swingup", (2,) * 6),
                                         ("double_cartpole", (2,) * 6), ("pendulum", (2, 3)), ("mountain_car", (3, 2)),
                                         ("pendulum", (2, 37)), ("mountain_car", (41, 2)),
                                         ("cartpole_swingup", (5, 2, 7, 4)), ("double_cartpole", (3, 3, 2, 3, 4, 3))])
def test_oracle_on_degenerate_grids_against_float64_numpy(name, shape):
    """The oracle is the reference of tests/test_gpu_edges.py; on grids with 2 bins in every dimension (one cell: every
    successor's base index is 0) or in one dimension it had never been used.  One evaluation sweep and one improvement
    sweep against a plain float64 numpy statement of the backup (helpers.backup_float64)."""
    cls = envs.ENVS[name]
    bins = H.env_bins(name, shape)
    acts = H.edge_actions(name)
    lo, hi, gshape, strides = oracle.grid_metadata(bins)
    states = oracle.states_from_bins(bins)
    n = len(states)
    term, tval = H.terminal_mask(name, states)
    rng = np.random.default_rng(17)
    # V is rough white noise like the one the GPU tests draw; its RANGE follows from the number format, written out per
    # dimension, not from a result.  float32 places a successor in dimension d at t = (x - lo) / span * (g_d - 1): three
    # roundings of at most 2^-24 relative on up to g_d - 1 cells, so t is off by at most 3 * 2^-24 * (g_d - 1) cells
    # against float64, and E by that times the difference of V across the cell, at most 2 max|V|.  The 2^D-term sum of
    # products and r + gamma * E add at most (D + 3) * 2^-24 * max|V| (the reward's own share scales with |V'| and is
    # inside max(1, |V|)).  So |dV| <= 2^-24 * max|V| * (6 * sum_d (g_d - 1) + D + 3), and that stays within 1e-5 for
    #   max|V| = 1e-5 * 2^24 / (6 * sum_d (g_d - 1) + D + 3):
    # 9.9 on 2 x 2 (the GPU tests' 3 sigma is 9), 3.7 on 2^6, 7.3 on 3 x 2, 0.67 on 41 x 2 — where noise of sigma 3
    # measures 1.07e-5 at a state whose four corners span -2.6 .. 3.4: the format's error, not the oracle's.
    vmax = min(9.0, 1e-5 * 2.0 ** 24 / (6 * sum(g - 1 for g in shape) + len(shape) + 3))
    V = rng.uniform(-vmax, vmax, size=n).astype(np.float32)
    V[term] = np.float32(tval)
    pol = rng.integers(0, len(acts), size=n).astype(np.int32)
    pol[term] = 0
    gamma = float(np.float32(cls.CONFIG["gamma"]))
    chk = H.oracle_for(name)
    if 2 in shape and all(g == 2 for g in shape):
        idx, _ = chk.interp(chk.step(states, acts[0])[0], lo, hi, gshape, strides)
        assert (idx[:, 0] == 0).all() and (idx[:, -1] == n - 1).all()            # the one cell
    Q = H.backup_float64(chk, bins, acts, V, gamma)
    want_V = np.where(term, V.astype(np.float64), Q[pol, np.arange(n)])
    got_V, got_delta = chk.eval_sweep(states, acts, pol, V, term, lo, hi, gshape, strides, gamma)
    err = np.abs(got_V - want_V) / np.maximum(1.0, np.abs(want_V))
    print(f"[oracle-f64] {name} {shape}: max relative |dV| {err.max():.3g}")
    assert err.max() <= ORACLE_TOL
    assert abs(got_delta - np.abs(want_V - V).max()) <= ORACLE_TOL * max(1.0, float(np.abs(want_V).max()))
    got_pol, got_changed = chk.improve_sweep(states, acts, pol, V, term, lo, hi, gshape, strides, gamma)
    best = Q.argmax(axis=0)                                                      # the first maximum
    top2 = np.sort(Q, axis=0)[-2:] if len(acts) > 1 else np.stack([Q[0] - 1.0, Q[0]])
    firm = (top2[1] - top2[0]) > ORACLE_TOL * np.maximum(1.0, np.abs(top2[1]))
    live = ~term
    assert np.array_equal(got_pol[term], pol[term])                              # terminal states keep their entry
    assert np.array_equal(got_pol[live & firm], best[live & firm])
    print(f"[oracle-f64] {name} {shape}: {int((got_pol[live] != best[live]).sum())} of {int(live.sum())} live entries differ "
          f"from the float64 argmax ({int((live & ~firm).sum())} within the tolerance of a tie)")
    assert got_changed == int((got_pol != pol).sum())
