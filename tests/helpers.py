"""Shared helpers for the test-suite (grids, masks, bit-level comparisons, checker backend)."""
from __future__ import annotations

from pathlib import Path

import numpy as np

import oracle
from dynamicprogramming_amd import envs
from dynamicprogramming_amd.solver import _CudaPolicyIterationBase

GOLDEN = Path(__file__).resolve().parent / "golden"
ENV_NAMES = list(envs.ENVS)


def env_bins(name: str, shape) -> list[np.ndarray]:
    """The env's reference grid ranges with shape[d] points in dimension d."""
    cls = envs.ENVS[name]
    out = []
    for d, g in enumerate(shape):
        space = cls.bins_space(int(g))
        out.append(np.asarray(list(space.values())[d], dtype=np.float32))
    return out


def env_bins_space(name: str, shape) -> dict:
    cls = envs.ENVS[name]
    keys = list(cls.bins_space(2).keys())
    return dict(zip(keys, env_bins(name, shape)))


def terminal_mask(name: str, states: np.ndarray):
    cls = envs.ENVS[name]
    inst = object.__new__(cls)
    if name == "overhead_crane":
        inst.target_x = 0.0
    if cls._terminal_fn is _CudaPolicyIterationBase._terminal_fn:
        return np.zeros(len(states), dtype=bool), 0.0
    mask, val = cls._terminal_fn(inst, states)
    return np.asarray(mask, dtype=bool), float(val)


def sample_states(rng, bins, m):
    """Seeded query points: inside the grid, beyond its borders, on nodes, in the edge cells."""
    D = len(bins)
    lo = np.array([b.min() for b in bins], dtype=np.float64)
    hi = np.array([b.max() for b in bins], dtype=np.float64)
    span = hi - lo
    pts = lo + span * rng.uniform(-0.15, 1.15, size=(m, D))
    k = m // 8
    nodes = np.stack([b[rng.integers(0, len(b), size=k)] for b in bins], axis=1)
    pts[:k] = nodes
    pts[k:2 * k] = hi - span * rng.uniform(0, 1e-3, size=(k, D))
    pts[2 * k:3 * k] = lo + span * rng.uniform(0, 1e-3, size=(k, D))
    pts[3 * k] = hi
    pts[3 * k + 1] = lo
    return pts.astype(np.float32)


def bits_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == np.float32 and b.dtype == np.float32:      # bit patterns: +0 != -0, NaN payloads count
        return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    return bool(np.array_equal(a, b))


def assert_bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    if not bits_equal(a, b):
        bad = np.flatnonzero((a != b).ravel())
        raise AssertionError(f"{what}: {len(bad)} of {a.size} entries differ; first at {bad[:5]}: "
                             f"{a.ravel()[bad[:5]]} vs {b.ravel()[bad[:5]]}")


def golden(name: str):
    return np.load(GOLDEN / f"{name}.npz")


# ---- ahead-of-time builds of the units the library hands to hipRTC (the *_do_not_spill and register-budget tests) ----
ROOT = GOLDEN.parents[1]


def kernel_resource_usage(text: str, tmp_path, stem: str = "unit") -> dict:
    """{kernel: {"vgpr", "sgpr", "scratch", "lds"}} of the translation unit `text`, built for gfx950 with the library's
    flags; the figures are the compiler's own (-Rpass-analysis=kernel-resource-usage)."""
    import subprocess
    import __graft_entry__ as G
    src = Path(tmp_path) / f"{stem}.hip"
    src.write_text(text)
    res = subprocess.run([G.HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "--genco",
                          "-include", "hip/hip_runtime.h", "-Rpass-analysis=kernel-resource-usage", str(src),
                          "-o", str(Path(tmp_path) / f"{stem}.hsaco")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    usage, fn = {}, None
    for line in res.stderr.splitlines():
        if "Function Name:" in line:
            fn = line.split("Function Name:")[1].split()[0]
            usage[fn] = {}
        elif fn and " VGPRs:" in line:
            usage[fn]["vgpr"] = int(line.split("VGPRs:")[1].split()[0])
        elif fn and "TotalSGPRs:" in line:
            usage[fn]["sgpr"] = int(line.split("TotalSGPRs:")[1].split()[0])
        elif fn and "ScratchSize" in line:
            usage[fn]["scratch"] = int(line.split(":")[-1].split()[0])
        elif fn and "LDS Size" in line:
            usage[fn]["lds"] = int(line.split(":")[-1].split()[0])
    return usage


def inference_grid(name: str, bins: int):
    """(lo, hi, grid_shape, strides, corner_bits) of the env's grid with `bins` points per dimension, as pi_infer_create
    takes them."""
    from itertools import product
    tabs = env_bins(name, (bins,) * envs.ENVS[name]._D)
    return (*oracle.grid_metadata(tabs), np.array(list(product([0, 1], repeat=len(tabs))), dtype=np.int32))


def inference_unit(grid, plugin, defines: str = "", kernel_files=(), second_grid=None) -> str:
    """The translation unit of a module of the inference handle, restated from the kernel files' headers: `defines`, the
    grid (then `second_grid` as PI2_*, the hybrid's), pi_math.h and the env `plugin` (None: a unit without dynamics has
    neither), then the files of csrc/ in order."""
    def braces(v, fmt):
        return "{" + ",".join(fmt(x) for x in v) + "}"

    def hexf(x):
        return float(np.float32(x)).hex() + "f"

    def grid_defines(prefix, lo, hi, gshape, strides, bits):
        return (f"#define {prefix}_D {len(lo)}\n#define {prefix}_LO_INIT {braces(lo, hexf)}\n"
                f"#define {prefix}_HI_INIT {braces(hi, hexf)}\n#define {prefix}_SHAPE_INIT {braces(gshape, str)}\n"
                f"#define {prefix}_STRIDES_INIT {braces(strides, str)}\n"
                f"#define {prefix}_BITS_INIT {braces(bits, lambda r: braces(r, str))}\n")
    text = defines + grid_defines("PI", *grid)
    if second_grid is not None:
        text += grid_defines("PI2", *second_grid)
    if plugin is not None:
        text += ((ROOT / "include" / "pi_math.h").read_text() + "\n#define sinf pi_sinf\n#define cosf pi_cosf\n"
                 "#define fmodf pi_fmodf\n" + envs.dynamics_source(plugin) + "\n")
    return text + "".join((ROOT / "dynamicprogramming_amd" / "csrc" / f).read_text() + "\n" for f in kernel_files)


# ---- exchange plans pinned to a record (tests/golden/shard_plans.json, tests/golden/make_shard_plans_golden.py) ----
PLAN_INFO_KEYS = ("mode", "recv_elems", "send_elems", "send_ranges", "interior_ranges")      # info[0..4] of pi_exchange_plan
PLAN_SELECTORS = ("PLAN", "REACH_UNITS", "ROW_EXACT", "FUSED", "PAIR_EXACT", "FUSED_VALUES", "FIRST_ENTRIES",
                  "INTERIOR_ENTRIES")


def plan_record(eng, info: dict) -> dict:
    """Everything a rank can say about its exchange plan, as JSON-able data: the five info[] values of
    pi_exchange_plan, pi_plan_ranges and every plan selector of pi_comm_info."""
    from dynamicprogramming_amd._native import CommInfo
    return {"info": [info[k] for k in PLAN_INFO_KEYS], "ranges": [list(r) for r in eng.plan_ranges()],
            "comm_info": {k: int(eng.comm_info(CommInfo[k])) for k in PLAN_SELECTORS}}


def plan_key(transport: str, world: int, name: str, shape, env: dict) -> str:
    """Name of a recorded case.  TEST_* variables steer the test's worker, not the library: they do not name a plan."""
    knobs = ",".join(f"{k}={v}" for k, v in sorted(env.items()) if not k.startswith("TEST_"))
    return f"{transport} world={world} {name} {'x'.join(str(g) for g in shape)} {knobs}"


def golden_plans(key: str) -> list:
    """The recorded plan of every rank of the case `key`."""
    import json
    return json.loads((GOLDEN / "shard_plans.json").read_text())["plans"][key]


def oracle_for(name: str, libm: bool = False) -> oracle.OracleLib:
    return oracle.build(envs.ENVS[name]._D, envs.dynamics_source(name), libm=libm)


def with_checker_backend(cls):
    """Subclass of a solver class whose sweeps run on the CPU checker below instead of the HIP
    backend — for HOST-LOGIC tests only.  The product has exactly one backend and offers no hook to
    swap it: while such a solver is being constructed the test patches the module's own names
    (``solver.HipSweepBackend``, ``solver.GPU_AVAILABLE``) and restores them afterwards."""
    def __init__(self, *args, **kwargs):
        from dynamicprogramming_amd import solver as S
        saved = (S.HipSweepBackend, S.GPU_AVAILABLE)
        S.HipSweepBackend, S.GPU_AVAILABLE = OracleSweepBackend, True
        try:
            cls.__init__(self, *args, **kwargs)
        finally:
            S.HipSweepBackend, S.GPU_AVAILABLE = saved
    return type(cls.__name__ + "OnChecker", (cls,), {"__init__": __init__})


class OracleSweepBackend:
    """CPU stand-in for HipSweepBackend, for HOST-LOGIC tests only (run-loop semantics,
    sharding over gloo ranks).  Lives under tests/ so the product can never pick it up; tests
    install it with ``with_checker_backend``."""

    def __init__(self, D, grid_shape, lo, hi, bins, actions, dynamics_src, device=None, order=None):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        # memory order of the dimensions (solver.MEMORY_ORDER): the "device" arrays the solver hands over are in that
        # order; the checker itself works in the user's order, whole grids only
        self.order = None if order is None else tuple(int(d) for d in order)
        self.lib = oracle.build(int(D), dynamics_src)
        self.lo, self.hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        self.shape = np.asarray(grid_shape, np.int32)
        st = np.ones(int(D), dtype=np.int64)
        for d in range(int(D) - 2, -1, -1):
            st[d] = st[d + 1] * self.shape[d + 1]
        self.strides = st.astype(np.int32)
        self.actions = np.asarray(actions, np.float32)
        self.states = oracle.states_from_bins(bins)
        self.n = len(self.states)
        self.calls = {"eval": 0, "improve": 0}

    def to_memory(self, a):
        if self.order is None:
            return a
        b = a.reshape([int(g) for g in self.shape])
        b = b.permute(*self.order).contiguous() if hasattr(b, "permute") else np.ascontiguousarray(b.transpose(self.order))
        return b.reshape(-1)

    def to_user(self, a):
        if self.order is None:
            return a
        inv = [self.order.index(d) for d in range(len(self.order))]
        b = a.reshape([int(self.shape[d]) for d in self.order])
        b = b.permute(*inv).contiguous() if hasattr(b, "permute") else np.ascontiguousarray(b.transpose(inv))
        return b.reshape(-1)

    def _u(self, t):
        """numpy view (user's order) of a whole-grid device tensor; a copy when the memory order differs."""
        a = t.numpy()[: self.n]
        return a if self.order is None else self.to_user(a)

    def _whole(self, s_begin, s_end):
        assert self.order is None or (s_begin == 0 and s_end == self.n), "memory orders: whole-grid sweeps only"

    def _mask(self, term):
        """The solver passes None for a grid without terminal states (the product then streams no mask)."""
        return np.zeros(self.n, dtype=np.uint8) if term is None else self._u(term)

    def eval_sweeps(self, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta,
                    rebuild=True):
        n = self.n
        self._whole(s_begin, s_end)
        for i in range(n_sweeps):
            src, dst = (Vb, Va) if (i & 1) else (Va, Vb)
            out = np.ascontiguousarray(self._u(dst))
            _, delta = self.lib.eval_sweep(self.states, self.actions, self._u(policy),
                                           self._u(src), self._mask(term), self.lo, self.hi,
                                           self.shape, self.strides, gamma, s_begin, s_end,
                                           out=out)
            dst.numpy()[:n] = self.to_memory(out)
            self.calls["eval"] += 1
            if d_delta is not None and i == n_sweeps - 1:
                d_delta[0] = delta

    def reach_planes(self, term, s_begin, s_end, n_planes):
        """CPU restatement of pi_reach_planes: planes of every successor cell (+1), any action."""
        n = self.n
        out = np.zeros(n_planes, dtype=bool)
        live = ~self._mask(term)[s_begin:s_end].astype(bool)
        st = self.states[s_begin:s_end][live]
        for a in self.actions:
            nxt, _, done = self.lib.step(st, a)
            idx, _ = self.lib.interp(nxt[~done], self.lo, self.hi, self.shape, self.strides)
            planes = np.unique(idx // int(self.strides[0]))
            out[planes] = True
        return out

    def reach_units(self, term, s_begin, s_end, depth):
        """CPU restatement of pi_reach_units: units of the leading `depth` dimensions (planes of
        dimension 0, rows (i0, i1)) holding any corner of any successor cell, any action."""
        n = self.n
        unit = int(self.strides[depth - 1])
        out = np.zeros(n // unit, dtype=bool)
        live = ~self._mask(term)[s_begin:s_end].astype(bool)
        st = self.states[s_begin:s_end][live]
        for a in self.actions:
            nxt, _, done = self.lib.step(st, a)
            idx, _ = self.lib.interp(nxt[~done], self.lo, self.hi, self.shape, self.strides)
            out[np.unique(idx // unit)] = True
        return out

    def improve_sweep(self, V, policy, term, s_begin, s_end, gamma, d_changed):
        n = self.n
        self._whole(s_begin, s_end)
        new_pol, changed = self.lib.improve_sweep(self.states, self.actions, self._u(policy),
                                                  self._u(V), self._mask(term), self.lo, self.hi,
                                                  self.shape, self.strides, gamma, s_begin, s_end)
        if self.order is None:
            policy.numpy()[:n][s_begin:s_end] = new_pol[s_begin:s_end]
        else:
            policy.numpy()[:n] = self.to_memory(new_pol)
        self.calls["improve"] += 1
        if d_changed is not None:
            d_changed[0] = changed

    def value_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta, d_changed):
        n = self.n
        self._whole(s_begin, s_end)
        out = np.ascontiguousarray(self._u(Vnew))
        _, new_pol, delta, changed = self.lib.value_sweep(
            self.states, self.actions, self._u(policy), self._u(V), self._mask(term), self.lo,
            self.hi, self.shape, self.strides, gamma, s_begin, s_end, out=out)
        Vnew.numpy()[:n] = self.to_memory(out)
        if self.order is None:
            policy.numpy()[:n][s_begin:s_end] = new_pol[s_begin:s_end]
        else:
            policy.numpy()[:n] = self.to_memory(new_pol)
        if d_delta is not None:
            d_delta[0] = delta
        if d_changed is not None:
            d_changed[0] = changed

    def close(self):
        pass


# -- reference-EXECUTED dynamics (tests/golden/step_python.npz) -----------------------------------------
# The reference's own float64 `_step_python` mirrors, run in the build container on seeded (state, action)
# pairs (tests/golden/make_step_python_golden.py).  Tolerances of a float32 kernel against a float64 mirror,
# written out once for the CPU and the GPU test:
STEP_PYTHON_ENVS = {            # env -> wrapped angle dimensions (compared on the circle)
    "cartpole_swingup": (2,),
    "double_pendulum_swingup": (0, 2),
    "overhead_crane": (),
    "double_cartpole": (),
    "double_cartpole_swingup": (2, 4),
}
STEP_NEXT_TOL = 1e-5            # |d next| <= tol * max(1, |next|)        (measured 2.3e-6)
STEP_REWARD_TOL = 5e-5          # |d reward| <= tol * max(1, |reward|)    (measured 9.1e-6)
STEP_MARGIN = 1e-4              # flag / reward compared only this far from a comparison threshold


def check_against_step_python(name: str, nxt, rew, done, what: str) -> dict:
    """next state / reward / terminated of an implementation of env `name` on the fixture's inputs, against what
    the reference's own `_step_python` returned for them.  Returns the measured maxima."""
    g = np.load(GOLDEN / "step_python.npz")
    r_next, r_rew = g[f"{name}_next"].astype(np.float64), g[f"{name}_reward"]
    r_term, margin = g[f"{name}_term"], g[f"{name}_margin"]
    far = margin > STEP_MARGIN
    d = np.asarray(nxt, np.float64) - r_next
    for k in STEP_PYTHON_ENVS[name]:
        d[:, k] = (d[:, k] + np.pi) % (2.0 * np.pi) - np.pi
    e_next = float(np.abs(d / np.maximum(1.0, np.abs(r_next))).max())
    assert e_next <= STEP_NEXT_TOL, f"{what} {name}: next state off by {e_next:.3g} (relative)"
    done = np.asarray(done, bool)
    bad = np.flatnonzero((done != r_term) & far)
    assert len(bad) == 0, f"{what} {name}: terminated differs at {bad[:5]} away from every threshold"
    rew = np.asarray(rew, np.float64)
    if name == "double_cartpole":
        # the reference's kernel string has reward 1 - 0.0 * xn^2 (double_cartpole_cuda.py:98,:163)
        # while its Python mirror kept 1 - 0.5 * (nx / 2.4)^2 (:234).  The kernel string is the ground truth of the
        # sweep; the mirror pins next state and flag, and the reward through the mirror's own formula un-drifted.
        r_rew = r_rew + 0.5 * (r_next[:, 0] / 2.4) ** 2
    e_rew = float((np.abs(rew - r_rew) / np.maximum(1.0, np.abs(r_rew)))[far].max())
    assert e_rew <= STEP_REWARD_TOL, f"{what} {name}: reward off by {e_rew:.3g} (relative)"
    return {"next": e_next, "reward": e_rew, "flags_compared": int(far.sum()), "pairs": len(far)}


def schedule_groups(sched: dict, n_chunks: int) -> np.ndarray:
    """Host restatement of the kernels' workgroup -> group map (pi_first_chunk in csrc/pi_sweep_kernels.hip): the group
    every workgroup of the launch `sched` (Engine.plan_schedule) takes, in dispatch order (x fastest), -1 for a workgroup
    that leaves at once.  Column 1 is the XCD (dispatch index mod 8)."""
    gx, gy, T, phase, cpw = (sched[k] for k in ("grid_x", "grid_y", "period", "phase", "cpw"))
    assert gx % 8 == 0
    b = np.arange(gx * gy, dtype=np.int64)
    bx, p = b % gx, b // gx
    x, r = bx % 8, bx // 8
    if T == 0:                                  # slab schedule: XCD x walks the x-th contiguous run of groups
        assert gy == 1
        g = x * (gx // 8) + r
        valid = np.ones(len(b), dtype=bool)
    else:                                       # strip schedule: y = period, XCD x takes its eighth of it
        lo8 = x * T + ((p * 3) & 7)
        b0, b1 = lo8 >> 3, (lo8 + T) >> 3
        g = p * T + b0 + r - phase
        valid = (r < b1 - b0) & (g >= 0)
    valid &= g * cpw < n_chunks
    return np.stack([np.where(valid, g, -1), b % 8], axis=1)


# -- dispatch thresholds and degenerate grids (tests/test_edge_dispatch.py, tests/test_gpu_edges.py) ---------------------
def edge_actions(name: str, actions=None) -> np.ndarray:
    return np.asarray(envs.ENVS[name].ACTIONS if actions is None else actions, np.float32)


def table_floats(name: str, shape, actions=None) -> int:
    """Floats pi_stage_table copies to LDS for this specialisation: the actions and every dimension's bin table."""
    return len(edge_actions(name, actions)) + int(sum(int(g) for g in shape))


# What pi_create must decide at every threshold of its dispatch, WRITTEN OUT from the design (the comments on
# the launch geometry and the one-launch kernels in csrc/pi_api.cpp's choose_dispatch), not computed by the code under test: a
# threshold that moves has to be moved here as well, on purpose.  Per row: env, shape, then
#   k        states per thread of the LDS-resident kernels (Info.RESIDENT_STATES_PER_THREAD; 0: not resident).  Limits
#            12 288 (2-D, 1024 threads), 4 096 (4-D, 512 threads), 1 024 (6-D, 512 threads); k = ceil(n / threads)
#   flow     pi_eval_flow_kernel is built: 2-D and 4-D, resident limit < n <= 2^17 (2-D: from 4 096 < n where the
#            XCD-local kernel is wanted)
#   xcd_s    states per workgroup of pi_xcd_kernel, None where it is not built: 2-D, 4 096 < n <= 2^16;
#            ceil(ceil(n / 32) / 32) * 32 (n over the 32 CUs of an XCD, whole 128-byte lines)
#   eb, ib   threads per workgroup of the evaluation / improvement sweeps: 1024 / 512 on 2-D and 4-D grids of >= 2^24
#            states, 256 / 256 otherwise
#   ecpw, icpw  chunks per workgroup: evaluation 2 from 2^20 states on; 6-D grids of >= 2^24 states 4 and 3
#   placed   (rows with flow) whether a 256-CU MI355X HAS the dataflow kernel after loading it: all ceil(n / 256) workgroups
#            must be resident at once within 3/4 (rounded down) of the occupancy the runtime reports.  The 2-D plugins are
#            reported 3 or more workgroups per CU and place 512; every 4-D plugin is reported 2, which leaves ONE per CU:
#            256 workgroups, 2^16 states.  pi_create's 4-D limit of 2^17 is therefore never reached on this device
#            (measured: cartpole, cartpole_swingup, double_pendulum_swingup and overhead_crane are all placed at 16^4 and
#            all refused at 16.16.16.24 and 16.16.16.32); the refusals are pinned as such, the sweeps serve those grids
#   live     (rows whose solver path is run) whether the solver's sweeps go through a live-state list: from 2^20 states
#            on (PI_MI355_LIVE_MIN), on grids with terminal states, where at least 3 % of the lanes of the waves that
#            hold a live state are dead (pi_prepare_mask).  The list then holds every non-terminal state
DISPATCH_TABLE = [
    # resident limit, 2-D (12 288) — both sides lie inside the XCD window
    dict(name="mountain_car", shape=(96, 128), k=12, flow=True, xcd_s=384, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="mountain_car", shape=(97, 127), k=0, flow=True, xcd_s=416, eb=256, ib=256, ecpw=1, icpw=1),
    # XCD_MIN (4 096): at the limit one CU serves the grid alone, one state more and the XCD-local kernel is preferred
    dict(name="pendulum", shape=(64, 64), k=4, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="pendulum", shape=(64, 65), k=5, flow=True, xcd_s=160, eb=256, ib=256, ecpw=1, icpw=1),
    # XCD_MAX (2^16)
    dict(name="pendulum", shape=(256, 256), k=0, flow=True, xcd_s=2048, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="pendulum", shape=(256, 257), k=0, flow=True, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    # dataflow kernel, 2-D (2^17)
    dict(name="mountain_car", shape=(256, 512), k=0, flow=True, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="mountain_car", shape=(363, 362), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    # dataflow kernel, 4-D (2^17)
    dict(name="cartpole_swingup", shape=(16, 16, 16, 32), k=0, flow=True, placed=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="cartpole_swingup", shape=(16, 16, 16, 33), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    # ... and where the 4-D dataflow kernel stops being placed on 256 CUs: one workgroup per CU
    dict(name="cartpole_swingup", shape=(16, 16, 16, 16), k=0, flow=True, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="cartpole_swingup", shape=(16, 16, 16, 17), k=0, flow=True, placed=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    # resident limit, 4-D (4 096): beyond it the dataflow kernel
    dict(name="cartpole", shape=(8, 8, 8, 8), k=8, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="cartpole", shape=(8, 8, 8, 9), k=0, flow=True, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    # resident limit, 6-D (1 024): beyond it no one-launch kernel at all
    dict(name="double_cartpole", shape=(2, 2, 4, 4, 4, 4), k=2, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    dict(name="double_cartpole", shape=(2, 2, 4, 4, 4, 5), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1),
    # 2^20: two chunks per evaluation workgroup, and the live-state list (which only a device can build: `live`)
    dict(name="cartpole", shape=(32, 32, 32, 31), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1, live=False),
    dict(name="cartpole", shape=(32, 32, 32, 32), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=True),
    dict(name="double_cartpole", shape=(8, 8, 8, 8, 16, 15), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=1, icpw=1, live=False),
    dict(name="double_cartpole", shape=(8, 8, 8, 8, 16, 16), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=True),
    # ... cartpole_swingup has terminal states too, but whole rows of them: no wave mixes live and dead lanes, no list
    dict(name="cartpole_swingup", shape=(32, 32, 32, 32), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=False),
    # 2^22: nothing changes in pi_create; the solver applies / measures a memory order (SOLVER_ORDER_TABLE)
    dict(name="double_pendulum_swingup", shape=(64, 64, 32, 31), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=False),
    dict(name="double_pendulum_swingup", shape=(64, 64, 32, 32), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=False),
    # 2^24, 4-D: 1024- and 512-thread workgroups
    dict(name="double_pendulum_swingup", shape=(64, 64, 64, 63), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=False),
    dict(name="double_pendulum_swingup", shape=(64, 64, 64, 64), k=0, flow=False, xcd_s=None, eb=1024, ib=512, ecpw=2, icpw=1, live=False),
    # 2^24, 6-D: four and three chunks per workgroup
    dict(name="double_cartpole", shape=(16, 16, 16, 16, 16, 15), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=2, icpw=1, live=True),
    dict(name="double_cartpole", shape=(16, 16, 16, 16, 16, 16), k=0, flow=False, xcd_s=None, eb=256, ib=256, ecpw=4, icpw=3, live=True),
]

# (env, shape) -> the memory order a single-rank solver takes WITHOUT measuring anything: the class's own MEMORY_ORDER
# from 2^22 states on (solver._ORDER_MIN_STATES), the env's order (None) below.
SOLVER_ORDER_TABLE = [
    ("double_pendulum_swingup", (64, 64, 32, 31), None), ("double_pendulum_swingup", (64, 64, 32, 32), (0, 2, 1, 3)),
    ("double_cartpole", (8, 8, 8, 16, 16, 31), None), ("double_cartpole", (8, 8, 8, 16, 16, 32), (5, 4, 2, 3, 0, 1)),
]

_PENDULUM_BEYOND_CLAMP_64 = np.linspace(-3.0, 3.0, 64, dtype=np.float32)      # 11 entries <= -2 and 11 >= 2: exact ties in Q
_PENDULUM_BEYOND_CLAMP_257 = np.linspace(-4.0, 4.0, 257, dtype=np.float32)    # 65 + 65 of them clamp

# The degenerate specialisations: (id, env, shape, actions or None for the env's own).  21 pendulum torques: the tables
# of (2, 2025) hold exactly 2048 floats (the last size staged through registers at 256 threads), (2, 2026) 2049 (the
# first one through the strided loop), (2, 15337) 15 360 (pi_create's limit).  2.2.2.1500 with its 11 actions holds 1517
# floats and does NOT reach the strided loop; 2.2.2.2100 (2117) is the 4-D case that does.  257 is prime and no grid has 257 states:
# 258 and 259 stand in for it, 1025 = 256 * 4 + 1.  With the envs' own bounds every node of the 2-bin cartpole and 6-D
# grids is terminal (x = +-bound): those cases pin that such a grid is copied through, the 2-D and double-pendulum ones sweep.
EDGE_CASES = [
    ("all2-2d", "pendulum", (2, 2), None), ("all2-4d", "double_pendulum_swingup", (2, 2, 2, 2), None),
    ("all2-4d-terminal", "cartpole", (2, 2, 2, 2), None), ("all2-6d", "double_cartpole_swingup", (2,) * 6, None),
    ("one2-slowest", "pendulum", (2, 3000), None), ("one2-fastest", "mountain_car", (3000, 2), None),
    ("one2-4d", "double_pendulum_swingup", (2, 2, 2, 1500), None),
    ("one2-4d-strided", "double_pendulum_swingup", (2, 2, 2, 2100), None),
    ("tab2048", "pendulum", (2, 2025), None), ("tab2049", "pendulum", (2, 2026), None),
    ("tab15360", "pendulum", (2, 15337), None),
    ("n63", "mountain_car", (7, 9), None), ("n255", "pendulum", (15, 17), None), ("n256", "mountain_car", (16, 16), None),
    ("n258", "pendulum", (6, 43), None), ("n259", "mountain_car", (37, 7), None),
    ("n513-4d", "cartpole", (3, 3, 3, 19), None), ("n1025", "pendulum", (25, 41), None),
    ("act1", "pendulum", (33, 29), np.array([0.5], np.float32)), ("act1-4d", "cartpole", (5, 4, 6, 3), np.array([10.0], np.float32)),
    ("act2", "pendulum", (33, 29), np.array([-2.5, 2.5], np.float32)),
    ("act64", "pendulum", (33, 29), _PENDULUM_BEYOND_CLAMP_64), ("act257", "pendulum", (21, 13), _PENDULUM_BEYOND_CLAMP_257),
]
# case id -> (k, flow, xcd_s) of the degenerate specialisations, by the rules in front of DISPATCH_TABLE (all of them
# sweep with 256-thread workgroups, one chunk each; every dataflow kernel among them is placed: at most 120 workgroups)
EDGE_DISPATCH = {
    "all2-2d": (1, False, None), "all2-4d": (1, False, None), "all2-4d-terminal": (1, False, None), "all2-6d": (1, False, None),
    "one2-slowest": (6, True, 192), "one2-fastest": (6, True, 192), "one2-4d": (0, True, None), "one2-4d-strided": (0, True, None),
    "tab2048": (4, False, None), "tab2049": (4, False, None), "tab15360": (0, True, 960),
    "n63": (1, False, None), "n255": (1, False, None), "n256": (1, False, None), "n258": (1, False, None), "n259": (1, False, None),
    "n513-4d": (2, False, None), "n1025": (2, False, None),
    "act1": (1, False, None), "act1-4d": (1, False, None), "act2": (1, False, None), "act64": (1, False, None), "act257": (1, False, None),
}
EDGE_ROWS = [dict(name=name, shape=shape, actions=acts, k=EDGE_DISPATCH[cid][0], flow=EDGE_DISPATCH[cid][1],
                  xcd_s=EDGE_DISPATCH[cid][2], eb=256, ib=256, ecpw=1, icpw=1) for cid, name, shape, acts in EDGE_CASES]
THRESHOLD_CASES = [("x".join(str(g) for g in row["shape"]) + "-" + row["name"], row["name"], row["shape"], None) for row in DISPATCH_TABLE]


def edge_case_params():
    """pytest parameters (case id, env, shape, actions) of every specialisation both edge modules go through."""
    import pytest
    return [pytest.param(*c, id=c[0] if c[0].endswith(c[1]) else f"{c[0]}-{c[1]}") for c in EDGE_CASES + THRESHOLD_CASES]


def host_engine(name: str, shape, actions=None):
    """A handle without a device (pi_create's device -1): dispatch decisions and hipRTC compiles only."""
    from dynamicprogramming_amd import _native
    bins = env_bins(name, shape)
    return _native.Engine(envs.ENVS[name]._D, [len(b) for b in bins], [b.min() for b in bins], [b.max() for b in bins],
                          bins, edge_actions(name, actions), device=-1)


def backup_float64(chk, bins, actions, V, gamma):
    """Plain float64 statement of the backup on the grid `bins`: Q[a, s] = r + gamma * E, E the multilinear interpolation
    of V over the 2^D corners of the successor's cell (0 for a `done` successor).  Successor, reward and flag come from
    the oracle's `step`; position, cell, weights and sums are numpy float64."""
    D = len(bins)
    shape = [len(b) for b in bins]
    lo = np.array([np.float32(b.min()) for b in bins], np.float64)
    hi = np.array([np.float32(b.max()) for b in bins], np.float64)
    states = oracle.states_from_bins(bins)
    V64 = np.asarray(V, np.float64).reshape(shape)
    Q = np.empty((len(actions), len(states)), np.float64)
    for a, u in enumerate(actions):
        nxt, rew, done = chk.step(states, np.float32(u))
        cell, frac = [], []
        for d in range(D):
            t = np.clip((nxt[:, d].astype(np.float64) - lo[d]) / (hi[d] - lo[d]) * (shape[d] - 1), 0.0, shape[d] - 1.0)
            i = np.minimum(np.floor(t).astype(np.int64), shape[d] - 2)
            cell.append(i)
            frac.append(t - i)
        E = np.zeros(len(states), np.float64)
        for corner in range(1 << D):
            w = np.ones(len(states), np.float64)
            at = []
            for d in range(D):
                bit = (corner >> (D - 1 - d)) & 1
                w = w * (frac[d] if bit else 1.0 - frac[d])
                at.append(cell[d] + bit)
            E += w * V64[tuple(at)]
        Q[a] = rew.astype(np.float64) + float(gamma) * np.where(done, 0.0, E)
    return Q
