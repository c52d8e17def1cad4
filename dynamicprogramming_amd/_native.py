"""
ctypes binding of libpi_mi355.so (C ABI: include/pi_mi355.h).

The library is the only compute path of this package.  There is no CPU or eager
fallback: if the shared object is missing or fails to load, importing this module
still succeeds (so ``load()``-only workflows work on machines without ROCm) but
``lib()`` raises, and so does every solver constructor.
"""
from __future__ import annotations

import ctypes
import enum
from pathlib import Path

import numpy as np

from . import _knobs

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libpi_mi355.so"
KERNEL_CACHE = Path(_knobs.read("KERNEL_CACHE"))

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); must list every symbol include/pi_mi355.h declares.
SIGNATURES = {
    "pi_abi_version": (ctypes.c_int, []),
    "pi_last_error": (ctypes.c_char_p, []),
    "pi_create": (_vp, [ctypes.c_int, ctypes.c_int, _i32p, _f32p, _f32p,
                        ctypes.POINTER(_f32p), _f32p, ctypes.c_int]),
    "pi_destroy": (None, [_vp]),
    "pi_compile": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                  ctypes.c_size_t]),
    "pi_kernel_source": (ctypes.c_size_t, [_vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_eval_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                     ctypes.c_float, _vp, _vp]),
    "pi_eval_sweeps": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_float, ctypes.c_int, _vp, _vp]),
    "pi_policy_evaluation": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_double, ctypes.c_int,
                                            ctypes.c_int, _vp, _vp, _vp, _vp]),
    "pi_policy_iteration": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_double, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "pi_improve_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                        ctypes.c_float, _vp, _vp]),
    "pi_value_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_float, _vp, _vp, _vp]),
    "pi_set_disturbances": (ctypes.c_int, [_vp, ctypes.c_int, _f32p, _f32p, _f32p]),
    "pi_expect_eval_sweeps": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_float, ctypes.c_int, _vp, _vp]),
    "pi_expect_improve_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_float, _vp, _vp]),
    "pi_expect_value_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_float, _vp, _vp, _vp]),
    "pi_robust_eval_sweeps": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_float, ctypes.c_int, _vp, _vp]),
    "pi_robust_improve_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_float, _vp, _vp]),
    "pi_robust_value_sweep": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_float, _vp, _vp, _vp]),
    "pi_accel_update": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int64, _vp, _vp]),
    "pi_accel_combine": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_int64, _vp,
                                        _vp]),
    "pi_reach_planes": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _vp, _vp]),
    "pi_reach_depth_max": (ctypes.c_int, [_vp]),
    "pi_reach_units": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _vp, _vp]),
    "pi_comm_unique_id": (ctypes.c_int, [_vp]),
    "pi_comm_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "pi_comm_init_local": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    "pi_p2p_describe": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp]),
    "pi_comm_init_p2p": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_char_p]),
    "pi_p2p_compile_check": (ctypes.c_int, [ctypes.c_char_p]),
    "pi_comm_destroy": (ctypes.c_int, [_vp]),
    "pi_comm_info": (ctypes.c_int, [_vp, ctypes.c_int]),
    "pi_allgather_V": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp]),
    "pi_allgather_policy": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp]),
    "pi_allreduce_max_f32": (ctypes.c_int, [_vp, _vp, _vp]),
    "pi_allreduce_sum_u32": (ctypes.c_int, [_vp, _vp, _vp]),
    "pi_plan_segments": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_int64, _vp, _vp, ctypes.c_int64]),
    "pi_exchange_plan": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "pi_plan_ranges": (ctypes.c_int64, [_vp, _vp, ctypes.c_int64]),
    "pi_exchange_V": (ctypes.c_int, [_vp, _vp, _vp]),
    "pi_eval_sweep_part": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_float, _vp]),
    "pi_eval_sweeps_sharded": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_int,
                                              _vp, _vp]),
    "pi_improve_sweep_sharded": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp]),
    "pi_probe_step": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp]),
    "pi_probe_interp": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp]),
    "pi_probe_coords": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_int, _vp]),
    "pi_infer_create": (_vp, [ctypes.c_int, ctypes.c_int, _f32p, _f32p, _i32p, _i32p, _i32p, ctypes.c_int64,
                              ctypes.c_char_p]),
    "pi_infer_destroy": (None, [_vp]),
    "pi_infer_set_policy": (ctypes.c_int, [_vp, _i32p, ctypes.c_int64, _f32p, ctypes.c_int]),
    "pi_infer_query": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "pi_infer_set_dynamics": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_rollout": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, _vp, _vp, _vp, _vp,
                                        _vp, ctypes.c_int, _vp]),
    "pi_infer_set_partner": (ctypes.c_int, [_vp, _vp, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_rollout_hybrid": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, _f32p, _f32p,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "pi_infer_set_values": (ctypes.c_int, [_vp, _f32p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_resample": (ctypes.c_int, [_vp, _i32p, ctypes.POINTER(ctypes.c_int64), _f32p, _i32p, ctypes.c_int, _vp, _vp,
                                         _vp, _vp]),
    "pi_infer_set_greedy": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_greedy": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp, _vp, _vp]),
    "pi_infer_rollout_greedy": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                               _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "pi_infer_set_stochastic": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_rollout_stochastic": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                   ctypes.c_float, _f32p, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, _vp,
                                                   _vp, _vp, ctypes.c_int, _vp]),
    "pi_infer_random_words": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32,
                                             ctypes.c_uint32, _vp, _vp]),
    "pi_infer_set_expect_greedy": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_set_disturbances": (ctypes.c_int, [_vp, ctypes.c_int, _f32p, _f32p, _f32p]),
    "pi_infer_expect_greedy": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp, _vp, _vp]),
    "pi_infer_set_robust": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_robust": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pi_infer_rollout_adversary": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                  ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "pi_infer_rollout_expect_greedy": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                      ctypes.c_float, ctypes.c_float, _f32p, ctypes.c_uint64, ctypes.c_uint64,
                                                      _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "pi_infer_set_partner_stochastic": (ctypes.c_int, [_vp, _vp, _f32p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "pi_infer_rollout_hybrid_stochastic": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_float, _f32p,
                                                          _f32p, ctypes.c_float, ctypes.c_float, _f32p, ctypes.c_uint64,
                                                          ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                          ctypes.c_int, _vp]),
    "pi_plan_schedule": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_uint64)]),
    "pi_set_option": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64]),
    "pi_info": (ctypes.c_int64, [_vp, ctypes.c_int]),
    "pi_debug_report": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32)]),
    "pi_prepare_mask": (ctypes.c_int, [_vp, _vp, _vp]),
    "pi_prepare_mask_range": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp]),
    "pi_live_list": (ctypes.c_int64, [_vp, _vp, ctypes.c_int64, _vp]),
    "pi_eval_begin": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "pi_eval_end": (ctypes.c_int, [_vp]),
}

ABI_VERSION = 12
_lib = None
_load_error: Exception | None = None


# Selector codes of pi_info / pi_set_option / pi_comm_info and the categories they report: a literal copy of the
# enums of include/pi_mi355.h, which documents every member (tests/test_native_abi.py checks that the two agree).
class Info(enum.IntEnum):
    """enum pi_info_code (PI_INFO_*): the `what` of Engine.info."""
    N_STATES = 0
    N_ACTIONS = 1
    DIMS = 2
    EVAL_CPW = 3
    EVAL_VGPRS = 4
    IMPROVE_VGPRS = 5
    COMPUTE_UNITS = 6
    CACHE_HIT = 7
    IMPROVE_CPW = 8
    CACHED_GRAPHS = 9
    GRAPHS_ENABLED = 10
    EVAL_BLOCK = 11
    IMPROVE_BLOCK = 12
    RESIDENT_STATES_PER_THREAD = 13
    RESIDENT_ENABLED = 14
    DEBUG_CHECKS = 15
    LIVE_STATES = 16
    EVAL_LIST_ENTRIES = 17
    MEMORY_ORDER = 18
    FLOW_WORKGROUPS = 19
    RECIPROCAL_DIV = 20         # base: RECIPROCAL_DIV + d for dimension d < D
    XCD_ENABLED = 30
    XCD_EVALUATIONS = 31
    XCD_FALLBACKS = 32
    WHOLE_RUNS = 33
    WHOLE_RUN_AVAILABLE = 34
    STRIP_STATES = 35
    PAIR_TABLE = 37
    DISTURBANCES = 38


class Option(enum.IntEnum):
    """enum pi_option_code (PI_OPTION_*): the `what` of Engine.set_option."""
    EVAL_CPW = 0
    IMPROVE_CPW = 1
    GRAPHS = 2
    RESIDENT = 3
    MEMORY_ORDER = 4
    BUILD_PUSH = 5
    KEEP_LIVE_LIST = 6
    STRIP_STATES = 7
    XCD_RUN_FAILED = 8
    PAIR_TABLE = 9


class XcdFailure(enum.IntEnum):
    """enum pi_xcd_failure (PI_XCD_FAILURE_*): the values of Option.XCD_RUN_FAILED."""
    COUNT = 1
    SWITCH_OFF = 2


class CommInfo(enum.IntEnum):
    """enum pi_comm_info_code (PI_COMM_INFO_*): the `what` of Engine.comm_info."""
    RANK = 0
    WORLD = 1
    TRANSPORT = 2
    PLAN = 3
    REACH_UNITS = 4
    ROW_EXACT = 5
    FUSED = 6
    PAIR_EXACT = 7
    FUSED_VALUES = 8
    FIRST_ENTRIES = 9
    INTERIOR_ENTRIES = 10


class Transport(enum.IntEnum):
    """enum pi_transport (PI_TRANSPORT_*): CommInfo.TRANSPORT."""
    RCCL = 1
    IN_PROCESS = 2
    P2P = 3


class Plan(enum.IntEnum):
    """enum pi_plan (PI_PLAN_*): CommInfo.PLAN, and the `mode` of Engine.exchange_plan (NONE: let the library choose)."""
    NONE = 0
    ALLGATHER = 1
    HALO = 2


class ReachUnits(enum.IntEnum):
    """enum pi_reach_unit (PI_REACH_*): CommInfo.REACH_UNITS, the `depth` of Engine.reach_units."""
    PLANES = 1
    ROWS = 2


class NativeError(RuntimeError):
    pass


def kernel_source_hash() -> str:
    """Fingerprint of the device code (kernel template + math header): profiles record it so that
    counters measured on one version of the kernels are never quoted for another (bench.py)."""
    import hashlib
    h = hashlib.sha256()
    for path in (_PKG / "csrc" / "pi_sweep_kernels.hip", _PKG.parent / "include" / "pi_math.h"):
        h.update(path.read_bytes())
    return h.hexdigest()[:16]


def lib() -> ctypes.CDLL:
    """The loaded library; raises NativeError (never falls back) when unavailable."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise NativeError(str(_load_error)) from _load_error
    try:
        # torch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Two HIP runtimes in
        # one process do not work ("no ROCm-capable device"), so make sure torch's copy is the
        # one already mapped before ours is resolved: device pointers and streams handed
        # across the C ABI then belong to the same runtime.
        import torch  # noqa: F401
        if not LIB_PATH.exists():
            raise FileNotFoundError(
                f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; "
                f"g.build()'` or `make -C dynamicprogramming_amd/csrc`")
        handle = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.pi_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libpi_mi355 ABI {handle.pi_abi_version()} != binding {ABI_VERSION}")
        _lib = handle
        return _lib
    except Exception as exc:  # noqa: BLE001 - recorded and re-raised on every call
        _load_error = exc
        raise NativeError(f"libpi_mi355.so unavailable: {exc}") from exc


def available() -> bool:
    try:
        lib()
        return True
    except NativeError:
        return False


def last_error() -> str:
    return lib().pi_last_error().decode(errors="replace")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise NativeError(f"{what} failed: {last_error()}")


def p2p_compile_check(cache_dir: Path | str | None = KERNEL_CACHE) -> None:
    """The peer-to-peer transport's device code builds for gfx950 (needs no GPU; fills the kernel cache)."""
    cdir = None
    if cache_dir is not None:
        Path(cache_dir).mkdir(parents=True, exist_ok=True)
        cdir = str(cache_dir).encode()
    _check(lib().pi_p2p_compile_check(cdir), "pi_p2p_compile_check")


def comm_unique_id() -> bytes:
    """A fresh 128-byte RCCL id (create on one rank, hand to every rank's `Engine.comm_init`)."""
    buf = ctypes.create_string_buffer(128)
    _check(lib().pi_comm_unique_id(buf), "pi_comm_unique_id")
    return buf.raw


def plan_segments(world, g0, stride0, n_states, per, reach) -> np.ndarray:
    """Host-only planner of the halo exchange (pi_plan_segments): reach is a (world, g0) bool
    array over g0 units of stride0 consecutive states each (planes of dimension 0, or rows
    (i0, i1)); returns an (m, 4) int64 array of {src, dst, a, b}."""
    r = np.ascontiguousarray(reach, dtype=np.uint8)
    assert r.shape == (world, g0)
    fn = lib().pi_plan_segments
    m = fn(world, g0, stride0, n_states, per, r.ctypes.data_as(_vp), None, 0)
    if m < 0:
        raise NativeError(f"pi_plan_segments failed: {last_error()}")
    out = np.zeros((max(int(m), 1), 4), dtype=np.int64)
    fn(world, g0, stride0, n_states, per, r.ctypes.data_as(_vp), out.ctypes.data_as(_vp), int(m))
    return out[: int(m)]


class Engine:
    """One pi_handle: a grid + action set + (after compile) its specialised kernels."""

    def __init__(self, D, grid_shape, lo, hi, bins, actions, device: int = -1, order=None):
        """`order` (optional): memory order of the dimensions — order[k] is the user dimension stored as memory
        dimension k, 0 = slowest (Option.MEMORY_ORDER).  Every flat state index and every device array of this engine
        is then in that order (`to_memory` / `to_user` convert whole-grid arrays); results do not depend on it."""
        L = lib()
        self.D = int(D)
        self._shape = np.ascontiguousarray(grid_shape, dtype=np.int32)
        self._lo = np.ascontiguousarray(lo, dtype=np.float32)
        self._hi = np.ascontiguousarray(hi, dtype=np.float32)
        self._bins = [np.ascontiguousarray(b, dtype=np.float32) for b in bins]
        self._actions = np.ascontiguousarray(actions, dtype=np.float32)
        assert len(self._bins) == self.D and all(len(b) == g for b, g in zip(self._bins, self._shape))
        arr = (_f32p * self.D)(*[b.ctypes.data_as(_f32p) for b in self._bins])
        self._h = L.pi_create(int(device), self.D, self._shape.ctypes.data_as(_i32p),
                              self._lo.ctypes.data_as(_f32p), self._hi.ctypes.data_as(_f32p), arr,
                              self._actions.ctypes.data_as(_f32p), len(self._actions))
        if not self._h:
            raise NativeError(f"pi_create failed: {last_error()}")
        self.device = int(device)
        self.n_states = self.info(Info.N_STATES)
        self.compile_log = ""
        self.order = tuple(range(self.D))
        if order is not None and tuple(int(d) for d in order) != self.order:
            order = tuple(int(d) for d in order)
            if sorted(order) != list(range(self.D)):
                raise NativeError(f"memory order {order} is not a permutation of the {self.D} dimensions")
            self.set_option(Option.MEMORY_ORDER, sum(d << (3 * k) for k, d in enumerate(order)))
            self.order = order

    # -- memory order of the dimensions ----------------------------------------
    def to_memory(self, a):
        """A whole-grid array (numpy or torch, n_states entries, the user's row-major order) in this engine's
        memory order.  The identity when no order was given."""
        if self.order == tuple(range(self.D)):
            return a
        shape = [int(g) for g in self._shape]
        b = a.reshape(shape)
        b = b.permute(*self.order) if hasattr(b, "permute") else b.transpose(self.order)
        return b.reshape(-1) if not hasattr(b, "contiguous") else b.contiguous().reshape(-1)

    def to_user(self, a):
        """The inverse of `to_memory`."""
        if self.order == tuple(range(self.D)):
            return a
        shape = [int(self._shape[d]) for d in self.order]
        inv = [self.order.index(d) for d in range(self.D)]
        b = a.reshape(shape)
        b = b.permute(*inv) if hasattr(b, "permute") else b.transpose(inv)
        return b.reshape(-1) if not hasattr(b, "contiguous") else b.contiguous().reshape(-1)

    # -- compilation ---------------------------------------------------------
    def kernel_source(self, dynamics_src: str) -> str:
        L = lib()
        src = dynamics_src.encode()
        n = L.pi_kernel_source(self._h, src, None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        L.pi_kernel_source(self._h, src, buf, n + 1)
        return buf.value.decode()

    def compile(self, dynamics_src: str, cache_dir: Path | str | None = KERNEL_CACHE) -> None:
        L = lib()
        log = ctypes.create_string_buffer(1 << 16)
        cdir = None
        if cache_dir is not None:
            Path(cache_dir).mkdir(parents=True, exist_ok=True)
            cdir = str(cache_dir).encode()
        rc = L.pi_compile(self._h, dynamics_src.encode(), cdir, log, len(log))
        self.compile_log = log.value.decode(errors="replace")
        if rc != 0:
            raise NativeError(f"kernel compilation failed:\n{last_error()}")

    def info(self, what: int) -> int:
        return int(lib().pi_info(self._h, what))

    def prepare_mask(self, term, stream=0, s_begin=None, s_end=None) -> int:
        """Let later sweeps of a batch visit only the non-terminal states of the mask at `term` (0 drops the list);
        [s_begin, s_end) restricts the list to a rank's shard.  Returns the number of live states listed, 0 when
        the library keeps none."""
        if s_begin is None:
            _check(lib().pi_prepare_mask(self._h, term or None, stream or None), "pi_prepare_mask")
        else:
            _check(lib().pi_prepare_mask_range(self._h, term or None, int(s_begin), int(s_end), stream or None),
                   "pi_prepare_mask_range")
        return self.info(Info.LIVE_STATES)

    def live_list(self, d_out=0, capacity=0, stream=0) -> int:
        """Copy the live-state list into the device buffer at `d_out` (`capacity` int32 entries); returns its length
        (0: the library keeps no list).  Without a buffer: the length only."""
        m = int(lib().pi_live_list(self._h, d_out or None, int(capacity), stream or None))
        if m < 0:
            raise NativeError(f"pi_live_list failed: {last_error()}")
        return m

    def eval_begin(self, policy, term, stream=0) -> int:
        """Start of one policy evaluation under the policy at `policy`: returns the length of the shorter list the
        following whole-grid batches may use (0: none).  Pair with eval_end()."""
        _check(lib().pi_eval_begin(self._h, policy, term or None, stream or None), "pi_eval_begin")
        return self.info(Info.EVAL_LIST_ENTRIES)

    def eval_end(self) -> None:
        _check(lib().pi_eval_end(self._h), "pi_eval_end")

    def debug_report(self) -> dict:
        """Checked build only (PI_MI355_DEBUG=1 when the engine was created): index violations of the sweeps
        launched since the last report — {"violations", "kind" (1 policy entry, 2 cell), "where", "value"}."""
        out = (ctypes.c_uint32 * 4)()
        _check(lib().pi_debug_report(self._h, out), "pi_debug_report")
        return {"violations": int(out[0]), "kind": int(out[1]), "where": int(out[2]), "value": int(out[3])}

    # -- launches (raw device pointers; all asynchronous on `stream`) ---------
    def eval_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta=0, stream=0):
        _check(lib().pi_eval_sweep(self._h, V, Vnew, policy, term, s_begin, s_end, gamma,
                                   d_delta or None, stream or None), "pi_eval_sweep")

    def eval_sweeps(self, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta=0, stream=0):
        _check(lib().pi_eval_sweeps(self._h, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps,
                                    d_delta or None, stream or None), "pi_eval_sweeps")

    def policy_evaluation(self, V, policy, term, gamma, theta, max_sweeps, check_interval, d_sweeps, d_delta,
                          d_residual_log, stream=0):
        _check(lib().pi_policy_evaluation(self._h, V, policy, term, gamma, float(theta), int(max_sweeps),
                                          int(check_interval), d_sweeps, d_delta or None, d_residual_log,
                                          stream or None), "pi_policy_evaluation")

    def policy_iteration(self, V, policy, term, gamma, theta, max_eval_sweeps, check_interval, max_pi_iter, d_result,
                         d_iter_log, stream=0):
        _check(lib().pi_policy_iteration(self._h, V, policy, term, gamma, float(theta), int(max_eval_sweeps),
                                         int(check_interval), int(max_pi_iter), d_result, d_iter_log, stream or None),
               "pi_policy_iteration")

    def improve_sweep(self, V, policy, term, s_begin, s_end, gamma, d_changed=0, stream=0):
        _check(lib().pi_improve_sweep(self._h, V, policy, term, s_begin, s_end, gamma,
                                      d_changed or None, stream or None), "pi_improve_sweep")

    def value_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta=0, d_changed=0, stream=0):
        _check(lib().pi_value_sweep(self._h, V, Vnew, policy, term, s_begin, s_end, gamma,
                                    d_delta or None, d_changed or None, stream or None), "pi_value_sweep")

    # -- noise-aware solving: the expected backup over a disturbance set -------
    def set_disturbances(self, action_offsets, state_offsets, weights) -> int:
        """Install the disturbance set of the expectation sweeps (pi_set_disturbances; host arrays): K weights, K action
        offsets or None (zeros), (K, D) state offsets in the order of step_dynamics' arguments or None (zeros).
        `weights=None` drops the set.  The first call after compile() builds the expectation kernels (a compile check on
        a host-only engine).  Returns K in use."""
        if weights is None:
            _check(lib().pi_set_disturbances(self._h, 0, None, None, None), "pi_set_disturbances")
            return 0
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        K = len(w)
        da = None if action_offsets is None else np.ascontiguousarray(action_offsets, dtype=np.float32).ravel()
        dx = None if state_offsets is None else np.ascontiguousarray(state_offsets, dtype=np.float32).reshape(-1)
        if K == 0 or (da is not None and len(da) != K) or (dx is not None and len(dx) != K * self.D):
            raise ValueError(f"a disturbance set needs K >= 1 weights, K action offsets and (K, {self.D}) state offsets")
        _check(lib().pi_set_disturbances(self._h, K, None if da is None else da.ctypes.data_as(_f32p),
                                         None if dx is None else dx.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p)),
               "pi_set_disturbances")
        return self.info(Info.DISTURBANCES)

    def expect_eval_sweeps(self, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta=0, stream=0):
        _check(lib().pi_expect_eval_sweeps(self._h, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps,
                                           d_delta or None, stream or None), "pi_expect_eval_sweeps")

    def expect_improve_sweep(self, V, policy, term, s_begin, s_end, gamma, d_changed=0, stream=0):
        _check(lib().pi_expect_improve_sweep(self._h, V, policy, term, s_begin, s_end, gamma,
                                             d_changed or None, stream or None), "pi_expect_improve_sweep")

    def expect_value_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta=0, d_changed=0, stream=0):
        _check(lib().pi_expect_value_sweep(self._h, V, Vnew, policy, term, s_begin, s_end, gamma,
                                           d_delta or None, d_changed or None, stream or None), "pi_expect_value_sweep")

    # -- worst-case solving: the minimum over the points of the same set (weight 0: no part) --
    def robust_eval_sweeps(self, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps, d_delta=0, stream=0):
        _check(lib().pi_robust_eval_sweeps(self._h, Va, Vb, policy, term, s_begin, s_end, gamma, n_sweeps,
                                           d_delta or None, stream or None), "pi_robust_eval_sweeps")

    def robust_improve_sweep(self, V, policy, term, s_begin, s_end, gamma, d_changed=0, stream=0):
        _check(lib().pi_robust_improve_sweep(self._h, V, policy, term, s_begin, s_end, gamma,
                                             d_changed or None, stream or None), "pi_robust_improve_sweep")

    def robust_value_sweep(self, V, Vnew, policy, term, s_begin, s_end, gamma, d_delta=0, d_changed=0, stream=0):
        _check(lib().pi_robust_value_sweep(self._h, V, Vnew, policy, term, s_begin, s_end, gamma,
                                           d_delta or None, d_changed or None, stream or None), "pi_robust_value_sweep")

    # -- Anderson-accelerated policy evaluation (csrc/pi_accel_kernels.hip; dynamicprogramming_amd/accel.py is the twin) --
    def accel_update(self, x, g, f_prev, g_prev, dF, dG, m, slot, k_used, first, n, d_dots, stream=0):
        """One pass after a full batch (pi_accel_update; raw device pointers, asynchronous): the new column of the (m, n)
        rings dF / dG at `slot`, (f_prev, g_prev) replaced, 2 k_used + 1 float64 dot products into d_dots."""
        _check(lib().pi_accel_update(self._h, x or None, g or None, f_prev or None, g_prev or None, dF or None, dG or None,
                                     int(m), int(slot), int(k_used), int(bool(first)), int(n), d_dots or None,
                                     stream or None), "pi_accel_update")

    def accel_combine(self, g, dG, coeffs, k_used, n, out, stream=0):
        """out <- g - dG c over the first k_used ring positions (pi_accel_combine; raw device pointers, `coeffs` host
        floats; `out` may be `g`; asynchronous)."""
        c = (ctypes.c_double * max(int(k_used), 1))(*[float(v) for v in list(coeffs)[:max(int(k_used), 0)]])
        _check(lib().pi_accel_combine(self._h, g or None, dG or None, c, int(k_used), int(n), out or None, stream or None),
               "pi_accel_combine")

    def reach_planes(self, term, s_begin, s_end, d_bitmap, stream=0, dim=0):
        _check(lib().pi_reach_planes(self._h, term, s_begin, s_end, int(dim), d_bitmap, stream or None),
               "pi_reach_planes")

    def reach_depth_max(self) -> int:
        return int(lib().pi_reach_depth_max(self._h))

    def reach_units(self, term, s_begin, s_end, depth, d_bitmap, stream=0):
        _check(lib().pi_reach_units(self._h, term, s_begin, s_end, int(depth), d_bitmap, stream or None),
               "pi_reach_units")

    def probe_coords(self, s_begin, s_end, out, chunks_per_workgroup=1, stream=0):
        _check(lib().pi_probe_coords(self._h, s_begin, s_end, out, int(chunks_per_workgroup),
                                     stream or None), "pi_probe_coords")

    def plan_schedule(self, block, first, count, total=None, chunks_per_workgroup=1):
        """{grid_x, grid_y, period, phase, cpw} of the launch the sweeps would make (pi_plan_schedule)."""
        out = (ctypes.c_uint64 * 6)()
        _check(lib().pi_plan_schedule(self._h, int(block), int(first), int(count),
                                      int(self.info(Info.N_STATES) if total is None else total), int(chunks_per_workgroup), out),
               "pi_plan_schedule")
        return dict(zip(("grid_x", "grid_y", "period", "phase", "cpw"), (int(v) for v in out)))

    def set_option(self, what: int, value: int) -> None:
        _check(lib().pi_set_option(self._h, int(what), int(value)), "pi_set_option")

    # -- multi-GPU (RCCL or the in-process test transport) ---------------------
    def comm_init(self, rank: int, world: int, unique_id: bytes) -> None:
        assert len(unique_id) == 128
        buf = ctypes.create_string_buffer(unique_id, 128)
        _check(lib().pi_comm_init(self._h, int(rank), int(world), buf), "pi_comm_init")

    def comm_init_local(self, rank: int, world: int, group: str) -> None:
        _check(lib().pi_comm_init_local(self._h, int(rank), int(world), group.encode()),
               "pi_comm_init_local")

    P2P_DESC_BYTES = 512

    def p2p_describe(self, rank: int, world: int, buffers) -> bytes:
        """Register `buffers` — (device pointer, bytes) pairs: the arrays sends and receives will name — for the
        peer-to-peer transport and return this rank's 512-byte descriptor (pi_p2p_describe)."""
        n = len(buffers)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p, _ in buffers])
        sizes = (ctypes.c_int64 * max(n, 1))(*[int(b) for _, b in buffers])
        out = ctypes.create_string_buffer(self.P2P_DESC_BYTES)
        _check(lib().pi_p2p_describe(self._h, int(rank), int(world), ptrs, sizes, n, out), "pi_p2p_describe")
        return out.raw

    def comm_init_p2p(self, rank: int, world: int, descriptors, cache_dir: Path | str | None = KERNEL_CACHE) -> None:
        """`descriptors`: the p2p_describe results of ALL ranks, ordered by rank (pi_comm_init_p2p)."""
        blob = b"".join(descriptors)
        if len(blob) != self.P2P_DESC_BYTES * int(world):
            raise NativeError(f"comm_init_p2p needs {world} descriptors of {self.P2P_DESC_BYTES} bytes")
        cdir = None
        if cache_dir is not None:
            Path(cache_dir).mkdir(parents=True, exist_ok=True)
            cdir = str(cache_dir).encode()
        _check(lib().pi_comm_init_p2p(self._h, int(rank), int(world), ctypes.create_string_buffer(blob, len(blob)), cdir),
               "pi_comm_init_p2p")

    def comm_destroy(self) -> None:
        _check(lib().pi_comm_destroy(self._h), "pi_comm_destroy")

    def comm_info(self, what: int) -> int:
        return int(lib().pi_comm_info(self._h, int(what)))

    def allgather_V(self, V_full, shard_elems, stream=0):
        _check(lib().pi_allgather_V(self._h, V_full, shard_elems, stream or None), "pi_allgather_V")

    def allgather_policy(self, policy_full, shard_elems, stream=0):
        _check(lib().pi_allgather_policy(self._h, policy_full, shard_elems, stream or None),
               "pi_allgather_policy")

    def allreduce_max_f32(self, d_value, stream=0):
        _check(lib().pi_allreduce_max_f32(self._h, d_value, stream or None), "pi_allreduce_max_f32")

    def allreduce_sum_u32(self, d_value, stream=0):
        _check(lib().pi_allreduce_sum_u32(self._h, d_value, stream or None), "pi_allreduce_sum_u32")

    def exchange_plan(self, term, per, mode=Plan.NONE, overlap=True, stream=0):
        info = (ctypes.c_int64 * 5)()
        _check(lib().pi_exchange_plan(self._h, term, int(per), int(mode), int(bool(overlap)), info,
                                      stream or None), "pi_exchange_plan")
        units = self.comm_info(CommInfo.REACH_UNITS)
        return {"mode": "halo" if info[0] == Plan.HALO else "allgather", "recv_elems": int(info[1]),
                "send_elems": int(info[2]), "send_ranges": int(info[3]), "interior_ranges": int(info[4]),
                "row_exact": self.comm_info(CommInfo.ROW_EXACT) == 1,
                "reach_units": ("planes of dimension 0" if units == ReachUnits.PLANES else
                                "rows (i0, i1)" if units == ReachUnits.ROWS else "none")}

    def plan_ranges(self):
        """[(kind, begin, end)] of the current exchange plan: kind 0 = swept first, 1 = interior."""
        fn = lib().pi_plan_ranges
        m = fn(self._h, None, 0)
        if m < 0:
            raise NativeError(f"pi_plan_ranges failed: {last_error()}")
        buf = (ctypes.c_int64 * (3 * max(int(m), 1)))()
        fn(self._h, buf, int(m))
        return [(int(buf[3 * i]), int(buf[3 * i + 1]), int(buf[3 * i + 2])) for i in range(int(m))]

    def eval_sweep_part(self, V, Vnew, policy, term, part, gamma, stream=0):
        """Part 0 (swept first) or 1 (interior) of one sharded evaluation sweep, without the exchange."""
        _check(lib().pi_eval_sweep_part(self._h, V, Vnew, policy, term or None, int(part), gamma, stream or None),
               "pi_eval_sweep_part")

    def exchange_V(self, V_full, stream=0):
        _check(lib().pi_exchange_V(self._h, V_full, stream or None), "pi_exchange_V")

    def eval_sweeps_sharded(self, Va, Vb, policy, term, gamma, n_sweeps, d_delta=0, stream=0):
        _check(lib().pi_eval_sweeps_sharded(self._h, Va, Vb, policy, term, gamma, n_sweeps,
                                            d_delta or None, stream or None), "pi_eval_sweeps_sharded")

    def improve_sweep_sharded(self, V, policy, term, gamma, d_changed=0, stream=0):
        _check(lib().pi_improve_sweep_sharded(self._h, V, policy, term, gamma, d_changed or None,
                                              stream or None), "pi_improve_sweep_sharded")

    def probe_step(self, states, acts, nxt, reward, done, m, stream=0):
        _check(lib().pi_probe_step(self._h, states, acts, nxt, reward, done, m, stream or None),
               "pi_probe_step")

    def probe_interp(self, pts, idxs, wgts, m, stream=0):
        _check(lib().pi_probe_interp(self._h, pts, idxs, wgts, m, stream or None), "pi_probe_interp")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().pi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class InferenceEngine:
    """One pi_infer handle: batched device interpolation of a trained policy (the reference's
    utils/barycentric.py as one kernel; include/pi_mi355.h "Inference")."""

    def __init__(self, bounds_low, bounds_high, grid_shape, strides, corner_bits, device: int = -1,
                 cache_dir: Path | str | None = KERNEL_CACHE):
        L = lib()
        self._lo = np.ascontiguousarray(bounds_low, dtype=np.float32)
        self._hi = np.ascontiguousarray(bounds_high, dtype=np.float32)
        self._shape = np.ascontiguousarray(grid_shape, dtype=np.int32)
        self._strides = np.ascontiguousarray(strides, dtype=np.int32)
        self._bits = np.ascontiguousarray(corner_bits, dtype=np.int32)
        self.D = len(self._shape)
        assert self._bits.ndim == 2 and self._bits.shape[1] == self.D
        cdir = None
        if cache_dir is not None:
            Path(cache_dir).mkdir(parents=True, exist_ok=True)
            cdir = str(cache_dir).encode()
        self._h = L.pi_infer_create(int(device), self.D, self._lo.ctypes.data_as(_f32p), self._hi.ctypes.data_as(_f32p),
                                    self._shape.ctypes.data_as(_i32p), self._strides.ctypes.data_as(_i32p),
                                    self._bits.ctypes.data_as(_i32p), len(self._bits), cdir)
        if not self._h:
            raise NativeError(f"pi_infer_create failed: {last_error()}")
        self.device = int(device)
        self.n_corners = len(self._bits)

    # -- marshalling: every group of C arguments that several entry points share is built here, once ----------------
    def _build(self, name, *args, failed=None) -> str:
        """pi_infer_<name>(h, *args, log, log_len), a call that builds a module: returns the compiler's log, raises
        NativeError — "pi_infer_<name> failed:", or `failed` — with the library's message."""
        log = ctypes.create_string_buffer(1 << 16)
        rc = getattr(lib(), "pi_infer_" + name)(self._h, *args, log, len(log))
        text = log.value.decode(errors="replace")
        if rc != 0:
            raise NativeError(f"{failed or f'pi_infer_{name} failed:'}\n{last_error()}")
        return text

    @staticmethod
    def _table(action_space):
        """(const float* action_space, int n_actions) of a host table of any shape; None travels as (NULL, 0)."""
        if action_space is None:
            return None, 0
        act = np.ascontiguousarray(action_space, dtype=np.float32).ravel()
        return act.ctypes.data_as(_f32p), len(act)          # the pointer keeps its array alive

    def _vector(self, values, message):
        """`const float*` of a host vector of D floats, NULL for None; ValueError(message, its {D} filled in) for another
        shape."""
        if values is None:
            return None
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.shape != (self.D,):
            raise ValueError(message.format(D=self.D))
        return v.ctypes.data_as(_f32p)                      # the pointer keeps its array alive

    def _thresholds(self, enter, leave):
        """(const float* enter, const float* leave) of the hybrid rollouts."""
        message = "enter and leave must hold {D} thresholds each"
        return self._vector(enter, message), self._vector(leave, message)

    def _noise(self, epsilon, action_noise, state_noise, seed, first_episode):
        """(float epsilon, float action_noise, const float* state_noise, uint64 seed, uint64 first_episode) of the noisy
        rollouts."""
        return (float(epsilon), float(action_noise), self._vector(state_noise, "state_noise must hold {D} values"),
                int(seed), int(first_episode))

    def _rollout(self, name, handles, d_start, m, n_steps, gamma, middle, d_final, d_return, d_length, d_terminated, d_traj,
                 traj_every, stream, *d_counts) -> None:
        """One rollout launch, the arguments in the ABI's order: `handles`, the batch, `middle` (what only this rollout
        takes), then the group every rollout ends with — the four per-episode outputs, the per-episode counts of the
        hybrid rollouts (`d_counts`: secondary_steps, last_mode, switches), the trajectory, its period, the stream."""
        _check(getattr(lib(), name)(*handles, d_start or None, int(m), int(n_steps), float(gamma), *middle, d_final or None,
                                    d_return or None, d_length or None, d_terminated or None,
                                    *[p or None for p in d_counts], d_traj or None, int(traj_every), stream or None), name)

    def _pair(self, partner):
        return self._h, partner._h if partner is not None else None

    def _lookahead(self, name, d_points, m, gamma, d_best, d_action, d_q_best, d_q_all, stream) -> None:
        _check(getattr(lib(), name)(self._h, d_points or None, int(m), float(gamma), d_best or None, d_action or None,
                                    d_q_best or None, d_q_all or None, stream or None), name)

    def set_policy(self, policy, action_space) -> None:
        pol = np.ascontiguousarray(policy, dtype=np.int32)
        act = np.ascontiguousarray(action_space, dtype=np.float32)
        _check(lib().pi_infer_set_policy(self._h, pol.ctypes.data_as(_i32p), len(pol), act.ctypes.data_as(_f32p),
                                         len(act)), "pi_infer_set_policy")
        self._n_actions = len(act)

    def query(self, d_points, m, d_actions=0, d_weights=0, d_indices=0, stream=0) -> None:
        _check(lib().pi_infer_query(self._h, d_points, int(m), d_actions or None, d_weights or None,
                                    d_indices or None, stream or None), "pi_infer_query")

    def set_dynamics(self, dynamics_src: str) -> str:
        """Build the rollout kernel for the env plugin `dynamics_src` on this handle's grid (a compile check on a
        host-only handle); returns the compiler's log.  Calling it again replaces the plugin."""
        return self._build("set_dynamics", dynamics_src.encode(), failed="rollout kernel compilation failed:")

    def rollout(self, d_start, m, n_steps, gamma=1.0, d_final=0, d_return=0, d_length=0, d_terminated=0, d_traj=0,
                traj_every=0, stream=0) -> None:
        """m episodes of n_steps closed-loop steps in one launch (pi_infer_rollout; raw device pointers, asynchronous)."""
        self._rollout("pi_infer_rollout", (self._h,), d_start, m, n_steps, gamma, (), d_final, d_return, d_length, d_terminated,
                      d_traj, traj_every, stream)

    def set_partner(self, partner: "InferenceEngine") -> str:
        """Build this handle's hybrid module: its grid + `partner`'s grid + the plugin of the last set_dynamics + the hybrid
        rollout kernel (a compile check on host-only handles); returns the compiler's log."""
        return self._build("set_partner", partner._h, failed="hybrid rollout kernel compilation failed:")

    def rollout_hybrid(self, partner: "InferenceEngine", d_start, m, n_steps, enter, leave, gamma=1.0, d_final=0,
                       d_return=0, d_length=0, d_terminated=0, d_secondary_steps=0, d_last_mode=0, d_traj=0, traj_every=0,
                       stream=0) -> None:
        """m episodes of n_steps closed-loop steps that switch between this handle's policy and `partner`'s, in one launch
        (pi_infer_rollout_hybrid; raw device pointers, `enter` / `leave` host arrays of D thresholds; asynchronous)."""
        self._rollout("pi_infer_rollout_hybrid", self._pair(partner), d_start, m, n_steps, gamma,
                      self._thresholds(enter, leave), d_final, d_return, d_length, d_terminated, d_traj, traj_every, stream,
                      d_secondary_steps, d_last_mode)

    def set_partner_stochastic(self, partner: "InferenceEngine", action_space) -> str:
        """Upload the pair's exploration table and build this handle's stochastic hybrid module: its grid + `partner`'s
        grid + the plugin of the last set_dynamics + the stochastic hybrid rollout kernel (a compile check on host-only
        handles); returns the compiler's log.  A later set_dynamics drops the module again."""
        return self._build("set_partner_stochastic", self._pair(partner)[1], *self._table(action_space))

    def rollout_hybrid_stochastic(self, partner: "InferenceEngine", d_start, m, n_steps, enter, leave, gamma=1.0, epsilon=0.0,
                                  action_noise=0.0, state_noise=None, seed=0, first_episode=0, d_final=0, d_return=0,
                                  d_length=0, d_terminated=0, d_secondary_steps=0, d_last_mode=0, d_switches=0, d_traj=0,
                                  traj_every=0, stream=0) -> None:
        """`rollout_hybrid` with the epsilon-random actions, action noise and state noise of `rollout_stochastic` from the
        same stream, in one launch (pi_infer_rollout_hybrid_stochastic; raw device pointers, `enter` / `leave` /
        `state_noise` host arrays of D floats; `d_switches` counts an episode's mode changes; asynchronous)."""
        self._rollout("pi_infer_rollout_hybrid_stochastic", self._pair(partner), d_start, m, n_steps, gamma,
                      (*self._thresholds(enter, leave), *self._noise(epsilon, action_noise, state_noise, seed, first_episode)),
                      d_final, d_return, d_length, d_terminated, d_traj, traj_every, stream, d_secondary_steps, d_last_mode,
                      d_switches)

    def set_values(self, values) -> str:
        """Upload the value function of this handle's grid (the user's order) and build the resample kernel (a compile
        check on a host-only handle); returns the compiler's log."""
        val = np.ascontiguousarray(values, dtype=np.float32).ravel()
        return self._build("set_values", val.ctypes.data_as(_f32p), len(val))

    def resample(self, dst_shape, dst_strides, dst_bins, d_term=0, d_values=0, d_policy=0, action_map=None, n_actions=0,
                 stream=0) -> None:
        """This handle's solution interpolated onto the nodes of another grid in one launch (pi_infer_resample; host
        arrays for the destination's shape, element strides and per-dimension bin tables, raw device pointers for its
        mask and outputs; asynchronous).  `action_map`: one destination action index per source action, None = identity."""
        shape = np.ascontiguousarray(dst_shape, dtype=np.int32)
        strides = np.ascontiguousarray(dst_strides, dtype=np.int64)
        tables = [np.ascontiguousarray(b, dtype=np.float32).ravel() for b in dst_bins]
        if shape.shape != (self.D,) or strides.shape != (self.D,) or [len(t) for t in tables] != shape.tolist():
            raise ValueError(f"the destination needs {self.D} dimensions: a shape, a stride and a bin table of that length each")
        bins = np.concatenate(tables)
        amap = None
        if action_map is not None:
            amap = np.ascontiguousarray(action_map, dtype=np.int32)
            if amap.ndim != 1 or ((amap < 0) | (amap >= int(n_actions))).any():
                raise ValueError(f"action_map must hold indices into the destination's {int(n_actions)} actions")
            if len(amap) != getattr(self, "_n_actions", len(amap)):
                raise ValueError(f"action_map needs one entry per source action ({self._n_actions})")
        _check(lib().pi_infer_resample(self._h, shape.ctypes.data_as(_i32p), strides.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                       bins.ctypes.data_as(_f32p), None if amap is None else amap.ctypes.data_as(_i32p),
                                       int(n_actions), d_term or None, d_values or None, d_policy or None, stream or None),
               "pi_infer_resample")

    def set_greedy(self, action_space) -> str:
        """Upload the action table of the value-greedy controller and build the greedy kernels behind the plugin of the
        last set_dynamics (a compile check on a host-only handle); needs set_values and set_dynamics; returns the
        compiler's log.  A later set_dynamics drops the module again."""
        return self._build("set_greedy", *self._table(action_space))

    def greedy(self, d_points, m, gamma, d_best=0, d_action=0, d_q_best=0, d_q_all=0, stream=0) -> None:
        """The one-step lookahead on the value function at m query points in one launch (pi_infer_greedy; raw device
        pointers, asynchronous): greedy index, its action value, its Q and the (m, n_actions) matrix of all Q."""
        self._lookahead("pi_infer_greedy", d_points, m, gamma, d_best, d_action, d_q_best, d_q_all, stream)

    def rollout_greedy(self, d_start, m, n_steps, lookahead_gamma, gamma=1.0, d_final=0, d_return=0, d_length=0,
                       d_terminated=0, d_traj=0, traj_every=0, stream=0) -> None:
        """m episodes of n_steps closed-loop steps under the value-greedy controller in one launch
        (pi_infer_rollout_greedy; raw device pointers, asynchronous)."""
        self._rollout("pi_infer_rollout_greedy", (self._h,), d_start, m, n_steps, gamma, (float(lookahead_gamma),), d_final,
                      d_return, d_length, d_terminated, d_traj, traj_every, stream)

    def set_stochastic(self, action_space) -> str:
        """Upload the action table exploring steps draw from and build the stochastic rollout kernels behind the plugin
        of the last set_dynamics (a compile check on a host-only handle); needs set_dynamics, neither a policy nor
        values; returns the compiler's log.  A later set_dynamics drops the module again."""
        return self._build("set_stochastic", *self._table(action_space))

    def rollout_stochastic(self, d_start, m, n_steps, gamma=1.0, epsilon=0.0, action_noise=0.0, state_noise=None, seed=0,
                           first_episode=0, d_final=0, d_return=0, d_length=0, d_terminated=0, d_traj=0, traj_every=0,
                           stream=0) -> None:
        """m episodes of n_steps closed-loop steps with epsilon-random actions, action noise and state noise from the
        counter-based stream (seed, first_episode + row, step), in one launch (pi_infer_rollout_stochastic; raw device
        pointers, `state_noise` a host array of D floats or None; asynchronous)."""
        self._rollout("pi_infer_rollout_stochastic", (self._h,), d_start, m, n_steps, gamma,
                      self._noise(epsilon, action_noise, state_noise, seed, first_episode), d_final, d_return, d_length,
                      d_terminated, d_traj, traj_every, stream)

    def random_words(self, seed, first_episode, m, step, block, d_words, stream=0) -> None:
        """The four Philox words of (seed, first_episode + row, step, block) for rows 0 .. m into the (m, 4) uint32 device
        buffer at `d_words` (pi_infer_random_words; asynchronous)."""
        _check(lib().pi_infer_random_words(self._h, int(seed), int(first_episode), int(m), int(step), int(block),
                                           d_words or None, stream or None), "pi_infer_random_words")

    def set_robust(self, action_space) -> str:
        """Upload the action table of the robust lookahead and build the adversary kernels behind the plugin of the last
        set_dynamics (a compile check on a host-only handle); needs set_values and set_dynamics; returns the compiler's
        log.  A later set_dynamics drops the module again.  The set is that of set_disturbances."""
        return self._build("set_robust", *self._table(action_space))

    def robust(self, d_points, m, gamma, d_best=0, d_action=0, d_q_best=0, d_q_all=0, d_worst=0, stream=0) -> None:
        """The robust one-step lookahead at m query points in one launch (pi_infer_robust; raw device pointers,
        asynchronous): the outputs of `greedy` plus d_worst (m) int32, the adversary's point against the winner."""
        _check(lib().pi_infer_robust(self._h, d_points or None, int(m), float(gamma), d_best or None, d_action or None,
                                     d_q_best or None, d_q_all or None, d_worst or None, stream or None), "pi_infer_robust")

    def rollout_adversary(self, d_start, m, n_steps, lookahead_gamma, controller, gamma=1.0, d_final=0, d_return=0,
                          d_length=0, d_terminated=0, d_traj=0, traj_every=0, stream=0) -> None:
        """m episodes of n_steps closed-loop steps against the adversary in one launch (pi_infer_rollout_adversary; raw
        device pointers, asynchronous).  controller: 0, the policy table; 1, the robust lookahead."""
        self._rollout("pi_infer_rollout_adversary", (self._h,), d_start, m, n_steps, gamma,
                      (float(lookahead_gamma), int(controller)), d_final, d_return, d_length, d_terminated, d_traj,
                      traj_every, stream)

    def set_expect_greedy(self, action_space) -> str:
        """Upload the action table of the expected-value greedy controller and build its kernels behind the plugin of the
        last set_dynamics (a compile check on a host-only handle); needs set_values and set_dynamics; returns the
        compiler's log.  A later set_dynamics drops the module again."""
        return self._build("set_expect_greedy", *self._table(action_space))

    def set_disturbances(self, action_offsets, state_offsets, weights) -> int:
        """The disturbance set the expected-value greedy controller takes its expectation over
        (pi_infer_set_disturbances; host arrays, the rules of Engine.set_disturbances): K weights, K action offsets or
        None (zeros), (K, D) state offsets or None (zeros).  `weights=None` drops the set.  An upload, never a build.
        Returns K."""
        if weights is None:
            _check(lib().pi_infer_set_disturbances(self._h, 0, None, None, None), "pi_infer_set_disturbances")
            return 0
        w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
        K = len(w)
        da = None if action_offsets is None else np.ascontiguousarray(action_offsets, dtype=np.float32).ravel()
        dx = None if state_offsets is None else np.ascontiguousarray(state_offsets, dtype=np.float32).reshape(-1)
        if K == 0 or (da is not None and len(da) != K) or (dx is not None and len(dx) != K * self.D):
            raise ValueError(f"a disturbance set needs K >= 1 weights, K action offsets and (K, {self.D}) state offsets")
        _check(lib().pi_infer_set_disturbances(self._h, K, None if da is None else da.ctypes.data_as(_f32p),
                                               None if dx is None else dx.ctypes.data_as(_f32p), w.ctypes.data_as(_f32p)),
               "pi_infer_set_disturbances")
        return K

    def expect_greedy(self, d_points, m, gamma, d_best=0, d_action=0, d_q_best=0, d_q_all=0, stream=0) -> None:
        """The one-step lookahead with the expectation over the disturbance set at m query points in one launch
        (pi_infer_expect_greedy; raw device pointers, asynchronous): the outputs of `greedy`."""
        self._lookahead("pi_infer_expect_greedy", d_points, m, gamma, d_best, d_action, d_q_best, d_q_all, stream)

    def rollout_expect_greedy(self, d_start, m, n_steps, lookahead_gamma, gamma=1.0, epsilon=0.0, action_noise=0.0,
                              state_noise=None, seed=0, first_episode=0, d_final=0, d_return=0, d_length=0, d_terminated=0,
                              d_traj=0, traj_every=0, stream=0) -> None:
        """m episodes of n_steps closed-loop steps under the expected-value greedy controller, with the epsilon-random
        actions, action noise and state noise of `rollout_stochastic` from the same stream, in one launch
        (pi_infer_rollout_expect_greedy; raw device pointers, `state_noise` a host array of D floats or None;
        asynchronous)."""
        self._rollout("pi_infer_rollout_expect_greedy", (self._h,), d_start, m, n_steps, gamma,
                      (float(lookahead_gamma), *self._noise(epsilon, action_noise, state_noise, seed, first_episode)),
                      d_final, d_return, d_length, d_terminated, d_traj, traj_every, stream)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().pi_infer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
