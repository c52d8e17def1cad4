"""
bench.py — state-action Bellman backups/s of the policy-iteration hot path on MI355X.

Workload (BASELINE.json metric config, SURVEY.md §8d "C4"): double-pendulum swing-up, 4-D
grid 80^4 = 40.96 M states x 11 torques, gamma 0.999, fp32.  Synthetic inputs: V ~ N(0,1),
policy ~ U{0..10} (seeded), no terminal states (the env has none).  Everything is resident
in HBM before the timed region.

A STEP = one pass of the hot path over the whole grid in the sweep mix of SURVEY §8(d)'s
protocol (100 evaluation + 10 improvement sweeps): 10 evaluation sweeps (fused residual on the
last) followed by 1 greedy improvement sweep (fused changed-count) = 10 n + 11 n = 21 n
state-action backups, through the product path (solver -> C ABI -> HIP).

N > 1: one process per GPU, the SAME grid cut into N contiguous state ranges (strong scaling); the
exchange between sweeps runs inside libpi_mi355.so over RCCL (halo exchange of the reachable rows,
or an all-gather: csrc/pi_comm.cpp); torch.distributed only hands the RCCL id around and times the
run.  Either the caller starts the ranks (`python -m torch.distributed.run --nproc-per-node N ...
bench.py --gpus N`: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment) or plain
`python bench.py --gpus N` does: it then starts exactly that command as a CHILD process (before
anything touches the GPU; never an exec), relays rank 0's JSON line and exits with the child's
code.  `--launch-dry-run` prints the child command and the fallback ladder instead of running them.

N > 1 cannot be rehearsed before the driver's scaling run (one GPU per development box), so a rank
started by the launcher does not touch the GPU itself: it SUPERVISES.  Every rank's supervisor joins a
gloo (CPU) group over the launcher's rendezvous and starts the real rank as a fresh child process
(`PI_BENCH_WORKER=1`, its own rendezvous port agreed over gloo), once per rung of a fallback ladder —
halo exchange overlapped with the interior sweep (the library's default) -> halo exchange without overlap
-> all-gather -> all-gather with nothing optional in this script — each rung with a time limit (`--attempt-timeout`, 240 s).  The supervisors agree twice a
second on "some rank failed / every rank is done / time is up" (a three-word all-reduce); a failed or
late rung is killed everywhere (process groups) and the next one starts in new processes — a process that
has touched the GPU is never re-executed.  Rank 0 relays the first successful line with
`check.exchange.attempts` = what happened on every rung.  Inside the ranks, before the timed region, two
sharded evaluation sweeps and one sharded improvement sweep are compared bit for bit with the unsharded
sweeps of the same state (`check.exchange.bit_identical`); a mismatch fails the rung.

Prints ONE JSON line on rank 0: the headline (`value` over the timed steps, `ms_per_step`, the per-sweep times of
those steps from HIP events on the launch stream, the residual and change count of the last one).  A plain run on one
GPU does nothing else; `--dump-outputs DIR` writes what its last timed step computed (dump_outputs).  `--full` adds, outside
the timed region,
  roofline      — dominant kernel of the step (pi_eval_sweep_kernel in every BASELINE config; pi_eval_live_kernel,
                  the same sweep over the listed non-terminal states, on the double cartpole grid).  The headline
                  fraction is the one the north star names: HBM-side bytes per launch — rocprofv3 FETCH_SIZE x 2.0 +
                  WRITE_SIZE from the committed PMC profile of THIS kernel version and THIS config (profiles/rNN/
                  counters_bench_<config>.json, matched on env, bins, memory order and the hash of the device code) —
                  over the launch time measured live (HIP events on the launch stream), against 8 TB/s: `bound` "hbm",
                  `achieved` / `peak` / `frac` (= `frac_hbm`), `traffic`, with the uncorrected `hbm_frac_raw` beside it.
                  The x 2.0 is measured on the sweeps' own load shapes (tools/fetch_calibration.hip, profiles/r05/
                  fetch_calibration.txt: every L2 read request moves a 128-B line and is tallied at 64 B).  These sweeps
                  are a divergent gather plus 300-600 fp32 VALU instructions of dynamics per state and are NOT HBM-bound;
                  `units` prices the two units that do limit them, each against its hardware peak, and
                  `most_utilised_unit` names the busiest:
                    valu  wave64 VALU instructions/s against 1228.8 G/s (MI355X_MICROARCH.md: a wave64
                          fp32 instruction per 2 cycles per SIMD x 1024 SIMDs x 2.4 GHz).  The chip measures
                          ~950 G/s for fp32 fma/mul/add streams AND for mixes with compares / selects /
                          conversions up to 1:1, clustered or not (tools/valu_issue_bench.hip,
                          profiles/r03/valu_issue.txt);
                    l1    the CU's vector-memory path: wave-wide vector loads/s (SQ_INSTS_VMEM_RD) against
                          CUs x clock / 16 = 38.4 G/s — a wave-wide 8- or 16-byte load occupies the path for
                          max(16, runs) cycles, a run being up to 4 consecutive lanes in one 128-B line
                          (tools/tcp_gather_bench.hip, profiles/r03/tcp_gather.txt), so 2^(D-1) corner-pair
                          loads per state need at least 16 x 2^(D-1) cycles per wave — 512 per 64 states in
                          6-D; how long the TCP is clocked and how long it waits for L2 fills come with it;
                    hbm   the headline unit again.
                  Everything that comes from the profile is withheld (null) when no committed profile
                  matches the config and the kernel version.
  extra_configs — N = 1, default config: the other single-GPU BASELINE configs (C2 pendulum 200^2, C3 cartpole swing-up
                  50^4, C5 double cartpole 25^6 and its 9-action swing-up variant) timed the same way after the headline —
                  10 evaluation + 1 improvement sweeps per step from a synthetic resident state — each with its per-sweep
                  times, whole-step throughput and roofline fractions; a compact copy sits in `roofline.extra_configs`.
                  `--time-budget` (420 s) decides what is skipped when a box is slow: the run to convergence first.
  roofline_algorithmic — the SURVEY §8(d) byte model (89 B per 4-D evaluation backup) over the
                  launch time, for reference only: those bytes are cache hits, not a bound.
  sweeps_to_converge — a full run() of policy iteration from V = 0 with the env's own settings (N = 1,
                  outside the timed region; --no-full-run skips it): outer iterations, sweeps, seconds.
  kernels       — every kernel of the step, plus `eval_converged_policy`: the same evaluation
                  sweep on a policy-iteration state (3 outer iterations from V = 0), which is what
                  the sweeps of a real run() see.
  cpu_baseline  — the oracle (oracle/pi_oracle.cpp) on a strided sample of the same workload on
                  this box's host cores, 1 thread and all cores (rank 0, N = 1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import socket
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

T_PROCESS_START = time.perf_counter()
ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# FETCH_SIZE tallies every L2 read request at 64 B while the request moves a 128-B line — measured on the sweeps' own
# access shapes (overlapping 4-byte-aligned 8-byte pairs, 4- and 1-byte non-temporal streams, lone 8-byte loads per line:
# factor 1.97-2.00 on every one; tools/fetch_calibration.hip, profiles/r05/fetch_calibration.txt).  WRITE_SIZE is exact.
FETCH_CORRECTION = 2.0
VALU_PEAK_GIPS = 256 * 4 * 2.4 / 2.0     # wave64 fp32 VALU instructions/s: 2 cycles each per SIMD-32
VALU_MEASURED_GIPS = 950.0               # what the chip sustains for fp32 and mixed streams (profiles/r03/valu_issue.txt)
# Vector L1 (TCP / TA).  Every wave-wide 8- or 16-byte load occupies the CU's vector-memory path for at least 16 cycles
# (4 lanes per cycle) and for max(16, runs) when its lanes fall into more than 16 runs of up to 4 consecutive lanes per
# 128-B line (profiles/r03/tcp_gather.txt: every pattern measured, none faster).  The unit's roofline is therefore the
# wave-load rate: achieved = vector load instructions per second (SQ_INSTS_VMEM_RD), peak = CUs x clock / 16.
# (TCP_TOTAL_CACHE_ACCESSES is NOT a utilisation: it counts (4-lane quad, line) pairs and reaches 2 per cycle on
# run-structured gathers without the unit being busier; it is reported as accesses_per_cu_cycle for reference.)
TA_CYCLES_PER_WAVE_LOAD = 16.0
TCP_PEAK_GLOADS = 256 * 2.4 / TA_CYCLES_PER_WAVE_LOAD          # G wave-wide loads per second
ENV = "double_pendulum_swingup"
BINS = 80
EVAL_PER_STEP = 10
IMPROVE_PER_STEP = 1


def algorithmic_bytes_eval(D: int) -> int:
    return 4 * (1 << D) + 4 * D + 9          # 89 B for D = 4


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def cpu_baseline(env: str, bins: int, sample_states: int, seed: int = 0) -> dict:
    """Oracle timed on host cores over every k-th state of the same grid / V / policy: on every core of this
    process's affinity mask (`value`, `cores`), on 16 threads (a one-GPU box's share) and on one thread."""
    import oracle
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env]
    tables = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    lo, hi, shape, strides = oracle.grid_metadata(tables)
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    V = rng.standard_normal(n).astype(np.float32)
    chk = oracle.build(cls._D, envs.dynamics_source(env))
    gamma = np.float32(cls.CONFIG["gamma"])
    checker_threads = chk.threads
    try:
        all_cores = len(os.sched_getaffinity(0))
    except AttributeError:
        all_cores = os.cpu_count() or 1

    def run(m, threads):
        stride = max(n // m, 1)
        flat = np.arange(0, n, stride, dtype=np.int64)[:m]
        idx = np.stack(np.unravel_index(flat, tuple(shape)), axis=1)
        states = np.stack([tables[d][idx[:, d]] for d in range(len(tables))], axis=1).astype(np.float32)
        pol = rng.integers(0, len(cls.ACTIONS), size=len(flat)).astype(np.int32)
        term = np.zeros(len(flat), dtype=np.uint8)
        out = np.zeros(len(flat), dtype=np.float32)
        chk.set_threads(threads)
        chk.eval_sweep(states, cls.ACTIONS, pol, V, term, lo, hi, shape, strides, gamma, 0, len(flat), out=out)
        t0 = time.perf_counter()
        for _ in range(EVAL_PER_STEP):
            chk.eval_sweep(states, cls.ACTIONS, pol, V, term, lo, hi, shape, strides, gamma, 0, len(flat), out=out)
        for _ in range(IMPROVE_PER_STEP):
            chk.improve_sweep(states, cls.ACTIONS, pol, V, term, lo, hi, shape, strides, gamma, 0, len(flat))
        dt = time.perf_counter() - t0
        return len(flat) * (EVAL_PER_STEP + IMPROVE_PER_STEP * len(cls.ACTIONS)) / dt, dt, stride

    m_all = min(sample_states, n)
    many, dt_many, stride_many = run(m_all, all_cores)
    mid_threads = min(16, all_cores)
    mid, dt_mid, stride_mid = (many, dt_many, stride_many) if mid_threads == all_cores else run(max(m_all // 2, 1), mid_threads)
    one, dt_one, stride_one = run(max(m_all // 16, 1), 1)
    chk.set_threads(checker_threads)
    quota = None
    try:                                                    # cgroup v2 CPU quota of this box's share, if any
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        quota = None if q == "max" else float(q) / float(period)
    except (OSError, ValueError):
        pass
    # `value` / `cores`: the faster of the two multi-thread runs with the threads it used (on a box whose CPU share is
    # smaller than its affinity mask, one thread per listed core oversubscribes the share and is slower)
    best, best_threads = (many, all_cores) if many >= mid else (mid, mid_threads)
    return {"value": best, "unit": "backups/s", "cores": best_threads, "kind": "port",
            "value_all_affinity_threads": many, "affinity_threads": all_cores,
            "value_16_threads": mid, "threads_16": mid_threads, "cgroup_cpu_quota_cores": quota,
            "value_1_thread": one, "cpu_model": cpu_model(), "os_cpu_count": os.cpu_count(),
            "numpy_reference_c1": numpy_reference_c1(),
            "sample": f"one step (10 eval + 1 improve sweeps) over every {stride_many}-th state of the same "
                      f"{bins}^{cls._D} grid ({m_all} states, {dt_many:.1f} s wall, oracle/pi_oracle.cpp with OpenMP on "
                      f"all {all_cores} threads of the affinity mask); {mid_threads} threads: every {stride_mid}-th state, "
                      f"{dt_mid:.1f} s; 1 thread: every {stride_one}-th state, {dt_one:.1f} s"}


def numpy_reference_c1() -> dict:
    """BASELINE config 1: the vectorised numpy sweep (oracle/numpy_reference.py) on Pendulum 50 x 50 x 11."""
    from oracle import numpy_reference as NR
    from dynamicprogramming_amd import envs
    cls = envs.ENVS["pendulum"]
    ref = NR.PendulumNumpy([np.asarray(b, np.float32) for b in cls.bins_space(50).values()],
                           np.linspace(-2.0, 2.0, 11, dtype=np.float32))
    ref.gamma = np.float32(0.99)
    rng = np.random.default_rng(0)
    V = rng.standard_normal(ref.n).astype(np.float32)
    pol = rng.integers(0, 11, ref.n).astype(np.int32)
    ref.eval_sweep(V, pol)
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        for _ in range(EVAL_PER_STEP):
            ref.eval_sweep(V, pol)
        ref.improve_sweep(V, pol)
    dt = time.perf_counter() - t0
    return {"value": reps * ref.n * (EVAL_PER_STEP + 11) / dt, "unit": "backups/s", "cores": 1,
            "config": "Pendulum 50 x 50 x 11 actions, numpy float32, one thread"}


def kernel_units(name, ms, backups, alg_bytes_per_backup, *, prof, prof_scale, n, n_live, live_per_launch,
                 states_per_launch, counters=None):
    """Timing of one kernel plus, when a matching profile exists, the utilisation of the three
    units it can be bound by (VALU issue, vector-L1 tag look-ups, HBM)."""
    sec = ms * 1e-3
    e = {"kernel": name, "avg_launch_ms": ms, "backups_per_launch": backups, "backups_per_s": backups / sec}
    if n_live != n:
        e["backups_per_launch_live"] = int(round(backups * live_per_launch / float(states_per_launch)))
        e["backups_per_s_live"] = e["backups_per_launch_live"] / sec
    alg = alg_bytes_per_backup * backups / sec / 1e9
    e["algorithmic"] = {"bytes_per_backup": alg_bytes_per_backup, "achieved_GBps": alg,
                        "note": "SURVEY 8(d) byte model; served by L1/L2/Infinity Cache, not a bound"}
    k = ((prof or {}).get("kernels", {}) if counters is None else counters).get(name)
    if not k or "valu_insts_per_wave" not in k:
        return e
    c = k["counters"]
    waves = c["SQ_WAVES"] * prof_scale
    units = {}
    insts = k["valu_insts_per_wave"] * waves
    ach = insts / sec / 1e9
    units["valu"] = {"achieved": ach, "peak": VALU_PEAK_GIPS, "unit": "G wave64 VALU instructions/s",
                     "frac": ach / VALU_PEAK_GIPS, "frac_of_measured_peak": ach / VALU_MEASURED_GIPS,
                     "measured_peak": VALU_MEASURED_GIPS, "insts_per_wave": k["valu_insts_per_wave"],
                     "waves_per_launch": waves, "class_split_per_wave": k.get("issue_cycles_model")}
    acc, req = c.get("TCP_TOTAL_CACHE_ACCESSES_sum"), c.get("TCP_TCC_READ_REQ_sum")
    acc, req = (None if acc is None else acc * prof_scale), (None if req is None else req * prof_scale)
    loads = (k.get("vmem_rd_insts_per_wave") or 0.0) * waves
    if loads:
        ach = loads / sec / 1e9
        tcp = k.get("tcp_per_cu_cycle") or {}
        units["l1"] = {"achieved": ach, "peak": TCP_PEAK_GLOADS, "unit": "G wave-wide vector loads/s",
                       "frac": ach / TCP_PEAK_GLOADS, "loads_per_wave": k.get("vmem_rd_insts_per_wave"),
                       "loads_per_launch": loads,
                       "accesses_per_launch": acc, "l2_served_lines_per_launch": req,
                       "accesses_per_cu_cycle": None if not acc else acc / sec / 1e9 / (256 * 2.4),
                       "l1_hit_rate": k.get("l1_hit_rate"),
                       "tcp_clocked_frac": tcp.get("TCP_GATE_EN1_sum"),
                       "tcp_waiting_for_l2_frac": tcp.get("TCP_PENDING_STALL_CYCLES_sum"),
                       "note": "frac = 16 cycles x vector loads per CU / launch cycles at 2.4 GHz: the share of the "
                               "launch the vector-memory path needs at the very least (4 lanes per cycle; loads "
                               "whose lanes fall into more than 16 runs need more, 1- and 4-byte loads less).  "
                               "tcp_clocked / waiting_for_l2: share of the launch the TCP is clocked / stalled on "
                               "L2 fills (same profile).  accesses_per_cu_cycle is the raw counter, not a "
                               "utilisation (profiles/r03/tcp_gather.txt)"}
    if "FETCH_SIZE_bytes" in k and "WRITE_SIZE_bytes" in k:
        traffic = (FETCH_CORRECTION * k["FETCH_SIZE_bytes"] + k["WRITE_SIZE_bytes"]) * prof_scale
        raw = (k["FETCH_SIZE_bytes"] + k["WRITE_SIZE_bytes"]) * prof_scale
        units["hbm"] = {"achieved": traffic / sec / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": traffic / sec / 1e9 / HBM_PEAK_GBS, "bytes_per_launch": traffic,
                        "frac_raw": raw / sec / 1e9 / HBM_PEAK_GBS, "bytes_per_launch_raw": raw,
                        "fetch_bytes_counted": k["FETCH_SIZE_bytes"] * prof_scale, "write_bytes": k["WRITE_SIZE_bytes"] * prof_scale,
                        "l2_hit_rate": k.get("l2_hit_rate")}
    e["units"] = units
    gui, prof_ms = c.get("GRBM_GUI_ACTIVE"), k.get("ms_under_profiler")
    if gui and prof_ms:
        e["clock_GHz_under_profiler"] = gui / 8.0 / (prof_ms * 1e-3) / 1e9      # summed over the 8 XCDs
    return e


def build_roofline(dom: dict, khash: str, prof_path, compulsory_per_state: float, compulsory: float, prof_scale=None) -> dict:
    """The `roofline` object of the line for the dominant kernel `dom` (a kernel_units entry).  The headline fraction is
    the one the north star names — measured HBM-side bytes per launch (rocprofv3 FETCH_SIZE x the calibrated 2.0 +
    WRITE_SIZE, committed profile of this kernel version) over the launch time measured live, against 8 TB/s — with the
    uncorrected figure and the two other units the kernel can be bound by (VALU issue, vector-load issue) beside it."""
    roofline = {"bound": "hbm", "kernel": dom["kernel"], "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None,
                "frac_hbm": None, "hbm_frac_raw": None, "traffic": None, "traffic_raw": None,
                "avg_launch_ms": dom["avg_launch_ms"], "kernel_source_hash": khash, "profile": prof_path,
                "profile_scaled_to_rank_share": prof_scale,
                "compulsory_bytes_per_state": compulsory_per_state,
                "fetch_correction": {"factor": FETCH_CORRECTION, "source": "profiles/r05/fetch_calibration.txt",
                                     "note": "every L2 read request moves a 128-B line and is tallied at 64 B: measured "
                                             "1.97-2.00 on the sweeps' own load shapes; WRITE_SIZE exact; Infinity-Cache "
                                             "hits are counted, so `traffic` is an upper bound of what reaches HBM"},
                "peak_source": "MI355X_MICROARCH.md: HBM3E 8 TB/s; VALU 1228.8 G wave64 instr/s (2 cycles x 1024 SIMDs x "
                               "2.4 GHz); vector-memory path one wave-wide load per 16 cycles per CU = 38.4 G/s"}
    units = dom.get("units")
    sec = dom["avg_launch_ms"] * 1e-3
    # compulsory bytes (every V value read once, V' written, the policy entry, the mask byte) against 8 TB/s: the fraction a
    # traffic cut cannot lower — `frac` (measured traffic, re-fetches included) goes DOWN when re-fetches are removed
    roofline["frac_hbm_compulsory"] = compulsory / sec / 1e9 / HBM_PEAK_GBS
    if units:
        roofline["units"] = units
        roofline["clock_GHz_under_profiler"] = dom.get("clock_GHz_under_profiler")
        # the binding floor: the time each unit needs at the very least for this launch's instruction / load / byte
        # counts (same committed profile), the largest of them, and how close the launch is to it
        floor = {"hbm_compulsory_ms": compulsory / (HBM_PEAK_GBS * 1e9) * 1e3}
        if "valu" in units:
            floor["valu_ms"] = units["valu"]["insts_per_wave"] * units["valu"]["waves_per_launch"] / (VALU_PEAK_GIPS * 1e9) * 1e3
        if "l1" in units:
            floor["load_issue_ms"] = units["l1"]["loads_per_launch"] / (TCP_PEAK_GLOADS * 1e9) * 1e3
        names = {"valu_ms": "valu-issue", "load_issue_ms": "l1-load-issue", "hbm_compulsory_ms": "hbm (compulsory bytes)"}
        top = max(floor, key=lambda k: floor[k])
        floor["max"] = floor[top]
        floor["binding"] = names[top]
        roofline["floor"] = floor
        roofline["frac_of_floor"] = floor["max"] / dom["avg_launch_ms"]
        roofline["bound_note"] = ("`bound` names the roofline the north star prices this path against (HBM); the unit whose "
                                  "floor is highest is floor.binding, and frac_of_floor = that floor / the measured launch")
        name = max(units, key=lambda u: units[u]["frac"])
        roofline["most_utilised_unit"] = {"name": {"valu": "valu-issue", "l1": "l1-load-issue", "hbm": "hbm"}[name],
                                          "frac": units[name]["frac"], "achieved": units[name]["achieved"],
                                          "peak": units[name]["peak"], "unit": units[name]["unit"]}
        if "hbm" in units:
            h = units["hbm"]
            roofline.update({"achieved": h["achieved"], "frac": h["frac"], "frac_hbm": h["frac"], "hbm_frac": h["frac"],
                             "hbm_frac_raw": h["frac_raw"], "traffic": h["bytes_per_launch"],
                             "traffic_raw": h["bytes_per_launch_raw"],
                             "traffic_vs_compulsory": h["bytes_per_launch"] / compulsory,
                             "traffic_vs_compulsory_raw": h["bytes_per_launch_raw"] / compulsory})
            roofline["north_star_target"] = {
                "hbm_frac_at_least_0.40": bool(h["frac"] >= 0.40),
                "note": "not an HBM-bound kernel: the sweep is co-limited by wave latency, VALU issue and vector-load "
                        "issue (units); at its instruction count the VALU-issue floor alone is at or above the time "
                        "40 % of HBM would allow (DESIGN.md section 4)"}
    return roofline


def load_profile(env: str, bins: int, n_states: int, kernel_hash: str, label: str = "bench", order=None):
    """Latest committed PMC profile (tools/profile_config.sh) of this config — env, bins, memory order of the
    dimensions — on the bench (or policy-iteration: label "real") state whose kernel hash is the current one."""
    for path in sorted(ROOT.glob(f"profiles/r*/counters_{label}_*.json"), reverse=True):
        try:
            prof = json.loads(path.read_text())
        except (OSError, ValueError):
            continue
        if prof.get("kernel_source_hash") != kernel_hash or prof.get("states", n_states) != n_states:
            continue
        if order is not None and list(prof.get("memory_order", range(len(order)))) != list(order):
            continue
        if prof.get("env", ENV) == env and prof.get("bins", BINS) == bins:
            return prof, str(path.relative_to(ROOT))
    return None, None


# The other single-GPU BASELINE configs, timed by a --full run after the headline (N = 1 only):
# (label, env, bins, timed steps, warm-up steps).  One step = 10 evaluation sweeps + 1 improvement sweep, as the headline's.
EXTRA_CONFIGS = [
    ("c2", "pendulum", 200, 200, 20),
    ("c3", "cartpole_swingup", 50, 40, 5),
    ("c5", "double_cartpole", 25, 4, 1),
    ("c5_swingup", "double_cartpole_swingup", 25, 2, 1),
]
# rough wall seconds an extra config needs on a GPU box (construction incl. the terminal hook and the live list, the
# timed steps, the state transfer): what the time budget is checked against before it starts
EXTRA_COST_S = {"c2": 5.0, "c3": 6.0, "c5": 20.0, "c5_swingup": 20.0}   # measured: 0.1 / 0.2 / 1.8 / 1.9 s with a warm kernel cache


def measure_extra_config(label: str, env: str, bins: int, steps: int, warmup: int, dev, khash: str) -> dict:
    """10 evaluation sweeps + 1 improvement sweep of one more BASELINE config through the product path (solver -> C ABI ->
    HIP), from the same kind of synthetic resident state as the headline: per-sweep times (HIP events on the launch
    stream), whole-step throughput, and the roofline units from the committed profile of this kernel version."""
    import torch
    from dynamicprogramming_amd import envs
    t_wall = time.perf_counter()
    cls = envs.ENVS[env]
    solver = envs.make(env, bins, config=envs.CudaPIConfig(**cls.CONFIG), device=dev)
    n, nA, D = solver.n_states, solver.n_actions, cls._D
    gamma = float(np.float32(solver.config.gamma))
    eng = solver._backend.engine
    gen = torch.Generator(device="cpu").manual_seed(0)
    solver.d_value_function[:n].copy_(torch.randn(n, generator=gen, dtype=torch.float32))
    solver.d_new_value_function.copy_(solver.d_value_function)
    solver.d_policy[:n].copy_(torch.randint(0, nA, (n,), generator=gen, dtype=torch.int32))
    n_live = n - int(solver.d_terminal_mask[:n].sum().item())
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]

    def step(k=None):
        if k is not None:
            ev[k][0].record()
        solver._evaluation_sweeps(EVAL_PER_STEP, gamma)
        if k is not None:
            ev[k][1].record()
        solver._improvement_sweep(gamma)
        if k is not None:
            ev[k][2].record()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    eval_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev])) / EVAL_PER_STEP
    improve_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev])) / IMPROVE_PER_STEP
    live_states = eng.info(16)
    dominant, dom_ms = ("pi_eval_sweep_kernel", eval_ms)
    if live_states > 0:                    # later sweeps of a batch run over the live-state list: their own launch time
        def batch_ms(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            solver._evaluation_sweeps(k, gamma)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        batch_ms(2)
        first_ms = min(batch_ms(1) for _ in range(2))
        dominant, dom_ms = "pi_eval_live_kernel", (min(batch_ms(11) for _ in range(2)) - first_ms) / 10.0
    backups_per_step = n * (EVAL_PER_STEP + IMPROVE_PER_STEP * nA)
    prof, prof_path = load_profile(env, bins, n, khash, order=eng.order)
    compulsory_per_state = 12.0 if solver._mask_arg() is None else 13.0
    entry = kernel_units(dominant, dom_ms, n, algorithmic_bytes_eval(D), prof=prof, prof_scale=1.0, n=n, n_live=n_live,
                         live_per_launch=n_live, states_per_launch=n)
    roof = build_roofline(entry, khash, prof_path, compulsory_per_state, compulsory_per_state * n)
    units = roof.get("units") or {}
    out = {"label": label, "workload": f"{env} {D}D grid bins={bins}/dim ({n} states) x {nA} actions, gamma={solver.config.gamma}; "
                                       f"step = {EVAL_PER_STEP} eval sweeps + {IMPROVE_PER_STEP} improve sweep",
           "env": env, "bins": bins, "states": n, "nonterminal_states": n_live, "actions": nA, "steps": steps, "warmup": warmup,
           "ms_per_step": elapsed / steps * 1e3, "eval_ms": eval_ms, "improve_ms": improve_ms,
           "backups_per_s": backups_per_step * steps / elapsed,
           "backups_per_s_nonterminal": n_live * (EVAL_PER_STEP + IMPROVE_PER_STEP * nA) * steps / elapsed,
           "memory_order": list(eng.order),
           "roofline": {"kernel": dominant, "avg_launch_ms": dom_ms, "frac_hbm": roof.get("frac_hbm"),
                        "hbm_frac_raw": roof.get("hbm_frac_raw"), "traffic_vs_compulsory": roof.get("traffic_vs_compulsory"),
                        "valu_frac": (units.get("valu") or {}).get("frac"), "l1_load_issue_frac": (units.get("l1") or {}).get("frac"),
                        "most_utilised_unit": roof.get("most_utilised_unit"), "profile": prof_path,
                        "frac_hbm_compulsory": roof.get("frac_hbm_compulsory"), "floor": roof.get("floor"),
                        "frac_of_floor": roof.get("frac_of_floor")},
           "check": {"last_residual": float(solver._d_delta.item()), "last_changed": int(solver._d_changed.item()),
                     "live_list_states": live_states},
           "wall_seconds": None}
    if getattr(solver._backend, "whole_run", False):
        # launch-bound grid: the run to convergence is one launch (pi_policy_iteration) and costs milliseconds — time it too
        best = None
        for _ in range(3):
            fresh = envs.make(env, bins, config=envs.CudaPIConfig(**cls.CONFIG), device=dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fresh.run()
            dt = time.perf_counter() - t1
            if best is None or dt < best[0]:
                best = (dt, fresh)
        dt, fresh = best
        out["full_run"] = {"seconds": dt, "pi_iterations": fresh.stats["pi_iterations"], "eval_sweeps": fresh.stats["eval_sweeps"],
                           "stable": bool(fresh.stats["stable"]), "us_per_eval_sweep": dt / max(fresh.stats["eval_sweeps"], 1) * 1e6,
                           "launches": int(fresh._backend.whole_runs), "round_by_round_evaluations": int(fresh._backend.xcd_evaluations),
                           "note": "run() from the env's initial state, best of 3; launches = 1: evaluation and improvement "
                                   "rounds in ONE kernel launch on the CUs of one XCD"}
    solver._backend.close()
    del solver
    torch.cuda.empty_cache()
    out["wall_seconds"] = time.perf_counter() - t_wall
    return out


# Runs to convergence (the metric's "sweeps-to-converge" half) a --full run makes after the timed region, in this
# order, each only if its estimated wall seconds still fit --time-budget: (label, env, bins, estimated seconds on one MI355X).
# What every run must reproduce — policy-iteration rounds, evaluation sweeps, sha256[:16] of the bytes of V and of the policy
# (host side, the env's own order) — has been the same since round 2 (profiles/r05/full_runs.txt): results are a property of
# the arithmetic, not of the schedule, the memory order or the kernel family that ran them.
FULL_RUNS = [
    ("c3", "cartpole_swingup", 50, 8.0),
    ("c4", "double_pendulum_swingup", 80, 45.0),
    ("c5", "double_cartpole", 25, 185.0),
]
FULL_RUN_EXPECTED = {
    "c3": {"pi_iterations": 22, "eval_sweeps": 96597, "sha256_V": "b02a3b180957e958", "sha256_policy": "fa86d09d962901e2"},
    "c4": {"pi_iterations": 19, "eval_sweeps": 100668, "sha256_V": "f4273576334e09b3", "sha256_policy": "956b9129034ba3ba"},
    "c5": {"pi_iterations": 15, "eval_sweeps": 65540, "sha256_V": "ef4e764816a78bd4", "sha256_policy": "1674736d1a6f6ec6"},
}


def run_to_convergence(label: str, env: str, bins: int, dev) -> dict:
    """One full run() of (env, bins) from the env's initial state with its own settings through the product path: rounds,
    sweeps, wall seconds and the digests of the results, compared with the committed ones (reference run() :357-370)."""
    import hashlib
    import torch
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env]
    fresh = envs.make(env, bins, config=envs.CudaPIConfig(**cls.CONFIG), device=dev)
    n, nA = fresh.n_states, fresh.n_actions
    torch.cuda.synchronize()
    t_run = time.perf_counter()
    fresh.run()
    t_run = time.perf_counter() - t_run
    st = fresh.stats
    out = {"env": env, "bins": bins, "states": n, "pi_iterations": st["pi_iterations"], "eval_sweeps": st["eval_sweeps"],
           "improve_sweeps": st["improve_sweeps"], "stable": st.get("stable"), "seconds": t_run,
           "backups_per_s": n * (st["eval_sweeps"] + st["improve_sweeps"] * nA) / t_run,
           "us_per_eval_sweep": t_run / max(st["eval_sweeps"], 1) * 1e6,
           "sha256_V": hashlib.sha256(fresh.value_function.tobytes()).hexdigest()[:16],
           "sha256_policy": hashlib.sha256(fresh.policy.tobytes()).hexdigest()[:16],
           "settings": dict(cls.CONFIG)}
    want = FULL_RUN_EXPECTED.get(label)
    if want and (env, bins) == next((e, b) for l, e, b, _ in FULL_RUNS if l == label):
        out["expected"] = want
        out["matches_committed_digests"] = all(out[k] == v for k, v in want.items())
    del fresh
    torch.cuda.empty_cache()
    return out


DUMP_SAMPLES = 1 << 21


def dump_outputs(solver, out_dir: str, residual: float, changed: int) -> None:
    """--dump-outputs: what the timed path hands its caller after the last timed step, as .npy files in `out_dir` — V and
    the policy in the env's own order (the host arrays run() returns), the residual of the last evaluation sweep and the
    number of policy entries the improvement sweep changed.  Grids of more than DUMP_SAMPLES states are sampled at a fixed,
    seeded set of flat indices (`state_index`), so that two builds can be compared array for array (32 MB at most)."""
    n = solver.n_states
    V = solver._to_user(solver.d_value_function[:n].cpu().numpy())
    P = solver._to_user(solver.d_policy[:n].cpu().numpy())
    idx = (np.arange(n) if n <= DUMP_SAMPLES
           else np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLES, replace=False)))
    arrays = {"value_function": V[idx].astype(np.float32),
              "policy": P[idx].astype(np.float32),              # action indices: exact in float32
              "state_index": idx.astype(np.float64),
              "residual": np.array([residual], dtype=np.float64),
              "changed": np.array([changed], dtype=np.float64)}
    path = Path(out_dir)
    path.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(path / f"{name}.npy", a)


def launch_command(n_gpus: int, argv: list[str], port: int | None = None) -> list[str]:
    """The command `python bench.py --gpus N` runs as a child when it was not started by
    torch.distributed.run: the launch line of the bench contract, one rank per GPU on this node."""
    if port is None:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
    rest = [a for a in argv if a != "--launch-dry-run"]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + rest


# Fallback ladder of an N-rank run: (name, environment of the ranks).  The library reads PI_MI355_EXCHANGE /
# PI_MI355_OVERLAP when the exchange is planned (dynamicprogramming_amd/transport.py, csrc/pi_comm.cpp).
LADDER = [
    ("halo+overlap", {}),                                         # library default: halo unless it is > 60 % of an all-gather
    ("halo", {"PI_MI355_OVERLAP": "0"}),                          # whole shard, then the exchange on the same stream
    ("allgather", {"PI_MI355_EXCHANGE": "allgather", "PI_MI355_OVERLAP": "0"}),   # one ncclAllGather per sweep
    # last resort — against a fault in this script's own N > 1 reporting rather than in the exchange: the same all-gather
    # run with nothing optional in it (no self-check, no per-rank table, no CPU baseline, no profile look-up)
    ("allgather-minimal", {"PI_MI355_EXCHANGE": "allgather", "PI_MI355_OVERLAP": "0", "PI_BENCH_MINIMAL": "1"}),
]
ATTEMPT_TIMEOUT = 240.0
# After the first rung that succeeds, the SAME exchange runs once more over the library's peer-to-peer transport
# (csrc/pi_p2p.cpp: halo rows stored straight into IPC-mapped peer buffers, no RCCL) in fresh processes, best effort: its
# figures are attached to the line as check.exchange.p2p and its failure costs nothing but its time limit.  Both runs check
# their sharded sweeps against the unsharded ones bit for bit before AND after the timed region; `value` stays the primary
# (RCCL) rung's — the transport chosen up front — and both figures stand under `value_by_transport`.
BONUS_P2P = {"PI_MI355_TRANSPORT": "p2p", "PI_MI355_COMM_TIMEOUT": "30", "PI_BENCH_BONUS": "1"}
BONUS_TIMEOUT = 150.0
# ... and when NO RCCL rung works (a broken RCCL installation is not a reason to report nothing), the peer-to-peer transport
# is the last rung of the ladder in its own right, complete line included.
LADDER.append(("halo+overlap over p2p", {**BONUS_P2P, "PI_BENCH_BONUS": "0"}))


def _free_port() -> int:
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def worker_command(argv: list[str]) -> list[str]:
    """What a supervisor starts as the real rank (a fresh process per rung of the ladder)."""
    return [sys.executable, str(Path(__file__).resolve())] + [a for a in argv if a != "--launch-dry-run"]


def kill_process_group(proc: subprocess.Popen, grace: float = 5.0) -> None:
    """End a child started with start_new_session=True together with everything it started."""
    import signal
    if proc.poll() is not None:
        return
    for sig, wait in ((signal.SIGTERM, grace), (signal.SIGKILL, grace)):
        try:
            os.killpg(proc.pid, sig)
        except (ProcessLookupError, PermissionError):
            pass
        try:
            proc.wait(timeout=wait)
            return
        except subprocess.TimeoutExpired:
            continue


def result_line(text: str):
    """The last stdout line that is a bench result (a JSON object with "metric"), or None."""
    line = None
    for cand in text.splitlines():
        try:
            obj = json.loads(cand)
        except ValueError:
            continue
        if isinstance(obj, dict) and "metric" in obj:
            line = cand
    return line


def rehearsal_ladder():
    """PI_BENCH_SHARE_GPU=1: the three exchange modes, each over the peer-to-peer transport (RCCL refuses two ranks on one GPU)."""
    return [(m + " over p2p", {**e, **BONUS_P2P, "PI_BENCH_BONUS": "0"}) for m, e in LADDER[:3]]


def supervise(argv: list[str], attempt_timeout: float = ATTEMPT_TIMEOUT, ladder=None, bonus_p2p: bool = True) -> int:
    """One rank of an N-rank run as started by the launcher: never touches the GPU.  Runs the real rank as a child
    process, rung by rung of the fallback ladder, in lockstep with the other ranks' supervisors (gloo)."""
    import datetime
    import threading
    import torch
    import torch.distributed as dist
    if ladder is None and share_gpu():            # rehearsal on one GPU: only the peer-to-peer transport can run there
        ladder = rehearsal_ladder()
        bonus_p2p = False
    ladder = LADDER if ladder is None else ladder
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    # The worker of the current rung lives in a session of its own (so that it can be killed with everything it started):
    # nobody else reaps it.  SIGTERM / SIGINT — the launcher tearing the remaining ranks down after one supervisor died,
    # self_launch killing the launcher's process group on overrun — end it first, then this supervisor exits non-zero.
    import signal
    current: dict = {"proc": None}

    def _reap_and_exit(signum, _frame):
        if current["proc"] is not None:
            kill_process_group(current["proc"], grace=2.0)
        os._exit(128 + signum)

    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, _reap_and_exit)
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=attempt_timeout * len(ladder) + BONUS_TIMEOUT + 300))
    attempts, line = [], None
    try:
        def run_rung(k, mode, extra, limit):
            """One rung in fresh child processes on every rank; returns (record, rank 0's line or None)."""
            port = [_free_port() if rank == 0 else None]          # the ranks' own rendezvous: a fresh port per rung
            dist.broadcast_object_list(port, src=0)
            # The child rendezvouses on its OWN port with rank 0 hosting the store: the launcher's agent store
            # (TORCHELASTIC_USE_AGENT_STORE) lives on the launcher's port and belongs to the supervisors.
            env = {k_: v for k_, v in os.environ.items() if not k_.startswith("TORCHELASTIC_")}
            env.update({**extra, "PI_BENCH_WORKER": "1", "PI_BENCH_ATTEMPT": str(k), "PI_BENCH_MODE": mode,
                        "MASTER_PORT": str(port[0])})
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            proc = subprocess.Popen(worker_command(argv), env=env, text=True, start_new_session=True,
                                    stdout=subprocess.PIPE if rank == 0 else sys.stderr)
            current["proc"] = proc                                # what the signal handler and the finally below reap
            chunks: list[str] = []
            reader = None
            if rank == 0:
                reader = threading.Thread(target=lambda: chunks.append(proc.stdout.read()), daemon=True)
                reader.start()
            t0 = time.monotonic()
            ok = False
            try:
                while True:
                    rc = proc.poll()
                    flags = torch.tensor([int(rc not in (None, 0)), int(rc == 0), int(time.monotonic() - t0 > limit)],
                                         dtype=torch.int32)
                    dist.all_reduce(flags)                        # the same verdict on every rank, twice a second
                    failed, done, late = (int(v) for v in flags.tolist())
                    if failed or late or done == world:
                        break
                    time.sleep(0.5)
                ok = done == world and not failed
            finally:
                # a worker never outlives its rung: not when the rung failed or ran late, and not when a collective above
                # raised because a peer supervisor died or timed out (the worker would sit in an RCCL collective for
                # minutes and poison the next run on the box)
                if not ok:
                    kill_process_group(proc)
            if reader is not None:
                reader.join(timeout=10.0)
            codes = [None] * world
            dist.all_gather_object(codes, proc.poll() if (ok or rc is not None) else None)
            got = result_line("".join(chunks)) if rank == 0 else None
            verdict = [bool(ok and (rank != 0 or got is not None))]
            dist.broadcast_object_list(verdict, src=0)            # rank 0 also needs the line
            record = {"mode": mode, "ok": verdict[0], "seconds": round(time.monotonic() - t0, 1),
                      "exit_codes": codes, "timeout": bool(late and not failed and not ok)}
            if rank == 0:
                print(f"bench.py: rung {k} ({mode}): {'ok' if verdict[0] else 'failed'} "
                      f"{json.dumps(record)}", file=sys.stderr, flush=True)
            return record, got

        bonus = bonus_obj = None
        for k, (mode, extra) in enumerate(ladder):
            record, got = run_rung(k, mode, extra, attempt_timeout)
            attempts.append(record)
            if record["ok"]:
                line = got
                if bonus_p2p and extra.get("PI_BENCH_MINIMAL") != "1" and extra.get("PI_MI355_TRANSPORT") != "p2p":
                    rec2, got2 = run_rung(len(ladder), mode + " over p2p", {**extra, **BONUS_P2P},
                                          min(attempt_timeout, BONUS_TIMEOUT))
                    bonus = dict(rec2)
                    if rank == 0 and rec2["ok"] and got2 is not None:      # figures of a rung that failed somewhere are not quoted
                        try:
                            o2 = json.loads(got2)
                            bonus_obj = o2
                            x2 = (o2.get("check") or {}).get("exchange") or {}
                            bonus.update({"value": o2.get("value"), "ms_per_step": o2.get("ms_per_step"),
                                          "transport": x2.get("transport"), "bit_identical": x2.get("bit_identical"),
                                          "eval_ms_max": x2.get("eval_ms_max"), "eval_ms_min": x2.get("eval_ms_min"),
                                          "per_rank": x2.get("per_rank"), "plan_mode": x2.get("mode"),
                                          "row_exact": x2.get("row_exact"), "fused": x2.get("fused")})
                        except Exception as exc:  # noqa: BLE001 - the bonus never costs the result
                            bonus["parse_error"] = repr(exc)
                break
        if rank == 0 and line is not None:
            obj = json.loads(line)
            obj.setdefault("check", {})
            if not isinstance(obj["check"].get("exchange"), dict):
                obj["check"]["exchange"] = {}
            if bonus is not None:
                obj["check"]["exchange"]["p2p"] = bonus
            # `value` is the rung that succeeded FIRST — the transport chosen up front (RCCL unless every RCCL rung failed).
            # The best-effort rerun over the peer-to-peer transport is reported beside it and never replaces it: picking
            # the faster of two runs after the fact would bias the metric upward.
            if bonus_obj is not None:
                obj["value_by_transport"] = {"rccl": obj.get("value"), "p2p": bonus_obj.get("value"),
                                             "reported": "rccl (the primary rung; the p2p figure is a best-effort rerun)"}
            obj["check"]["exchange"]["attempts"] = attempts
            print(json.dumps(obj), flush=True)
        success = bool(attempts and attempts[-1]["ok"])
        if rank == 0 and not success:
            print(f"bench.py: every rung of the ladder failed: {json.dumps(attempts)}", file=sys.stderr, flush=True)
        return 0 if success else 1
    finally:
        if current["proc"] is not None:
            kill_process_group(current["proc"])                   # no-op for a worker that has exited
        dist.destroy_process_group()


def self_launch(n_gpus: int, argv: list[str], dry_run: bool, attempt_timeout: float = ATTEMPT_TIMEOUT) -> int:
    """Start the ranks as a child process (never exec: nothing here has touched the GPU, and nothing
    will), pass their stderr through, relay rank 0's one JSON line, return the child's exit code
    (non-zero when any rank failed or no line was printed).  The child is bounded in time (the whole
    ladder plus start-up) and killed with its process group when it overruns."""
    cmd = launch_command(n_gpus, argv)
    if dry_run:
        print(json.dumps({"launch": cmd, "worker": worker_command(argv),
                          "ladder": [{"mode": m, "env": e, "timeout_s": attempt_timeout}
                                     for m, e in (rehearsal_ladder() if share_gpu() else LADDER)],
                          **({"rehearsal": "PI_BENCH_SHARE_GPU=1: the rank processes share ONE GPU; no best-effort rerun"}
                             if share_gpu() else {}),
                          "bonus_after_first_success": {"mode": "<that rung> over p2p", "env": BONUS_P2P,
                                                        "timeout_s": min(attempt_timeout, BONUS_TIMEOUT),
                                                        "reported_as": "check.exchange.p2p", "affects_exit_code": False},
                          "note": "dry run: the ranks were not started.  Every rank started by the launch line supervises: "
                                  "it runs `worker` as a fresh child per rung until one rung succeeds on all ranks"}),
              flush=True)
        return 0
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: RCCL between processes needs it
    limit = attempt_timeout * len(LADDER) + BONUS_TIMEOUT + 300.0
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        stdout, _ = proc.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        kill_process_group(proc)
        stdout = ""
        try:
            stdout, _ = proc.communicate(timeout=10.0)
        except subprocess.TimeoutExpired:
            pass
        print(f"bench.py: the {n_gpus}-rank child overran {limit:.0f} s and was killed", file=sys.stderr)
        return 124
    line = result_line(stdout or "")
    if line is not None:
        print(line, flush=True)
    if proc.returncode != 0:
        print(f"bench.py: the {n_gpus}-rank child exited with code {proc.returncode}", file=sys.stderr)
        return proc.returncode
    if line is None:
        print("bench.py: the ranks printed no result line", file=sys.stderr)
        return 1
    return 0


def share_gpu() -> bool:
    """PI_BENCH_SHARE_GPU=1 — REHEARSAL of the N > 1 path on a box with ONE GPU: every rank's process uses device 0,
    torch.distributed runs over gloo, and the library exchanges over its peer-to-peer transport (RCCL refuses two ranks
    on one GPU).  Everything the ranks do — plan, self-check, sharded sweeps, per-rank table, the line — is the code a
    real N-GPU run executes; the NUMBERS are N processes sharing one GPU and the line says so (`rehearsal`)."""
    return os.environ.get("PI_BENCH_SHARE_GPU") == "1"


def over_p2p() -> bool:
    """This rank's exchange runs over the library's peer-to-peer transport (the rehearsal, the best-effort rerun, and the
    ladder's last rung — the one that is left when RCCL itself is what fails): torch.distributed then runs over gloo and its
    small tensors live on the host, so that nothing in the process creates an RCCL communicator."""
    return share_gpu() or os.environ.get("PI_MI355_TRANSPORT", "").lower() == "p2p"


def _collective_device(dev):
    """Where the small tensors of torch.distributed collectives live: on the GPU under RCCL, on the host under gloo."""
    import torch
    return torch.device("cpu") if over_p2p() else dev


def sharded_equals_unsharded(solver, eng, gamma, torch, dist, n_eval: int = 2, gather_first: bool = False) -> dict:
    """Two evaluation sweeps (the second one reads what the first one's exchange delivered) and one improvement sweep
    through the sharded driver, then the same three sweeps over the whole grid on this rank alone (every rank holds a
    full-size V), compared with torch.equal on every rank.  Restores the solver's V / policy afterwards."""
    n = solver.n_states
    if gather_first:
        # after sharded steps a rank's full-size arrays are current only where it sweeps and reads (halo plan) and its
        # policy only in its own shard: make every rank hold the same whole state before the whole-grid comparison
        solver._comm.all_gather(solver, solver.d_value_function)
        solver._comm.all_gather(solver, solver.d_policy)
    V0, P0 = solver.d_value_function.clone(), solver.d_policy.clone()
    term = solver._backend._ptr(solver._mask_arg())
    stream = torch.cuda.current_stream().cuda_stream
    solver._evaluation_sweeps(n_eval, gamma)           # one batch: the first sweep and the later ones take different paths
    solver._improvement_sweep(gamma)
    solver._comm.all_gather(solver, solver.d_value_function)
    solver._comm.all_gather(solver, solver.d_policy)
    residual, changed = float(solver._d_delta.item()), int(solver._d_changed.item())
    A, B, P = V0.clone(), V0.clone(), P0.clone()
    d_delta = torch.zeros(1, dtype=torch.float32, device=V0.device)
    d_changed = torch.zeros(1, dtype=torch.int32, device=V0.device)
    for i in range(n_eval):                            # one sweep per call: the plain whole-grid kernel, nothing batched
        eng.eval_sweep(A.data_ptr(), B.data_ptr(), P.data_ptr(), term, 0, n, gamma,
                       d_delta.data_ptr() if i == n_eval - 1 else 0, stream)
        A, B = B, A
    eng.improve_sweep(A.data_ptr(), P.data_ptr(), term, 0, n, gamma, d_changed.data_ptr(), stream)
    torch.cuda.synchronize()
    same = [bool(torch.equal(A[:n], solver.d_value_function[:n])), bool(torch.equal(P[:n], solver.d_policy[:n])),
            float(d_delta.item()) == residual, int(d_changed.item()) == changed]
    verdict = torch.tensor([int(all(same))], dtype=torch.int32, device=_collective_device(V0.device))
    dist.all_reduce(verdict, op=dist.ReduceOp.MIN)
    solver.d_value_function.copy_(V0)
    solver.d_new_value_function.copy_(V0)
    solver.d_policy.copy_(P0)
    torch.cuda.synchronize()
    return {"ok": bool(verdict.item()), "V": same[0], "policy": same[1], "residual": same[2], "changed": same[3],
            "sweeps": f"{n_eval} evaluation (one batch) + 1 improvement, sharded vs whole grid on one rank, torch.equal on every rank"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bins", type=int, default=None, help="grid points per dimension (default: the BASELINE config)")
    ap.add_argument("--env", default=ENV, help="env plugin (default: the BASELINE metric config, "
                    "double_pendulum_swingup at 80 bins; other BASELINE configs: cartpole_swingup@50, "
                    "double_cartpole@25, double_cartpole_swingup@25, pendulum@200)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: the policy-iteration-state sweep, "
                         "the other BASELINE configs, runs to convergence with their digests, the CPU baseline, per-kernel "
                         "and roofline figures.  The --no-* options, --full-run, --cpu-sample and --time-budget shape "
                         "that part and do nothing without it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-converged-state", action="store_true",
                    help="skip the policy-iteration-state measurement (3 outer iterations, ~4 s)")
    ap.add_argument("--no-full-run", action="store_true",
                    help="skip the run of policy iteration to convergence from V = 0 (the metric's "
                         "'sweeps-to-converge' part: sweeps, outer iterations, wall time; ~45 s on C4, "
                         "N = 1 only, outside the timed region)")
    ap.add_argument("--full-run", action="store_true",
                    help="run to convergence even on grids of 2^27 states or more, where it takes minutes "
                         "(25^6: 263 s, profiles/r03/full_runs.txt) and is skipped by default")
    ap.add_argument("--cpu-sample", type=int, default=1 << 26,
                    help="states of the same grid the all-core CPU baseline sweeps, taken with a uniform "
                         "stride over the whole grid (default: all of the 80^4 grid, ~6 s on 16 threads; "
                         "the 1-thread run takes every 16th of those)")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="N = 1, default config only: skip the other single-GPU BASELINE configs (C2, C3, C5, C5 swing-up) "
                         "that are timed after the headline and reported under `extra_configs`")
    ap.add_argument("--time-budget", type=float, default=420.0,
                    help="wall seconds a whole --full run may take: optional parts that would not fit are skipped — the "
                         "run to convergence first, then extra configs — and say so in the line")
    ap.add_argument("--launch-dry-run", action="store_true",
                    help="with --gpus N > 1 outside torch.distributed.run: print the child command that "
                         "would start the N ranks and the fallback ladder, and exit")
    ap.add_argument("--attempt-timeout", type=float, default=ATTEMPT_TIMEOUT,
                    help="N > 1: seconds one rung of the fallback ladder may take before it is killed on every rank")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")

    launched = "WORLD_SIZE" in os.environ and "RANK" in os.environ      # started by torch.distributed.run
    if not launched and (args.gpus > 1 or args.launch_dry_run):
        sys.exit(self_launch(args.gpus, sys.argv[1:], args.launch_dry_run, args.attempt_timeout))
    if launched and int(os.environ["WORLD_SIZE"]) > 1 and os.environ.get("PI_BENCH_WORKER") != "1":
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}: the launcher's "
                             f"--nproc-per-node must equal --gpus")
        sys.exit(supervise(sys.argv[1:], args.attempt_timeout))

    import torch
    import torch.distributed as dist
    from dynamicprogramming_amd import _native, envs

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if share_gpu() else int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node must equal --gpus")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if share_gpu():
            os.environ["PI_MI355_TRANSPORT"] = "p2p"
        if over_p2p():
            dist.init_process_group("gloo")               # no RCCL anywhere in this process (P2pTransport gathers on any backend)
        else:
            dist.init_process_group("nccl", device_id=dev)

    cls = envs.ENVS[args.env]
    if args.bins is None:
        args.bins = BINS if args.env == ENV else cls.DEFAULT_BINS
    cfg = envs.CudaPIConfig(**cls.CONFIG)
    solver = envs.make(args.env, args.bins, config=cfg, device=dev)
    n, nA, D = solver.n_states, solver.n_actions, cls._D
    gamma = float(np.float32(solver.config.gamma))
    eng = solver._backend.engine

    # synthetic resident inputs (identical on every rank)
    gen = torch.Generator(device="cpu").manual_seed(0)
    V0 = torch.randn(n, generator=gen, dtype=torch.float32)
    P0 = torch.randint(0, nA, (n,), generator=gen, dtype=torch.int32)
    solver.d_value_function[:n].copy_(V0)
    solver.d_new_value_function.copy_(solver.d_value_function)
    solver.d_policy[:n].copy_(P0)
    del V0, P0
    n_live = n - int(solver.d_terminal_mask[:n].sum().item())     # non-terminal states: the ones a sweep backs up

    # ── N > 1: sharded sweeps against the unsharded sweeps of the same state, bit for bit, before anything is timed ──
    minimal = os.environ.get("PI_BENCH_MINIMAL") == "1"        # last rung of the N > 1 ladder: nothing optional
    bit_identical = None
    if world > 1 and minimal:
        bit_identical = {"ok": None, "skipped": "minimal rung of the fallback ladder"}
    elif world > 1:
        bit_identical = sharded_equals_unsharded(solver, eng, gamma, torch, dist)
        if not bit_identical["ok"]:
            if rank == 0:
                print(f"bench.py: sharded sweeps differ from the unsharded ones: {json.dumps(bit_identical)}",
                      file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            dist.barrier()
            sys.exit(3)

    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]

    def step(k=None):
        if k is not None:
            ev[k][0].record()
        solver._evaluation_sweeps(EVAL_PER_STEP, gamma)
        if k is not None:
            ev[k][1].record()
        solver._improvement_sweep(gamma)
        if k is not None:
            ev[k][2].record()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=_collective_device(dev))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # sanity: the sweeps really ran (residual and change count of the last step)
    last_delta = float(solver._d_delta.item())
    last_changed = int(solver._d_changed.item())
    # N > 1: once more after the timed region, over a whole 25-sweep batch + 1 (the later sweeps of a batch run over the
    # live-state lists and, on the peer-to-peer transport, through the fused exchange): a wrong exchange fails the rung
    if world > 1 and not minimal:
        after = sharded_equals_unsharded(solver, eng, gamma, torch, dist, n_eval=26, gather_first=True)
        bit_identical["after_timed_region"] = after
        if not after["ok"]:
            if rank == 0:
                print(f"bench.py: sharded sweeps differ from the unsharded ones after the timed region: {json.dumps(after)}",
                      file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            dist.barrier()
            sys.exit(3)

    if args.dump_outputs:
        if world > 1:                     # a rank's V is current only where it sweeps and reads, its policy in its shard
            solver._comm.all_gather(solver, solver.d_value_function)
            solver._comm.all_gather(solver, solver.d_policy)
        if rank == 0:
            dump_outputs(solver, args.dump_outputs, last_delta, last_changed)

    eval_ms = float(np.mean([e[0].elapsed_time(e[1]) for e in ev])) / EVAL_PER_STEP
    improve_ms = float(np.mean([e[1].elapsed_time(e[2]) for e in ev])) / IMPROVE_PER_STEP
    backups_per_step = n * (EVAL_PER_STEP + IMPROVE_PER_STEP * nA)
    value = backups_per_step * args.steps / elapsed
    # terminal states are COUNTED in `value` ("count terminal states too if simpler, but say which"); they do
    # no work, so the figure over the states a sweep really backs up stands beside it
    value_nonterminal = n_live * (EVAL_PER_STEP + IMPROVE_PER_STEP * nA) * args.steps / elapsed
    states_per_launch = solver._s_end - solver._s_begin
    share = {"eval_sweeps": eval_ms * EVAL_PER_STEP, "improve_sweep": improve_ms * IMPROVE_PER_STEP}

    exchange = None
    if solver._comm is not None and getattr(solver._comm, "info", None) and minimal:
        exchange = {"mode": solver._comm.info.get("mode"), "world": eng.comm_info(1), "bit_identical": bit_identical,
                    "transport": {1: "rccl", 2: "in-process", 3: "p2p"}.get(eng.comm_info(2), "none"),
                    "ladder_mode": os.environ.get("PI_BENCH_MODE"), "recv_elems": solver._comm.info.get("recv_elems")}
    elif solver._comm is not None and getattr(solver._comm, "info", None):
        # what the driver needs to see that RCCL really ran with N ranks: the communicator's own view
        # (pi_comm_info), this rank's plan, and every rank's evaluation time and halo volume
        exchange = dict(solver._comm.info)
        exchange["world"] = eng.comm_info(1)
        exchange["transport"] = {1: "rccl", 2: "in-process", 3: "p2p"}.get(eng.comm_info(2), "none")
        exchange["comm_rank"] = eng.comm_info(0)
        exchange["row_exact"] = eng.comm_info(5) == 1
        exchange["fused"] = eng.comm_info(6) == 1        # the swept-first kernel stores its rows into the peers itself
        exchange["pair_exact"] = eng.comm_info(7) == 1   # destination masks at (i_0, i_v) granularity (any memory order)
        exchange["fused_send_elems"] = eng.comm_info(8)  # values one fused sweep delivers from this rank (-1: not fused)
        mine = torch.tensor([eval_ms, improve_ms, float(exchange["recv_elems"]), float(exchange["send_elems"]),
                             float(states_per_launch)], dtype=torch.float64, device=_collective_device(dev))
        everyone = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(everyone, mine)
        table = torch.stack(everyone).cpu().numpy()
        exchange["per_rank"] = {"eval_ms": table[:, 0].tolist(), "improve_ms": table[:, 1].tolist(),
                                "bytes_received_per_sweep": (table[:, 2] * 4).astype(np.int64).tolist(),
                                "bytes_sent_per_sweep": (table[:, 3] * 4).astype(np.int64).tolist(),
                                "states": table[:, 4].astype(np.int64).tolist()}
        exchange["bit_identical"] = bit_identical
        exchange["ladder_mode"] = os.environ.get("PI_BENCH_MODE")
        exchange["eval_ms_max"], exchange["eval_ms_min"] = float(table[:, 0].max()), float(table[:, 0].min())
        exchange["bytes_received_per_sweep_max"] = int(table[:, 2].max() * 4)
    out = {
        "metric": "state-action Bellman backups/sec",
        "value": value,
        "value_nonterminal": value_nonterminal,
        "unit": "backups/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        **({"rehearsal": f"PI_BENCH_SHARE_GPU=1: {world} rank processes share ONE GPU over the peer-to-peer transport — "
                         f"exercises the N > 1 code path, says nothing about {world} GPUs"} if share_gpu() and world > 1 else {}),
        "config": {"workload": f"{args.env} {D}D grid bins={args.bins}/dim "
                               f"({n} states) x {nA} actions, gamma={solver.config.gamma}; step = {EVAL_PER_STEP} "
                               f"eval sweeps + {IMPROVE_PER_STEP} improve sweep = {backups_per_step} backups; terminal "
                               f"states are counted in `value` ({n - n_live} of {n}: value_nonterminal leaves them out)",
                   "states": n, "nonterminal_states": n_live, "actions": nA, "eval_sweeps_per_step": EVAL_PER_STEP,
                   "improve_sweeps_per_step": IMPROVE_PER_STEP,
                   "parallelism": f"state-range shards x{world}" + (
                       f", {exchange['mode']} exchange of V' per eval sweep over {'peer-to-peer stores' if exchange.get('transport') == 'p2p' else 'RCCL'} inside libpi_mi355"
                       if exchange else "")},
        "time_share_ms": share,
        "eval_backups_per_s": states_per_launch * world / (eval_ms * 1e-3),
        "improve_backups_per_s": states_per_launch * world * nA / (improve_ms * 1e-3),
        "check": {"last_residual": last_delta, "last_changed": last_changed,
                  "vgpr_eval": eng.info(4), "vgpr_improve": eng.info(5),
                  "eval_threads_per_workgroup": eng.info(11), "eval_chunks_per_workgroup": eng.info(3),
                  "improve_threads_per_workgroup": eng.info(12), "improve_chunks_per_workgroup": eng.info(8),
                  "interpolation_reciprocal_division": [eng.info(20 + d) for d in range(D)],
                  "memory_order": {"order": list(eng.order), "dimensions": [solver._bin_keys[d] for d in eng.order],
                                   "note": "device arrays hold the grid with its dimensions in this order (slowest first); "
                                           "host-side arrays and all arithmetic stay in the env's own order"},
                  "exchange": exchange},
    }

    # ── --full: everything beyond the headline, outside the timed region ──────────────────────
    extra_configs, extra_skipped = [], []
    full_runs, full_runs_skipped = {}, []
    if args.full:
        # Grids with many terminal states: the library listed the live states (pi_prepare_mask) and the later
        # sweeps of a batch / the improvement sweeps run pi_eval_live_kernel / pi_improve_live_kernel over them.
        # Their own launch time: (a 21-sweep batch - a 1-sweep batch) / 20, outside the timed region.
        live_states = eng.info(16) if world == 1 else 0
        first_ms = live_ms = None
        if live_states > 0:
            def batch_ms(k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                solver._evaluation_sweeps(k, gamma)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            batch_ms(2)
            first_ms = min(batch_ms(1) for _ in range(3))
            live_ms = (min(batch_ms(21) for _ in range(2)) - first_ms) / 20.0
        live_per_launch = (states_per_launch - int(solver.d_terminal_mask[solver._s_begin:solver._s_end].sum().item()))

        # ── the evaluation sweep on a policy-iteration state (what a real run() sweeps) ──────────
        converged = None
        if world == 1 and not args.no_converged_state:
            solver.d_value_function.zero_()
            solver.d_new_value_function.zero_()
            solver.d_policy.zero_()
            keep = solver.config.max_eval_iter
            solver.config.max_eval_iter = 2000
            t_prep = time.perf_counter()
            for _ in range(3):
                solver.policy_evaluation()
                solver.policy_improvement()
            solver.config.max_eval_iter = keep
            torch.cuda.synchronize()
            t_prep = time.perf_counter() - t_prep
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            solver._evaluation_sweeps(10, gamma)
            e0.record()
            solver._evaluation_sweeps(50, gamma)
            e1.record()
            e1.synchronize()
            converged = {"ms": e0.elapsed_time(e1) / 50, "state": "3 policy-iteration rounds from V = 0, "
                         "policy = 0 with at most 2000 evaluation sweeps each", "prepare_seconds": t_prep,
                         "residual": float(solver._d_delta.item())}

        # ── the other single-GPU BASELINE configs on the same clock (N = 1, default config only) ──────────────
        khash = _native.kernel_source_hash()
        t_start = T_PROCESS_START
        cpu_cost = 0.0 if args.no_cpu_baseline else 25.0
        if world == 1 and not args.no_extra_configs and (args.env, args.bins) == (ENV, BINS):
            # the headline's device arrays are not needed while the extras run (25^6 wants ~4 GB): keep them, 288 GB is plenty
            for label, x_env, x_bins, x_steps, x_warm in EXTRA_CONFIGS:
                spent = time.perf_counter() - t_start
                if spent + EXTRA_COST_S[label] + cpu_cost > args.time_budget:
                    extra_skipped.append({"label": label, "reason": f"time budget: {spent:.0f} s spent of {args.time_budget:.0f}"})
                    continue
                try:
                    extra_configs.append(measure_extra_config(label, x_env, x_bins, x_steps, x_warm, dev, khash))
                except Exception as exc:                  # never lose the headline over an extra
                    extra_skipped.append({"label": label, "reason": repr(exc)})

        # ── sweeps-to-converge: full run()s from the envs' initial states with their own settings (N = 1, outside the timed
        # region).  Default config: C3 -> C4 (the headline, `sweeps_to_converge`) -> C5, each only while its estimate fits the
        # time budget; another --env / --bins: that config alone.  Digests of V and the policy are compared with the committed ones.
        full_run = None
        if world == 1 and not args.no_full_run:
            default_cfg = (args.env, args.bins) == (ENV, BINS)
            plan = FULL_RUNS if default_cfg else [("this", args.env, args.bins, 0.0)]
            for label, r_env, r_bins, est in plan:
                spent = time.perf_counter() - t_start
                if not default_cfg and n >= (1 << 27) and not args.full_run:
                    full_runs_skipped.append({"label": label, "reason": f"{n} states: a run to convergence takes minutes; pass --full-run"})
                    continue
                if not args.full_run and spent + est + cpu_cost > args.time_budget:
                    full_runs_skipped.append({"label": label, "reason": f"time budget: {spent:.0f} s spent of {args.time_budget:.0f}, "
                                                                        f"this run needs ~{est:.0f} s; pass --full-run "
                                                                        f"(profiles/r05/full_runs.txt holds the measured runs)"})
                    continue
                try:
                    full_runs[label] = run_to_convergence(label, r_env, r_bins, dev)
                except Exception as exc:                  # never lose the timed result over an extra run
                    full_runs[label] = {"error": repr(exc)}
            key = "c4" if default_cfg else "this"
            full_run = full_runs.get(key) or next(({"skipped": x["reason"]} for x in full_runs_skipped if x["label"] == key), None)
            for x in extra_configs:                       # C3 / C5: beside their sweep timings as well
                if x["label"] in full_runs and "full_run" not in x:
                    x["full_run"] = full_runs[x["label"]]

        # ── roofline ──────────────────────────────────────────────────────────────────────────
        prof, prof_path = (None, None) if minimal else load_profile(args.env, args.bins, n, khash, order=eng.order)
        # N > 1: the committed profile is the single-GPU launch of the same kernel; per-wave figures carry over, the number
        # of waves (and every per-launch total) scales with this rank's share of the states
        prof_scale = states_per_launch / float(n)
        bytes_eval = algorithmic_bytes_eval(D)
        bytes_improve = 4 * (1 << D) + (4 * D + 1 + 4) / nA
        # cache-perfect HBM bytes of one evaluation sweep: every V value read once (4) + V' written (4) + the policy entry (4),
        # + the mask byte on grids that have terminal states (the old-value stream is read on residual sweeps only, 1 in 25)
        compulsory_per_state = 12.0 if solver._mask_arg() is None else 13.0
        compulsory = compulsory_per_state * states_per_launch

        def kernel_entry(name, ms, backups, alg_bytes_per_backup, counters=None):
            return kernel_units(name, ms, backups, alg_bytes_per_backup, prof=prof, prof_scale=prof_scale, n=n, n_live=n_live,
                                live_per_launch=live_per_launch, states_per_launch=states_per_launch, counters=counters)

        if live_states > 0:
            kernels = {
                "eval_sweep": kernel_entry("pi_eval_live_kernel", live_ms, states_per_launch, bytes_eval),
                "eval_sweep_first_of_batch": kernel_entry("pi_eval_sweep_kernel", first_ms, states_per_launch, bytes_eval),
                "improve_sweep": kernel_entry("pi_improve_live_kernel", improve_ms, states_per_launch * nA, bytes_improve),
            }
            kernels["eval_sweep"]["live_states"] = live_states
            kernels["eval_sweep"]["batch_average_ms"] = eval_ms
        else:
            kernels = {
                "eval_sweep": kernel_entry("pi_eval_sweep_kernel", eval_ms, states_per_launch, bytes_eval),
                "improve_sweep": kernel_entry("pi_improve_sweep_kernel", improve_ms, states_per_launch * nA, bytes_improve),
            }
        if converged:
            # the same units for the policy-iteration state, from ITS committed counters
            rprof, rpath = load_profile(args.env, args.bins, n, khash, "real", order=eng.order)
            if rprof:
                conv = kernel_entry("pi_eval_sweep_kernel", converged["ms"], states_per_launch, bytes_eval,
                                    counters=rprof.get("kernels", {}))
                converged["profile"] = rpath
                converged["units"] = conv.get("units")
            kernels["eval_converged_policy"] = converged
        dom = kernels["eval_sweep"] if share["eval_sweeps"] >= share["improve_sweep"] else kernels["improve_sweep"]
        roofline = build_roofline(dom, khash, prof_path, compulsory_per_state, compulsory, None if world == 1 else prof_scale)
        alg_gbps = dom["algorithmic"]["achieved_GBps"]
        roofline_algorithmic = {"bound": "hbm", "kernel": dom["kernel"], "achieved": alg_gbps, "peak": HBM_PEAK_GBS,
                                "unit": "GB/s", "frac": None, "ratio_to_hbm_peak": alg_gbps / HBM_PEAK_GBS,
                                "bytes_per_backup": dom["algorithmic"]["bytes_per_backup"],
                                "note": "SURVEY 8(d)'s algorithmic bytes over the launch time: above the HBM peak because the 2^D "
                                        "corner reads are L1 / L2 / Infinity-Cache hits; not a bound, no fraction is claimed "
                                        "against it — the measured HBM-side fraction is roofline.frac"}
        out.update({"roofline": roofline, "roofline_algorithmic": roofline_algorithmic, "kernels": kernels,
                    "sweeps_to_converge": full_run, "full_runs": full_runs, "full_runs_skipped": full_runs_skipped,
                    "extra_configs": extra_configs, "extra_configs_skipped": extra_skipped})
        if extra_configs:
            out["roofline"]["extra_configs"] = {
                x["label"]: {"env": x["env"], "bins": x["bins"], "eval_ms": round(x["eval_ms"], 5), "improve_ms": round(x["improve_ms"], 5),
                             "backups_per_s": float(f"{x['backups_per_s']:.4g}"), "frac_hbm": x["roofline"]["frac_hbm"],
                             "hbm_frac_raw": x["roofline"]["hbm_frac_raw"], "valu_frac": x["roofline"]["valu_frac"],
                             "l1_load_issue_frac": x["roofline"]["l1_load_issue_frac"],
                             "frac_hbm_compulsory": x["roofline"].get("frac_hbm_compulsory"),
                             "traffic_vs_compulsory": x["roofline"].get("traffic_vs_compulsory"),
                             "floor": x["roofline"].get("floor"), "frac_of_floor": x["roofline"].get("frac_of_floor")}
                for x in extra_configs}
        if rank == 0 and not args.no_cpu_baseline and not minimal and os.environ.get("PI_BENCH_BONUS") != "1":   # rank 0's host cores; the other ranks wait at the barrier below
            out["cpu_baseline"] = cpu_baseline(args.env, args.bins, args.cpu_sample)
    if rank == 0:
        print(json.dumps(out), flush=True)
        if extra_configs or extra_skipped:       # and in short on stderr, where a truncated log still shows it
            brief = [f"{x['label']}: eval {x['eval_ms']:.4f} ms, improve {x['improve_ms']:.4f} ms, {x['backups_per_s']:.3e} backups/s, "
                     f"frac_hbm {x['roofline']['frac_hbm']}" for x in extra_configs]
            print("bench.py extra_configs | " + " | ".join(brief + [f"{x['label']}: skipped ({x['reason']})" for x in extra_skipped]),
                  file=sys.stderr, flush=True)
        if full_runs or full_runs_skipped:
            brief = [f"{k}: {v.get('eval_sweeps')} sweeps in {v.get('pi_iterations')} rounds, {v.get('seconds', float('nan')):.2f} s, "
                     f"digests {'match' if v.get('matches_committed_digests') else v.get('matches_committed_digests')}"
                     if "error" not in v else f"{k}: {v['error']}" for k, v in full_runs.items()]
            print("bench.py full_runs | " + " | ".join(brief + [f"{x['label']}: skipped ({x['reason']})" for x in full_runs_skipped]),
                  file=sys.stderr, flush=True)
    if world > 1:
        # tear down in a defined order: drain the GPU, let every rank arrive, destroy the library's
        # RCCL communicator (it dies with the engine handle), then torch's process group
        torch.cuda.synchronize()
        dist.barrier()
        solver._backend.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
