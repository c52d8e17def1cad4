"""tools/accel_bench.py — Anderson-accelerated policy evaluation against the plain loop.

    python tools/accel_bench.py --cpu [--cases pendulum:50 ...] [--out FILE]     # no GPU: checker backend + numpy twin
    python tools/accel_bench.py --gpu [--cases C2 C3 C4] [--window 4] [--out FILE]

--cpu: whole run() calls on the CPU checker backend (tests/accel_backend.py: the oracle's sweeps and the twin of the two
kernels), plain and with windows 2, 4 and 8 — rounds, evaluation sweeps, extrapolations, restarts, and max|dV| between the
accelerated and the plain result against 2 theta gamma / (1 - gamma).  The sizes a CPU can sweep to convergence.
--gpu: the BASELINE configs to convergence on the device, plain and accelerated in the same process, interleaved
(plain, accelerated, plain, accelerated; the accelerated run is run()'s loop spelled out round by round so that it can
report progress and stop at --budget); wall seconds of run(), sweeps, rounds, and the two kernels alone by HIP events
on the config's own array sizes with their bytes/s as a fraction of 8 TB/s.  Whatever comes out is written, a loss included.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np

from dynamicprogramming_amd import accel, envs
from dynamicprogramming_amd.solver import CudaPIConfig

CPU_CASES = [("pendulum", (50, 50)), ("pendulum", (200, 200)), ("mountain_car", (60, 60)),
             ("cartpole_swingup", (9, 7, 11, 5)), ("cartpole_swingup", (15, 15, 15, 15)), ("double_cartpole", (7,) * 6)]
GPU_CASES = {"C2": ("pendulum", 200), "C3": ("cartpole_swingup", 50), "C4": ("double_pendulum_swingup", 80),
             "C5": ("double_cartpole", 25)}
HBM_BYTES_PER_S = 8.0e12
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def bins_for(name, shape):
    """The env's reference ranges with shape[d] points in dimension d."""
    cls = envs.ENVS[name]
    return {key: np.asarray(cls.bins_space(int(g))[key], dtype=np.float32) for key, g in zip(cls.bins_space(2), shape)}


def cpu_case(name, shape, windows):
    from tests.accel_backend import with_accel_backend
    cls = with_accel_backend(envs.ENVS[name])
    cfg = CudaPIConfig(**envs.ENVS[name].CONFIG)
    label = f"{name} {'x'.join(str(g) for g in shape)}, gamma {cfg.gamma}"
    bound = 2 * cfg.theta * cfg.gamma / (1 - cfg.gamma)
    plain = None
    for window in [0] + list(windows):
        solver = cls(bins_for(name, shape), envs.ENVS[name].ACTIONS, CudaPIConfig(**envs.ENVS[name].CONFIG))
        if window:
            solver.set_acceleration(accel.Anderson(window=window))
        t0 = time.perf_counter()
        solver.run()
        st = solver.stats
        row = (f"  {label:44s} {'plain' if not window else f'm = {window}':6s} rounds {st['pi_iterations']:3d}  sweeps {st['eval_sweeps']:7d}  "
               f"extrapolations {st.get('accel_extrapolations', 0):5d}  restarts {st.get('accel_restarts', 0):3d}  stable={st.get('stable')}")
        if plain is None:
            plain = solver
        else:
            row += (f"  x{plain.stats['eval_sweeps'] / st['eval_sweeps']:.2f}  max|dV| {np.abs(solver.value_function - plain.value_function).max():.3e}"
                    f" (bound {bound:.3e})  policy agreement {(solver.policy == plain.policy).mean():.6f}")
        say(row + f"  [{time.perf_counter() - t0:.0f} s]")


def time_kernels(solver, window):
    """pi_accel_update and pi_accel_combine alone on arrays of this grid's size: a warm-up launch, then the median of 5
    launches between HIP events.  Bytes: update reads x, g, f_prev, g_prev and k - 1 columns of dF and writes f_prev, g_prev
    and one column of each ring: (7 + k) floats per state; combine reads g and k columns and writes V: (2 + k) floats."""
    import torch
    n, dev, eng = solver.n_states, solver.d_value_function.device, solver._backend.engine
    gen = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32).to(dev)   # noqa: E731
    x, g, fp, gp = rnd(n), rnd(n), rnd(n), rnd(n)
    dF, dG = rnd(window, n), rnd(window, n)
    d_dots = torch.zeros(18, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    k = window

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    up = timed(lambda: eng.accel_update(x.data_ptr(), g.data_ptr(), fp.data_ptr(), gp.data_ptr(), dF.data_ptr(), dG.data_ptr(),
                                        window, k - 1, k, False, n, d_dots.data_ptr(), st))
    co = timed(lambda: eng.accel_combine(g.data_ptr(), dG.data_ptr(), [0.1] * k, k, n, g.data_ptr(), st))
    for label, ms, floats in (("pi_accel_update", up, 7 + k), ("pi_accel_combine", co, 2 + k)):
        rate = floats * 4 * n / (ms * 1e-3)
        say(f"    {label:17s} k = {k}: {ms:8.3f} ms per call, {floats * 4} B/state -> {rate / 1e9:7.1f} GB/s = "
            f"{rate / HBM_BYTES_PER_S:.3f} of 8 TB/s")


def run_rounds(solver, budget):
    """run() spelled out round by round (what run() does whenever the one-launch path is not taken), with a line per ten
    rounds and a wall-clock budget: a run that exceeds it is stopped after the round in flight and reported as unfinished."""
    t0 = time.perf_counter()
    cfg, finished = solver.config, True
    solver.stats["stable"] = False
    for n in range(cfg.max_pi_iter):
        solver.policy_evaluation()
        solver.stats["pi_iterations"] = n + 1
        if solver.policy_improvement():
            solver.stats["stable"] = True
            break
        if (n + 1) % 10 == 0:
            say(f"      ... round {n + 1}: {solver.stats['eval_sweeps']} sweeps, {time.perf_counter() - t0:.1f} s")
        if time.perf_counter() - t0 > budget:
            finished = False
            break
    solver._pull_tensors_from_gpu()
    return finished


def gpu_case(label, window, repeats, budget):
    import torch
    name, bins = GPU_CASES[label]
    say(f"{label}: {name} {bins}^{envs.ENVS[name]._D}, window {window}")
    results = {}
    for rep in range(repeats):
        for mode in ("plain", "accelerated"):
            solver = envs.make(name, bins)
            if mode == "accelerated":
                solver.set_acceleration(accel.Anderson(window=window))
                if rep == 0:
                    time_kernels(solver, window)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            finished = True
            if mode == "accelerated":
                finished = run_rounds(solver, budget)
            else:
                solver.run()
            dt = time.perf_counter() - t0
            st = solver.stats
            if not finished:
                say(f"    {mode:12s} run {rep}: STOPPED UNFINISHED after the --budget of {budget:.0f} s")
            say(f"    {mode:12s} run {rep}: {dt:8.2f} s  rounds {st['pi_iterations']:4d}  eval sweeps {st['eval_sweeps']:7d}  "
                f"extrapolations {st.get('accel_extrapolations', 0):5d}  restarts {st.get('accel_restarts', 0):3d}  "
                f"stable={st.get('stable')}")
            results[mode] = (solver, dt)
    (p, tp), (a, ta) = results["plain"], results["accelerated"]
    cfg = p.config
    say(f"    last pair: wall x{tp / ta:.2f}, sweeps x{p.stats['eval_sweeps'] / a.stats['eval_sweeps']:.2f}; policy agreement "
        f"{(p.policy == a.policy).mean():.6f}, max|dV| {np.abs(p.value_function - a.value_function).max():.3e} "
        f"(2 theta gamma / (1 - gamma) = {2 * cfg.theta * cfg.gamma / (1 - cfg.gamma):.3e})")
    say()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cases", nargs="+", default=None)
    ap.add_argument("--windows", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--budget", type=float, default=240.0, help="--gpu: wall seconds after which an accelerated run is stopped")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.cpu:
        cases = CPU_CASES if args.cases is None else [(c.split(":")[0], tuple(int(g) for g in c.split(":")[1].split("x")))
                                                      for c in args.cases]
        say("accelerated against plain policy iteration on the CPU checker backend — python tools/accel_bench.py --cpu"
            + (" --cases " + " ".join(args.cases) if args.cases else ""))
        for name, shape in cases:
            cpu_case(name, shape, args.windows)
            if args.out:
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text("\n".join(LINES) + "\n")
    if args.gpu:
        import torch
        labels = args.cases or ["C2", "C3", "C4"]
        say(f"accelerated against plain policy iteration — {torch.cuda.get_device_name(0)}, one process, interleaved, "
            f"python tools/accel_bench.py --gpu --cases {' '.join(labels)} --window {args.window} --repeats {args.repeats}")
        say("run() wall seconds exclude construction (kernel compilation, allocation); theta, gamma and limits are the envs' own.")
        say()
        for label in labels:
            gpu_case(label, args.window, args.repeats, args.budget)
            if args.out:
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
