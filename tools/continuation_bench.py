"""tools/continuation_bench.py — grid continuation against a cold start, on the BASELINE configs (GPU box).

For every case, in ONE process: the cold run() on the fine grid; then the chain of coarse runs, each level continued from
the one before it (solver.continue_from), and the fine run continued from the last.  Per piece rounds, evaluation sweeps
and wall seconds of run(); the resample kernel alone by HIP events after a warm-up launch, with its bytes/s on the
compulsory traffic (V and policy written, the mask read where the grid has terminal states: 8-9 B per destination state)
as a fraction of 8 TB/s; policy agreement and max|dV| between the cold and the continued result.

    python tools/continuation_bench.py [--big] [--out profiles/r08/continuation.txt]

Cases: C3 (cartpole_swingup 50^4 from 25^4), C4 (double_pendulum_swingup 80^4 from 40^4, and the cascade 20 -> 40 -> 80);
--big adds C5 (double_cartpole 25^6 from 13^6).  Whatever comes out is written, a loss included.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from dynamicprogramming_amd import envs
from utils.barycentric import DevicePolicy, action_map

CASES = [("C3", "cartpole_swingup", [25], 50), ("C4", "double_pendulum_swingup", [40], 80),
         ("C4 cascade", "double_pendulum_swingup", [20, 40], 80)]
BIG = [("C5", "double_cartpole", [13], 25)]
HBM_BYTES_PER_S = 8.0e12

LINES = []
COLD = {}


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def run(solver):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    solver.run()
    dt = time.perf_counter() - t0
    st = solver.stats
    return dict(rounds=st["pi_iterations"], sweeps=st["eval_sweeps"], seconds=dt, stable=st.get("stable"))


def piece(label, r):
    say(f"    {label:28s} rounds {r['rounds']:4d}  eval sweeps {r['sweeps']:7d}  run() {r['seconds']:8.2f} s  stable={r['stable']}")


def time_resample(source, solver):
    """The kernel alone: a warm-up launch, then one launch between two HIP events, into the solver's own arrays (what
    continue_from is about to write there anyway)."""
    dev = solver.d_value_function.device
    dp = DevicePolicy(source.policy, source.action_space, source.bounds_low, source.bounds_high, source.grid_shape,
                      source.strides, source.corner_bits, device=dev)
    try:
        dp.set_values(source.value_function)
        args = (solver._bins, solver._memory_strides(), solver._mask_arg(), solver.d_value_function, solver.d_policy)
        kw = dict(action_map=action_map(source.action_space, solver.action_space), n_actions=solver.n_actions)
        dp.resample(*args, **kw)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dp.resample(*args, **kw)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
    finally:
        dp.close()
    per_state = 8 + (1 if solver._mask_arg() is not None else 0)
    rate = per_state * solver.n_states / (ms * 1e-3)
    say(f"    resample {'x'.join(str(int(g)) for g in source.grid_shape)} -> {'x'.join(str(int(g)) for g in solver.grid_shape)}: "
        f"kernel {ms:.3f} ms, {per_state} B/state compulsory -> {rate / 1e9:.1f} GB/s = {rate / HBM_BYTES_PER_S:.3f} of 8 TB/s")
    return ms * 1e-3


def case(label, name, coarse_bins, fine_bins):
    D = envs.ENVS[name]._D
    say(f"{label}: {name} {fine_bins}^{D} from {' -> '.join(f'{b}^{D}' for b in coarse_bins)}")
    if (name, fine_bins) not in COLD:                     # the cascade shares the cold run of its config
        cold = envs.make(name, fine_bins)
        COLD.clear()
        COLD[(name, fine_bins)] = (cold, run(cold))
    cold, r_cold = COLD[(name, fine_bins)]
    piece(f"cold {fine_bins}^{D}", r_cold)
    total, previous = 0.0, None
    for bins in coarse_bins + [fine_bins]:
        solver = envs.make(name, bins)
        if previous is not None:
            total += time_resample(previous, solver)
            solver.continue_from(previous)
        r = run(solver)
        piece(("continued " if previous is not None else "coarse ") + f"{bins}^{D}", r)
        total += r["seconds"]
        previous = solver
    agree = float((previous.policy == cold.policy).mean())
    gap = float(np.abs(previous.value_function - cold.value_function).max())
    say(f"    continued chain {total:.2f} s (runs + resample kernels) against cold {r_cold['seconds']:.2f} s: "
        f"x{r_cold['seconds'] / total:.2f}; fine-grid sweeps {r['sweeps']} against {r_cold['sweeps']}")
    say(f"    policy agreement {agree:.6f}, max|dV| {gap:.3e}")
    say()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--big", action="store_true", help="also C5 (double_cartpole 25^6 from 13^6)")
    ap.add_argument("--out", type=Path, default=Path("profiles/r08/continuation.txt"))
    args = ap.parse_args()
    say(f"grid continuation against a cold start — {torch.cuda.get_device_name(0)}, one process, "
        f"python tools/continuation_bench.py{' --big' if args.big else ''}")
    say("run() wall seconds exclude construction (kernel compilation, allocation); theta, gamma and limits are the envs' own.")
    say()
    for c in CASES + (BIG if args.big else []):
        case(*c)
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
