"""tools/expect_bench.py — what the expected Bellman backup over a disturbance set costs and what it buys, on one MI355X
(pi_set_disturbances / pi_expect_*, csrc/pi_expect_kernels.hip; dynamicprogramming_amd/noise.py).

Sweep time per kind: on C3 (cartpole swing-up 50^4 x 5 actions), C4 (double pendulum 80^4 x 11) and C5 (double cart-pole
25^6 x 3), for K = 1 (the zero set), 9 and 27 state-only points (Disturbances.uniform, 3 nodes in 2 / 3 dimensions at half a
cell width) and a 3-action x 9-state set (K = 27, a tenth of the action range): one evaluation sweep (a batch of four,
divided by four), one improvement sweep and one value sweep through the expectation entry points, beside the
deterministic entry point of the same kind on the same handle in the same process — csrc/pi_sweep_kernels.hip is
byte-identical to the parent commit's, so that IS the parent's sweep.  Seeded random V and policy (timing needs no
training).  Each figure is the best of --repeat timings (device events around the call, a synchronise at the end), the
two paths alternating, after one warm-up of each.  "x K" is the ratio to K deterministic sweeps: a backup that repeated
the deterministic one K times would be at 1.00.

Closed-loop effect: cartpole swing-up 50^4 and pendulum 200^2, trained twice with the same caps — nominal, and with
Disturbances.uniform of the rollout's noise (solver.set_disturbances) — then both policies rolled out under
solver.rollout(action_noise=..., state_noise=...) with the same noise, seed and starts, 4 096 episodes of --steps
steps: mean return and the share of episodes that terminated.

--risk worst adds the WORST-CASE backup over the same sets (pi_robust_*, the same module; solver.set_disturbances(d,
risk="worst")): the sweep table gains C2 (pendulum 200^2 x 21), the worst-case sweep timed in the same alternation, and the
spread (max - min) of the expectation sweep's own --repeat samples, the margin the two are compared within; the closed
loop trains a third, worst-case table under the same caps.  The table then goes to profiles/r16/robust.txt.

The driver (no --part) runs every part in a child process of its own under `timeout -k 10`, one after the other, and
stops at the first child that fails.  The table goes to --out.
usage: python tools/expect_bench.py [--out profiles/r11/expected_backup.txt] [--repeat 5] [--steps 1000] [--risk worst]
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CONFIGS = {"c2": ("pendulum", 200), "c3": ("cartpole_swingup", 50), "c4": ("double_pendulum_swingup", 80), "c5": ("double_cartpole", 25)}
# closed loop: env -> (bins, action noise as a share of the action range, state noise per dimension in cell widths,
# training caps).  Velocities are disturbed (a push), positions are not.
LOOPS = {"pendulum": (200, 0.2, (0.0, 1.0), dict(max_eval_iter=2000, max_pi_iter=30)),
         "cartpole_swingup": (50, 0.2, (0.0, 1.0, 0.0, 1.0), dict(max_eval_iter=2000, max_pi_iter=20))}
CHILD_SECONDS = 400


def _sets(D, cell, arange):
    from dynamicprogramming_amd.noise import Disturbances
    half = 0.5 * cell
    dims = lambda k: [half[d] if d < k else 0.0 for d in range(D)]      # noqa: E731
    return [("K=1 (zero set)", Disturbances.none(D)),
            ("K=9 state", Disturbances.uniform(D, state_noise=dims(2), points=3)),
            ("K=27 state", Disturbances.uniform(D, state_noise=dims(3), points=3)),
            ("K=27 3 action x 9 state", Disturbances.uniform(D, state_noise=dims(2), action_noise=0.1 * arange, points=3))]


def part_sweeps(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    env, bins = CONFIGS[args.config]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    acts = np.asarray(cls.ACTIONS, np.float32)
    lo, hi = np.array([t.min() for t in tabs], np.float64), np.array([t.max() for t in tabs], np.float64)
    cell = (hi - lo) / (np.array([len(t) for t in tabs]) - 1)
    eng = _native.Engine(D, [len(t) for t in tabs], lo, hi, tabs, acts, device=0)
    eng.compile(envs.dynamics_source(env))
    n = eng.n_states
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    Va = torch.randn(n, device=dev, generator=gen) * 30.0
    Vb = Va.clone()
    pol = torch.randint(0, len(acts), (n,), device=dev, generator=gen, dtype=torch.int32)
    gamma = float(np.float32(cls.CONFIG["gamma"]))
    p = [t.data_ptr() for t in (Va, Vb, pol)]

    def calls(prefix):                                         # "": deterministic, "expect_", "robust_"
        fn = lambda name: getattr(eng, prefix + name)          # noqa: E731
        return {"eval": (lambda: fn("eval_sweeps")(p[0], p[1], p[2], 0, 0, n, gamma, 4), 4),
                "improve": (lambda: fn("improve_sweep")(p[0], p[2], 0, 0, n, gamma), 1),
                "value": (lambda: fn("value_sweep")(p[0], p[1], p[2], 0, 0, n, gamma), 1)}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    rows = []
    for label, d in _sets(D, cell, float(acts.max() - acts.min())):
        eng.set_disturbances(d.action_offsets, d.state_offsets, d.weights)
        for kind in ("eval", "improve", "value"):
            (det, per), (exp, _) = calls("")[kind], calls("expect_")[kind]
            worst = calls("robust_")[kind][0] if args.risk == "worst" else None
            det(), exp()                                       # warm-up of both paths
            if worst:
                worst()
            t_det, t_exp, t_worst = [], [], []
            for _ in range(args.repeat):                       # alternating, so that drift hits both alike
                t_det.append(timed(det) / per)
                t_exp.append(timed(exp) / per)
                if worst:
                    t_worst.append(timed(worst) / per)
            rows.append({"set": label, "K": d.K, "kind": kind, "det_ms": min(t_det), "expect_ms": min(t_exp),
                         "det_ms_all": t_det, "expect_ms_all": t_exp})
            if worst:
                rows[-1].update({"worst_ms": min(t_worst), "worst_ms_all": t_worst})
    print(json.dumps({"config": args.config, "env": env, "bins": bins, "D": D, "actions": len(acts), "states": n, "rows": rows}))


def part_loop(args):
    import time
    import numpy as np
    from dynamicprogramming_amd import envs
    from dynamicprogramming_amd.noise import Disturbances
    from dynamicprogramming_amd.solver import CudaPIConfig
    env = args.env
    bins, a_share, x_cells, caps = LOOPS[env]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float64) for b in cls.bins_space(bins).values()]
    cell = np.array([(t.max() - t.min()) / (len(t) - 1) for t in tabs])
    acts = np.asarray(cls.ACTIONS, np.float64)
    a_noise = a_share * float(acts.max() - acts.min())
    x_noise = [float(c * w) for c, w in zip(x_cells, cell)]
    cfg = CudaPIConfig(**{**cls.CONFIG, **caps})
    starts = cls.start_states(np.random.default_rng(args.seed), 4096)
    out = {"env": env, "bins": bins, "action_noise": a_noise, "state_noise": x_noise, "caps": caps, "steps": args.steps, "runs": {}}
    rule = Disturbances.uniform(len(tabs), state_noise=x_noise, action_noise=a_noise)
    tables = [("nominal", None, {}), ("noise-aware", rule, {})] + ([("worst-case", rule, {"risk": "worst"})] if args.risk == "worst" else [])
    for label, d, risk in tables:
        solver = envs.make(env, bins, cfg, device="cuda:0", transport=False)
        if d is not None:
            solver.set_disturbances(d, **risk)
        t0 = time.perf_counter()
        solver.run()
        seconds = time.perf_counter() - t0
        run = {"K": 0 if d is None else d.K, "train_seconds": seconds, "pi_iterations": solver.stats["pi_iterations"],
               "eval_sweeps": solver.stats["eval_sweeps"], "stable": bool(solver.stats.get("stable"))}
        for world, kw in (("noisy", dict(action_noise=a_noise, state_noise=x_noise, seed=args.seed)), ("noise-free", {})):
            res = solver.rollout(starts, args.steps, gamma=1.0, **kw)
            run[world] = {"mean_return": float(np.mean(res.returns)), "terminated_share": float(np.mean(res.terminated)),
                          "mean_length": float(np.mean(res.lengths))}
        out["runs"][label] = run
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("sweeps", "loop"), default=None)
    ap.add_argument("--config", choices=tuple(CONFIGS), default="c3")
    ap.add_argument("--env", choices=tuple(LOOPS), default="pendulum")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--risk", choices=("expected", "worst"), default="expected")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if args.part == "sweeps":
        return part_sweeps(args)
    if args.part == "loop":
        return part_loop(args)
    worst = args.risk == "worst"
    if args.out is None:
        args.out = ROOT / "profiles" / ("r16/robust.txt" if worst else "r11/expected_backup.txt")
    lines = [("worst-case and expected" if worst else "expected") + " Bellman backup over a disturbance set (tools/expect_bench.py"
             + (" --risk worst)" if worst else ")") + (f", commit {args.commit}" if args.commit else ""),
             "", "sweep time per kind, ms per sweep, best of %d (deterministic = csrc/pi_sweep_kernels.hip, byte-identical to the parent's)" % args.repeat,
             f"{'config':28s} {'set':26s} {'kind':8s} {'det ms':>9s} {'expect ms':>10s} {'x det':>7s} {'x K det':>8s}"
             + (f" {'spread':>8s} {'worst ms':>9s} {'- expect':>9s}" if worst else "")]
    common = ["--repeat", str(args.repeat), "--steps", str(args.steps), "--seed", str(args.seed), "--risk", args.risk]
    parts = [("sweeps", ["--config", c]) for c in CONFIGS if worst or c != "c2"] + [("loop", ["--env", e]) for e in LOOPS]
    loops = []
    for part, extra in parts:
        cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, str(Path(__file__).resolve()), "--part", part] + extra + common
        res = subprocess.run(cmd, capture_output=True, text=True)
        print(f"[expect_bench] {part} {' '.join(extra)}: status {res.returncode}", flush=True)
        if res.returncode != 0:
            lines.append(f"NOT MEASURED: {part} {' '.join(extra)} ended with status {res.returncode}: {res.stderr.strip()[-400:]}")
            break
        r = json.loads(res.stdout.strip().splitlines()[-1])
        if part == "sweeps":
            name = f"{r['config']} {r['env']} {r['bins']}^{r['D']} x {r['actions']}"
            for row in r["rows"]:
                ratio = row["expect_ms"] / row["det_ms"]
                lines.append(f"{name:28s} {row['set']:26s} {row['kind']:8s} {row['det_ms']:9.4f} {row['expect_ms']:10.4f} "
                             f"{ratio:7.2f} {ratio / row['K']:8.2f}")
                if worst:
                    spread = max(row["expect_ms_all"]) - min(row["expect_ms_all"])
                    lines[-1] += f" {spread:8.4f} {row['worst_ms']:9.4f} {row['worst_ms'] - row['expect_ms']:+9.4f}"
        else:
            loops.append(r)
    for r in loops:
        lines += ["", f"closed loop: {r['env']} {r['bins']} bins, action noise {r['action_noise']:.4g}, state noise "
                      f"{[round(x, 5) for x in r['state_noise']]}, caps {r['caps']}, 4096 episodes of {r['steps']} steps",
                  f"{'trained':12s} {'K':>3s} {'train s':>8s} {'PI it':>6s} {'sweeps':>8s} {'stable':>6s} | "
                  f"{'noisy: return':>14s} {'terminated':>10s} {'length':>8s} | {'noise-free: return':>18s} {'terminated':>10s} {'length':>8s}"]
        for label, run in r["runs"].items():
            a, b = run["noisy"], run["noise-free"]
            lines.append(f"{label:12s} {run['K']:3d} {run['train_seconds']:8.2f} {run['pi_iterations']:6d} {run['eval_sweeps']:8d} "
                         f"{str(run['stable']):>6s} | {a['mean_return']:14.3f} {a['terminated_share']:10.4f} {a['mean_length']:8.1f} | "
                         f"{b['mean_return']:18.3f} {b['terminated_share']:10.4f} {b['mean_length']:8.1f}")
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
