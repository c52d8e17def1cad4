"""
Shared command line and training entry point of the runner scripts.

The reference's runners share ONE argparse surface (README.md:323-347; e.g.
runners/pendulum_cuda.py:268-287) plus two crane-only flags (overhead_crane_cuda.py:588-591).
Every flag is accepted here with the reference's name, type and default, so a command line
written for the reference works unchanged:

  solver-side, honoured      --bins N, --retrain, --save-path PATH, crane: --target-x X
  rollout-side, accepted     --render, --record PATH, --random [N], --episodes N, --steps N,
  and ignored (with a note)  --seed N, --no-plot, crane: --start-x X    (but see --rollout below)

One flag is an extension (the reference has no counterpart; off by default): --value-iteration trains with
the fused max-backup sweep of SURVEY.md section 8f.4 instead of policy iteration — the same fixed point
(measured: identical V and policy on the 80^4 double pendulum) in fewer sweeps.

A second extension flag, --rollout (off by default), runs the closed-loop evaluation that follows training in the
reference — on the GPU, all episodes in one kernel launch (solver.rollout): --episodes episodes of --steps steps from
the env's start distribution (envs.<Env>.start_states, seeded by --seed; crane: around --start-x), one line per
episode; those four flags are then honoured, not ignored.  The 6-D swing-up also writes results/last_trajectory.npz
(the last 100 states of every episode), the file the reference's scoring script reads.

--controller {policy,greedy,expected} (extension, default policy) chooses what acts in those episodes: the interpolated
policy table, the greedy one-step lookahead on the interpolated value function (solver.rollout(controller="greedy")), which
needs only V, or that lookahead with the expectation over a disturbance set inside it (solver.rollout(controller=
"expected"); csrc/pi_expect_greedy_kernels.hip).  The set is the solver's — trained with --train-*, or carried by the
archive; failing that it is the rule --action-noise, --state-noise and --train-noise-points name (training_disturbances);
with neither the runner exits with a message.  Unlike greedy, expected runs under --epsilon, --action-noise and
--state-noise.  The printed lines and last_trajectory.npz keep their form.

--epsilon E, --action-noise A and --state-noise X [X ...] (extensions, with --rollout, default 0) make those episodes
stochastic (solver.rollout(epsilon=..., action_noise=..., state_noise=...); csrc/pi_stochastic_kernels.hip): a step takes
a uniformly random action of the env's action set with probability E, every action gains A * u and is clamped to the
set's range, every successor gains X * u per dimension (one X for all dimensions, or one per dimension), u uniform in
[-1, 1).  --seed seeds the starts and this noise.  Without --rollout the three are listed as ignored.

--rollout --random [N] runs the reference's random-policy baseline (evaluate_random(), e.g. pendulum_cuda.py:192-205) on
the GPU: N episodes of --steps steps from the env's start states under uniformly random actions, no training and no
archive, one "[random] Episode k: L steps | reward = R" line each.  Without --rollout, --random keeps skipping training
and doing nothing else.

A third extension flag, --coarse-bins N [N ...] (off by default), trains by grid continuation: the env is solved at
each N in turn — each level started from the previous level's solution interpolated onto its grid
(solver.continue_from) — and then at --bins; sweeps and seconds are printed per level.  Only the --bins solution is saved.

--train-action-noise A, --train-state-noise X [X ...] and --train-noise-points P (extensions, default 0 / none / 3) make
TRAINING noise-aware: the solver plans for the noise model of --action-noise / --state-noise instead of the one
deterministic successor — every sweep backs up the expectation over the tensor Gauss-Legendre rule with P nodes per noisy
quantity (dynamicprogramming_amd.noise.Disturbances.uniform, solver.set_disturbances; csrc/pi_expect_kernels.hip), on
every continuation level.  The set is saved with the policy.  They act on training only: when a saved policy is loaded
instead, a note says that they had no effect.
--rollout --adversary [policy|robust] (extension) runs the episodes against an adversary instead: at every step the worst
point of the policy's disturbance set (the archive's, or the one the --train-*-noise flags name) for the action taken moves
the episode (solver.adversary_rollout; csrc/pi_adversary_kernels.hip), under the policy table or the robust lookahead.
--train-risk worst (extension, default expected) backs up the WORST point of that set instead of its expectation
(solver.set_disturbances(set, risk="worst"): the max-min policy); the archive then carries a `risk` entry.

--accelerate [M] (extension, off by default; M = 4 when the flag stands alone) Anderson-accelerates the policy evaluations
of training: once per batch of 25 sweeps the solver extrapolates over a window of M past batches
(solver.set_acceleration(accel.Anderson(window=M)); csrc/pi_accel_kernels.hip), on every continuation level.  The sweeps,
extrapolations and restarts of every round are printed.  It does not act on --value-iteration, nor with --train-risk worst.

The ignored group drives the reference's gymnasium / pygame / matplotlib evaluation harness, which is
outside the scope of this package: training, saving and loading behave as in
the reference (train when the archive is missing or --retrain is given, otherwise load it), the
rollouts are simply not run.  `--random` skips training like the reference does (it only ever ran
random rollouts).  The hybrid runner of the reference accepts-and-ignores flags the same way
(README.md:346-347).
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]  # repository root: makes `dynamicprogramming_amd` importable
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def bins_space_for(env_name: str, bins: int) -> dict:
    """The env's reference grid ranges with `bins` points per dimension (the reference rebuilds
    BINS_SPACE the same way when --bins is given: pendulum_cuda.py:293-296)."""
    from dynamicprogramming_amd import envs
    return envs.ENVS[env_name].bins_space(bins)


def training_disturbances(env_name: str, action_noise: float = 0.0, state_noise=None, points: int = 3):
    """The disturbance set --train-action-noise / --train-state-noise / --train-noise-points name for this env, or None
    when both amplitudes are zero (deterministic training)."""
    import numpy as np
    from dynamicprogramming_amd import envs
    from dynamicprogramming_amd.noise import Disturbances
    if float(action_noise) == 0.0 and (state_noise is None or not np.any(np.asarray(state_noise, dtype=np.float64) != 0)):
        return None
    return Disturbances.uniform(envs.ENVS[env_name]._D, state_noise=state_noise, action_noise=action_noise, points=points)


def train(env_name: str, bins: int | None = None, save_path: Path | str | None = None,
          value_iteration: bool = False, coarse_bins=(), train_action_noise: float = 0.0, train_state_noise=None,
          train_noise_points: int = 3, train_risk: str = "expected", accelerate: int | None = None, **kw):
    """Build the env on its reference grid, run policy iteration on the GPU, save the .npz
    (reference: each runner's train(), e.g. pendulum_cuda.py:116-130).  value_iteration=True (extension):
    fused value-iteration sweeps to the same theta instead, at most max_pi_iter slices of max_eval_iter.
    coarse_bins (extension): grid continuation — solve at each of these bins per dimension first, every level
    (the last one at `bins`) continued from the one before it.  train_action_noise / train_state_noise /
    train_noise_points (extension): noise-aware training — every level plans for that noise (training_disturbances);
    train_risk="worst" (extension): against the worst point of that set instead of its expectation.
    accelerate (extension): the window of the Anderson acceleration of every policy evaluation (None: off)."""
    from dynamicprogramming_amd import accel, envs
    settings = None
    if accelerate is not None and (value_iteration or (train_risk == "worst" and training_disturbances(
            env_name, train_action_noise, train_state_noise, train_noise_points) is not None)):
        print(f"[{env_name}] note: --accelerate acts on the policy evaluations of expected-value policy iteration only; "
              "it had no effect")
    elif accelerate is not None:
        settings = accel.Anderson(window=int(accelerate))
        print(f"[{env_name}] accelerated policy evaluation: one extrapolation per 25 sweeps over a window of {settings.window}")
    noise = training_disturbances(env_name, train_action_noise, train_state_noise, train_noise_points)
    if noise is not None and train_risk == "worst":
        print(f"[{env_name}] worst-case training: max-min backup over {noise.K} disturbance points")
    elif noise is not None:
        print(f"[{env_name}] noise-aware training: expected backup over {noise.K} disturbance points")
    elif train_risk == "worst":
        print(f"[{env_name}] note: --train-risk worst chooses among the points of the training noise, and neither "
              "--train-action-noise nor --train-state-noise names any: it had no effect, training is deterministic")
    risk = {"risk": "worst"} if train_risk == "worst" else {}
    previous = None
    for level in coarse_bins:
        t0 = time.perf_counter()
        coarse = envs.make(env_name, int(level), **kw)
        if noise is not None:
            coarse.set_disturbances(noise, **risk)
        if settings is not None:
            coarse.set_acceleration(settings)
        if previous is not None:
            coarse.continue_from(previous)
        coarse.run()
        st = coarse.stats
        print(f"[{env_name}] continuation level {int(level)} bins: {st['pi_iterations']} PI iterations, "
              f"{st['eval_sweeps']} eval sweeps in {time.perf_counter() - t0:.2f} s")
        previous = coarse
    solver = envs.make(env_name, bins, **kw)
    if noise is not None:
        solver.set_disturbances(noise, **risk)
    if settings is not None:
        solver.set_acceleration(settings)
    t0 = time.perf_counter()
    if previous is not None:
        solver.continue_from(previous)
    if value_iteration:
        delta = float("inf")
        for _ in range(solver.config.max_pi_iter):
            delta = solver.value_iteration()
            if delta < solver.config.theta:
                break
        solver.stats["stable"] = bool(delta < solver.config.theta)
        solver._pull_tensors_from_gpu()
        dt = time.perf_counter() - t0
        sweeps = solver.stats["value_sweeps"]
        print(f"[{env_name}] value iteration: {sweeps} sweeps in {dt:.2f} s  "
              f"({solver.n_states * solver.n_actions * sweeps / dt:.3e} backups/s), residual {delta:.3e}, "
              f"converged={solver.stats['stable']}")
    else:
        solver.run()
        dt = time.perf_counter() - t0
        st = solver.stats
        backups = solver.n_states * (st["eval_sweeps"] + st["improve_sweeps"] * solver.n_actions)
        print(f"[{env_name}] {st['pi_iterations']} PI iterations, {st['eval_sweeps']} eval sweeps, "
              f"{st['improve_sweeps']} improve sweeps in {dt:.2f} s  ({backups / dt:.3e} backups/s), "
              f"stable={st.get('stable')}")
        if settings is not None:
            for k, (sweeps, (extrapolations, restarts)) in enumerate(zip(st["sweeps_per_iter"], st["accel_per_iter"])):
                print(f"[{env_name}]   round {k + 1}: {sweeps} sweeps, {extrapolations} extrapolations, {restarts} restarts")
    if save_path is not None:
        solver.save(save_path)
    return solver


def build_parser(env_name: str, default_save: str) -> argparse.ArgumentParser:
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env_name]
    p = argparse.ArgumentParser(description=(cls.__doc__ or env_name).strip().splitlines()[0])
    p.add_argument("--render", action="store_true", help="(rollout harness; accepted, ignored)")
    p.add_argument("--random", type=int, nargs="?", const=5, default=None, metavar="N",
                   help="(rollout harness) random-policy baseline: no training, like the reference")
    p.add_argument("--record", type=Path, default=None, metavar="PATH", help="(rollout harness; accepted, ignored)")
    p.add_argument("--episodes", type=int, default=5, help="(rollout harness; accepted, ignored)")
    p.add_argument("--steps", type=int, default=1000, help="(rollout harness; accepted, ignored)")
    if env_name == "overhead_crane":
        p.add_argument("--start-x", type=float, default=2.5, help="(rollout harness; accepted, ignored)")
        p.add_argument("--target-x", type=float, default=-2.5,
                       help="target trolley position (m), compiled into the dynamics (default: -2.5)")
    p.add_argument("--bins", type=int, default=cls.DEFAULT_BINS,
                   help=f"bins per dimension (default: {cls.DEFAULT_BINS})")
    p.add_argument("--seed", type=int, default=42, help="(rollout harness; accepted, ignored)")
    p.add_argument("--no-plot", action="store_true", help="(plots; accepted, ignored)")
    p.add_argument("--retrain", action="store_true", help="force retraining even if a saved policy exists")
    p.add_argument("--save-path", type=Path, default=Path(default_save))
    p.add_argument("--value-iteration", action="store_true",
                   help="(extension) train with fused value-iteration sweeps instead of policy iteration")
    p.add_argument("--coarse-bins", type=int, nargs="+", default=[], metavar="N",
                   help="(extension) grid continuation: solve at each N bins per dimension first, every level started "
                        "from the previous level's interpolated solution, then at --bins")
    p.add_argument("--rollout", action="store_true",
                   help="(extension) after training / loading, roll the policy out on the GPU: --episodes episodes of "
                        "--steps steps from the env's start states (--seed; crane: --start-x), one line per episode")
    p.add_argument("--controller", choices=("policy", "greedy", "expected"), default="policy",
                   help="(extension, with --rollout) what acts in the episodes: the interpolated policy table, the "
                        "greedy one-step lookahead on the interpolated value function, or that lookahead with the "
                        "expectation over the solver's disturbance set (else the rule --action-noise / --state-noise / "
                        "--train-noise-points name) inside it")
    p.add_argument("--epsilon", type=float, default=0.0, metavar="E",
                   help="(extension, with --rollout) probability that a step takes a uniformly random action instead")
    p.add_argument("--action-noise", type=float, default=0.0, metavar="A",
                   help="(extension, with --rollout) actuator noise: A * u, u uniform in [-1, 1), added to every action, "
                        "which is then clamped to the action set's range")
    p.add_argument("--state-noise", type=float, nargs="+", default=None, metavar="X",
                   help="(extension, with --rollout) state disturbance after every step: X * u per dimension (one value "
                        "for every dimension, or one per dimension)")
    p.add_argument("--train-action-noise", type=float, default=0.0, metavar="A",
                   help="(extension) noise-aware training: plan for actuator noise A * u, u uniform in [-1, 1)")
    p.add_argument("--train-state-noise", type=float, nargs="+", default=None, metavar="X",
                   help="(extension) noise-aware training: plan for a state disturbance X * u per dimension after every "
                        "step (one value for every dimension, or one per dimension)")
    p.add_argument("--train-noise-points", type=int, default=3, metavar="P",
                   help="(extension) Gauss-Legendre nodes per noisy quantity of the training noise (default: 3)")
    p.add_argument("--adversary", nargs="?", const="policy", default=None, choices=("policy", "robust"),
                   help="(extension, with --rollout) the disturbance is chosen against the controller at every step, from the "
                        "set the policy was trained with (or the one the --train-*-noise flags name): under the policy "
                        "table (default) or under the robust one-step lookahead")
    p.add_argument("--train-risk", choices=("expected", "worst"), default="expected",
                   help="(extension) what training backs up over the training noise's points: their expectation, or the "
                        "worst of them (max-min: the policy that is best against the worst disturbance)")
    p.add_argument("--accelerate", type=int, nargs="?", const=4, default=None, metavar="M", choices=range(1, 9),
                   help="(extension) Anderson-accelerate the policy evaluations of training: one extrapolation per 25 sweeps "
                        "over a window of M past batches (1 .. 8; 4 when M is left out)")
    return p


def training_noise_requested(args) -> bool:
    return (args.train_action_noise != 0.0 or args.train_state_noise is not None or args.train_noise_points != 3
            or args.train_risk != "expected")


STEADY_WINDOW = 100     # states per episode in results/last_trajectory.npz (the reference's STATS_WINDOW)


def evaluate(env_name: str, pi, episodes: int, steps: int, seed: int, start_x: float | None = None,
             traj_path: Path | None = None, controller: str = "policy", epsilon: float = 0.0, action_noise: float = 0.0,
             state_noise=None, disturbances=None, adversary=None):
    """--rollout: `episodes` closed-loop episodes of at most `steps` steps in one kernel launch (solver.rollout), one
    line each.  `traj_path`: also dump the last min(100, length + 1) states of every episode, concatenated, as the
    reference's evaluate() does for its scoring script (double_cartpole_swingup_cuda.py:583-592).  `controller`:
    "policy", "greedy" or "expected" (--controller; `disturbances`: the set of "expected" when the solver has none).  `epsilon`, `action_noise`, `state_noise` (--epsilon, --action-noise,
    --state-noise): a stochastic rollout, its stream seeded by `seed` like the starts.  `adversary` ("policy" or "robust",
    --adversary): the episodes run against the worst point of `disturbances` (None: the solver's own set) under that
    controller instead (solver.adversary_rollout); the lines keep their form.  Returns the RolloutResult."""
    import numpy as np
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env_name]
    rng = np.random.default_rng(seed)
    kw = {} if start_x is None else {"start_x": start_x}
    starts = cls.start_states(rng, episodes, **kw)
    extra = {} if disturbances is None else {"disturbances": disturbances}
    if adversary is not None:
        res = pi.adversary_rollout(starts, steps, controller=adversary, gamma=1.0,
                                   record_every=1 if traj_path is not None else 0, **extra)
    else:
        res = pi.rollout(starts, steps, gamma=1.0, record_every=1 if traj_path is not None else 0, controller=controller,
                         epsilon=epsilon, action_noise=action_noise, state_noise=state_noise, seed=seed, **extra)
    for ep in range(episodes):
        outcome = "terminated" if res.terminated[ep] else f"{steps} steps"
        final = "  ".join(f"{v:+.4f}" for v in res.states[ep])
        print(f"Episode {ep + 1}: {int(res.lengths[ep])} steps | return = {float(res.returns[ep]):.3f} | {outcome} | "
              f"final state: {final}")
    if traj_path is not None:
        windows = []
        for ep in range(episodes):
            n = int(res.lengths[ep]) + 1                      # rows 0 .. length of this episode: start + every step
            windows.append(res.trajectory[max(0, n - STEADY_WINDOW):n, ep, :])
        traj_path = Path(traj_path)
        traj_path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(traj_path, traj=np.concatenate(windows, axis=0).astype(np.float32), n_episodes=episodes,
                 steps_per_episode=STEADY_WINDOW)
        print(f"[{env_name}] steady-state windows of {episodes} episodes written to {traj_path}")
    return res


def evaluate_random(env_name: str, episodes: int, steps: int, seed: int, start_x: float | None = None, **kw):
    """--rollout --random [N]: the reference's evaluate_random() (e.g. pendulum_cuda.py:192-205) — `episodes` episodes of
    at most `steps` steps under uniformly random actions from the env's action set, from the env's start states — in
    one kernel launch (solver.rollout(controller="random")), one line each in the reference's form.  No training and
    no archive: a random rollout reads no table, so the env's smallest grid serves.  Returns the RolloutResult."""
    import numpy as np
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env_name]
    pi = envs.make(env_name, 2, **kw)
    starts = cls.start_states(np.random.default_rng(seed), episodes, **({} if start_x is None else {"start_x": start_x}))
    res = pi.rollout(starts, steps, gamma=1.0, controller="random", seed=seed)
    for ep in range(episodes):
        print(f"[random] Episode {ep + 1}: {int(res.lengths[ep])} steps | reward = {float(res.returns[ep]):.2f}")
    return res


def ignored_flags(args) -> list:
    """The flags of this command line that nothing here acts on.  --render, --record and --no-plot always; --episodes,
    --steps, --seed, --start-x, --controller, --epsilon, --action-noise and --state-noise unless --rollout runs the
    evaluation they belong to."""
    harness = not args.rollout
    return [f for f, on in (("--render", args.render), ("--record", args.record is not None),
                            ("--episodes", harness and args.episodes != 5), ("--steps", harness and args.steps != 1000),
                            ("--seed", harness and args.seed != 42), ("--no-plot", args.no_plot),
                            ("--start-x", harness and getattr(args, "start_x", 2.5) != 2.5),
                            ("--controller", harness and args.controller != "policy"),
                            ("--epsilon", harness and args.epsilon != 0.0),
                            ("--action-noise", harness and args.action_noise != 0.0),
                            ("--state-noise", harness and args.state_noise is not None),
                            ("--adversary", harness and args.adversary is not None)) if on]


def main(env_name: str, default_save: str, argv=None):
    """Reference control flow (pendulum_cuda.py:289-309): --random -> no training; otherwise load
    the archive when it exists and --retrain is absent, else train and save.  Returns the solver /
    loaded instance (None for --random)."""
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env_name]
    args = build_parser(env_name, default_save).parse_args(argv)
    ignored = ignored_flags(args)
    if ignored:
        print(f"[{env_name}] note: {', '.join(ignored)} belong to the rollout / plot harness, which this "
              "package does not include; accepted and ignored")
    kw = {"target_x": args.target_x} if env_name == "overhead_crane" else {}
    if args.random is not None and args.rollout:
        evaluate_random(env_name, args.random, args.steps, args.seed, start_x=getattr(args, "start_x", None), **kw)
        return None
    if args.random is not None:
        print(f"[{env_name}] --random runs rollouts only (no training) in the reference; nothing to do here")
        return None
    path = Path(args.save_path).with_suffix(".npz")
    if path.exists() and not args.retrain:
        print(f"[+] Loading existing policy from {path}")
        pi = cls.load(path)
        print(f"[{env_name}] {pi.n_states:,} states, {pi.n_actions} actions; use --retrain to recompute")
        if training_noise_requested(args) and not (args.rollout and args.adversary is not None):   # (there they name the set)
            print(f"[{env_name}] note: --train-action-noise, --train-state-noise and --train-noise-points act on training "
                  "only; a saved policy was loaded, so they had no effect"
                  + (" (nor had --train-risk)" if args.train_risk != "expected" else ""))
    else:
        print("[*] Training new policy...")
        pi = train(env_name, args.bins, path, value_iteration=args.value_iteration, coarse_bins=args.coarse_bins,
                   train_action_noise=args.train_action_noise, train_state_noise=args.train_state_noise,
                   train_noise_points=args.train_noise_points, train_risk=args.train_risk, accelerate=args.accelerate,
                   **kw)
    lookahead_set = None
    if args.rollout and args.controller == "expected" and getattr(pi, "disturbances", None) is None:
        lookahead_set = training_disturbances(env_name, args.action_noise, args.state_noise, args.train_noise_points)
        if lookahead_set is None:
            sys.exit(f"[{env_name}] --controller expected needs a disturbance set: train with --train-action-noise / "
                     "--train-state-noise, load an archive that carries one, or give --action-noise / --state-noise")
        print(f"[{env_name}] expected lookahead over {lookahead_set.K} disturbance points of the rollout's noise")
    if args.rollout and args.adversary is not None:
        # the set the adversary chooses from: what the --train-*-noise flags name when given, else the archive's own
        named = training_disturbances(env_name, args.train_action_noise, args.train_state_noise, args.train_noise_points)
        lookahead_set = named if named is not None else getattr(pi, "disturbances", None)
        if lookahead_set is None:
            sys.exit(f"[{env_name}] --adversary needs a disturbance set: load an archive trained with --train-action-noise / "
                     "--train-state-noise, or give those flags")
        print(f"[{env_name}] adversary over {lookahead_set.K} disturbance points, controller: {args.adversary}")
    if args.rollout:
        evaluate(env_name, pi, args.episodes, args.steps, args.seed, start_x=getattr(args, "start_x", None),
                 traj_path=Path("results") / "last_trajectory.npz" if env_name == "double_cartpole_swingup" else None,
                 controller=args.controller, epsilon=args.epsilon, action_noise=args.action_noise,
                 state_noise=args.state_noise, disturbances=lookahead_set, adversary=args.adversary)
    return pi
