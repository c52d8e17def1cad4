"""
runners/hybrid_double_cartpole.py — the hybrid double cart-pole controller: the swing-up policy (±π grid) until both
poles are nearly upright and slow, the balance policy (±23° grid) from then on, with hysteresis; same entry point,
flags and output lines as the reference runner (runners/hybrid_double_cartpole.py).

    python runners/hybrid_double_cartpole.py [--episodes N] [--steps N] [--seed N] [--swingup-path P] [--balance-path P]

It trains nothing: it loads the two archives the double cart-pole runners save and rolls ALL episodes out in one
kernel launch on the swing-up env's dynamics (utils.barycentric.HybridPolicy; csrc/pi_hybrid_kernels.hip), where the
reference makes one get_optimal_action and one _step_python call per step on the CPU (:105-125).  Switch rule and
thresholds are the reference's (_use_balance, :56-69); start states too (:97-98): [0, 0, π, 0, π, 0] with x and x'
moved by U(-0.05, 0.05) from default_rng(seed), in episode order.

Flags: --episodes, --steps, --seed act; --render, --record, --random, --bins, --no-plot, --retrain, --save-path are
accepted and ignored with a note, as the reference's runner ignores the last five.  --swingup-path / --balance-path
are extensions (the reference's paths are fixed).

--epsilon E, --action-noise A and --state-noise X [X ...] (extensions, default 0; the flags of the other runners,
runners/_cli.py) run the same episodes in a noisy world (HybridPolicy.rollout(epsilon=..., action_noise=...,
state_noise=...); csrc/pi_hybrid_stochastic_kernels.hip): a step takes a uniformly random action of the swing-up
policy's action set with probability E, actuator noise A * u is added to every action, X * u to the state after every
step, and the switch rule sees the disturbed state.  The stream is seeded by --seed like the starts, as in the other
runners.  Every episode line then gains switches=N, how often the episode changed its mode, and one summary line
follows: mean reward, share of episodes terminated, share ending in BALANCE, mean switches.  Without these flags the
output is what it was.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]  # repository root: makes `dynamicprogramming_amd` and `utils` importable
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

ENV = "hybrid_double_cartpole"
BALANCE_POLICY_PATH = Path("results/double_cartpole_cuda_policy.npz")
SWINGUP_POLICY_PATH = Path("results/double_cartpole_swingup_cuda_policy.npz")

# the reference's switch box (:56-59) over (x, x', th1, w1, th2, w2): the cart takes no part
INF = float("inf")
ENTER = (INF, INF, 0.32, 4.0, 0.32, 4.0)
LEAVE = (INF, INF, 0.38, 5.0, 0.38, 5.0)

ARCHIVE_KEYS = ("policy", "action_space", "bounds_low", "bounds_high", "grid_shape", "strides", "corner_bits")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Hybrid Double CartPole - DP swing-up + DP balance")
    p.add_argument("--render", action="store_true", help="(rollout harness; accepted, ignored)")
    p.add_argument("--record", type=Path, default=None, metavar="PATH", help="(rollout harness; accepted, ignored)")
    p.add_argument("--episodes", type=int, default=5, help="number of evaluation episodes (default: 5)")
    p.add_argument("--steps", type=int, default=1000, help="max steps per episode (default: 1000)")
    p.add_argument("--seed", type=int, default=42, help="random seed (default: 42)")
    p.add_argument("--random", type=int, nargs="?", const=5, default=None, metavar="N",
                   help="(ignored) the hybrid runner has no random baseline")
    p.add_argument("--bins", type=int, default=None, help="(ignored) policies are loaded with their saved bins")
    p.add_argument("--no-plot", action="store_true", help="(ignored) the hybrid runner produces no plots")
    p.add_argument("--retrain", action="store_true", help="(ignored) the hybrid runner only loads policies")
    p.add_argument("--save-path", type=Path, default=None, help="(ignored) see --swingup-path / --balance-path")
    p.add_argument("--swingup-path", type=Path, default=SWINGUP_POLICY_PATH,
                   help=f"(extension) the swing-up policy archive (default: {SWINGUP_POLICY_PATH})")
    p.add_argument("--balance-path", type=Path, default=BALANCE_POLICY_PATH,
                   help=f"(extension) the balance policy archive (default: {BALANCE_POLICY_PATH})")
    p.add_argument("--epsilon", type=float, default=0.0, metavar="E",
                   help="(extension) probability that a step takes a uniformly random action instead")
    p.add_argument("--action-noise", type=float, default=0.0, metavar="A",
                   help="(extension) actuator noise: A * u, u uniform in [-1, 1), added to every action, "
                        "which is then clamped to the action set's range")
    p.add_argument("--state-noise", type=float, nargs="+", default=None, metavar="X",
                   help="(extension) state disturbance after every step: X * u per dimension (one value "
                        "for every dimension, or one per dimension)")
    return p


def noise_requested(args) -> bool:
    return args.epsilon != 0.0 or args.action_noise != 0.0 or args.state_noise is not None


def ignored_flags(args) -> list:
    return [f for f, on in (("--render", args.render), ("--record", args.record is not None),
                            ("--random", args.random is not None), ("--bins", args.bins is not None),
                            ("--no-plot", args.no_plot), ("--retrain", args.retrain),
                            ("--save-path", args.save_path is not None)) if on]


def start_states(seed: int, episodes: int):
    """(episodes, 6) float32: the reference's starts, drawn in episode order."""
    import numpy as np
    rng = np.random.default_rng(seed)
    states = np.tile(np.array([0.0, 0.0, np.pi, 0.0, np.pi, 0.0], dtype=np.float32), (episodes, 1))
    for ep in range(episodes):
        states[ep, :2] += rng.uniform(-0.05, 0.05, size=2).astype(np.float32)
    return states


def load_tables(path: Path):
    import numpy as np
    d = np.load(path)
    return tuple(d[k] for k in ARCHIVE_KEYS)


def hybrid_policy(swingup_path: Path, balance_path: Path, device="cuda:0"):
    """HybridPolicy(swing-up, balance) with the reference's thresholds on the swing-up env's dynamics."""
    from dynamicprogramming_amd import envs
    from utils.barycentric import DevicePolicy, HybridPolicy
    swingup = DevicePolicy(*load_tables(swingup_path), device=device)
    balance = DevicePolicy(*load_tables(balance_path), device=device)
    swingup.set_dynamics(envs.dynamics_source("double_cartpole_swingup"))
    return HybridPolicy(swingup, balance, ENTER, LEAVE)


def evaluate(n_episodes: int = 3, steps: int = 1000, seed: int = 42, swingup_path: Path = SWINGUP_POLICY_PATH,
             balance_path: Path = BALANCE_POLICY_PATH, noise=None):
    """All episodes in one hybrid launch; one line per episode in the reference's format (:129-134).  `noise`: the
    keywords epsilon, action_noise, state_noise of a stochastic rollout (--epsilon, --action-noise, --state-noise), its
    stream seeded by `seed` like the starts; the lines then carry the switch count and a summary line follows.  Returns
    the HybridRolloutResult (the StochasticHybridRolloutResult)."""
    import numpy as np
    hp = hybrid_policy(swingup_path, balance_path)
    try:
        extra = {} if noise is None else dict(noise, seed=seed)
        res = hp.rollout(start_states(seed, n_episodes), steps, **extra)
    finally:
        hp.primary.close()
        hp.secondary.close()
    for ep in range(n_episodes):
        x, xd, th1, w1, th2, w2 = res.states[ep]
        mode = "BALANCE" if res.last_mode[ep] else "SWINGUP"
        switches = "" if noise is None else f"switches={int(res.switches[ep])} | "
        print(f"Ep {ep + 1}: {int(res.lengths[ep])} steps | reward={float(res.returns[ep]):.0f} | "
              f"balance_steps={int(res.secondary_steps[ep])} | {switches}last_mode={mode} | "
              f"th1={np.degrees(th1):+.1f}° th2={np.degrees(th2):+.1f}° "
              f"w1={w1:+.2f} w2={w2:+.2f}")
    if noise is not None and n_episodes > 0:
        print(f"Summary: {n_episodes} episodes | mean reward={float(np.mean(res.returns)):.1f} | "
              f"terminated={float(np.mean(res.terminated)):.2f} | ending in BALANCE={float(np.mean(res.last_mode != 0)):.2f} | "
              f"mean switches={float(np.mean(res.switches)):.2f}")
    return res


def main(argv=None):
    args = build_parser().parse_args(argv)
    ignored = ignored_flags(args)
    if ignored:
        print(f"[{ENV}] note: {', '.join(ignored)} belong to the rollout / plot harness or to training, which this "
              "runner does not do; accepted and ignored")
    missing = [p for p in (args.swingup_path, args.balance_path) if not Path(p).exists()]
    if missing:
        sys.exit(f"[{ENV}] missing policy archive(s): {', '.join(map(str, missing))}\n"
                 "train them first:\n"
                 "    python runners/double_cartpole_swingup_cuda.py   (writes results/double_cartpole_swingup_cuda_policy.npz)\n"
                 "    python runners/double_cartpole_cuda.py           (writes results/double_cartpole_cuda_policy.npz)\n"
                 "or name them with --swingup-path / --balance-path")
    noise = dict(epsilon=args.epsilon, action_noise=args.action_noise, state_noise=args.state_noise) \
        if noise_requested(args) else None
    return evaluate(args.episodes, args.steps, args.seed, args.swingup_path, args.balance_path, noise)


if __name__ == "__main__":
    main()
