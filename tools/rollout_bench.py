"""tools/rollout_bench.py — fused closed-loop rollouts (pi_infer_rollout, csrc/pi_rollout_kernels.hip) against the
step-by-step loop they replace (one pi_infer_query and one pi_probe_step launch per time step plus the host-side
bookkeeping of ended episodes), on one MI355X.

Configs: C2 (pendulum 200^2), C3 (cartpole swing-up 50^4) and the 25^6 double cart-pole, each with a seeded random
policy (timing needs no training) and starts drawn uniformly inside the grid; m in {5, 4 096, 262 144} episodes of
1 000 steps.  Under a random policy the cart-pole episodes of C3 and 25^6 end early (the share that terminated and the
mean length are in the table): for those rows the honest unit of work is the episode-steps actually taken.

The driver (no arguments) runs every (config, m) in a child process of its own under `timeout -k 10`, one after the
other, and stops at the first child that fails; then one `rocprofv3 --kernel-trace --stats` run of the fused call
alone (C3, m = 4 096).  Each child warms both paths up once and reports the better of `--repeat` timings (device
events around the whole call, a synchronise at the end), fused and loop alternating.  The table goes to --out.
--hybrid: the two-policy rollout instead (pi_infer_rollout_hybrid, csrc/pi_hybrid_kernels.hip): the 25^6 double cart-pole
swing-up grid with the 25^6 balance grid as its partner, seeded random policies, the reference's switch box, starts
uniform in the swing-up grid; per m the fused hybrid call, the loop it replaces (a query on each handle and one plugin
step per time step, the mode rule and the bookkeeping as torch ops) and the single-policy fused rollout of the same
batch.  The table is appended to --out.
--greedy: the value-greedy controller instead (pi_infer_rollout_greedy, csrc/pi_greedy_kernels.hip): C2, C3 and the 25^6
double cart-pole with the env plugins' action tables, a seeded value function V ~ 30 N(0, 1) and a seeded random policy,
m = 4 096 episodes of --steps steps; per config the fused greedy rollout, the loop it replaces (one pi_infer_greedy and
one pi_probe_step launch per time step plus the bookkeeping as torch ops) and the fused interpolated-policy rollout of the
same batch, then the registers and scratch of both greedy kernels (hipcc -Rpass-analysis=kernel-resource-usage on the
translation unit pi_infer_set_greedy builds).  The table is written to --out.
--stochastic: the stochastic rollout instead (pi_infer_rollout_stochastic, csrc/pi_stochastic_kernels.hip): C2, C3 and the
25^6 double cart-pole with a seeded random policy, epsilon 0.3, action noise a tenth of the action range and state noise in
every dimension, m = 4 096 episodes of --steps steps; per config the fused stochastic rollout, the loop it replaces (per
step a query, the words of pi_infer_random_words, one pi_probe_step and the mixing as torch ops), the fused deterministic
rollout of the same batch and the random-policy baseline, then the registers and scratch of both kernels.  The table is
written to --out.
--expected: the expected-value greedy controller instead (pi_infer_rollout_expect_greedy, csrc/pi_expect_greedy_kernels.hip):
C2, C3 and the 25^6 double cart-pole with V ~ 30 N(0, 1) and a random policy (seeded), the noise of --stochastic, m = 4 096
episodes of --steps steps; per config the fused expected rollout over K = 1 (the zero set), 9 (action x one velocity) and
27 (action x two state dimensions) disturbance points, the loop it replaces at K = 9 (per step one pi_infer_expect_greedy
launch, the words of pi_infer_random_words, one pi_probe_step and the mixing as torch ops) and the fused greedy and
interpolated-policy rollouts of the same batch, then the registers and scratch of both kernels; then the closed loop under
the noise planned for, on the two settings of tools/expect_bench.py with common seeds: nominal and noise-aware training,
each under its policy table and under the lookahead (zero set on the nominal V, the training set on the noise-aware V).
The table is written to --out.
--hybrid --stochastic: the two-policy rollout under noise (pi_infer_rollout_hybrid_stochastic,
csrc/pi_hybrid_stochastic_kernels.hip): a 2-D, a 4-D and the 6-D pair of --hybrid (HYBRID_PAIRS), seeded random policies, the
noise of --stochastic, m = 4 096 episodes of --steps steps (profiles/r15 was taken with --steps 300); per pair the fused
launch, the loop it replaces (per step a query on each handle, the words of pi_infer_random_words, one pi_probe_step and the
mixing as torch ops), the deterministic hybrid rollout and the single-policy stochastic rollout of the same batch — a sample
of a fused path is ten calls back to back —, then the registers and scratch of the kernel and of the hybrid kernel beside
it.  The table is written to --out.
--adversary: the adversary rollouts (pi_infer_rollout_adversary, csrc/pi_adversary_kernels.hip): per config the fused
adversary rollout under the policy table and under the robust lookahead at K = 9 and 27 beside the expected-greedy rollout of
the same batch and, for the robust controller, the step-by-step loop it replaces (robust() + torch + pi_probe_step per step)
with a comparison of the bits, then the closed loop of tools/expect_bench.py's two settings — nominal, noise-aware and worst-case tables
under the sampled noise and under the adversary.

usage: python tools/rollout_bench.py [--hybrid | --greedy | --stochastic | --expected | --adversary | --hybrid --stochastic] [--out profiles/r07/rollout.txt] [--commit HASH] [--steps 1000] [--repeat 3]
"""
import argparse
import json
import subprocess
import sys
from itertools import product
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CONFIGS = {"c2": ("pendulum", 200), "c3": ("cartpole_swingup", 50), "c5": ("double_cartpole", 25)}
BATCHES = (5, 4096, 262144)
CHILD_SECONDS = 420
DEFAULT_OUT = str(ROOT / "profiles" / "r07" / "rollout.txt")


def child(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    from utils import barycentric as B
    env, bins = CONFIGS[args.config]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    shape = np.array([len(t) for t in tabs], np.int32)
    lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
    strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
    bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
    acts = np.asarray(cls.ACTIONS, np.float32)
    rng = np.random.default_rng(0)
    policy = rng.integers(0, len(acts), size=int(np.prod(shape.astype(np.int64))), dtype=np.int32)
    m, steps = args.m, args.steps
    dev = torch.device("cuda:0")
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((m, D), dtype=np.float32)).astype(np.float32)).to(dev)
    dp = B.DevicePolicy(policy, acts, lo, hi, shape, strides, bits, device=dev)
    dp.set_dynamics(envs.dynamics_source(env))

    def fused():
        return dp.rollout(starts, steps)

    if args.fused_only:                                   # the profiled run: warm-up + one call
        fused()
        out = fused()
        torch.cuda.synchronize()
        print(json.dumps({"config": args.config, "m": m, "steps": steps, "episode_steps": int(out.lengths.sum().item())}))
        return
    eng = _native.Engine(D, shape, lo, hi, tabs, acts, device=0)
    eng.compile(envs.dynamics_source(env))
    st = torch.cuda.current_stream(dev).cuda_stream

    def loop():
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        for t in range(steps):
            act = dp(states)
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            run = ~ended
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        return B.RolloutResult(states, ret, length, ended, None)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    a, b = fused(), loop()                                # warm-up of both paths, and: same results
    torch.cuda.synchronize()
    same = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32)) and torch.equal(a.lengths, b.lengths)
                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32)))
    t_fused, t_loop = [], []
    for _ in range(args.repeat):                          # alternating, so that drift hits both alike
        t_fused.append(timed(fused)[0])
        t_loop.append(timed(loop)[0])
    taken = int(a.lengths.sum().item())
    print(json.dumps({"config": args.config, "env": env, "bins": bins, "D": D, "m": m, "steps": steps, "same_bits": same,
                      "fused_ms": min(t_fused), "loop_ms": min(t_loop), "fused_ms_all": t_fused, "loop_ms_all": t_loop,
                      "episode_steps": taken, "terminated_share": float(a.terminated.float().mean().item()),
                      "launches_loop": 2 * steps}))
    dp.close()
    eng.close()


def hybrid_child(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    from utils import barycentric as B
    sys.path.insert(0, str(ROOT / "runners"))
    from hybrid_double_cartpole import ENTER, LEAVE
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    bits = np.array(list(product([0, 1], repeat=6)), dtype=np.int32)
    pols, tabs0 = [], None
    for env in ("double_cartpole_swingup", "double_cartpole"):
        cls = envs.ENVS[env]
        tabs = [np.asarray(b, np.float32) for b in cls.bins_space(25).values()]
        tabs0 = tabs0 or tabs
        shape = np.array([len(t) for t in tabs], np.int32)
        lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
        strides = np.array([int(np.prod(shape[d + 1:])) for d in range(6)], np.int32)
        acts = np.asarray(cls.ACTIONS, np.float32)
        policy = rng.integers(0, len(acts), size=int(np.prod(shape.astype(np.int64))), dtype=np.int32)
        pols.append(B.DevicePolicy(policy, acts, lo, hi, shape, strides, bits, device=dev))
    dp, dp2 = pols
    dyn = envs.dynamics_source("double_cartpole_swingup")
    dp.set_dynamics(dyn)
    hp = B.HybridPolicy(dp, dp2, ENTER, LEAVE)
    m, steps = args.m, args.steps
    lo, hi = np.array([t.min() for t in tabs0], np.float32), np.array([t.max() for t in tabs0], np.float32)
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((m, 6), dtype=np.float32)).astype(np.float32)).to(dev)
    eng = _native.Engine(6, [len(t) for t in tabs0], lo, hi, tabs0, np.asarray(envs.ENVS["double_cartpole_swingup"].ACTIONS, np.float32), device=0)
    eng.compile(dyn)
    st = torch.cuda.current_stream(dev).cuda_stream
    ent, lea = torch.tensor(ENTER, dtype=torch.float32, device=dev), torch.tensor(LEAVE, dtype=torch.float32, device=dev)

    def loop():
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        second = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        mode = torch.zeros(m, dtype=torch.bool, device=dev)
        for t in range(steps):
            run = ~ended
            mag = states.abs()
            mode = torch.where(run, torch.where(mode, ~(mag > lea).any(dim=1), (mag < ent).all(dim=1)), mode)
            act = torch.where(mode, dp2(states), dp(states))
            second = second + (run & mode).to(torch.int32)
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        return B.HybridRolloutResult(states, ret, length, ended, None, second, mode.to(torch.uint8))

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    def fused():
        return hp.rollout(starts, steps)

    def single():
        return dp.rollout(starts, steps)
    a, b = fused(), loop()                                # warm-up of all paths, and: same results
    single()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32)) and torch.equal(a.lengths, b.lengths)
                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32))
                and torch.equal(a.secondary_steps, b.secondary_steps) and torch.equal(a.last_mode, b.last_mode))
    t_fused, t_loop, t_single = [], [], []
    for _ in range(args.repeat):
        t_fused.append(timed(fused)[0])
        t_loop.append(timed(loop)[0])
        t_single.append(timed(single)[0])
    print(json.dumps({"m": m, "steps": steps, "same_bits": same, "fused_ms": min(t_fused), "loop_ms": min(t_loop),
                      "single_ms": min(t_single), "episode_steps": int(a.lengths.sum().item()),
                      "secondary_steps": int(a.secondary_steps.sum().item()),
                      "terminated_share": float(a.terminated.float().mean().item()), "launches_loop": 3 * steps}))
    dp.close()
    dp2.close()
    eng.close()


def greedy_child(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    from utils import barycentric as B
    env, bins = CONFIGS[args.config]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    shape = np.array([len(t) for t in tabs], np.int32)
    lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
    strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
    bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
    acts = np.asarray(cls.ACTIONS, np.float32)
    rng = np.random.default_rng(0)
    n = int(np.prod(shape.astype(np.int64)))
    policy = rng.integers(0, len(acts), size=n, dtype=np.int32)
    V = (30.0 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    m, steps, lookahead = args.m, args.steps, 0.99
    dev = torch.device("cuda:0")
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((m, D), dtype=np.float32)).astype(np.float32)).to(dev)
    dp = B.DevicePolicy(policy, acts, lo, hi, shape, strides, bits, device=dev)
    dp.set_dynamics(envs.dynamics_source(env))
    dp.set_values(V)
    dp.set_greedy()
    eng = _native.Engine(D, shape, lo, hi, tabs, acts, device=0)
    eng.compile(envs.dynamics_source(env))
    st = torch.cuda.current_stream(dev).cuda_stream

    def fused():
        return dp.rollout(starts, steps, controller="greedy", lookahead_gamma=lookahead)

    def single():
        return dp.rollout(starts, steps)

    def loop():
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        for t in range(steps):
            act = dp.greedy(states, lookahead)[1]
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            run = ~ended
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        return B.RolloutResult(states, ret, length, ended, None)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    a, b = fused(), loop()                                # warm-up of all paths, and: same results
    c = single()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32)) and torch.equal(a.lengths, b.lengths)
                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32)))
    t_fused, t_loop, t_single = [], [], []
    for _ in range(args.repeat):
        t_fused.append(timed(fused)[0])
        t_loop.append(timed(loop)[0])
        t_single.append(timed(single)[0])
    print(json.dumps({"config": args.config, "env": env, "bins": bins, "D": D, "actions": len(acts), "m": m, "steps": steps,
                      "same_bits": same, "fused_ms": min(t_fused), "loop_ms": min(t_loop), "single_ms": min(t_single),
                      "episode_steps": int(a.lengths.sum().item()), "single_episode_steps": int(c.lengths.sum().item()),
                      "terminated_share": float(a.terminated.float().mean().item()), "launches_loop": 2 * steps}))
    dp.close()
    eng.close()


def greedy_usage(env, bins, define="PI_GREEDY", kernels="pi_greedy_kernels.hip"):
    """VGPRs and scratch bytes per lane of both greedy kernels for one grid: the translation unit pi_infer_set_greedy hands
    to hipRTC, built ahead of time with the same flags.  (`define`, `kernels`: the same for another module that sits
    behind the rollout helpers — the stochastic one; several defines as a tuple, `kernels` as a Path: a file elsewhere.)"""
    import tempfile
    import numpy as np
    from __graft_entry__ import HIPCC
    from dynamicprogramming_amd import envs
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    shape = [len(t) for t in tabs]
    strides = [int(np.prod(shape[d + 1:])) for d in range(D)]

    def braces(v, fmt):
        return "{" + ",".join(fmt(x) for x in v) + "}"

    def hexf(x):
        return float(np.float32(x)).hex() + "f"
    csrc = ROOT / "dynamicprogramming_amd" / "csrc"
    defines = "".join(f"#define {d} 1\n" for d in ([define] if isinstance(define, str) else define))
    text = (f"{defines}#define PI_D {D}\n#define PI_LO_INIT {braces([t.min() for t in tabs], hexf)}\n"
            f"#define PI_HI_INIT {braces([t.max() for t in tabs], hexf)}\n#define PI_SHAPE_INIT {braces(shape, str)}\n"
            f"#define PI_STRIDES_INIT {braces(strides, str)}\n"
            f"#define PI_BITS_INIT {braces(list(product([0, 1], repeat=D)), lambda r: braces(r, str))}\n"
            f"{(ROOT / 'include' / 'pi_math.h').read_text()}\n#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n"
            f"{envs.dynamics_source(env)}\n{(csrc / 'pi_rollout_kernels.hip').read_text()}\n"
            f"{(csrc / kernels).read_text() if isinstance(kernels, str) else Path(kernels).read_text()}\n")
    usage, fn = {}, None
    with tempfile.TemporaryDirectory(prefix="pi_greedy_") as tmp:
        src = Path(tmp) / "greedy.hip"
        src.write_text(text)
        res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "--genco",
                              "-include", "hip/hip_runtime.h", "-Rpass-analysis=kernel-resource-usage", str(src), "-o",
                              str(Path(tmp) / "greedy.hsaco")], capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"hipcc failed on the {kernels} translation unit of {env} {bins}^{D}\n{res.stderr[-2000:]}")
    for line in res.stderr.splitlines():
        if "Function Name:" in line:
            fn = line.split("Function Name:")[1].split()[0]
            usage[fn] = {}
        elif fn and " VGPRs:" in line:
            usage[fn]["vgpr"] = int(line.split("VGPRs:")[1].split()[0])
        elif fn and "ScratchSize" in line:
            usage[fn]["scratch"] = int(line.split(":")[-1].split()[0])
    return usage


def greedy_driver(args):
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    rows = []
    for config in CONFIGS:
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--greedy", "--config", config, "--m",
                              str(args.m), "--steps", str(args.steps), "--repeat", str(args.repeat)], capture_output=True, text=True)
        if res.returncode != 0:                           # a fault, an abort or a time limit: nothing more runs
            sys.exit(f"greedy {config} ended with status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
        rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    lines = [f"value-greedy rollouts (one-step lookahead on V) vs the step-by-step loop, MI355X, commit {args.commit}",
             f"{args.m} episodes of {args.steps} steps, the env plugins' action tables, V ~ 30 N(0, 1) and a random policy (seeded), "
             f"lookahead gamma 0.99, starts uniform in the grid; times in ms: the better of {args.repeat} after one warm-up, "
             "device events around the whole call",
             "policy: the fused interpolated-policy rollout (pi_infer_rollout) of the same batch; ep-steps: steps actually "
             "taken under the greedy controller (episodes that ended stop)",
             "",
             f"{'config':30s} {'actions':>7s} {'fused':>10s} {'loop':>10s} {'loop/fused':>10s} {'policy':>10s} {'ep-steps':>12s} "
             f"{'M ep-steps/s':>12s} {'ended':>6s} {'same bits':>9s}"]
    for r in rows:
        lines.append(f"{r['config'] + ' ' + r['env'] + ' ' + str(r['bins']) + '^' + str(r['D']):30s} {r['actions']:7d} "
                     f"{r['fused_ms']:10.3f} {r['loop_ms']:10.3f} {r['loop_ms'] / r['fused_ms']:10.1f} {r['single_ms']:10.3f} "
                     f"{r['episode_steps']:12d} {r['episode_steps'] / r['fused_ms'] / 1e3:12.2f} {r['terminated_share']:6.3f} "
                     f"{str(r['same_bits']):>9s}")
    slower = [r["config"] for r in rows if r["fused_ms"] >= r["loop_ms"]]
    lines += ["", "the fused kernel is faster than its own step-by-step loop on every config" if not slower else
              f"the fused kernel is NOT faster than its own step-by-step loop on: {', '.join(slower)}", "",
              "registers and scratch (hipcc -Rpass-analysis=kernel-resource-usage, the translation unit of pi_infer_set_greedy):"]
    for config, (env, bins) in CONFIGS.items():
        for fn, k in sorted(greedy_usage(env, bins).items()):
            lines.append(f"  {config} {env:24s} {fn:26s} VGPRs {k['vgpr']:4d}  scratch {k['scratch']} bytes/lane")
    out.write_text("\n".join(lines) + "\n")
    print(out.read_text())


def stochastic_child(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    from utils import barycentric as B
    env, bins = CONFIGS[args.config]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    shape = np.array([len(t) for t in tabs], np.int32)
    lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
    strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
    bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
    acts = np.asarray(cls.ACTIONS, np.float32)
    rng = np.random.default_rng(0)
    policy = rng.integers(0, len(acts), size=int(np.prod(shape.astype(np.int64))), dtype=np.int32)
    m, steps, seed = args.m, args.steps, 20261019
    epsilon, a_noise = 0.3, float(np.float32(0.1) * (acts.max() - acts.min()))
    s_noise = (np.float32(0.002) * (hi - lo)).astype(np.float32)             # every dimension: all the draw blocks of D
    dev = torch.device("cuda:0")
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((m, D), dtype=np.float32)).astype(np.float32)).to(dev)
    dp = B.DevicePolicy(policy, acts, lo, hi, shape, strides, bits, device=dev)
    dp.set_dynamics(envs.dynamics_source(env))
    dp.set_stochastic()
    eng = _native.Engine(D, shape, lo, hi, tabs, acts, device=0)
    eng.compile(envs.dynamics_source(env))
    st = torch.cuda.current_stream(dev).cuda_stream
    noisy = dict(epsilon=epsilon, action_noise=a_noise, state_noise=s_noise, seed=seed)

    def fused():
        return dp.rollout(starts, steps, **noisy)

    def baseline():                                       # uniformly random actions, nothing else: no table is read
        return dp.rollout(starts, steps, controller="random", seed=seed)

    def single():
        return dp.rollout(starts, steps)
    d_acts = torch.from_numpy(acts).to(dev)
    eps24, n_act = B.explore_threshold(epsilon), len(acts)
    amp = torch.tensor(a_noise, dtype=torch.float32, device=dev)
    d_noise = torch.from_numpy(s_noise).to(dev)
    a_lo, a_hi = d_acts.min(), d_acts.max()
    blocks = (1, 2) if D > 4 else (1,)

    def sym(x):                                           # int32 words holding uint32 bits -> [-1, 1), exact
        return (((x >> 8) & 0xFFFFFF) - 8388608).to(torch.float32) * 2.0 ** -23

    def loop():                                           # the words from the probe kernel, mixed in with torch float32 ops
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        w0 = torch.empty((m, 4), dtype=torch.int32, device=dev)
        w = torch.empty((len(blocks), m, 4), dtype=torch.int32, device=dev)
        for t in range(steps):
            act = dp(states)
            dp._engine.random_words(seed, 0, m, t, 0, w0.data_ptr(), stream=st)
            explore = ((w0[:, 0] >> 8) & 0xFFFFFF) < eps24
            index = ((w0[:, 1].to(torch.int64) & 0xFFFFFFFF) * n_act) >> 32
            act = torch.where(explore, d_acts[index], act)
            push = amp * sym(w0[:, 2])
            act = torch.fmin(torch.fmax(act + push, a_lo), a_hi).contiguous()
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            for k, j in enumerate(blocks):
                dp._engine.random_words(seed, 0, m, t, j, w[k].data_ptr(), stream=st)
            words = torch.cat(list(w), dim=1)[:, :D]
            push = d_noise * sym(words)
            nxt2 = torch.where((done == 0)[:, None], nxt + push, nxt)
            run = ~ended
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt2, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        return B.RolloutResult(states, ret, length, ended, None)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    a, b = fused(), loop()                                # warm-up of all paths, and: same results
    c, r = single(), baseline()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32)) and torch.equal(a.lengths, b.lengths)
                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32)))
    t_fused, t_loop, t_single, t_base = [], [], [], []
    for _ in range(args.repeat):
        t_fused.append(timed(fused)[0])
        t_loop.append(timed(loop)[0])
        t_single.append(timed(single)[0])
        t_base.append(timed(baseline)[0])
    print(json.dumps({"config": args.config, "env": env, "bins": bins, "D": D, "actions": len(acts), "m": m, "steps": steps,
                      "same_bits": same, "fused_ms": min(t_fused), "loop_ms": min(t_loop), "single_ms": min(t_single),
                      "random_ms": min(t_base), "fused_ms_all": t_fused, "single_ms_all": t_single,
                      "episode_steps": int(a.lengths.sum().item()), "single_episode_steps": int(c.lengths.sum().item()),
                      "random_episode_steps": int(r.lengths.sum().item()),
                      "terminated_share": float(a.terminated.float().mean().item()),
                      "launches_loop": (3 + len(blocks)) * steps}))
    dp.close()
    eng.close()


def stochastic_driver(args):
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    rows = []
    for config in CONFIGS:
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--stochastic", "--config", config, "--m",
                              str(args.m), "--steps", str(args.steps), "--repeat", str(args.repeat)], capture_output=True, text=True)
        if res.returncode != 0:                           # a fault, an abort or a time limit: nothing more runs
            sys.exit(f"stochastic {config} ended with status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
        rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    lines = [f"stochastic rollouts (Philox4x32-10 in the kernel) vs the step-by-step loop, MI355X, commit {args.commit}",
             f"{args.m} episodes of {args.steps} steps, the env plugins' action tables, a seeded random policy, epsilon 0.3, action "
             "noise a tenth of the action range, state noise 0.2 % of the span in every dimension, starts uniform in the grid; "
             f"times in ms: the better of {args.repeat} after one warm-up, device events around the whole call",
             "loop: per step a query, the probe kernel's words, the plugin step and the mixing as torch ops; policy: the fused "
             "deterministic rollout (pi_infer_rollout) of the same batch, policy ep-steps its steps; random: "
             "controller='random' alone; ep-steps: steps actually taken by the stochastic rollout (episodes that ended stop)",
             "",
             f"{'config':30s} {'fused':>10s} {'loop':>10s} {'loop/fused':>10s} {'policy':>10s} {'random':>10s} {'ep-steps':>12s} "
             f"{'policy ep-steps':>15s} {'ended':>6s} {'same bits':>9s}"]
    for r in rows:
        lines.append(f"{r['config'] + ' ' + r['env'] + ' ' + str(r['bins']) + '^' + str(r['D']):30s} "
                     f"{r['fused_ms']:10.3f} {r['loop_ms']:10.3f} {r['loop_ms'] / r['fused_ms']:10.1f} {r['single_ms']:10.3f} "
                     f"{r['random_ms']:10.3f} {r['episode_steps']:12d} {r['single_episode_steps']:15d} {r['terminated_share']:6.3f} "
                     f"{str(r['same_bits']):>9s}")
    lines += ["", "all timings per config (ms): " + "; ".join(
        f"{r['config']} fused {[round(t, 3) for t in r['fused_ms_all']]} policy {[round(t, 3) for t in r['single_ms_all']]}" for r in rows)]
    slower = [r["config"] for r in rows if r["fused_ms"] >= r["loop_ms"]]
    lines += ["", "the fused kernel is faster than its own step-by-step loop on every config" if not slower else
              f"the fused kernel is NOT faster than its own step-by-step loop on: {', '.join(slower)}", "",
              "registers and scratch (hipcc -Rpass-analysis=kernel-resource-usage, the translation unit of pi_infer_set_stochastic):"]
    for config, (env, bins) in CONFIGS.items():
        for fn, k in sorted(greedy_usage(env, bins, "PI_STOCHASTIC", "pi_stochastic_kernels.hip").items()):
            lines.append(f"  {config} {env:24s} {fn:30s} VGPRs {k['vgpr']:4d}  scratch {k['scratch']} bytes/lane")
    out.write_text("\n".join(lines) + "\n")
    print(out.read_text())


def expected_child(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    from dynamicprogramming_amd.noise import Disturbances
    from utils import barycentric as B
    env, bins = CONFIGS[args.config]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float32) for b in cls.bins_space(bins).values()]
    D = len(tabs)
    shape = np.array([len(t) for t in tabs], np.int32)
    lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
    strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
    bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
    acts = np.asarray(cls.ACTIONS, np.float32)
    rng = np.random.default_rng(0)
    n = int(np.prod(shape.astype(np.int64)))
    policy = rng.integers(0, len(acts), size=n, dtype=np.int32)
    V = (30.0 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    m, steps, seed, lookahead = args.m, args.steps, 20261019, 0.99
    epsilon, a_noise = 0.3, float(np.float32(0.1) * (acts.max() - acts.min()))
    s_noise = (np.float32(0.002) * (hi - lo)).astype(np.float32)
    one, two = np.zeros(D), np.zeros(D)
    one[1] = two[0] = two[1] = 1.0
    sets = {1: Disturbances.none(D), 9: Disturbances.uniform(D, state_noise=one * s_noise, action_noise=a_noise),
            27: Disturbances.uniform(D, state_noise=two * s_noise, action_noise=a_noise)}
    assert [d.K for d in sets.values()] == list(sets)
    dev = torch.device("cuda:0")
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((m, D), dtype=np.float32)).astype(np.float32)).to(dev)
    dp = B.DevicePolicy(policy, acts, lo, hi, shape, strides, bits, device=dev)
    dp.set_dynamics(envs.dynamics_source(env))
    dp.set_values(V)
    dp.set_greedy()
    dp.set_stochastic()
    dp.set_expected_greedy()
    eng = _native.Engine(D, shape, lo, hi, tabs, acts, device=0)
    eng.compile(envs.dynamics_source(env))
    st = torch.cuda.current_stream(dev).cuda_stream
    noisy = dict(epsilon=epsilon, action_noise=a_noise, state_noise=s_noise, seed=seed)

    def fused():
        return dp.rollout(starts, steps, controller="expected", lookahead_gamma=lookahead, **noisy)

    def greedy():
        return dp.rollout(starts, steps, controller="greedy", lookahead_gamma=lookahead)

    def single():
        return dp.rollout(starts, steps, **noisy)
    d_acts = torch.from_numpy(acts).to(dev)
    eps24, n_act = B.explore_threshold(epsilon), len(acts)
    amp = torch.tensor(a_noise, dtype=torch.float32, device=dev)
    d_noise = torch.from_numpy(s_noise).to(dev)
    a_lo, a_hi = d_acts.min(), d_acts.max()
    blocks = (1, 2) if D > 4 else (1,)

    def sym(x):                                           # int32 words holding uint32 bits -> [-1, 1), exact
        return (((x >> 8) & 0xFFFFFF) - 8388608).to(torch.float32) * 2.0 ** -23

    def loop():                                           # stochastic_child's loop with the lookahead as the controller
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        w0 = torch.empty((m, 4), dtype=torch.int32, device=dev)
        w = torch.empty((len(blocks), m, 4), dtype=torch.int32, device=dev)
        for t in range(steps):
            act = dp.expected_greedy(states, lookahead)[1]
            dp._engine.random_words(seed, 0, m, t, 0, w0.data_ptr(), stream=st)
            explore = ((w0[:, 0] >> 8) & 0xFFFFFF) < eps24
            index = ((w0[:, 1].to(torch.int64) & 0xFFFFFFFF) * n_act) >> 32
            act = torch.where(explore, d_acts[index], act)
            push = amp * sym(w0[:, 2])
            act = torch.fmin(torch.fmax(act + push, a_lo), a_hi).contiguous()
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            for k, j in enumerate(blocks):
                dp._engine.random_words(seed, 0, m, t, j, w[k].data_ptr(), stream=st)
            words = torch.cat(list(w), dim=1)[:, :D]
            push = d_noise * sym(words)
            nxt2 = torch.where((done == 0)[:, None], nxt + push, nxt)
            run = ~ended
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt2, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        return B.RolloutResult(states, ret, length, ended, None)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    dp.set_disturbances(sets[9])
    a, b = fused(), loop()                                # warm-up of all paths, and: same results
    greedy(), single()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32)) and torch.equal(a.lengths, b.lengths)
                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32)))
    t_fused, t_loop, t_greedy, t_single = {K: [] for K in sets}, [], [], []
    taken = {}
    for _ in range(args.repeat):
        for K, d in sets.items():
            dp.set_disturbances(d)
            ms, out = timed(fused)
            t_fused[K].append(ms)
            taken[K] = int(out.lengths.sum().item())
        dp.set_disturbances(sets[9])
        t_loop.append(timed(loop)[0])
        t_greedy.append(timed(greedy)[0])
        t_single.append(timed(single)[0])
    print(json.dumps({"config": args.config, "env": env, "bins": bins, "D": D, "actions": len(acts), "m": m, "steps": steps,
                      "same_bits": same, "fused_ms": {K: min(v) for K, v in t_fused.items()}, "fused_ms_all": t_fused,
                      "loop_ms": min(t_loop), "greedy_ms": min(t_greedy), "single_ms": min(t_single), "episode_steps": taken,
                      "terminated_share": float(a.terminated.float().mean().item()),
                      "launches_loop": (3 + len(blocks)) * steps}))
    dp.close()
    eng.close()


def expected_loop_child(args):
    """The closed loop under the noise planned for: nominal and noise-aware training of one setting of
    tools/expect_bench.py, each under its policy table and under the lookahead, common seeds."""
    import numpy as np
    from dynamicprogramming_amd import envs
    from dynamicprogramming_amd.noise import Disturbances
    from dynamicprogramming_amd.solver import CudaPIConfig
    sys.path.insert(0, str(ROOT / "tools"))
    from expect_bench import LOOPS
    env = args.env
    bins, a_share, x_cells, caps = LOOPS[env]
    cls = envs.ENVS[env]
    tabs = [np.asarray(b, np.float64) for b in cls.bins_space(bins).values()]
    cell = np.array([(t.max() - t.min()) / (len(t) - 1) for t in tabs])
    acts = np.asarray(cls.ACTIONS, np.float64)
    a_noise = a_share * float(acts.max() - acts.min())
    x_noise = [float(c * w) for c, w in zip(x_cells, cell)]
    planned = Disturbances.uniform(len(tabs), state_noise=x_noise, action_noise=a_noise)
    starts = cls.start_states(np.random.default_rng(args.seed), args.m)
    world = dict(action_noise=a_noise, state_noise=x_noise, seed=args.seed)
    out = {"env": env, "bins": bins, "action_noise": a_noise, "state_noise": x_noise, "caps": caps, "steps": args.steps,
           "m": args.m, "K": planned.K, "rows": []}
    for label, d, look in (("nominal", None, Disturbances.none(len(tabs))), ("noise-aware", planned, planned)):
        solver = envs.make(env, bins, CudaPIConfig(**{**cls.CONFIG, **caps}), device="cuda:0", transport=False)
        if d is not None:
            solver.set_disturbances(d)
        solver.run()
        for controller, kw in (("policy table", {}), ("lookahead", dict(controller="expected", disturbances=look))):
            res = solver.rollout(starts, args.steps, gamma=1.0, **world, **kw)
            out["rows"].append({"trained": label, "controller": controller + (f" K={look.K}" if kw else ""),
                                "mean_return": float(np.mean(res.returns)), "terminated_share": float(np.mean(res.terminated)),
                                "mean_length": float(np.mean(res.lengths))})
    print(json.dumps(out))


def expected_usage(env, bins):
    """greedy_usage for the unit pi_infer_set_expect_greedy builds: the greedy and the stochastic file ahead of the kernels."""
    import tempfile
    csrc = ROOT / "dynamicprogramming_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="pi_expect_greedy_") as tmp:
        unit = Path(tmp) / "unit.hip"
        unit.write_text("\n".join(
            (csrc / f).read_text() for f in ("pi_greedy_kernels.hip", "pi_stochastic_kernels.hip", "pi_expect_greedy_kernels.hip")))
        return greedy_usage(env, bins, ("PI_EXPECT_GREEDY", "PI_GREEDY", "PI_STOCHASTIC"), unit)


def expected_driver(args):
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    rows, loops, failed = [], [], None
    sys.path.insert(0, str(ROOT / "tools"))
    from expect_bench import LOOPS
    jobs = [("timing", ["--config", c, "--steps", str(args.steps)]) for c in CONFIGS] + \
           [("loop", ["--env", e, "--steps", str(args.loop_steps)]) for e in LOOPS]
    for kind, extra in jobs:
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--expected", "--part", kind, *extra,
                              "--m", str(args.m), "--repeat", str(args.repeat)], capture_output=True, text=True)
        if res.returncode != 0:                           # a fault, an abort or a time limit: nothing more runs
            failed = f"NOT MEASURED: {kind} {' '.join(extra)} ended with status {res.returncode}: {res.stderr.strip()[-400:]}"
            break
        (rows if kind == "timing" else loops).append(json.loads(res.stdout.strip().splitlines()[-1]))
        print((rows if kind == "timing" else loops)[-1], flush=True)
    lines = [f"expected-value greedy rollouts (lookahead over a disturbance set) vs the step-by-step loop, MI355X, commit {args.commit}",
             f"{args.m} episodes of {args.steps} steps, the env plugins' action tables, V ~ 30 N(0, 1) and a random policy (seeded), "
             "lookahead gamma 0.99, epsilon 0.3, action noise a tenth of the action range, state noise 0.2 % of the span in every "
             f"dimension, starts uniform in the grid; times in ms: the better of {args.repeat} after one warm-up, device events "
             "around the whole call",
             "K=1: the zero set; K=9: action x one velocity; K=27: action x two state dimensions (3 Gauss-Legendre nodes each); "
             "loop: at K=9, per step one expected_greedy launch, the probe kernel's words, the plugin step and the mixing as torch "
             "ops; greedy: the fused deterministic greedy rollout without noise; policy: the fused stochastic policy-table rollout "
             "under the same noise; ep-steps: steps taken at K=9",
             "",
             f"{'config':30s} {'actions':>7s} {'K=1':>9s} {'K=9':>9s} {'K=27':>9s} {'loop':>10s} {'loop/K=9':>9s} {'greedy':>9s} "
             f"{'policy':>9s} {'ep-steps':>10s} {'ended':>6s} {'same bits':>9s}"]
    for r in rows:
        f = {int(k): v for k, v in r["fused_ms"].items()}
        lines.append(f"{r['config'] + ' ' + r['env'] + ' ' + str(r['bins']) + '^' + str(r['D']):30s} {r['actions']:7d} "
                     f"{f[1]:9.3f} {f[9]:9.3f} {f[27]:9.3f} {r['loop_ms']:10.3f} {r['loop_ms'] / f[9]:9.1f} {r['greedy_ms']:9.3f} "
                     f"{r['single_ms']:9.3f} {r['episode_steps']['9']:10d} {r['terminated_share']:6.3f} {str(r['same_bits']):>9s}")
    lines += ["", "all fused timings per config (ms): " + "; ".join(
        f"{r['config']} " + " ".join(f"K={k} {[round(t, 3) for t in v]}" for k, v in r["fused_ms_all"].items()) for r in rows)]
    lines += ["", "registers and scratch (hipcc -Rpass-analysis=kernel-resource-usage, the translation unit of "
                  "pi_infer_set_expect_greedy):"]
    for config, (env, bins) in CONFIGS.items():
        for fn, k in sorted(expected_usage(env, bins).items()):
            lines.append(f"  {config} {env:24s} {fn:34s} VGPRs {k['vgpr']:4d}  scratch {k['scratch']} bytes/lane")
    for r in loops:
        lines += ["", f"closed loop under the noise planned for: {r['env']} {r['bins']} bins, action noise {r['action_noise']:.4g}, "
                      f"state noise {[round(x, 5) for x in r['state_noise']]}, caps {r['caps']}, {r['m']} episodes of {r['steps']} "
                      f"steps, common seeds; the planned set has K = {r['K']}",
                  f"{'trained':12s} {'controller':18s} {'mean return':>12s} {'terminated':>10s} {'mean length':>11s}"]
        for row in r["rows"]:
            lines.append(f"{row['trained']:12s} {row['controller']:18s} {row['mean_return']:12.3f} {row['terminated_share']:10.4f} "
                         f"{row['mean_length']:11.1f}")
    if failed:
        lines += ["", failed]
    lines += ["", "no counters were taken: which unit binds is not stated"]
    out.write_text("\n".join(lines) + "\n")
    print(out.read_text())


INF = float("inf")
# --hybrid --stochastic: (primary env, bins, secondary env, bins, enter, leave) per D; the 6-D pair and its box are --hybrid's
# (the runner's), the 2-D and 4-D pairs a coarser grid of the same env behind a box around the upright position
HYBRID_PAIRS = {
    "c2": ("pendulum", 200, "pendulum", 50, (1.0, 3.0), (1.4, 5.0)),
    "c3": ("cartpole_swingup", 50, "cartpole_swingup", 30, (INF, INF, 0.9, 5.0), (INF, INF, 1.1, 7.0)),
    "c5": ("double_cartpole_swingup", 25, "double_cartpole", 25, (INF, INF, 0.32, 4.0, 0.32, 4.0), (INF, INF, 0.38, 5.0, 0.38, 5.0)),
}
FUSED_PER_SAMPLE = 10       # a fused launch takes 0.3 to 2 ms: a sample times this many back to back


def _grid_tables(env, bins):
    import numpy as np
    from dynamicprogramming_amd import envs
    tabs = [np.asarray(b, np.float32) for b in envs.ENVS[env].bins_space(bins).values()]
    D = len(tabs)
    shape = np.array([len(t) for t in tabs], np.int32)
    lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
    strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
    bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
    return tabs, (lo, hi, shape, strides, bits)


def hybrid_stochastic_child(args):
    import numpy as np
    import torch
    from dynamicprogramming_amd import _native, envs
    from utils import barycentric as B
    env, bins, env2, bins2, enter, leave = HYBRID_PAIRS[args.config]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    pols = []
    for e, g in ((env, bins), (env2, bins2)):
        tabs, grid = _grid_tables(e, g)
        acts = np.asarray(envs.ENVS[e].ACTIONS, np.float32)
        policy = rng.integers(0, len(acts), size=int(np.prod(grid[2].astype(np.int64))), dtype=np.int32)
        pols.append(B.DevicePolicy(policy, acts, *grid, device=dev))
    dp, dp2 = pols
    tabs, (lo, hi, shape, _, _) = _grid_tables(env, bins)
    D = len(tabs)
    acts = np.asarray(envs.ENVS[env].ACTIONS, np.float32)
    dyn = envs.dynamics_source(env)
    dp.set_dynamics(dyn)
    dp.set_stochastic()                                   # the loop's words and the single-policy stochastic rollout
    hp = B.HybridPolicy(dp, dp2, enter, leave)
    m, steps, seed = args.m, args.steps, 20261020
    epsilon, a_noise = 0.3, float(np.float32(0.1) * (acts.max() - acts.min()))
    s_noise = (np.float32(0.002) * (hi - lo)).astype(np.float32)             # every dimension: all the draw blocks of D
    noisy = dict(epsilon=epsilon, action_noise=a_noise, state_noise=s_noise, seed=seed)
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((m, D), dtype=np.float32)).astype(np.float32)).to(dev)
    eng = _native.Engine(D, shape, lo, hi, tabs, acts, device=0)
    eng.compile(dyn)
    st = torch.cuda.current_stream(dev).cuda_stream
    ent, lea = torch.tensor(enter, dtype=torch.float32, device=dev), torch.tensor(leave, dtype=torch.float32, device=dev)
    d_acts = torch.from_numpy(acts).to(dev)
    eps24, n_act = B.explore_threshold(epsilon), len(acts)
    amp = torch.tensor(a_noise, dtype=torch.float32, device=dev)
    d_noise = torch.from_numpy(s_noise).to(dev)
    a_lo, a_hi = d_acts.min(), d_acts.max()
    blocks = (1, 2) if D > 4 else (1,)

    def sym(x):                                           # int32 words holding uint32 bits -> [-1, 1), exact
        return (((x >> 8) & 0xFFFFFF) - 8388608).to(torch.float32) * 2.0 ** -23

    def loop():                                           # two queries, the probe kernel's words, one plugin step, torch mixing
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        second = torch.zeros(m, dtype=torch.int32, device=dev)
        switches = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        mode = torch.zeros(m, dtype=torch.bool, device=dev)
        w0 = torch.empty((m, 4), dtype=torch.int32, device=dev)
        w = torch.empty((len(blocks), m, 4), dtype=torch.int32, device=dev)
        for t in range(steps):
            run = ~ended
            mag = states.abs()
            now = torch.where(mode, ~(mag > lea).any(dim=1), (mag < ent).all(dim=1))
            switches = switches + (run & (now != mode)).to(torch.int32)
            mode = torch.where(run, now, mode)
            second = second + (run & mode).to(torch.int32)
            act = torch.where(mode, dp2(states), dp(states))
            dp._engine.random_words(seed, 0, m, t, 0, w0.data_ptr(), stream=st)
            explore = ((w0[:, 0] >> 8) & 0xFFFFFF) < eps24
            index = ((w0[:, 1].to(torch.int64) & 0xFFFFFFFF) * n_act) >> 32
            act = torch.where(explore, d_acts[index], act)
            push = amp * sym(w0[:, 2])
            act = torch.fmin(torch.fmax(act + push, a_lo), a_hi).contiguous()
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            for k, j in enumerate(blocks):
                dp._engine.random_words(seed, 0, m, t, j, w[k].data_ptr(), stream=st)
            words = torch.cat(list(w), dim=1)[:, :D]
            push = d_noise * sym(words)
            nxt2 = torch.where((done == 0)[:, None], nxt + push, nxt)
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt2, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        return B.StochasticHybridRolloutResult(states, ret, length, ended, None, second, mode.to(torch.uint8), switches)

    def timed(fn, calls=1):                               # ms per call of `calls` back to back, one synchronise at the end
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / calls, out

    def fused():
        return hp.rollout(starts, steps, **noisy)

    def plain():                                          # the deterministic hybrid rollout of the same batch
        return hp.rollout(starts, steps)

    def single():                                         # the single-policy stochastic rollout of the same batch
        return dp.rollout(starts, steps, **noisy)
    a, b = fused(), loop()                                # warm-up of all paths, and: same results
    p, s = plain(), single()
    torch.cuda.synchronize()
    same = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32)) and torch.equal(a.lengths, b.lengths)
                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32))
                and torch.equal(a.secondary_steps, b.secondary_steps) and torch.equal(a.last_mode, b.last_mode)
                and torch.equal(a.switches, b.switches))
    t_fused, t_loop, t_plain, t_single = [], [], [], []
    for _ in range(args.repeat):                          # alternating, so that drift hits all alike
        t_fused.append(timed(fused, FUSED_PER_SAMPLE)[0])
        t_loop.append(timed(loop)[0])
        t_plain.append(timed(plain, FUSED_PER_SAMPLE)[0])
        t_single.append(timed(single, FUSED_PER_SAMPLE)[0])
    print(json.dumps({"config": args.config, "pair": f"{env} {bins}^{D} + {env2} {bins2}^{D}", "D": D, "m": m, "steps": steps,
                      "same_bits": same, "fused_ms": min(t_fused), "loop_ms": min(t_loop), "plain_ms": min(t_plain),
                      "single_ms": min(t_single), "fused_ms_all": t_fused, "loop_ms_all": t_loop,
                      "episode_steps": int(a.lengths.sum().item()), "plain_episode_steps": int(p.lengths.sum().item()),
                      "single_episode_steps": int(s.lengths.sum().item()),
                      "secondary_steps": int(a.secondary_steps.sum().item()), "switches": int(a.switches.sum().item()),
                      "terminated_share": float(a.terminated.float().mean().item()),
                      "launches_loop": (4 + len(blocks)) * steps}))
    dp.close()
    dp2.close()
    eng.close()


def hybrid_usage(config, stochastic):
    """VGPRs and scratch bytes per lane of the hybrid kernel (`stochastic`: of the stochastic hybrid kernel) for a pair of
    HYBRID_PAIRS: the translation unit pi_infer_set_partner (pi_infer_set_partner_stochastic) hands to hipRTC, built ahead
    of time with the same flags."""
    import tempfile
    import numpy as np
    from __graft_entry__ import HIPCC
    from dynamicprogramming_amd import envs
    env, bins, env2, bins2, _, _ = HYBRID_PAIRS[config]

    def braces(v, fmt):
        return "{" + ",".join(fmt(x) for x in v) + "}"

    def hexf(x):
        return float(np.float32(x)).hex() + "f"

    def grid_defines(prefix, e, g):
        _, (lo, hi, shape, strides, bits) = _grid_tables(e, g)
        return (f"#define {prefix}_D {len(lo)}\n#define {prefix}_LO_INIT {braces(lo, hexf)}\n"
                f"#define {prefix}_HI_INIT {braces(hi, hexf)}\n#define {prefix}_SHAPE_INIT {braces(shape, str)}\n"
                f"#define {prefix}_STRIDES_INIT {braces(strides, str)}\n"
                f"#define {prefix}_BITS_INIT {braces(bits, lambda r: braces(r, str))}\n")
    csrc = ROOT / "dynamicprogramming_amd" / "csrc"
    defines = "#define PI_HYBRID_STOCHASTIC 1\n#define PI_HYBRID 1\n#define PI_STOCHASTIC 1\n" if stochastic else "#define PI_HYBRID 1\n"
    files = ["pi_rollout_kernels.hip", "pi_hybrid_kernels.hip"] + (
        ["pi_stochastic_kernels.hip", "pi_hybrid_stochastic_kernels.hip"] if stochastic else [])
    text = (defines + grid_defines("PI", env, bins) + grid_defines("PI2", env2, bins2) +
            f"{(ROOT / 'include' / 'pi_math.h').read_text()}\n#define sinf pi_sinf\n#define cosf pi_cosf\n#define fmodf pi_fmodf\n"
            f"{envs.dynamics_source(env)}\n" + "".join((csrc / f).read_text() + "\n" for f in files))
    usage, fn = {}, None
    with tempfile.TemporaryDirectory(prefix="pi_hybrid_") as tmp:
        src = Path(tmp) / "hybrid.hip"
        src.write_text(text)
        res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "--genco",
                              "-include", "hip/hip_runtime.h", "-Rpass-analysis=kernel-resource-usage", str(src), "-o",
                              str(Path(tmp) / "hybrid.hsaco")], capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"hipcc failed on the hybrid translation unit of {config}\n{res.stderr[-2000:]}")
    for line in res.stderr.splitlines():
        if "Function Name:" in line:
            fn = line.split("Function Name:")[1].split()[0]
            usage[fn] = {}
        elif fn and " VGPRs:" in line:
            usage[fn]["vgpr"] = int(line.split("VGPRs:")[1].split()[0])
        elif fn and "ScratchSize" in line:
            usage[fn]["scratch"] = int(line.split(":")[-1].split()[0])
    return usage


def hybrid_stochastic_driver(args):
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    rows = []
    for config in HYBRID_PAIRS:
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--hybrid", "--stochastic", "--config",
                              config, "--m", str(args.m), "--steps", str(args.steps), "--repeat", str(args.repeat)],
                             capture_output=True, text=True)
        if res.returncode != 0:                           # a fault, an abort or a time limit: nothing more runs
            sys.exit(f"stochastic hybrid {config} ended with status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
        rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    lines = [f"stochastic hybrid rollouts (two policies, Philox4x32-10 in the kernel) vs the step-by-step loop, MI355X, commit {args.commit}",
             f"{args.m} episodes of {args.steps} steps, seeded random policies on both grids, epsilon 0.3, action noise a tenth of the "
             "action range, state noise 0.2 % of the span in every dimension, the primary's actions as the exploration table, "
             f"starts uniform in the primary grid; times in ms per call: the better of {args.repeat} samples after one warm-up, "
             f"device events around {FUSED_PER_SAMPLE} fused calls back to back (one call of the loop), the four paths alternating",
             "loop: per step a query on each handle, the probe kernel's words, one plugin step and the mixing as torch ops; "
             "hybrid: the deterministic hybrid rollout (pi_infer_rollout_hybrid) of the same batch; single: the single-policy "
             "stochastic rollout (pi_infer_rollout_stochastic) of the same batch; ep-steps: steps actually taken (episodes that "
             "ended stop), in the order fused / hybrid / single",
             "",
             f"{'pair':58s} {'fused':>8s} {'loop':>10s} {'loop/fused':>10s} {'hybrid':>8s} {'single':>8s} {'ep-steps':>28s} "
             f"{'mode-1':>9s} {'switches':>9s} {'ended':>6s} {'same bits':>9s}"]
    for r in rows:
        steps3 = f"{r['episode_steps']} / {r['plain_episode_steps']} / {r['single_episode_steps']}"
        lines.append(f"{r['config'] + ' ' + r['pair']:58s} {r['fused_ms']:8.3f} {r['loop_ms']:10.3f} {r['loop_ms'] / r['fused_ms']:10.1f} "
                     f"{r['plain_ms']:8.3f} {r['single_ms']:8.3f} {steps3:>28s} {r['secondary_steps']:9d} {r['switches']:9d} "
                     f"{r['terminated_share']:6.3f} {str(r['same_bits']):>9s}")
    lines += ["", "all samples per config (ms per call): " + "; ".join(
        f"{r['config']} fused {[round(t, 3) for t in r['fused_ms_all']]} loop {[round(t, 1) for t in r['loop_ms_all']]}" for r in rows)]
    slower = [r["config"] for r in rows if r["fused_ms"] >= r["loop_ms"] or not r["same_bits"]]
    lines += ["", "the fused kernel is faster than its own step-by-step loop, with the same bits, on every pair" if not slower else
              f"the fused kernel is NOT faster than its own step-by-step loop with the same bits on: {', '.join(slower)}", "",
              "registers and scratch (hipcc -Rpass-analysis=kernel-resource-usage, the translation units of "
              "pi_infer_set_partner_stochastic and pi_infer_set_partner):"]
    for config in HYBRID_PAIRS:
        for stochastic in (True, False):
            for fn, k in sorted(hybrid_usage(config, stochastic).items()):
                lines.append(f"  {config} {fn:38s} VGPRs {k['vgpr']:4d}  scratch {k['scratch']} bytes/lane")
    lines += ["", "closed loop of the reference pair (trained 6-D archives) under noise: not measured"]
    out.write_text("\n".join(lines) + "\n")
    print(out.read_text())


def hybrid_driver(args):
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    me = [sys.executable, str(Path(__file__).resolve())]
    rows = []
    for m in BATCHES:
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--hybrid", "--m", str(m), "--steps",
                              str(args.steps), "--repeat", str(args.repeat)], capture_output=True, text=True)
        if res.returncode != 0:                           # a fault, an abort or a time limit: nothing more runs
            sys.exit(f"hybrid m={m} ended with status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
        rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    lines = ["", f"hybrid rollouts (25^6 swing-up + 25^6 balance, the reference's switch box), MI355X, commit {args.commit}",
             f"{'m':>7s} {'fused':>10s} {'loop':>10s} {'loop/fused':>10s} {'single':>10s} {'ep-steps':>12s} {'mode-1 steps':>12s} "
             f"{'ended':>6s} {'same bits':>9s}"]
    for r in rows:
        lines.append(f"{r['m']:7d} {r['fused_ms']:10.3f} {r['loop_ms']:10.3f} {r['loop_ms'] / r['fused_ms']:10.1f} "
                     f"{r['single_ms']:10.3f} {r['episode_steps']:12d} {r['secondary_steps']:12d} {r['terminated_share']:6.3f} "
                     f"{str(r['same_bits']):>9s}")
    with out.open("a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def driver(args):
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    rows = []
    me = [sys.executable, str(Path(__file__).resolve())]
    common = ["--steps", str(args.steps), "--repeat", str(args.repeat)]
    for config in CONFIGS:
        for m in BATCHES:
            res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--config", config, "--m", str(m),
                                  *common], capture_output=True, text=True)
            if res.returncode != 0:                       # a fault, an abort or a time limit: nothing more runs
                sys.exit(f"{config} m={m} ended with status {res.returncode}; stopping\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            rows.append(json.loads(res.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)
    lines = [f"fused rollouts vs the step-by-step loop, MI355X, commit {args.commit}",
             f"{args.steps} steps per episode, seeded random policy, starts uniform in the grid; times in ms: the better of "
             f"{args.repeat} after one warm-up, device events around the whole call",
             "episode-steps: steps actually taken (episodes that ended stop); launch-bound time of the loop: "
             "2 launches per step x ~5 us = the time the loop cannot go below whatever the kernels cost",
             "",
             f"{'config':28s} {'m':>7s} {'fused':>10s} {'loop':>10s} {'loop/fused':>10s} {'ep-steps':>12s} {'M ep-steps/s':>12s} "
             f"{'ended':>6s} {'same bits':>9s}"]
    for r in rows:
        lines.append(f"{r['config'] + ' ' + r['env'] + ' ' + str(r['bins']) + '^' + str(r['D']):28s} {r['m']:7d} "
                     f"{r['fused_ms']:10.3f} {r['loop_ms']:10.3f} {r['loop_ms'] / r['fused_ms']:10.1f} {r['episode_steps']:12d} "
                     f"{r['episode_steps'] / r['fused_ms'] / 1e3:12.2f} {r['terminated_share']:6.3f} {str(r['same_bits']):>9s}")
    out.write_text("\n".join(lines) + "\n")
    # kernel time of the fused call alone, in a run of its own (tracing slows the host)
    trace_dir = out.parent / "rollout_trace"
    res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), "rocprofv3", "--kernel-trace", "--stats", "-d", str(trace_dir),
                          "--", *me, "--child", "--fused-only", "--config", "c3", "--m", "4096", *common],
                         capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(f"rocprofv3 run ended with status {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    stats = sorted(trace_dir.rglob("*kernel_stats.csv"))
    with out.open("a") as f:
        f.write("\nrocprofv3 --kernel-trace --stats, fused call alone (c3, m = 4096; warm-up + one call):\n")
        for p in stats:
            for line in p.read_text().splitlines()[:6]:
                f.write("  " + line + "\n")
    print(out.read_text())


# ── --adversary: the adversary rollouts (pi_infer_rollout_adversary, csrc/pi_adversary_kernels.hip) ───────────────────────
def adversary_child(args):
    """Timing on one config: 4 096 episodes x --steps steps on a random V and policy, K = 9 and 27: the adversary rollout
    under both controllers beside the expected-greedy rollout (no noise) of the same batch, better of --repeat; and, for
    the robust controller, the step-by-step loop it replaces — per step one robust() query, the adversary's answer applied
    with torch (the clamp of a + da_k*, dx_k* on steps that are not done) and one pi_probe_step launch — with its bits."""
    import numpy as np
    import torch
    import utils.barycentric as B
    from itertools import product
    from dynamicprogramming_amd import _native, envs
    from dynamicprogramming_amd.noise import Disturbances
    env, bins = CONFIGS[args.config]
    cls = envs.ENVS[env]
    tabs = [np.asarray(t, np.float32) for t in cls.bins_space(bins).values()]
    D = len(tabs)
    shape = np.array([len(t) for t in tabs], np.int32)
    lo, hi = np.array([t.min() for t in tabs], np.float32), np.array([t.max() for t in tabs], np.float32)
    strides = np.array([int(np.prod(shape[d + 1:])) for d in range(D)], np.int32)
    bits = np.array(list(product([0, 1], repeat=D)), dtype=np.int32)
    acts = np.asarray(cls.ACTIONS, np.float32)
    rng = np.random.default_rng(0)
    n = int(np.prod(shape.astype(np.int64)))
    policy = rng.integers(0, len(acts), size=n, dtype=np.int32)
    V = (30.0 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    a_noise = float(np.float32(0.1) * (acts.max() - acts.min()))
    s_noise = (np.float32(0.002) * (hi - lo)).astype(np.float32)
    one, two = np.zeros(D), np.zeros(D)
    one[1] = two[0] = two[1] = 1.0
    sets = {9: Disturbances.uniform(D, state_noise=one * s_noise, action_noise=a_noise),
            27: Disturbances.uniform(D, state_noise=two * s_noise, action_noise=a_noise)}
    dev = torch.device("cuda:0")
    starts = torch.from_numpy((lo + (hi - lo) * rng.random((args.m, D), dtype=np.float32)).astype(np.float32)).to(dev)
    dp = B.DevicePolicy(policy, acts, lo, hi, shape, strides, bits, device=dev)
    dp.set_dynamics(envs.dynamics_source(env))
    dp.set_values(V)
    dp.set_expected_greedy()
    dp.set_robust()
    eng = _native.Engine(D, shape, lo, hi, tabs, acts, device=0)
    eng.compile(envs.dynamics_source(env))
    st = torch.cuda.current_stream(dev).cuda_stream
    m = args.m
    a_lo, a_hi = torch.tensor(float(acts.min()), device=dev), torch.tensor(float(acts.max()), device=dev)

    def loop(d):                                          # the robust controller against the adversary, one launch per piece
        da = torch.from_numpy(d.action_offsets).to(dev)
        dx = torch.from_numpy(d.state_offsets).to(dev)
        states = starts.clone()
        nxt = torch.empty_like(states)
        rew = torch.empty(m, dtype=torch.float32, device=dev)
        done = torch.empty(m, dtype=torch.uint8, device=dev)
        ret = torch.zeros(m, dtype=torch.float32, device=dev)
        length = torch.zeros(m, dtype=torch.int32, device=dev)
        ended = torch.zeros(m, dtype=torch.bool, device=dev)
        won = torch.ones((), dtype=torch.bool, device=dev)
        for t in range(args.steps):
            _, act, _, worst = dp.robust(states, 0.99)
            won = won & (worst >= 0).all()                # (no winner: the fused kernel keeps action 0's step, which this
            k = worst.clamp(min=0).to(torch.int64)        # loop cannot know — never the case on a finite V)
            push = da[k]
            act = torch.where(push == 0, act, torch.fmin(torch.fmax(act + push, a_lo), a_hi)).contiguous()
            eng.probe_step(states.data_ptr(), act.data_ptr(), nxt.data_ptr(), rew.data_ptr(), done.data_ptr(), m, st)
            shift = dx[k]
            moved = torch.where(shift != 0, nxt + shift, nxt)
            nxt2 = torch.where((done == 0)[:, None], moved, nxt)
            run = ~ended
            ret = torch.where(run, ret + rew, ret)
            states = torch.where(run[:, None], nxt2, states)
            length = torch.where(run, torch.full_like(length, t + 1), length)
            ended = ended | (run & (done != 0))
        assert bool(won.item()), "an episode had no winning action: the loop is not the fused rollout there"
        return B.RolloutResult(states, ret, length, ended, None)

    def timed(fn):
        best = float("inf")
        fn()
        for _ in range(args.repeat):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            res = fn()
            t1.record()
            torch.cuda.synchronize()
            best = min(best, t0.elapsed_time(t1))
        return best, float(res.lengths.float().mean())
    rows = []
    for K, d in sets.items():
        dp.set_disturbances(d)
        row = {"K": K}
        for label, fn in (("expected", lambda: dp.rollout(starts, args.steps, controller="expected", lookahead_gamma=0.99)),
                          ("adv_policy", lambda: dp.adversary_rollout(starts, args.steps, controller="policy", lookahead_gamma=0.99)),
                          ("adv_robust", lambda: dp.adversary_rollout(starts, args.steps, controller="robust", lookahead_gamma=0.99))):
            row[label + "_ms"], row[label + "_len"] = timed(fn)
        a, b = dp.adversary_rollout(starts, args.steps, controller="robust", lookahead_gamma=0.99), loop(d)
        torch.cuda.synchronize()
        row["same_bits"] = bool(torch.equal(a.states.view(torch.int32), b.states.view(torch.int32))
                                and torch.equal(a.returns.view(torch.int32), b.returns.view(torch.int32))
                                and torch.equal(a.lengths, b.lengths) and torch.equal(a.terminated != 0, b.terminated))
        row["loop_ms"], row["loop_len"] = timed(lambda: loop(d))
        row["launches_loop"] = 2 * args.steps
        rows.append(row)
    print(json.dumps({"config": args.config, "env": env, "bins": bins, "D": D, "actions": len(acts), "m": args.m,
                      "steps": args.steps, "rows": rows}))
    dp.close()
    eng.close()


def adversary_loop_child(args):
    """Closed loop on one env of tools/expect_bench.py's settings: the nominal, noise-aware and worst-case tables, each under
    the sampled noise planned for and under the adversary over the same set (its policy table acting): mean return and the
    share of episodes that terminated."""
    import numpy as np
    sys.path.insert(0, str(ROOT / "tools"))
    from expect_bench import LOOPS
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
    rule = Disturbances.uniform(len(tabs), state_noise=x_noise, action_noise=a_noise)
    starts = cls.start_states(np.random.default_rng(args.seed), args.m)
    out = {"env": env, "bins": bins, "K": rule.K, "steps": args.loop_steps, "m": args.m, "runs": {}}
    for label, d, risk in (("nominal", None, {}), ("noise-aware", rule, {}), ("worst-case", rule, {"risk": "worst"})):
        solver = envs.make(env, bins, CudaPIConfig(**{**cls.CONFIG, **caps}), device="cuda:0", transport=False)
        if d is not None:
            solver.set_disturbances(d, **risk)
        solver.run()
        run = {}
        for world, res in (("sampled", solver.rollout(starts, args.loop_steps, gamma=1.0, action_noise=a_noise, state_noise=x_noise, seed=args.seed)),
                           ("adversary", solver.adversary_rollout(starts, args.loop_steps, controller="policy", disturbances=rule)),
                           ("adversary_robust", solver.adversary_rollout(starts, args.loop_steps, controller="robust", disturbances=rule))):
            run[world] = {"mean_return": float(np.mean(res.returns)), "terminated_share": float(np.mean(res.terminated)),
                          "mean_length": float(np.mean(res.lengths))}
        out["runs"][label] = run
    print(json.dumps(out))


def adversary_driver(args):
    if args.out == DEFAULT_OUT:                            # not the first rollout profile: a file of this part's own
        args.out = str(ROOT / "profiles" / "r16" / "adversary_rollouts.txt")
    me = [sys.executable, str(Path(__file__).resolve())]
    lines = [f"adversary rollouts (tools/rollout_bench.py --adversary), MI355X, commit {args.commit}", "",
             f"timing: {args.m} episodes x {args.steps} steps, random V and policy, ms per launch (better of {args.repeat}) and mean "
             "episode length",
             f"{'config':28s} {'K':>3s} {'expected-greedy':>16s} {'len':>7s} {'adversary, table':>17s} {'len':>7s} {'adversary, robust':>18s} {'len':>7s}"
             f" {'its per-step loop':>18s} {'same bits':>10s}"]
    jobs = [("timing", ["--config", c]) for c in CONFIGS] + [("loop", ["--env", e]) for e in ("pendulum", "cartpole_swingup")]
    loops = []
    for kind, extra in jobs:
        res = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), *me, "--child", "--adversary", "--part", kind, *extra,
                              "--steps", str(args.steps), "--repeat", str(args.repeat), "--m", str(args.m),
                              "--loop-steps", str(args.loop_steps), "--seed", str(args.seed)], capture_output=True, text=True)
        print(f"[rollout_bench --adversary] {kind} {' '.join(extra)}: status {res.returncode}", flush=True)
        if res.returncode != 0:
            lines.append(f"NOT MEASURED: {kind} {' '.join(extra)} ended with status {res.returncode}: {res.stderr.strip()[-400:]}")
            break
        r = json.loads(res.stdout.strip().splitlines()[-1])
        if kind == "timing":
            name = f"{r['config']} {r['env']} {r['bins']}^{r['D']} x {r['actions']}"
            for row in r["rows"]:
                lines.append(f"{name:28s} {row['K']:3d} {row['expected_ms']:16.3f} {row['expected_len']:7.1f} {row['adv_policy_ms']:17.3f} "
                             f"{row['adv_policy_len']:7.1f} {row['adv_robust_ms']:18.3f} {row['adv_robust_len']:7.1f} "
                             f"{row['loop_ms']:18.3f} {str(row['same_bits']):>10s}")
        else:
            loops.append(r)
    for r in loops:
        lines += ["", f"closed loop: {r['env']} {r['bins']} bins, the {r['K']}-point rule of tools/expect_bench.py, {r['m']} episodes of "
                      f"{r['steps']} steps: mean return / share terminated",
                  f"{'table':12s} | {'sampled noise':>22s} | {'adversary, its table':>22s} | {'adversary, robust lookahead on its V':>36s}"]
        for label, run in r["runs"].items():
            cell = lambda w: f"{run[w]['mean_return']:12.3f} / {run[w]['terminated_share']:.4f}"      # noqa: E731
            lines.append(f"{label:12s} | {cell('sampled'):>22s} | {cell('adversary'):>22s} | {cell('adversary_robust'):>36s}")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--hybrid", action="store_true")
    ap.add_argument("--greedy", action="store_true")
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--expected", action="store_true")
    ap.add_argument("--adversary", action="store_true")
    ap.add_argument("--part", choices=("timing", "loop"), default="timing")
    ap.add_argument("--env", default="pendulum")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--loop-steps", type=int, default=1000)
    ap.add_argument("--config", choices=list(CONFIGS), default="c3")
    ap.add_argument("--m", type=int, default=4096)
    args = ap.parse_args()
    if args.hybrid and args.stochastic:
        (hybrid_stochastic_child if args.child else hybrid_stochastic_driver)(args)
    elif args.greedy:
        (greedy_child if args.child else greedy_driver)(args)
    elif args.stochastic:
        (stochastic_child if args.child else stochastic_driver)(args)
    elif args.adversary:
        ((adversary_child if args.part == "timing" else adversary_loop_child) if args.child else adversary_driver)(args)
    elif args.expected:
        ((expected_child if args.part == "timing" else expected_loop_child) if args.child else expected_driver)(args)
    elif args.hybrid:
        (hybrid_child if args.child else hybrid_driver)(args)
    else:
        (child if args.child else driver)(args)


if __name__ == "__main__":
    main()
