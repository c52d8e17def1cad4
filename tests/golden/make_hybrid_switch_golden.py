"""
tests/golden/make_hybrid_switch_golden.py — the hybrid runner's switch rule pinned to reference-EXECUTED code.

The reference's hybrid double cart-pole runner (runners/hybrid_double_cartpole.py) chooses between its two policies
with `_use_balance(th1, w1, th2, w2, currently_balancing)` (:62-69) and four threshold constants (:56-59).  This
script RUNS that function — the reference's own Python, in the build container — along seeded state sequences that
wander across all four thresholds in both directions, and stores states in, modes out, as data
(tests/golden/hybrid_switch.npz).  The reference cannot travel; only the vectors are committed.

The runner module cannot be imported here (it imports the solver stack), so its text is parsed with `ast` as in
make_step_python_golden.py and exactly the constant assignments and `def _use_balance` are executed.  Nothing of the
reference is written anywhere.

    python -m tests.golden.make_hybrid_switch_golden

The archive holds  states (n_seq, T, 6) float32 — (x, x', th1, w1, th2, w2), float32-representable and handed to the
function as float64 —, modes (n_seq, T) bool — `balancing` after step t, every sequence starting from False —, and
thresholds (4,) float64 = (_ENTER_TH, _ENTER_W, _EXIT_TH, _EXIT_W).  No emitted |th| or |w| lies within 1e-5 of one of
its thresholds (such states are resampled), so a float32 comparison decides every step as the reference's float64 one.
"""
from __future__ import annotations

import ast
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests.golden.make_step_python_golden import REF  # noqa: E402

OUT = Path(__file__).resolve().parent / "hybrid_switch.npz"
N_SEQ, T = 6, 3000
MARGIN = 1e-5
NAMES = ("_ENTER_TH", "_ENTER_W", "_EXIT_TH", "_EXIT_W")


def load_use_balance(path: Path):
    """(_use_balance, namespace) from the runner's text: constant assignments + the one function."""
    ns = {"np": np, "__name__": "reference_use_balance"}
    found = False
    for node in ast.parse(path.read_text()).body:
        keep = isinstance(node, ast.Assign) and all(isinstance(t, ast.Name) for t in node.targets)
        if isinstance(node, ast.FunctionDef) and node.name == "_use_balance":
            keep = found = True
        if not keep:
            continue
        try:
            exec(compile(ast.Module(body=[node], type_ignores=[]), str(path), "exec"), ns)
        except Exception:                       # a constant built from something outside numpy: not needed
            if isinstance(node, ast.FunctionDef):
                raise
    if not found or not all(k in ns for k in NAMES):
        raise LookupError(f"_use_balance or its thresholds not found in {path}")
    return ns["_use_balance"], ns


def sequence(rng, th_enter, w_enter, th_exit, w_exit):
    """T states whose pole coordinates wander around the band between the two boxes: a shared slow excursion moves all
    four through the thresholds together (so that the box is entered and left), independent noise on each makes single
    coordinates cross alone, and the signs flip now and then (the rule sees magnitudes)."""
    z = 0.0
    own = np.zeros(4)
    sign = np.ones(4)
    centre = np.array([(th_enter + th_exit) / 2, (w_enter + w_exit) / 2] * 2)
    reach = np.array([(th_exit - th_enter) * 1.6, (w_exit - w_enter) * 1.6] * 2)
    thr = np.array([[th_enter, th_exit], [w_enter, w_exit]] * 2)
    out = np.empty((T, 6), np.float32)
    for t in range(T):
        z += 0.08 * (0.0 - z) + 0.35 * rng.standard_normal()
        own += 0.3 * (0.0 - own) + 0.25 * rng.standard_normal(4)
        sign = np.where(rng.random(4) < 0.02, -sign, sign)
        while True:
            v = (sign * (centre + reach * (z + own))).astype(np.float32)
            if (np.abs(np.abs(v.astype(np.float64))[:, None] - thr) > MARGIN).all():
                break
            own += 1e-3 * rng.standard_normal(4)                # resample: too close to a threshold
        out[t, :2] = rng.uniform(-2.0, 2.0, 2)
        out[t, 2:] = v
    return out


def main() -> None:
    path = REF / "hybrid_double_cartpole.py"
    if not path.exists():
        raise SystemExit(f"{path} is not present: fixtures can only be generated in the build container")
    use_balance, ns = load_use_balance(path)
    thr = np.array([float(ns[k]) for k in NAMES])
    rng = np.random.default_rng(6200)
    states = np.stack([sequence(rng, *thr) for _ in range(N_SEQ)])
    modes = np.zeros((N_SEQ, T), bool)
    for q in range(N_SEQ):
        balancing = False
        for t in range(T):
            x, xd, th1, w1, th2, w2 = states[q, t].astype(np.float64)
            balancing = bool(use_balance(th1, w1, th2, w2, balancing))
            modes[q, t] = balancing
    mag = np.abs(states[:, :, 2:].astype(np.float64))
    for j, name in enumerate(("th1", "w1", "th2", "w2")):
        for k, which in ((0, "enter"), (2, "exit")):
            level = thr[k + j % 2]
            above = mag[:, :, j] > level
            up = int((~above[:, :-1] & above[:, 1:]).sum())
            down = int((above[:, :-1] & ~above[:, 1:]).sum())
            assert up > 20 and down > 20, (name, which, up, down)
            print(f"|{name}| crosses its {which} threshold {level}: {up} times upward, {down} downward")
    prev = np.concatenate([np.zeros((N_SEQ, 1), bool), modes[:, :-1]], axis=1)
    print(f"{N_SEQ} sequences of {T} states: {int((~prev & modes).sum())} entries, {int((prev & ~modes).sum())} exits, "
          f"{modes.mean():.3f} of the steps in balance mode")
    assert (~prev & modes).sum() > 50 and (prev & ~modes).sum() > 50
    np.savez_compressed(OUT, states=states, modes=modes, thresholds=thr)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
