"""
Anderson-accelerated policy evaluation: the method, once, and the numpy twin of its device kernels.

Evaluating a fixed policy solves (I - gamma P) V = r by Richardson iteration, whose error shrinks by gamma per sweep.
Once per FULL batch of SYNC_INTERVAL sweeps — where the host synchronises anyway — the loop below extrapolates over a ring
of up to 8 past batches (type-II Anderson acceleration on the batch map) and lets the next batch start from the result.
The stopping rule is untouched: the evaluation ends when the residual of a batch's last sweep is below theta, so the
returned V is a plain sweep's output with ||V - V_pi|| < gamma theta / (1 - gamma), whatever produced that sweep's input.

``evaluate`` is the one definition of the loop; the solver runs it over device tensors and the kernels of
csrc/pi_accel_kernels.hip, ``accelerated_evaluation`` runs it over numpy arrays and the functions of this module.
``dots``, ``combine`` and ``solve`` are exactly the arithmetic include/pi_mi355.h defines at pi_accel_update, the
reduction tree included, so the two agree bit for bit (``solve`` is the same host code on both sides).  Arrays enter in
MEMORY order: the reduction order is over the flat index of the array as it lies in memory.  No torch, no GPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

TILE = 4096            # consecutive elements per tile of a dot product (PI_ACCEL_TILE)
BLOCK = 256            # threads per tile (PI_ACCEL_BLOCK)
MAX_WINDOW = 8         # columns of the ring, at most (PI_ACCEL_MAXK)
MAX_RESTARTS = 3       # after this many restarts the rest of an evaluation runs plain
REGULARISATION = 1e-12  # lambda = this * trace of the Gram matrix
_TILES_PER_PASS = 2048  # twin only: tiles reduced at a time (bounds the float64 temporaries)


@dataclass(frozen=True)
class Anderson:
    """Settings of the acceleration: ``window`` columns (1 .. 8) and the restart factor kappa — a full batch whose residual
    exceeds kappa times the previous full batch's clears the history."""
    window: int = 4
    restart: float = 2.0

    def __post_init__(self):
        if not (isinstance(self.window, (int, np.integer)) and 1 <= int(self.window) <= MAX_WINDOW):
            raise ValueError(f"window must be an integer in [1, {MAX_WINDOW}], not {self.window!r}")
        if not (math.isfinite(float(self.restart)) and float(self.restart) > 0.0):
            raise ValueError(f"restart must be a positive finite factor, not {self.restart!r}")


# ── the arithmetic ──────────────────────────────────────────────────────────────────────
def _tree(v: np.ndarray) -> np.ndarray:
    """(.., 256) float64 thread sums -> (..) sums: per wave of 64 lanes, lanes 0 .. o-1 add lanes o .. 2o-1 for
    o = 32 .. 1; then (w0 + w2) + (w1 + w3)."""
    p = v.reshape(v.shape[:-1] + (BLOCK // 64, 64)).copy()
    o = 32
    while o:
        p[..., :o] = p[..., :o] + p[..., o:2 * o]
        o >>= 1
    w = p[..., 0]
    return (w[..., 0] + w[..., 2]) + (w[..., 1] + w[..., 3])


def _fold(parts: np.ndarray) -> float:
    """Tile sums -> the dot product: thread t adds sums t, t + 256, .. to 0.0 in ascending order, then the tree."""
    rounds = -(-len(parts) // BLOCK)
    padded = np.zeros(rounds * BLOCK, dtype=np.float64)
    padded[:len(parts)] = parts
    acc = np.zeros(BLOCK, dtype=np.float64)
    for row in padded.reshape(rounds, BLOCK):
        acc = acc + row
    return float(_tree(acc))


def _tile_sums(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Per tile of 4 096 elements the sum of (double)a * (double)b: thread t owns elements 4t .. 4t + 3 of each of the
    four 1 024-element chunks and adds their products to 0.0 in ascending index.  Elements past the end take no part
    (a product of +0.0 added to a sum that started at +0.0 changes nothing)."""
    n = len(a)
    tiles = -(-n // TILE)
    out = np.empty(tiles, dtype=np.float64)
    for t0 in range(0, tiles, _TILES_PER_PASS):
        t1 = min(tiles, t0 + _TILES_PER_PASS)
        lo, hi = t0 * TILE, min(n, t1 * TILE)
        prod = np.zeros((t1 - t0) * TILE, dtype=np.float64)
        prod[:hi - lo] = a[lo:hi].astype(np.float64) * b[lo:hi].astype(np.float64)
        prod = prod.reshape(t1 - t0, TILE // (4 * BLOCK), BLOCK, 4)
        acc = np.zeros((t1 - t0, BLOCK), dtype=np.float64)
        for c in range(prod.shape[1]):
            for i in range(4):
                acc = acc + prod[:, c, :, i]
        out[t0:t1] = _tree(acc)
    return out


def dot(a, b) -> float:
    """One dot product of two float32 arrays in the fixed tree (float64 products and sums)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32).ravel(), np.ascontiguousarray(b, dtype=np.float32).ravel()
    assert len(a) == len(b) and len(a) > 0
    return _fold(_tile_sums(a, b))


def dots(x, g, f_prev, g_prev, dF, dG, slot: int, k_used: int, first: bool) -> np.ndarray:
    """Twin of pi_accel_update, in place on float32 numpy arrays (dF, dG: (m, n)): f = g - x; unless `first`, column
    `slot` of dF / dG becomes (f - f_prev, g - g_prev); (f_prev, g_prev) <- (f, g).  Returns the 2 k_used + 1 float64
    values {dF_j . f | dF_j . dF_slot | f . f} over ring positions j < k_used (`first`: k_used = 0, only f . f)."""
    m = dF.shape[0]
    if not (0 <= k_used <= min(m, MAX_WINDOW)) or not (0 <= slot < m):
        raise ValueError("k_used must be in [0, min(m, 8)] and slot in [0, m)")
    if (k_used != 0) if first else (k_used < 1 or slot >= k_used):
        raise ValueError("the first push takes k_used = 0, every later one k_used >= 1 and slot < k_used")
    f = g - x                                               # one float32 subtraction
    if not first:
        dF[slot] = f - f_prev
        dG[slot] = g - g_prev
    f_prev[...] = f
    g_prev[...] = g
    out = np.empty(2 * k_used + 1, dtype=np.float64)
    for j in range(k_used):
        out[j] = dot(dF[j], f)
        out[k_used + j] = dot(dF[j], dF[slot])
    out[2 * k_used] = dot(f, f)
    return out


def combine(g, dG, coeffs, k_used: int, out=None) -> np.ndarray:
    """Twin of pi_accel_combine: out[s] = (float)((double)g[s] - S), S = 0.0 + c_0 dG_0[s] + c_1 dG_1[s] + .. in ascending
    ring position (float64, a multiply then an add each).  `out` may be `g`."""
    s = np.zeros(g.shape, dtype=np.float64)
    for j in range(k_used):
        if not math.isfinite(float(coeffs[j])):
            raise ValueError(f"coefficient {j} is not finite")
        s = s + float(coeffs[j]) * dG[j].astype(np.float64)
    res = (g.astype(np.float64) - s).astype(np.float32)
    if out is None:
        return res
    out[...] = res
    return out


def solve(gram, rhs):
    """(G + lambda I) c = rhs with lambda = 1e-12 trace(G), by one Cholesky factorisation in plain Python floats.  Returns
    the list c, or None for "failed": a pivot <= 0 or anything that is not finite.  The solver and the twin both call
    this function, so the coefficients are the same bits on both sides."""
    k = len(rhs)
    a = [[float(gram[i][j]) for j in range(k)] for i in range(k)]
    b = [float(v) for v in rhs]
    trace = 0.0
    for i in range(k):
        trace = trace + a[i][i]
    lam = REGULARISATION * trace
    if not math.isfinite(lam):
        return None
    low = [[0.0] * k for _ in range(k)]
    for i in range(k):
        for j in range(i + 1):
            s = a[i][j] + (lam if i == j else 0.0)
            for p in range(j):
                s = s - low[i][p] * low[j][p]
            if i == j:
                if not (s > 0.0) or not math.isfinite(s):
                    return None
                low[i][i] = math.sqrt(s)
            else:
                low[i][j] = s / low[j][j]
    y = [0.0] * k
    for i in range(k):
        s = b[i]
        for p in range(i):
            s = s - low[i][p] * y[p]
        y[i] = s / low[i][i]
    c = [0.0] * k
    for i in reversed(range(k)):
        s = y[i]
        for p in range(i + 1, k):
            s = s - low[p][i] * c[p]
        c[i] = s / low[i][i]
    if not all(math.isfinite(v) for v in c):
        return None
    return c


# ── the loop ────────────────────────────────────────────────────────────────────────────
class History:
    """Host bookkeeping of the ring: how many columns are in use, which position the next push overwrites, the Gram matrix
    of the columns in use.  The columns themselves live with the caller."""

    def __init__(self, window: int):
        self.window = int(window)
        self.clear()

    def clear(self) -> None:
        self.columns = 0            # ring positions 0 .. columns - 1 hold a column
        self.slot = 0               # the position the next push writes
        self.have_prev = False      # f_prev / g_prev hold a full batch of this history
        self.gram = [[0.0] * self.window for _ in range(self.window)]

    def next_push(self):
        """(slot, k_used, first) of the update that follows the batch in flight."""
        if not self.have_prev:
            return 0, 0, True
        return self.slot, min(self.columns + 1, self.window), False

    def commit(self, slot: int, k_used: int, values) -> list:
        """Take the dot products of an update that pushed a column: the new row of the Gram matrix; returns dF^T f."""
        for j in range(k_used):
            self.gram[slot][j] = self.gram[j][slot] = float(values[k_used + j])
        self.columns = k_used
        self.slot = (slot + 1) % self.window
        return [float(values[j]) for j in range(k_used)]


def evaluate(ops, theta: float, max_iter: int, settings: Anderson | None, interval: int, on_check=None):
    """One policy evaluation.  The check schedule is the plain loop's: batches of 1, `interval`, `interval`, .. sweeps (the
    last one cut at `max_iter`), the residual delta of a batch's last sweep is looked at after it, delta < theta ends the
    evaluation.  Only batches of exactly `interval` sweeps take part in the acceleration:

      before the batch   ops.snapshot()                      x <- V
      after it           ops.update(slot, k_used, first)     f = g - x, the ring's new column, the dot products
      one host sync      ops.read(count) -> (delta, dots)
      restart            when delta > kappa * (delta of the previous full batch), when a dot product is not finite or the
                         solve fails: the history is cleared, nothing is extrapolated, the next batch goes on from g;
                         after MAX_RESTARTS restarts the rest of the evaluation runs plain
      otherwise          the first full batch of a history only stores (f_prev, g_prev); with k >= 1 columns
                         c = solve(dF^T dF, dF^T f) and ops.combine(c, k): V <- g - dG c.

    `ops` also has sweeps(n).  settings = None: the plain loop.  Returns (delta, sweeps, extrapolations, restarts,
    converged)."""
    history = History(settings.window) if settings is not None else None
    kappa = float(settings.restart) if settings is not None else 0.0
    active = settings is not None
    delta, delta_prev = float("inf"), None
    i = sweeps = extrapolations = restarts = 0
    converged = False
    while i < max_iter:
        check = i if i % interval == 0 else (i // interval + 1) * interval
        check = min(check, max_iter - 1)
        n = check - i + 1
        full = active and n == interval
        if full:
            ops.snapshot()
        ops.sweeps(n)
        sweeps += n
        i = check + 1
        push = None
        if full:
            push = history.next_push()
            ops.update(*push)
        delta, values = ops.read(0 if push is None else 2 * push[1] + 1)
        if on_check is not None:
            on_check(check, delta)
        if delta < theta:
            converged = True
            break
        if not full:
            continue
        slot, k_used, first = push
        grew = delta_prev is not None and delta > kappa * delta_prev
        delta_prev = delta
        coeffs = None
        ok = not grew and all(math.isfinite(float(v)) for v in values)
        if ok and first:
            history.have_prev = True
            continue
        if ok:
            rhs = history.commit(slot, k_used, values)
            coeffs = solve([row[:k_used] for row in history.gram[:k_used]], rhs)
            ok = coeffs is not None
        if not ok:
            history.clear()
            restarts += 1
            if restarts >= MAX_RESTARTS:
                active = False
            continue
        ops.combine(coeffs, k_used)
        extrapolations += 1
    return delta, sweeps, extrapolations, restarts, converged


class _ArrayOps:
    """`evaluate` over numpy arrays: the twin's side."""

    def __init__(self, sweep_batch, V, window):
        n = len(V)
        self.sweep_batch, self.V = sweep_batch, V
        self.x, self.f_prev, self.g_prev = (np.zeros(n, dtype=np.float32) for _ in range(3))
        self.dF, self.dG = (np.zeros((window, n), dtype=np.float32) for _ in range(2))
        self.delta, self.values = float("inf"), ()

    def snapshot(self):
        self.x[...] = self.V

    def sweeps(self, n):
        self.delta = float(self.sweep_batch(self.V, n))

    def update(self, slot, k_used, first):
        with np.errstate(all="ignore"):
            self.values = dots(self.x, self.V, self.f_prev, self.g_prev, self.dF, self.dG, slot, k_used, first)

    def read(self, count):
        return self.delta, list(self.values[:count])

    def combine(self, coeffs, k_used):
        combine(self.V, self.dG, coeffs, k_used, out=self.V)


def accelerated_evaluation(sweep_batch, V, theta: float, max_iter: int, settings: Anderson | None, interval: int = 25):
    """The loop of `evaluate` over a callable: ``sweep_batch(V, n)`` does n sweeps on the float32 array V in place (memory
    order) and returns the residual of the last one.  Returns (V, sweeps, extrapolations, restarts)."""
    V = np.ascontiguousarray(V, dtype=np.float32)
    ops = _ArrayOps(sweep_batch, V, settings.window if settings is not None else 1)
    _, sweeps, extrapolations, restarts, _ = evaluate(ops, theta, max_iter, settings, interval)
    return V, sweeps, extrapolations, restarts
