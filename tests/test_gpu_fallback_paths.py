"""The sweeps' exact pass on the GPU (csrc/pi_sweep_kernels.hip, "common paths first"): synthetic plugins whose sinf /
cosf / fmodf calls leave their common path on SOME lanes of a wave and for SOME actions only, against the oracle built
from the same string, bit for bit (a NaN matches any NaN; only the grid's top corner, where one term is Inf, makes one).
Ranges are no multiple of the block size; every grid has more than one block.  The 6-D grid runs the single-instantiation
form (pi_compile.cpp build_source) and is compared all the same.  The nine shipped envs go through the small-grid parity
helpers of tests/test_gpu_edges.py once more."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from dynamicprogramming_amd import _native, envs
from tests import helpers as H

pytestmark = pytest.mark.gpu

GRIDS = [(24, 17), (9, 7, 11, 5), (5, 4, 6, 4, 5, 4)]
ACTIONS = np.array([-2.0, -0.5, 0.0, 1.0, 2.0], dtype=np.float32)
GAMMA = 0.97
POS_HI, VEL_HI = 0.5, 0.6


def _plugin(D):
    names = ["pos", "vel"] + [f"x{k}" for k in range(2, D)]
    args = ", ".join(f"float {n}" for n in names)
    outs = ", ".join(f"float* n_{n}" for n in names)
    rest = "\n".join(f"    *n_{n} = 0.9f * {n} + 0.01f * w;" for n in names[2:])
    return f'''
__device__ float syn_wrap(float v) {{ return fmodf(v, 1.5f); }}
__device__ void step_dynamics({args}, float action, {outs}, float* reward, bool* terminated) {{
    float s = sinf(pos * 3.0e5f);                      /* rare where |pos| > 1/3 */
    float c = cosf(vel * 1.0e5f * action);             /* rare for the big actions at |vel| > 1/2 */
    float w = syn_wrap(pos * 50.0f);                   /* general fmodf where |pos| >= 0.06, through a helper */
    float u = 1.0f / (({POS_HI}f - pos) + ({VEL_HI}f - vel));   /* Inf at the top corner of (pos, vel) */
    float z = sinf(u);                                 /* NaN there */
    *n_pos = pos + 0.05f * vel + 0.02f * s;
    *n_vel = vel + 0.02f * action * c + 0.01f * w;
{rest}
    *reward = -(pos * pos) + 0.1f * c + 0.001f * z;
    *terminated = false;
}}
'''


def _bins(shape):
    # pos: most points inside |pos| < 0.06 (every call on its common path), the others out to +-0.5; vel: uniform
    g0 = shape[0]
    inner = int(np.ceil(0.65 * g0))
    k = (g0 - inner + 1) // 2
    hi_part = np.linspace(POS_HI, 0.2, k)[::-1]
    lo_part = np.linspace(-POS_HI, -0.2, g0 - inner - k)
    pos = np.concatenate([lo_part, np.linspace(-0.05, 0.05, inner), hi_part]).astype(np.float32)
    assert len(pos) == g0 and np.all(np.diff(pos) > 0) and pos[-1] == np.float32(POS_HI)
    bins = [pos, np.linspace(-VEL_HI, VEL_HI, shape[1]).astype(np.float32)]
    bins += [np.linspace(-1.0, 1.0, g).astype(np.float32) for g in shape[2:]]
    return bins


def _flagged(states):
    """Per state: would any call of the plugin, for any action, leave its common path?  The full functions' own
    predicates on the float32 arguments the plugin forms."""
    f = np.float32
    pos, vel = states[:, 0].astype(f), states[:, 1].astype(f)
    with np.errstate(all="ignore"):
        sin_rare = ~(np.abs(pos * f(3.0e5)) <= f(1.0e5))
        cos_rare = np.zeros(len(pos), bool)
        for a in ACTIONS:
            cos_rare |= ~(np.abs((vel * f(1.0e5)) * f(a)) <= f(1.0e5))
        fmod_rare = ~(np.abs(pos * f(50.0)) < f(2.0) * f(1.5))
        u = f(1.0) / ((f(POS_HI) - pos) + (f(VEL_HI) - vel))
        z_rare = ~(np.abs(u) <= f(1.0e5))
    return sin_rare | cos_rare | fmod_rare | z_rare, cos_rare & ~(sin_rare | fmod_rare | z_rare)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == np.float32:
        ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    else:
        ok = a == b
    bad = np.flatnonzero(~ok)
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} vs {b.ravel()[bad[:5]]}"


class _Syn:
    def __init__(self, shape, dev):
        import torch
        self.torch, self.dev = torch, dev
        D = len(shape)
        self.src = _plugin(D)
        self.bins = _bins(shape)
        self.eng = _native.Engine(D, list(shape), [b.min() for b in self.bins], [b.max() for b in self.bins], self.bins,
                                  ACTIONS, device=dev.index or 0)
        self.eng.compile(self.src)
        self.chk = oracle.build(D, self.src)
        self.meta = oracle.grid_metadata(self.bins)
        self.states = oracle.states_from_bins(self.bins)
        self.n = len(self.states)
        rng = np.random.default_rng(7 + D)
        self.V = (rng.standard_normal(self.n) * 3.0).astype(np.float32)
        self.pol = rng.integers(0, len(ACTIONS), size=self.n).astype(np.int32)
        self.rng = rng

    def dev_arr(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)


@pytest.fixture(scope="module", params=GRIDS, ids=lambda s: "x".join(map(str, s)))
def syn(request):
    import torch
    c = _Syn(request.param, torch.device("cuda:0"))
    yield c
    c.eng.close()


def test_the_plugins_take_rare_paths_on_some_lanes_and_some_actions(syn):
    flag, cos_only = _flagged(syn.states)
    share = flag.mean()
    print(f"flagged share {share:.3f}, by the big actions alone {cos_only.mean():.3f}")
    assert 0.05 <= share <= 0.60
    assert cos_only.any()                                        # flagged for some actions only
    lo, hi = 3, syn.n - 5
    f = flag[lo:hi]
    waves = [f[k:k + 64] for k in range(0, len(f), 64)]          # lane = thread: 64 consecutive states of the range
    assert any(w.any() and not w.all() for w in waves)           # at least one mixed wave
    nan_rows = np.flatnonzero(np.isnan(syn.chk.eval_sweep(syn.states, ACTIONS, syn.pol, syn.V, np.zeros(syn.n, bool),
                                                          *syn.meta, GAMMA)[0]))
    top = (syn.states[:, 0] == syn.bins[0][-1]) & (syn.states[:, 1] == syn.bins[1][-1])
    assert set(nan_rows) <= set(np.flatnonzero(top))             # at most the Inf corner makes a NaN


@pytest.mark.parametrize("masked", [False, True], ids=["state-order", "live-list"])
def test_sweeps_match_the_oracle_bit_for_bit(syn, masked, monkeypatch):
    monkeypatch.setenv("PI_MI355_LIVE_MIN", "1")                  # the live list on grids this small
    torch, eng, n = syn.torch, syn.eng, syn.n
    assert n > 256 and (n - 8) % 256 != 0
    lo, hi = 3, n - 5
    term = np.zeros(n, bool)
    V = syn.V.copy()
    if masked:
        term = syn.rng.random(n) < 0.4
        V[term] = np.float32(-7.0)
    pol = syn.pol.copy()
    pol[term] = 0
    d_V, d_pol, d_term = syn.dev_arr(V), syn.dev_arr(pol), syn.dev_arr(term.astype(np.uint8))
    eng.prepare_mask(d_term.data_ptr() if masked else 0)
    if masked:
        assert eng.info(_native.Info.LIVE_STATES) == int((~term).sum())          # the live-list kernels run below
    d_delta = torch.full((1,), 123.0, dtype=torch.float32, device=syn.dev)
    d_changed = torch.full((1,), 77, dtype=torch.int32, device=syn.dev)
    oargs = (syn.states, ACTIONS)

    # evaluation sweep with and without the residual
    for with_delta in (True, False):
        d_Vn = d_V.clone()
        eng.eval_sweep(d_V.data_ptr(), d_Vn.data_ptr(), d_pol.data_ptr(), d_term.data_ptr(), lo, hi, GAMMA,
                       d_delta.data_ptr() if with_delta else 0)
        o_Vn, o_delta = syn.chk.eval_sweep(*oargs, pol, V, term, *syn.meta, GAMMA, lo, hi)
        _same(d_Vn.cpu().numpy(), o_Vn, "V' of the evaluation sweep")
        if with_delta:
            _same(np.float32(d_delta.item()), np.float32(o_delta), "its residual")
    # improvement sweep with its changed count
    d_p2 = d_pol.clone()
    eng.improve_sweep(d_V.data_ptr(), d_p2.data_ptr(), d_term.data_ptr(), lo, hi, GAMMA, d_changed.data_ptr())
    o_pol, o_changed = syn.chk.improve_sweep(*oargs, pol, V, term, *syn.meta, GAMMA, lo, hi)
    _same(d_p2.cpu().numpy(), o_pol, "improved policy")
    assert int(d_changed.item()) == o_changed and o_changed > 0

    # value sweep
    d_p3, d_Vm = d_pol.clone(), d_V.clone()
    eng.value_sweep(d_V.data_ptr(), d_Vm.data_ptr(), d_p3.data_ptr(), d_term.data_ptr(), lo, hi, GAMMA,
                    d_delta.data_ptr(), d_changed.data_ptr())
    o_Vm, o_pol3, o_delta3, o_changed3 = syn.chk.value_sweep(*oargs, pol, V, term, *syn.meta, GAMMA, lo, hi)
    _same(d_Vm.cpu().numpy(), o_Vm, "V' of the value sweep")
    _same(d_p3.cpu().numpy(), o_pol3, "policy of the value sweep")
    _same(np.float32(d_delta.item()), np.float32(o_delta3), "the value sweep's residual")
    assert int(d_changed.item()) == o_changed3
    eng.prepare_mask(0)


@pytest.mark.parametrize("name", H.ENV_NAMES)
def test_shipped_envs_on_their_small_grids(name):
    import torch
    from tests.test_gpu_edges import _Case, _single_sweeps
    shape = {2: (24, 17), 4: (9, 7, 11, 5), 6: (5, 4, 6, 4, 5, 4)}[envs.ENVS[name]._D]
    c = _Case(name, shape, None, torch.device("cuda:0"))
    try:
        _single_sweeps(c)
    finally:
        c.eng.close()
