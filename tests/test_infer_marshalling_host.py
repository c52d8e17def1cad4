"""
What InferenceEngine hands to the C ABI, argument by argument (include/pi_mi355.h "Inference"): the library is replaced by
a recorder, every method is called with a distinct sentinel per parameter, and the positional tuple the C function
received is written out here.  Needs neither a GPU nor libpi_mi355.so.

The arguments travel as ``void*`` / ``float`` / ``int`` by position: a slip there is silent until a GPU test compares
bits.  This file is where it shows first.
"""
import ctypes

import numpy as np
import pytest

from dynamicprogramming_amd import _native

H, P = 0x1000, 0x2000                           # the handles the recorder gives the first and the second engine
LOG_BYTES = 1 << 16
SEED, FIRST = 2 ** 64 - 3, 2 ** 40 + 1          # past 32 and 63 bits: they travel as uint64
# the calls that take (..., char* log, size_t log_len) last
LOGGED = ("pi_infer_set_dynamics", "pi_infer_set_partner", "pi_infer_set_partner_stochastic", "pi_infer_set_values",
          "pi_infer_set_greedy", "pi_infer_set_stochastic", "pi_infer_set_expect_greedy")


class Recorder:
    """Stands in for the loaded library: every pi_* attribute stores its arguments and returns `rc`."""

    def __init__(self):
        self.calls = []
        self.rc = 0
        self._handles = iter((H, P))

    def __getattr__(self, name):
        if not name.startswith("pi_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == "pi_infer_create":
                return next(self._handles)
            if name == "pi_last_error":
                return b"boom"
            if name == "pi_infer_destroy":
                return None
            if name in LOGGED:
                args[-2].value = b"log of " + name.encode()
            return self.rc
        return call

    def last(self, name):
        """The arguments of the one call made since the last look, which must be `name`."""
        made = [c for c in self.calls if c[0] != "pi_last_error"]
        self.calls = []
        assert [c[0] for c in made] == [name]
        return made[0][1]


class Ptr:
    """An expected host pointer: the ctypes pointer type the ABI declares, and the values it points at."""

    def __init__(self, ctype, *values):
        self.type, self.values = ctypes.POINTER(ctype), list(values)

    def matches(self, got):
        return isinstance(got, self.type) and got[:len(self.values)] == self.values

    def __repr__(self):
        return f"Ptr({self.type.__name__}, {self.values})"


def f32(*values):
    return Ptr(ctypes.c_float, *values)


def i32(*values):
    return Ptr(ctypes.c_int32, *values)


def i64(*values):
    return Ptr(ctypes.c_int64, *values)


class Log:
    """The expected log buffer: a writable char array of LOG_BYTES bytes."""

    @staticmethod
    def matches(got):
        return isinstance(got, ctypes.Array) and got._type_ is ctypes.c_char and len(got) == LOG_BYTES


LOG = Log()


def same(got, want):
    """The received tuple is exactly the expected one: same length, None where None is expected (never a 0), pointers by
    type and by the values behind them, everything else by value and by Python type."""
    assert len(got) == len(want), (got, want)
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, (Ptr, Log)):
            assert w.matches(g), f"argument {k}: {g!r} is not {w!r}"
        elif w is None:
            assert g is None, f"argument {k}: {g!r} is not None"
        else:
            assert type(g) is type(w) and g == w, f"argument {k}: {g!r} is not {w!r}"


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(_native, "lib", lambda: r)
    return r


def _engine():
    return _native.InferenceEngine([-1.0, -2.0], [1.0, 2.0], [3, 4], [4, 1], [[0, 0], [0, 1], [1, 0], [1, 1]],
                                   cache_dir=None)


@pytest.fixture
def eng(rec):
    e = _engine()
    assert rec.last("pi_infer_create")[0] == -1
    yield e
    e.close()                                   # while the recorder is still in place: the handle is not a real one


@pytest.fixture
def partner(rec, eng):
    p = _engine()
    rec.last("pi_infer_create")
    yield p
    p.close()


def test_create_and_destroy(rec, tmp_path):
    e = _native.InferenceEngine([-1.0, -2.0], [1.0, 2.0], [3, 4], [4, 1], [[0, 0], [0, 1], [1, 0], [1, 1]], device=3,
                                cache_dir=tmp_path / "cache")
    same(rec.last("pi_infer_create"), (3, 2, f32(-1.0, -2.0), f32(1.0, 2.0), i32(3, 4), i32(4, 1),
                                       i32(0, 0, 0, 1, 1, 0, 1, 1), 4, str(tmp_path / "cache").encode()))
    assert (tmp_path / "cache").is_dir() and (e.D, e.n_corners, e.device) == (2, 4, 3)
    e.close()
    same(rec.last("pi_infer_destroy"), (H,))
    e.close()                                   # closed once
    assert rec.calls == []
    rec._handles = iter((0,))
    with pytest.raises(_native.NativeError, match=r"^pi_infer_create failed: boom$"):
        _engine()
    same(rec.last("pi_infer_create"), (-1, 2, f32(-1.0, -2.0), f32(1.0, 2.0), i32(3, 4), i32(4, 1),
                                       i32(0, 0, 0, 1, 1, 0, 1, 1), 4, None))


def test_set_policy_and_query(rec, eng):
    eng.set_policy([2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1], [-0.5, 0.25, 0.75])
    same(rec.last("pi_infer_set_policy"), (H, i32(2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1), 12, f32(-0.5, 0.25, 0.75), 3))
    eng.query(11, 5, 41, 42, 43, 99)
    same(rec.last("pi_infer_query"), (H, 11, 5, 41, 42, 43, 99))
    eng.query(11, 5)
    same(rec.last("pi_infer_query"), (H, 11, 5, None, None, None, None))
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_set_policy failed: boom$"):
        eng.set_policy([0], [0.0])
    with pytest.raises(_native.NativeError, match=r"^pi_infer_query failed: boom$"):
        eng.query(11, 5)


TABLE = [-0.5, 0.25, 0.75]
# method -> (its arguments, what follows the handle up to the log, the prefix of its NativeError)
SETTERS = {
    "set_dynamics": (("float step;",), (b"float step;",), "rollout kernel compilation failed:"),
    "set_values": ((np.arange(12.0).reshape(3, 4),), (f32(*range(12)), 12), "pi_infer_set_values failed:"),
    "set_greedy": ((TABLE,), (f32(*TABLE), 3), "pi_infer_set_greedy failed:"),
    "set_stochastic": ((TABLE,), (f32(*TABLE), 3), "pi_infer_set_stochastic failed:"),
    "set_expect_greedy": ((TABLE,), (f32(*TABLE), 3), "pi_infer_set_expect_greedy failed:"),
}
C_NAME = {"set_dynamics": "pi_infer_set_dynamics", "set_values": "pi_infer_set_values", "set_greedy": "pi_infer_set_greedy",
          "set_stochastic": "pi_infer_set_stochastic", "set_expect_greedy": "pi_infer_set_expect_greedy"}


@pytest.mark.parametrize("method", sorted(SETTERS))
def test_setters(rec, eng, method):
    args, middle, prefix = SETTERS[method]
    name = C_NAME[method]
    assert getattr(eng, method)(*args) == "log of " + name
    same(rec.last(name), (H,) + middle + (LOG, LOG_BYTES))
    if method != "set_dynamics" and method != "set_values":          # a missing table travels as (NULL, 0): the library refuses
        assert getattr(eng, method)(None) == "log of " + name
        same(rec.last(name), (H, None, 0, LOG, LOG_BYTES))
        getattr(eng, method)([[-0.5, 0.25], [0.75, 1.0]])            # any shape: flattened
        same(rec.last(name), (H, f32(-0.5, 0.25, 0.75, 1.0), 4, LOG, LOG_BYTES))
    rec.rc = 1
    with pytest.raises(_native.NativeError) as err:
        getattr(eng, method)(*args)
    assert str(err.value) == prefix + "\nboom"


def test_partner_setters(rec, eng, partner):
    assert eng.set_partner(partner) == "log of pi_infer_set_partner"
    same(rec.last("pi_infer_set_partner"), (H, P, LOG, LOG_BYTES))
    assert eng.set_partner_stochastic(partner, TABLE) == "log of pi_infer_set_partner_stochastic"
    same(rec.last("pi_infer_set_partner_stochastic"), (H, P, f32(*TABLE), 3, LOG, LOG_BYTES))
    assert eng.set_partner_stochastic(None, None) == "log of pi_infer_set_partner_stochastic"
    same(rec.last("pi_infer_set_partner_stochastic"), (H, None, None, 0, LOG, LOG_BYTES))
    rec.rc = 1
    with pytest.raises(_native.NativeError) as err:
        eng.set_partner(partner)
    assert str(err.value) == "hybrid rollout kernel compilation failed:\nboom"
    with pytest.raises(_native.NativeError) as err:
        eng.set_partner_stochastic(partner, TABLE)
    assert str(err.value) == "pi_infer_set_partner_stochastic failed:\nboom"


def test_rollout(rec, eng):
    eng.rollout(11, 5, 7, 0.5, 21, 22, 23, 24, 25, 3, 99)
    same(rec.last("pi_infer_rollout"), (H, 11, 5, 7, 0.5, 21, 22, 23, 24, 25, 3, 99))
    eng.rollout(0, 5, 7)
    same(rec.last("pi_infer_rollout"), (H, None, 5, 7, 1.0, None, None, None, None, None, 0, None))
    eng.rollout(np.int64(11), np.int32(5), np.int64(7), np.float32(0.5), traj_every=np.int64(3))     # plain C scalars
    same(rec.last("pi_infer_rollout"), (H, np.int64(11), 5, 7, 0.5, None, None, None, None, None, 3, None))
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_rollout failed: boom$"):
        eng.rollout(11, 5, 7)


def test_rollout_greedy(rec, eng):
    eng.rollout_greedy(11, 5, 7, 0.875, 0.5, 21, 22, 23, 24, 25, 3, 99)
    same(rec.last("pi_infer_rollout_greedy"), (H, 11, 5, 7, 0.5, 0.875, 21, 22, 23, 24, 25, 3, 99))
    eng.rollout_greedy(0, 5, 7, 0.875)
    same(rec.last("pi_infer_rollout_greedy"), (H, None, 5, 7, 1.0, 0.875, None, None, None, None, None, 0, None))
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_rollout_greedy failed: boom$"):
        eng.rollout_greedy(11, 5, 7, 0.875)


def test_rollout_stochastic(rec, eng):
    eng.rollout_stochastic(11, 5, 7, 0.5, 0.125, 0.375, [0.0625, 0.03125], SEED, FIRST, 21, 22, 23, 24, 25, 3, 99)
    same(rec.last("pi_infer_rollout_stochastic"), (H, 11, 5, 7, 0.5, 0.125, 0.375, f32(0.0625, 0.03125), SEED, FIRST,
                                                   21, 22, 23, 24, 25, 3, 99))
    eng.rollout_stochastic(0, 5, 7)
    same(rec.last("pi_infer_rollout_stochastic"), (H, None, 5, 7, 1.0, 0.0, 0.0, None, 0, 0,
                                                   None, None, None, None, None, 0, None))
    for bad in ([0.1, 0.1, 0.1], 0.1, [[0.1, 0.1]]):
        with pytest.raises(ValueError, match=r"^state_noise must hold 2 values$"):
            eng.rollout_stochastic(11, 5, 7, state_noise=bad)
    assert rec.calls == []                                           # refused before the library was asked
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_rollout_stochastic failed: boom$"):
        eng.rollout_stochastic(11, 5, 7)


def test_rollout_expect_greedy(rec, eng):
    eng.rollout_expect_greedy(11, 5, 7, 0.875, 0.5, 0.125, 0.375, [0.0625, 0.03125], SEED, FIRST, 21, 22, 23, 24, 25, 3, 99)
    same(rec.last("pi_infer_rollout_expect_greedy"), (H, 11, 5, 7, 0.5, 0.875, 0.125, 0.375, f32(0.0625, 0.03125), SEED,
                                                      FIRST, 21, 22, 23, 24, 25, 3, 99))
    eng.rollout_expect_greedy(0, 5, 7, 0.875)
    same(rec.last("pi_infer_rollout_expect_greedy"), (H, None, 5, 7, 1.0, 0.875, 0.0, 0.0, None, 0, 0,
                                                      None, None, None, None, None, 0, None))
    with pytest.raises(ValueError, match=r"^state_noise must hold 2 values$"):
        eng.rollout_expect_greedy(11, 5, 7, 0.875, state_noise=[0.1])
    assert rec.calls == []
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_rollout_expect_greedy failed: boom$"):
        eng.rollout_expect_greedy(11, 5, 7, 0.875)


def test_rollout_hybrid(rec, eng, partner):
    eng.rollout_hybrid(partner, 11, 5, 7, [0.25, 0.5], [0.75, 1.5], 0.5, 21, 22, 23, 24, 26, 27, 25, 3, 99)
    same(rec.last("pi_infer_rollout_hybrid"), (H, P, 11, 5, 7, 0.5, f32(0.25, 0.5), f32(0.75, 1.5), 21, 22, 23, 24, 26, 27,
                                               25, 3, 99))
    eng.rollout_hybrid(None, 0, 5, 7, None, None)
    same(rec.last("pi_infer_rollout_hybrid"), (H, None, None, 5, 7, 1.0, None, None, None, None, None, None, None, None,
                                               None, 0, None))
    for enter, leave in (([0.25], [0.75, 1.5]), ([0.25, 0.5], [0.75, 1.5, 2.0]), (None, 0.75), ([[0.25, 0.5]], None)):
        with pytest.raises(ValueError, match=r"^enter and leave must hold 2 thresholds each$"):
            eng.rollout_hybrid(partner, 11, 5, 7, enter, leave)
    assert rec.calls == []
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_rollout_hybrid failed: boom$"):
        eng.rollout_hybrid(partner, 11, 5, 7, None, None)


def test_rollout_hybrid_stochastic(rec, eng, partner):
    eng.rollout_hybrid_stochastic(partner, 11, 5, 7, [0.25, 0.5], [0.75, 1.5], 0.5, 0.125, 0.375, [0.0625, 0.03125], SEED,
                                  FIRST, 21, 22, 23, 24, 26, 27, 28, 25, 3, 99)
    same(rec.last("pi_infer_rollout_hybrid_stochastic"),
         (H, P, 11, 5, 7, 0.5, f32(0.25, 0.5), f32(0.75, 1.5), 0.125, 0.375, f32(0.0625, 0.03125), SEED, FIRST,
          21, 22, 23, 24, 26, 27, 28, 25, 3, 99))
    eng.rollout_hybrid_stochastic(None, 0, 5, 7, None, None)
    same(rec.last("pi_infer_rollout_hybrid_stochastic"),
         (H, None, None, 5, 7, 1.0, None, None, 0.0, 0.0, None, 0, 0,
          None, None, None, None, None, None, None, None, 0, None))
    with pytest.raises(ValueError, match=r"^enter and leave must hold 2 thresholds each$"):
        eng.rollout_hybrid_stochastic(partner, 11, 5, 7, [0.25, 0.5], [0.75])
    with pytest.raises(ValueError, match=r"^state_noise must hold 2 values$"):
        eng.rollout_hybrid_stochastic(partner, 11, 5, 7, [0.25, 0.5], [0.75, 1.5], state_noise=[0.1, 0.1, 0.1])
    with pytest.raises(ValueError, match=r"^enter and leave must hold 2 thresholds each$"):     # the thresholds are looked at first
        eng.rollout_hybrid_stochastic(partner, 11, 5, 7, [0.25], [0.75, 1.5], state_noise=[0.1, 0.1, 0.1])
    assert rec.calls == []
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_rollout_hybrid_stochastic failed: boom$"):
        eng.rollout_hybrid_stochastic(partner, 11, 5, 7, None, None)


@pytest.mark.parametrize("method, name", [("greedy", "pi_infer_greedy"), ("expect_greedy", "pi_infer_expect_greedy")])
def test_lookahead_queries(rec, eng, method, name):
    getattr(eng, method)(11, 5, 0.875, 31, 32, 33, 34, 99)
    same(rec.last(name), (H, 11, 5, 0.875, 31, 32, 33, 34, 99))
    getattr(eng, method)(0, 5, 0.875)
    same(rec.last(name), (H, None, 5, 0.875, None, None, None, None, None))
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=rf"^{name} failed: boom$"):
        getattr(eng, method)(11, 5, 0.875)


def test_random_words(rec, eng):
    eng.random_words(SEED, FIRST, 5, 6, 2, 51, 99)
    same(rec.last("pi_infer_random_words"), (H, SEED, FIRST, 5, 6, 2, 51, 99))
    eng.random_words(1, 0, 5, 0, 0, 0)
    same(rec.last("pi_infer_random_words"), (H, 1, 0, 5, 0, 0, None, None))
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_random_words failed: boom$"):
        eng.random_words(1, 0, 5, 0, 0, 51)


def test_set_disturbances(rec, eng):
    assert eng.set_disturbances([0.5, -0.5, 0.0], [[0.125, 0.25], [0.375, 0.625], [0.0, 0.0]], [0.25, 0.25, 0.5]) == 3
    same(rec.last("pi_infer_set_disturbances"), (H, 3, f32(0.5, -0.5, 0.0), f32(0.125, 0.25, 0.375, 0.625, 0.0, 0.0),
                                                 f32(0.25, 0.25, 0.5)))
    assert eng.set_disturbances(None, None, [1.0]) == 1
    same(rec.last("pi_infer_set_disturbances"), (H, 1, None, None, f32(1.0)))
    assert eng.set_disturbances([0.5], [[0.125, 0.25]], None) == 0               # no weights: the set is dropped
    same(rec.last("pi_infer_set_disturbances"), (H, 0, None, None, None))
    for da, dx, w in (([0.5], None, [0.5, 0.5]), (None, [[0.125, 0.25, 0.5]], [1.0]), (None, None, [])):
        with pytest.raises(ValueError, match=r"^a disturbance set needs K >= 1 weights, K action offsets and \(K, 2\) state "
                                             r"offsets$"):
            eng.set_disturbances(da, dx, w)
    assert rec.calls == []
    rec.rc = 1
    for w in (None, [1.0]):
        with pytest.raises(_native.NativeError, match=r"^pi_infer_set_disturbances failed: boom$"):
            eng.set_disturbances(None, None, w)


def test_resample(rec, eng):
    bins = [[-1.0, 0.0, 1.0], [-2.0, 2.0]]
    eng.resample([3, 2], [2, 1], bins, 61, 62, 63, [1, 0, 3], 4, 99)
    same(rec.last("pi_infer_resample"), (H, i32(3, 2), i64(2, 1), f32(-1.0, 0.0, 1.0, -2.0, 2.0), i32(1, 0, 3), 4, 61, 62, 63,
                                         99))
    eng.resample([3, 2], [2 ** 33, 1], bins)                                     # strides are 64-bit
    same(rec.last("pi_infer_resample"), (H, i32(3, 2), i64(2 ** 33, 1), f32(-1.0, 0.0, 1.0, -2.0, 2.0), None, 0, None, None,
                                         None, None))
    shape_rule = r"^the destination needs 2 dimensions: a shape, a stride and a bin table of that length each$"
    for shape, strides, tables in (([3], [2, 1], bins), ([3, 2], [1], bins), ([3, 3], [2, 1], bins), ([3, 2], [2, 1], bins[:1])):
        with pytest.raises(ValueError, match=shape_rule):
            eng.resample(shape, strides, tables)
    for amap in ([1, 4, 0], [-1, 0, 0], [[1, 0, 3]]):
        with pytest.raises(ValueError, match=r"^action_map must hold indices into the destination's 4 actions$"):
            eng.resample([3, 2], [2, 1], bins, action_map=amap, n_actions=4)
    eng.set_policy([0] * 12, TABLE)                                              # from here on the source has 3 actions
    rec.last("pi_infer_set_policy")
    with pytest.raises(ValueError, match=r"^action_map needs one entry per source action \(3\)$"):
        eng.resample([3, 2], [2, 1], bins, action_map=[1, 0], n_actions=4)
    assert rec.calls == []
    rec.rc = 1
    with pytest.raises(_native.NativeError, match=r"^pi_infer_resample failed: boom$"):
        eng.resample([3, 2], [2, 1], bins)
