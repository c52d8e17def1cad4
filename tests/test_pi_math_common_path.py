"""include/pi_math.h, the common-path entry points (pi_sinf_common / pi_cosf_common / pi_fmodf_common): the flag is set
exactly where the full function leaves its first branch, and wherever it stays clear the bits are the full function's.
Reaches the header the way tests/test_pi_math.py does (gcc, ctypes)."""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

SRC = r'''
#include "pi_math.h"
void t_sin(long n, const float* x, float* y) { for (long i = 0; i < n; ++i) y[i] = pi_sinf(x[i]); }
void t_cos(long n, const float* x, float* y) { for (long i = 0; i < n; ++i) y[i] = pi_cosf(x[i]); }
void t_fmod(long n, const float* x, const float* y, float* z) { for (long i = 0; i < n; ++i) z[i] = pi_fmodf(x[i], y[i]); }
void c_sin(long n, const float* x, float* y, unsigned int* f) { for (long i = 0; i < n; ++i) { f[i] = 0u; y[i] = pi_sinf_common(x[i], &f[i]); } }
void c_cos(long n, const float* x, float* y, unsigned int* f) { for (long i = 0; i < n; ++i) { f[i] = 0u; y[i] = pi_cosf_common(x[i], &f[i]); } }
void c_fmod(long n, const float* x, const float* y, float* z, unsigned int* f) { for (long i = 0; i < n; ++i) { f[i] = 0u; z[i] = pi_fmodf_common(x[i], y[i], &f[i]); } }
/* the flag is OR-ed in, never cleared */
unsigned int c_sticky(void) { unsigned int f = 4u; (void)pi_sinf_common(1.0f, &f); (void)pi_fmodf_common(1.0f, 6.0f, &f); return f; }
'''

_F = ctypes.POINTER(ctypes.c_float)
_U = ctypes.POINTER(ctypes.c_uint)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pimath_common")
    (d / "t.c").write_text(SRC)
    subprocess.run(["gcc", "-O2", "-mfma", "-msse4.1", "-ffp-contract=off", "-shared", "-fPIC",
                    f"-I{ROOT / 'include'}", str(d / "t.c"), "-o", str(d / "t.so"), "-lm"], check=True)
    return ctypes.CDLL(str(d / "t.so"))


def _full(fn, *arrs):
    out = np.empty_like(arrs[0])
    fn(ctypes.c_long(len(out)), *[a.ctypes.data_as(_F) for a in arrs], out.ctypes.data_as(_F))
    return out


def _common(fn, *arrs):
    out = np.empty_like(arrs[0])
    flag = np.full(len(out), 7, dtype=np.uint32)
    fn(ctypes.c_long(len(out)), *[a.ctypes.data_as(_F) for a in arrs], out.ctypes.data_as(_F), flag.ctypes.data_as(_U))
    return out, flag


def _inputs() -> np.ndarray:
    """Every 4 099th float32 bit pattern plus the edges: +-0, +-1e5 and its two neighbours, 2^30, +-Inf, NaN, denormals."""
    grid = np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32)
    e5 = np.float32(1.0e5)
    edges = [0.0, -0.0, e5, -e5, np.nextafter(e5, np.float32(np.inf)), np.nextafter(e5, np.float32(0)),
             -np.nextafter(e5, np.float32(np.inf)), -np.nextafter(e5, np.float32(0)), 2.0 ** 30, -(2.0 ** 30),
             np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5e-40]
    return np.concatenate([grid, np.array(edges, dtype=np.float32)])


@pytest.mark.parametrize("name", ["sin", "cos"])
def test_trig_flag_and_bits(lib, name):
    x = _inputs()
    want = _full(getattr(lib, "t_" + name), x)
    got, flag = _common(getattr(lib, "c_" + name), x)
    with np.errstate(invalid="ignore"):
        leaves = ~(np.abs(x) <= np.float32(1.0e5))            # the full function's `if`, negated (true for NaN)
    assert set(np.unique(flag)) <= {0, 1}
    assert np.array_equal(flag != 0, leaves)
    assert leaves.sum() > 1000 and (~leaves).sum() > 1000
    keep = ~leaves
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32))


@pytest.mark.parametrize("y", [2.0 * np.pi, 1.5, 2.0 ** -130, 3e38, 0.0, np.inf])
def test_fmod_flag_and_bits(lib, y):
    x = _inputs()
    yy = np.full_like(x, np.float32(y))
    want = _full(lib.t_fmod, x, yy)
    got, flag = _common(lib.c_fmod, x, yy)
    ay = np.abs(yy).view(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        first = ((ay - np.uint32(0x00800000)) < np.uint32(0x7E800000)) & (np.abs(x) < np.float32(2.0) * np.abs(yy))
    assert set(np.unique(flag)) <= {0, 1}
    assert np.array_equal(flag == 0, first)
    assert np.array_equal(got[first].view(np.uint32), want[first].view(np.uint32))
    if y in (0.0, np.inf, 3e38) or y == 2.0 ** -130:
        assert not first.any()                # zero, Inf, denormal and >= 2^127 divisors never take the first branch
    else:
        assert first.sum() > 1000 and (~first).sum() > 1000


def test_flag_is_sticky(lib):
    lib.c_sticky.restype = ctypes.c_uint
    assert lib.c_sticky() == 4
