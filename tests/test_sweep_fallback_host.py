"""The sweep unit's two instantiations of the plugin (csrc/pi_compile.cpp build_source, csrc/pi_sweep_kernels.hip "common
paths first") on a host-only handle: what the generated text holds, the register budgets of the 80^4 kernels in the
production memory order, and the plugins that keep the old single-instantiation form."""
from __future__ import annotations

import numpy as np
import pytest

import __graft_entry__ as G
from dynamicprogramming_amd import _native, envs
from tests import helpers as H

NAME = "double_pendulum_swingup"


def _engine_80(order="production"):
    cls = envs.ENVS[NAME]
    tables = [np.asarray(b, dtype=np.float32) for b in cls.bins_space(80).values()]
    if order == "production":
        order = cls.MEMORY_ORDER
    assert order is None or tuple(order) == (0, 2, 1, 3)
    return _native.Engine(cls._D, [len(t) for t in tables], [t.min() for t in tables], [t.max() for t in tables], tables,
                          np.asarray(cls.ACTIONS, dtype=np.float32), device=-1, order=order)


@pytest.fixture(scope="module")
def usage_80(tmp_path_factory):
    eng = _engine_80()
    usage = H.kernel_resource_usage(eng.kernel_source(envs.dynamics_source(NAME)), tmp_path_factory.mktemp("unit80"))
    eng.close()
    return usage


def test_evaluation_register_budget_at_80_4_in_the_production_order(usage_80):
    """<= 64 VGPRs and <= 80 SGPRs (eight waves, two 1 024-thread workgroups per CU), no private segment."""
    ev = usage_80["pi_eval_sweep_kernel"]
    print(ev)
    assert ev["vgpr"] <= 64 and ev["sgpr"] <= 80 and ev["scratch"] == 0, ev


def test_improvement_register_budget_at_80_4_in_the_production_order(usage_80):
    """<= 80 VGPRs (six waves per SIMD; the parent needed 86), no private segment."""
    im = usage_80["pi_improve_sweep_kernel"]
    print(im)
    assert im["scratch"] == 0, im
    assert im["vgpr"] <= 80, im


def test_the_unit_holds_both_instantiations():
    dyn = envs.dynamics_source(NAME)
    eng = _engine_80()
    text = eng.kernel_source(dyn)
    eng.close()
    head, rest = text.split("// ---- env plugin", 1)
    assert "#define PI_FAST_FIRST 1\n" in head
    assert text.count(dyn) == 2                                          # byte-identical copies of the caller's string
    first = text.index(dyn)
    second = text.index(dyn, first + 1)
    assert text.rfind("#define sinf pi_sinf\n", 0, first) > 0            # the exact instantiation, as ever
    between = text[first + len(dyn):second]
    assert "struct PiCommonEnv {" in between and "#define sinf pi_common_sinf\n" in between
    for fn in ("pi_sinf_common", "pi_cosf_common", "pi_fmodf_common"):
        assert fn + "(x" in between
    after = text[second + len(dyn):]
    assert after.lstrip().startswith("};") and "#define sinf pi_sinf\n" in after.split("// ---- sweep kernels", 1)[0]
    assert "pi_dynamics_common" in after and "PiCommonEnv env;" in after


def test_six_d_units_keep_the_single_instantiation():
    eng, dyn = G._engine_for("double_cartpole", 5)
    text = eng.kernel_source(dyn)
    eng.close()
    assert text.count(dyn) == 1 and "PI_FAST_FIRST 1" not in text and "struct PiCommonEnv {" not in text


CONSTANT_TABLE_PLUGIN = r'''
__constant__ float my_gain[2] = {0.25f, 0.75f};
__device__ void step_dynamics(float pos, float vel, float action, float* next_pos, float* next_vel,
                              float* reward, bool* terminated) {
    vel = fmaxf(-1.0f, fminf(1.0f, vel + 0.05f * action * my_gain[1] - my_gain[0] * sinf(pos)));
    pos = pos + 0.05f * vel;
    *next_pos = pos; *next_vel = vel;
    *reward = -fabsf(pos);
    *terminated = (pos > 2.0f) || (pos < -2.0f);
}
'''


def test_a_plugin_with_file_scope_constant_data_compiles_on_the_old_path(tmp_path):
    bins = [np.linspace(-2, 2, 21, dtype=np.float32), np.linspace(-1, 1, 11, dtype=np.float32)]
    eng = _native.Engine(2, [21, 11], [-2, -1], [2, 1], bins, [-1.0, 0.0, 1.0], device=-1)
    eng.compile(CONSTANT_TABLE_PLUGIN, cache_dir=tmp_path)
    assert "without the common-path-first instantiation" in eng.compile_log
    text = eng.kernel_source(CONSTANT_TABLE_PLUGIN)
    assert text.count(CONSTANT_TABLE_PLUGIN) == 1 and "PI_FAST_FIRST 1" not in text
    objs = list(tmp_path.glob("pi_*.hsaco"))
    assert len(objs) == 1 and objs[0].read_bytes()[:4] == b"\x7fELF"
    eng.close()
    # a plugin that fits the struct form says nothing
    eng = _native.Engine(2, [21, 11], [-2, -1], [2, 1], bins, [-1.0, 0.0, 1.0], device=-1)
    eng.compile(CONSTANT_TABLE_PLUGIN.replace("__constant__ float my_gain[2] = {0.25f, 0.75f};",
                                              "#define my_gain_0 0.25f\n").replace("my_gain[1]", "0.75f").replace("my_gain[0]", "my_gain_0"),
                cache_dir=tmp_path)
    assert "common-path-first" not in eng.compile_log
    eng.close()
