"""The randomisation of the floating-base env and the per-world ground friction
at the C ABI, without a GPU: libmwstep.so exports mw_floatenv_randomize,
mw_set_ground_friction and mw_ground_friction, the ctypes mirror of
mw_float_rand_config has the C struct's size and field offsets (an offsetof
printer compiled against include/mwstep.h, as test_float_env_abi.py does for
the task struct), null and uninitialised handles are refused, and the Python
layer carries the new arguments."""

import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

FIELDS = ["push_interval", "push_steps", "push_force", "push_torque", "friction_lo", "friction_hi"]
SYMBOLS = ["mw_floatenv_randomize", "mw_set_ground_friction", "mw_ground_friction"]


@pytest.fixture(scope="module")
def N():
    from mwstep import native
    native.lib()
    return native


def test_library_exports_the_new_symbols(N):
    L = ctypes.CDLL(N.LIB_PATH)
    declared = {name for name, _, _ in N.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "mwstep.h")).read()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in declared, sym
        assert f"int {sym}(" in header, sym


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_rand_config, {f}));\n' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_rand_config));\n'
                   '  printf("task %zu\\n", sizeof(mw_float_task_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatRandConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatRandConfig) == int(out["sizeof"])
    for f in FIELDS:
        assert getattr(N.MwFloatRandConfig, f).offset == int(out[f]), f
    # the task struct did not grow: the randomisation has its own
    assert ctypes.sizeof(N.MwFloatTaskConfig) == int(out["task"])


def test_null_and_uninitialised_handles_are_refused(N):
    cfg = N.MwFloatRandConfig(7, 2, 30.0, 5.0, 0.3, 1.2)
    assert N.lib().mw_floatenv_randomize(None, ctypes.byref(cfg), None, None) == N.MW_EINVAL
    assert "null" in N.last_error()
    mu = (ctypes.c_double * 2)(0.5, 0.5)
    assert N.lib().mw_set_ground_friction(None, 0, 2, mu) == N.MW_ESTATE
    assert N.lib().mw_ground_friction(None, 0, 2, mu) == N.MW_ESTATE
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, 2, 0, 0)
    N.check(N.lib().mw_create(ctypes.byref(mc), ctypes.byref(sim)))
    try:
        # no model, never initialized: refused before any device work
        assert N.lib().mw_set_ground_friction(sim, 0, 2, mu) == N.MW_ESTATE
        assert N.lib().mw_ground_friction(sim, 0, 2, mu) == N.MW_ESTATE
    finally:
        N.lib().mw_destroy(sim)


def test_python_layer_carries_the_arguments():
    from mwstep import FloatVecEnv
    from mwstep.sim import Simulator
    params = inspect.signature(FloatVecEnv.__init__).parameters
    defaults = {"push_interval": 0, "push_steps": 1, "push_force": 0.0, "push_torque": 0.0, "friction_range": None}
    for name, value in defaults.items():
        assert name in params and params[name].default == value, name
    for name in ("set_ground_friction", "ground_friction"):
        assert callable(getattr(Simulator, name))
