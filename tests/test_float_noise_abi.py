"""Observation noise and action latency of the floating-base env at the C ABI,
without a GPU: libmwstep.so exports mw_floatenv_noise, the ctypes mirror of
mw_float_noise_config has the C struct's size and field offsets (an offsetof
printer compiled against include/mwstep.h, as test_float_loco_abi.py does), the
task, rand, loco, inertia and joint structs keep their sizes, null arguments
are refused, and the Python layer carries the new arguments."""

import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

FIELDS = ["delay_lo", "delay_hi"]
OTHERS = {"mw_float_task_config": "MwFloatTaskConfig", "mw_float_rand_config": "MwFloatRandConfig",
          "mw_float_loco_config": "MwFloatLocoConfig", "mw_float_inertia_config": "MwFloatInertiaConfig",
          "mw_float_joint_config": "MwFloatJointConfig"}
# sizes of the five structs before this feature (LP64)
SIZES_BEFORE = {"mw_float_task_config": 104, "mw_float_rand_config": 24, "mw_float_loco_config": 76,
                "mw_float_inertia_config": 28, "mw_float_joint_config": 32}


@pytest.fixture(scope="module")
def N():
    from mwstep import native
    native.lib()
    return native


def test_library_exports_the_symbol(N):
    L = ctypes.CDLL(N.LIB_PATH)
    declared = {name: args for name, _, args in N.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "mwstep.h")).read()
    assert hasattr(L, "mw_floatenv_noise")
    assert len(declared["mw_floatenv_noise"]) == 6
    assert "int mw_floatenv_noise(" in header
    assert "#define MW_FLOAT_MAX_ACTION_DELAY 8" in header and N.FLOAT_MAX_ACTION_DELAY == 8


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_noise_config, {f}));\n' for f in FIELDS)
    prints += "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in OTHERS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_noise_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatNoiseConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatNoiseConfig) == int(out["sizeof"]) == 8
    for f in FIELDS:
        assert getattr(N.MwFloatNoiseConfig, f).offset == int(out[f]), f
    # no existing struct grew: the feature has its own
    for c_name, py_name in OTHERS.items():
        assert ctypes.sizeof(getattr(N, py_name)) == int(out[c_name]) == SIZES_BEFORE[c_name], c_name


def test_null_arguments_are_refused(N):
    cfg = N.MwFloatNoiseConfig(0, 2)
    amp = (ctypes.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    assert N.lib().mw_floatenv_noise(None, ctypes.byref(cfg), amp, None, None, None) == N.MW_EINVAL
    assert "null" in N.last_error()
    assert N.lib().mw_floatenv_noise(None, None, None, None, None, None) == N.MW_EINVAL
    assert "null" in N.last_error()


def test_python_layer_carries_the_arguments():
    from mwstep import FloatVecEnv
    params = inspect.signature(FloatVecEnv.__init__).parameters
    for name in ("obs_noise", "action_delay_range"):
        assert name in params and params[name].default is None, name
    for make in (FloatVecEnv.quadruped, FloatVecEnv.icub):
        assert "kw" in inspect.signature(make).parameters
