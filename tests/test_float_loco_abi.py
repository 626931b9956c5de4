"""The locomotion task of the floating-base env at the C ABI, without a GPU:
libmwstep.so exports mw_floatenv_locomotion, the ctypes mirror of
mw_float_loco_config has the C struct's size and field offsets (an offsetof
printer compiled against include/mwstep.h, as test_float_rand_abi.py does for
the randomisation struct), the task struct did not grow, a null handle is
refused, and the Python layer carries the new arguments."""

import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT

FIELDS = ["cmd_lo", "cmd_hi", "cmd_interval", "cmd_zero_prob", "cmd_min", "action_scale", "w_track_lin",
          "w_track_yaw", "track_sigma", "w_lin_z", "w_ang_xy", "w_action_rate", "w_air_time", "air_time_target",
          "contact_force_min"]
TASK_BYTES = 104    # sizeof(mw_float_task_config) before the locomotion task existed (LP64)


@pytest.fixture(scope="module")
def N():
    from mwstep import native
    native.lib()
    return native


def test_library_exports_the_symbol(N):
    L = ctypes.CDLL(N.LIB_PATH)
    declared = {name: args for name, _, args in N.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "mwstep.h")).read()
    assert hasattr(L, "mw_floatenv_locomotion")
    assert len(declared["mw_floatenv_locomotion"]) == 3
    assert "int mw_floatenv_locomotion(" in header


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_loco_config, {f}));\n' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_loco_config));\n'
                   '  printf("task %zu\\n", sizeof(mw_float_task_config));\n'
                   '  printf("rand %zu\\n", sizeof(mw_float_rand_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatLocoConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatLocoConfig) == int(out["sizeof"])
    for f in FIELDS:
        assert getattr(N.MwFloatLocoConfig, f).offset == int(out[f]), f
    # the task and randomisation structs did not grow: the locomotion task has its own
    assert int(out["task"]) == ctypes.sizeof(N.MwFloatTaskConfig) == TASK_BYTES
    assert int(out["rand"]) == ctypes.sizeof(N.MwFloatRandConfig) == 24


def test_null_arguments_are_refused(N):
    cfg = N.MwFloatLocoConfig()
    cfg.track_sigma = 0.25
    assert N.lib().mw_floatenv_locomotion(None, ctypes.byref(cfg), None) == N.MW_EINVAL
    assert "null" in N.last_error()


def test_python_layer_carries_the_arguments():
    from mwstep import FloatVecEnv
    params = inspect.signature(FloatVecEnv.__init__).parameters
    assert params["task"].default == "forward"
    assert len(params["command_ranges"].default) == 3
    for name in FIELDS[2:]:
        assert name in params, name
    assert params["action_scale"].default == 0.0 and params["cmd_interval"].default == 0
    assert FloatVecEnv.LOCOMOTION_DEFAULTS == dict(action_scale=0.25, track_sigma=0.25, air_time_target=0.3)
    for make in (FloatVecEnv.quadruped, FloatVecEnv.icub):
        assert "kw" in inspect.signature(make).parameters
