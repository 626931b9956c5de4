"""The floating-base env's C ABI without a GPU: libmwstep.so exports
mw_floatenv_create, the ctypes mirror of mw_float_task_config has the C
struct's size and field offsets (a three-line C file compiled against
include/mwstep.h), null arguments are refused, and the Python class is
exported."""

import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

FIELDS = ["action_mode", "max_episode_steps", "world_offset", "n_contact_links", "seed", "z_min", "cos_tilt_max",
          "alive_bonus", "w_forward", "w_action", "w_pose", "joint_noise", "pad_", "home_base", "home_q",
          "contact_links"]


@pytest.fixture(scope="module")
def N():
    from mwstep import native
    native.lib()
    return native


def test_library_exports_floatenv_create(N):
    L = ctypes.CDLL(N.LIB_PATH)
    assert hasattr(L, "mw_floatenv_create")
    assert "mw_floatenv_create" in {name for name, _, _ in N.SIGNATURES}
    assert (N.FLOAT_ACTION_TORQUE, N.FLOAT_ACTION_POSITION) == (0, 1)


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_task_config, {f}));\n' for f in FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_task_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatTaskConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatTaskConfig) == int(out["sizeof"])
    for f in FIELDS:
        assert getattr(N.MwFloatTaskConfig, f).offset == int(out[f]), f
    # mw_task_config keeps its size: the floating-base task has its own struct
    assert ctypes.sizeof(N.MwTaskConfig) == 48


def test_null_arguments_are_refused(N):
    h = ctypes.c_void_p()
    cfg = N.MwFloatTaskConfig()
    assert N.lib().mw_floatenv_create(None, ctypes.byref(cfg), ctypes.byref(h)) == N.MW_EINVAL
    assert "null" in N.last_error()
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, 2, 0, 0)
    N.check(N.lib().mw_create(ctypes.byref(mc), ctypes.byref(sim)))
    try:
        assert N.lib().mw_floatenv_create(sim, None, ctypes.byref(h)) == N.MW_EINVAL
        assert N.lib().mw_floatenv_create(sim, ctypes.byref(cfg), None) == N.MW_EINVAL
        # a simulator that was never initialized is refused too, before any device work
        assert N.lib().mw_floatenv_create(sim, ctypes.byref(cfg), ctypes.byref(h)) == N.MW_ESTATE
        assert not h.value
    finally:
        N.lib().mw_destroy(sim)


def test_python_class_is_exported():
    import mwstep
    from mwstep import FloatVecEnv
    assert FloatVecEnv is mwstep.floatenv.FloatVecEnv
    for name in ("reset", "step", "step_raw", "counters", "close", "icub", "quadruped"):
        assert callable(getattr(FloatVecEnv, name))
