"""Per-world link parameters and the inertia randomisation of the floating-base
env at the C ABI, without a GPU: libmwstep.so exports mw_set_link_params,
mw_link_params and mw_floatenv_inertia, the ctypes mirror of
mw_float_inertia_config has the C struct's size and field offsets (an offsetof
printer compiled against include/mwstep.h, as test_float_rand_abi.py does), the
task, randomisation and locomotion structs keep their sizes, null and
uninitialised handles are refused, and the Python layer carries the new
arguments."""

import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["mass_scale_lo", "mass_scale_hi", "payload_lo", "payload_hi", "payload_box"]
SYMBOLS = ["mw_set_link_params", "mw_link_params", "mw_floatenv_inertia"]
OTHERS = {"mw_float_task_config": "MwFloatTaskConfig", "mw_float_rand_config": "MwFloatRandConfig",
          "mw_float_loco_config": "MwFloatLocoConfig"}
# sizes of the three structs before this feature (LP64)
SIZES_BEFORE = {"mw_float_task_config": 104, "mw_float_rand_config": 24, "mw_float_loco_config": 76}


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
    # what the header promises about the parameters
    for phrase in ("mw_get_state /\n * mw_set_state records do not hold them", "keep the nominal model"):
        assert phrase in header, phrase


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_inertia_config, {f}));\n' for f in FIELDS)
    prints += "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in OTHERS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_inertia_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatInertiaConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatInertiaConfig) == int(out["sizeof"]) == 28
    for f in FIELDS:
        assert getattr(N.MwFloatInertiaConfig, f).offset == int(out[f]), f
    # the other structs did not grow: the inertia randomisation has its own
    for c_name, py_name in OTHERS.items():
        assert ctypes.sizeof(getattr(N, py_name)) == int(out[c_name]) == SIZES_BEFORE[c_name], c_name


def test_null_and_uninitialised_handles_are_refused(N):
    cfg = N.MwFloatInertiaConfig(0.8, 1.2, 0.0, 5.0, (ctypes.c_float * 3)(0.1, 0.1, 0.05))
    assert N.lib().mw_floatenv_inertia(None, ctypes.byref(cfg), None, None) == N.MW_EINVAL
    assert "null" in N.last_error()
    words = (ctypes.c_float * 20)(*([1.0] * 20))
    assert N.lib().mw_set_link_params(None, 0, 2, -1, words) == N.MW_ESTATE
    assert N.lib().mw_link_params(None, 0, 2, -1, words) == N.MW_ESTATE
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, 2, 0, 0)
    N.check(N.lib().mw_create(ctypes.byref(mc), ctypes.byref(sim)))
    try:
        # no model, never initialized: refused before any device work
        assert N.lib().mw_set_link_params(sim, 0, 2, -1, words) == N.MW_ESTATE
        assert N.lib().mw_link_params(sim, 0, 2, -1, words) == N.MW_ESTATE
        assert list(words) == [1.0] * 20
    finally:
        N.lib().mw_destroy(sim)


def test_python_layer_carries_the_arguments():
    from mwstep import FloatVecEnv
    from mwstep.sim import Simulator
    params = inspect.signature(FloatVecEnv.__init__).parameters
    defaults = {"mass_scale_range": None, "payload_range": None, "payload_box": (0.0, 0.0, 0.0)}
    for name, value in defaults.items():
        assert name in params and params[name].default == value, name
    for name in ("set_link_params", "link_params", "set_link_inertial", "link_index"):
        assert callable(getattr(Simulator, name))
    assert list(inspect.signature(Simulator.set_link_params).parameters) == ["self", "link", "params", "worlds"]
    assert list(inspect.signature(Simulator.set_link_inertial).parameters) == [
        "self", "link", "mass", "com", "inertia_about_com", "worlds"]


def test_inertial_words_shift_to_the_origin_in_fp64():
    """set_link_inertial's words: Io = Ic + m (|c|^2 1 - c c^T), rounded once."""
    from mwstep.sim import Simulator
    rng = np.random.default_rng(0)
    m, c = 3.7, np.array([0.11, -0.07, 0.23])
    A = rng.normal(size=(3, 3))
    Ic = A @ A.T + np.eye(3)
    Io = Ic + m * (c @ c * np.eye(3) - np.outer(c, c))
    want = np.float32([m, *c, Io[0, 0], Io[1, 1], Io[2, 2], Io[0, 1], Io[0, 2], Io[1, 2]])
    np.testing.assert_array_equal(Simulator.inertial_words(m, c, Ic), want)
    six = [Ic[0, 0], Ic[1, 1], Ic[2, 2], Ic[0, 1], Ic[0, 2], Ic[1, 2]]
    np.testing.assert_array_equal(Simulator.inertial_words(m, c, six), want)
    both = Simulator.inertial_words([m, 2 * m], c, six)
    assert both.shape == (2, 10) and both.dtype == np.float32
    np.testing.assert_array_equal(both[0], want)
