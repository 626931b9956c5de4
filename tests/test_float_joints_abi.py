"""Per-world joint dynamics and the joint randomisation of the floating-base env
at the C ABI, without a GPU: libmwstep.so exports mw_set_joint_dynamics,
mw_joint_dynamics and mw_floatenv_joints, the ctypes mirror of
mw_float_joint_config has the C struct's size and field offsets (an offsetof
printer compiled against include/mwstep.h, as test_float_inertia_abi.py does),
the other config structs keep their sizes, null and uninitialised handles are
refused with the documented codes through the host build, and the Python layer
carries the new arguments."""

import ctypes
import inspect
import os
import subprocess

import pytest

from conftest import ROOT
from host_build import build_host, fp as _fp, host_sim as _host_sim

FIELDS = ["damping_lo", "damping_hi", "friction_lo", "friction_hi", "effort_scale_lo", "effort_scale_hi", "dof_mask"]
SYMBOLS = ["mw_set_joint_dynamics", "mw_joint_dynamics", "mw_floatenv_joints"]
OTHERS = {"mw_float_task_config": "MwFloatTaskConfig", "mw_float_rand_config": "MwFloatRandConfig",
          "mw_float_loco_config": "MwFloatLocoConfig", "mw_float_inertia_config": "MwFloatInertiaConfig"}
# sizes of the four structs before this feature (LP64)
SIZES_BEFORE = {"mw_float_task_config": 104, "mw_float_rand_config": 24, "mw_float_loco_config": 76,
                "mw_float_inertia_config": 28}


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
    # what the header promises: the three decisions and the row budget
    for phrase in ("Instance choice", "Shared setters", "Host-derived quantities keep the nominal model",
                   "mw_constraint_overflow", "0x40000200 | d"):
        assert phrase in header, phrase


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_joint_config, {f}));\n' for f in FIELDS)
    prints += "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in OTHERS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_joint_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatJointConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatJointConfig) == int(out["sizeof"]) == 32
    for f in FIELDS:
        assert getattr(N.MwFloatJointConfig, f).offset == int(out[f]), f
    # the other structs did not grow: the joint randomisation has its own
    for c_name, py_name in OTHERS.items():
        assert ctypes.sizeof(getattr(N, py_name)) == int(out[c_name]) == SIZES_BEFORE[c_name], c_name


def test_null_and_uninitialised_handles_are_refused(N):
    cfg = N.MwFloatJointConfig(0.0, 0.5, 0.0, 2.0, 0.5, 1.0, 0)
    assert N.lib().mw_floatenv_joints(None, ctypes.byref(cfg), None, None) == N.MW_EINVAL
    assert "null" in N.last_error()
    words = (ctypes.c_float * 6)(*([1.0] * 6))
    assert N.lib().mw_set_joint_dynamics(None, 0, 2, 0, words) == N.MW_ESTATE
    assert N.lib().mw_joint_dynamics(None, 0, 2, 0, words) == N.MW_ESTATE
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, 2, 0, 0)
    N.check(N.lib().mw_create(ctypes.byref(mc), ctypes.byref(sim)))
    try:
        # no model, never initialized: refused before any device work
        assert N.lib().mw_set_joint_dynamics(sim, 0, 2, 0, words) == N.MW_ESTATE
        assert N.lib().mw_joint_dynamics(sim, 0, 2, 0, words) == N.MW_ESTATE
        assert N.lib().mw_floatenv_joints(None, None, None, None) == N.MW_EINVAL
        assert list(words) == [1.0] * 6
    finally:
        N.lib().mw_destroy(sim)


def test_python_layer_carries_the_arguments():
    from mwstep import FloatVecEnv
    from mwstep.sim import Simulator
    params = inspect.signature(FloatVecEnv.__init__).parameters
    for name in ("joint_damping_range", "joint_friction_range", "effort_scale_range", "joint_rand_dofs"):
        assert name in params and params[name].default is None, name
    for name in ("set_joint_dynamics", "joint_dynamics"):
        assert callable(getattr(Simulator, name))
    assert list(inspect.signature(Simulator.set_joint_dynamics).parameters) == ["self", "dof", "params", "worlds"]
    assert list(inspect.signature(Simulator.joint_dynamics).parameters) == ["self", "dof", "worlds"]


# ---- the argument checks and the host-side rules, through a host build ----
# host_build.py: the library's host layer over the stand-in for the HIP runtime,
# so everything the host decides -- validation, the mirror, the shared setter,
# ownership -- runs without a GPU.

@pytest.fixture(scope="module")
def host(N, tmp_path_factory):
    return build_host(N, tmp_path_factory.mktemp("hostlib"))


def _all_words(N, L, sim, W, n):
    import numpy as np
    out = np.zeros((n, W, 3), np.float32)
    for d in range(n):
        assert L.mw_joint_dynamics(sim, 0, W, d, _fp(out[d])) == N.MW_OK
    return out


def test_host_build_set_get_and_argument_checks(N, host):
    import numpy as np
    L, W, n = host, 9, 8
    sim = _host_sim(N, L, "quadruped", W)
    kernel = ctypes.c_int32()
    assert L.mw_float_kernel(sim, ctypes.byref(kernel)) == N.MW_OK and kernel.value == 2
    state_words = ctypes.c_int32()
    assert L.mw_state_words(sim, ctypes.byref(state_words)) == N.MW_OK
    before_words = state_words.value
    nominal = _all_words(N, L, sim, W, n)                       # no storage yet: the nominal words
    np.testing.assert_array_equal(nominal, np.tile(np.float32([0.0, 0.0, 60.0]), (n, W, 1)))
    rng = np.random.default_rng(5)
    words = np.column_stack([rng.uniform(0, 0.5, 4), rng.uniform(0, 2, 4), rng.uniform(6, 60, 4)]).astype(np.float32)
    words[1, 2] = np.finfo(np.float32).max                      # "unbounded" is allowed
    assert L.mw_set_joint_dynamics(sim, 3, 4, 5, _fp(words)) == N.MW_OK, L.mw_last_error()
    got = _all_words(N, L, sim, W, n)
    np.testing.assert_array_equal(got[5, 3:7], words)           # bit for bit
    want = nominal.copy()
    want[5, 3:7] = words
    np.testing.assert_array_equal(got, want)                    # and nothing else moved
    # the inertial words of the same records are untouched
    link = np.zeros((W, 10), np.float32)
    assert L.mw_link_params(sim, 0, W, 5, _fp(link)) == N.MW_OK
    assert len({row.tobytes() for row in link}) == 1 and link[0, 0] > 0
    # parameters, not state: the records of mw_get_state did not grow
    assert L.mw_state_words(sim, ctypes.byref(state_words)) == N.MW_OK and state_words.value == before_words
    bad_rows = [(0, -0.1, "damping must be >= 0"), (1, -1.0, "friction must be >= 0"), (2, 0.0, "effort limit must be > 0"),
                (2, -5.0, "effort limit must be > 0"), (0, np.nan, "must be finite"), (1, np.inf, "must be finite"),
                (2, np.inf, "must be finite")]
    for k, value, msg in bad_rows:
        w = words[:2].copy()
        w[1, k] = value                                         # the second world of the range is the bad one
        assert L.mw_set_joint_dynamics(sim, 0, 2, 5, _fp(w)) == N.MW_EINVAL, (k, value)
        assert msg in L.mw_last_error().decode(), L.mw_last_error()
    for w0, nw, dof in ((8, 2, 0), (-1, 1, 0), (0, -1, 0), (0, 1, -1), (0, 1, 8)):
        assert L.mw_set_joint_dynamics(sim, w0, nw, dof, _fp(words)) == N.MW_EINVAL, (w0, nw, dof)
        assert L.mw_joint_dynamics(sim, w0, nw, dof, _fp(words.copy())) == N.MW_EINVAL, (w0, nw, dof)
    assert L.mw_set_joint_dynamics(sim, 0, 1, 0, None) == N.MW_EINVAL
    np.testing.assert_array_equal(_all_words(N, L, sim, W, n), want)   # every refused call left nothing changed
    L.mw_destroy(sim)
    # a fixed-base chain is not on the world-per-wavefront kernel
    cart = _host_sim(N, L, "cartpole", 2)
    assert L.mw_set_joint_dynamics(cart, 0, 1, 0, _fp(words)) == N.MW_ESTATE
    assert L.mw_joint_dynamics(cart, 0, 1, 0, _fp(words.copy())) == N.MW_ESTATE
    assert "world-per-wavefront" in L.mw_last_error().decode()
    L.mw_destroy(cart)


def test_host_build_shared_setter_overwrites_one_word(N, host):
    """mw_set_joint_param after a per-world set: that word of that dof in every
    world, every other per-world joint word and the inertial words kept; a
    setter of another kind (gravity) keeps them all."""
    import numpy as np
    L, W, n = host, 5, 8
    sim = _host_sim(N, L, "quadruped", W)
    rng = np.random.default_rng(6)
    words = np.column_stack([rng.uniform(0.1, 0.5, W), rng.uniform(0.1, 2, W), rng.uniform(6, 60, W)]).astype(np.float32)
    for d in (1, 4):
        assert L.mw_set_joint_dynamics(sim, 0, W, d, _fp(words)) == N.MW_OK
    mass = np.zeros((W, 10), np.float32)
    assert L.mw_link_params(sim, 0, W, 1, _fp(mass)) == N.MW_OK
    mass[:, 0] *= np.float32([1.0, 1.5, 0.7, 2.0, 0.9])
    assert L.mw_set_link_params(sim, 0, W, 1, _fp(mass)) == N.MW_OK
    assert L.mw_set_joint_param(sim, 1, N.PARAM_MAX_GENERALIZED_FORCE, 5.0) == N.MW_OK
    assert L.mw_set_joint_param(sim, 2, N.PARAM_COULOMB_FRICTION, 0.75) == N.MW_OK
    g = np.float64([0.0, 0.0, -3.7])
    assert L.mw_set_gravity(sim, N.dptr(g)) == N.MW_OK
    got = _all_words(N, L, sim, W, n)
    want = np.tile(np.float32([0.0, 0.0, 60.0]), (n, W, 1))
    want[1] = want[4] = words
    want[1, :, 2] = 5.0                                          # the word the shared setter names, every world
    want[2, :, 1] = 0.75                                         # a joint never set per world takes the shared value
    np.testing.assert_array_equal(got, want)
    back = np.zeros((W, 10), np.float32)
    assert L.mw_link_params(sim, 0, W, 1, _fp(back)) == N.MW_OK
    np.testing.assert_array_equal(back, mass)
    L.mw_destroy(sim)


def _all_records(N, L, sim, W, n):
    """Every per-world word of every record: the ten inertial words of the base
    and of each link, and each dof's damping, friction and effort."""
    import numpy as np
    inertial = np.zeros((n + 1, W, 10), np.float32)
    for link in range(-1, n):
        assert L.mw_link_params(sim, 0, W, link, _fp(inertial[link + 1])) == N.MW_OK
    return inertial, _all_words(N, L, sim, W, n)


def test_host_build_shared_setters_keep_a_world_with_both_kinds_of_words(N, host):
    """One world holds its own inertial words (the base and link 3) and its own
    joint words (dofs 3 and 6) in one record; mw_set_joint_param on dof 3 and
    mw_set_gravity then rewrite every record from the shared blocks.  Every
    per-world word of every world afterwards: the set ones kept, the one word the
    shared setter names overwritten in all worlds, every other word nominal."""
    import numpy as np
    L, W, n, w = host, 3, 8, 1
    sim = _host_sim(N, L, "quadruped", W)
    inertial0, joints0 = _all_records(N, L, sim, W, n)       # nominal, before any storage exists
    rng = np.random.default_rng(11)
    want_i, want_j = inertial0.copy(), joints0.copy()
    for link in (-1, 3):
        words = (inertial0[link + 1, w] * rng.uniform(0.5, 2.0, 10)).astype(np.float32)
        words[0] = abs(words[0]) + np.float32(0.25)
        assert L.mw_set_link_params(sim, w, 1, link, _fp(words)) == N.MW_OK, L.mw_last_error()
        want_i[link + 1, w] = words
    for dof in (3, 6):
        words = np.float32([rng.uniform(0.1, 0.5), rng.uniform(0.1, 2.0), rng.uniform(6, 60)])
        assert L.mw_set_joint_dynamics(sim, w, 1, dof, _fp(words)) == N.MW_OK, L.mw_last_error()
        want_j[dof, w] = words
    got_i, got_j = _all_records(N, L, sim, W, n)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_j, want_j)
    assert L.mw_set_joint_param(sim, 3, N.PARAM_VISCOUS_FRICTION, 0.125) == N.MW_OK, L.mw_last_error()
    g = np.float64([0.5, 0.0, -3.7])
    assert L.mw_set_gravity(sim, N.dptr(g)) == N.MW_OK
    want_j[3, :, 0] = 0.125                                   # the named word, every world, the set one included
    got_i, got_j = _all_records(N, L, sim, W, n)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_j, want_j)
    L.mw_destroy(sim)


def test_host_build_env_call_order_and_ownership(N, host):
    import numpy as np
    L, W, n = host, 4, 8
    sim = _host_sim(N, L, "quadruped", W)
    assert L.mw_set_ground_plane(sim, 1, 1.0) == N.MW_OK and L.mw_enable_contacts(sim, 1) == N.MW_OK
    home_q = np.float32([0.6, -1.2] * 4)
    cfg = N.MwFloatTaskConfig(0, 100, 0, 0, 7, 0.0, -1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0,
                              (ctypes.c_float * 7)(0, 0, 0.45, 1, 0, 0, 0), _fp(home_q), None)
    env = ctypes.c_void_p()
    assert L.mw_floatenv_create(sim, ctypes.byref(cfg), ctypes.byref(env)) == N.MW_OK, L.mw_last_error()
    J = N.MwFloatJointConfig
    bad = [J(-0.1, 0.5, 0, 0, 0, 0, 0), J(0.6, 0.5, 0, 0, 0, 0, 0), J(0, 0, -1.0, 2.0, 0, 0, 0), J(0, 0, 2.0, 1.0, 0, 0, 0),
           J(0, 0, 0, 0, 0.0, 1.0, 0), J(0, 0, 0, 0, 1.5, 1.0, 0), J(0, 0, 0, 0, -0.5, 1.0, 0), J(0, 0, 0, 0, 0.5, 0.0, 0),
           J(0, float("nan"), 0, 0, 0, 0, 0), J(0, 0, 0, float("inf"), 0, 0, 0), J(0, 0.5, 0, 0, 0, 0, 1 << 8),
           J(0, 0, 0, 0, 0, -1.0, 0)]
    for k, c in enumerate(bad):
        assert L.mw_floatenv_joints(env, ctypes.byref(c), None, None) == N.MW_EINVAL, k
    words = np.float32([[0.1, 0.2, 30.0]])
    # the refused calls left the env without the feature: the simulator's setter works
    assert L.mw_set_joint_dynamics(sim, 0, 1, 0, _fp(words)) == N.MW_OK
    good = J(0.0, 0.5, 0.0, 2.0, 0.5, 1.0, 0b00110011)
    assert L.mw_floatenv_joints(env, ctypes.byref(good), None, None) == N.MW_OK, L.mw_last_error()
    assert L.mw_set_joint_dynamics(sim, 0, 1, 0, _fp(words)) == N.MW_ESTATE
    assert "joint randomisation owns" in L.mw_last_error().decode()
    assert L.mw_set_link_params(sim, 0, 1, 0, _fp(np.ones((1, 10), np.float32))) == N.MW_ESTATE
    got = np.zeros((1, 3), np.float32)
    assert L.mw_joint_dynamics(sim, 0, 1, 0, _fp(got)) == N.MW_OK      # reads the device copy back
    np.testing.assert_array_equal(got, words)
    # everything off returns the env as made
    off = J(0, 0, 0, 0, 0, 0, 0)
    assert L.mw_floatenv_joints(env, ctypes.byref(off), None, None) == N.MW_OK
    assert L.mw_set_joint_dynamics(sim, 0, 1, 0, _fp(words)) == N.MW_OK
    # any order with the inertia call; then the first reset closes the window
    ic = N.MwFloatInertiaConfig(0.8, 1.2, 0.0, 0.0, (ctypes.c_float * 3)(0, 0, 0))
    assert L.mw_floatenv_joints(env, ctypes.byref(good), None, None) == N.MW_OK
    assert L.mw_floatenv_inertia(env, ctypes.byref(ic), None, None) == N.MW_OK
    obs_n = ctypes.c_int32()
    assert L.mw_vecenv_obs_dim(env, ctypes.byref(obs_n)) == N.MW_OK
    obs = np.zeros((W, obs_n.value), np.float32)
    assert L.mw_vecenv_reset(env, obs.ctypes.data_as(ctypes.c_void_p)) == N.MW_OK, L.mw_last_error()
    assert L.mw_floatenv_joints(env, ctypes.byref(good), None, None) == N.MW_ESTATE
    assert "before the first mw_vecenv_reset" in L.mw_last_error().decode()
    L.mw_vecenv_destroy(env)
    # destroying the env hands the records back: the setter works, the getter reads the mirror
    assert L.mw_set_joint_dynamics(sim, 1, 1, 2, _fp(words)) == N.MW_OK
    assert L.mw_joint_dynamics(sim, 1, 1, 2, _fp(got)) == N.MW_OK
    np.testing.assert_array_equal(got, words)
    L.mw_destroy(sim)


def test_host_build_two_body_model_has_no_constraint_flags(N, host, tmp_path):
    """The model of the GPU instance-choice test: stepped by the
    world-per-wavefront kernel, nominal flags without limits or friction, an
    unbounded effort limit that mw_joint_dynamics reports as FLT_MAX."""
    import numpy as np
    from float_joints_ref import FLT_MAX, write_two_body
    L = host
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, 3, 0, 20)
    assert L.mw_create(ctypes.byref(mc), ctypes.byref(sim)) == N.MW_OK
    pose = np.float64([0, 0, 1, 1, 0, 0, 0])
    assert L.mw_load_model(sim, write_two_body(tmp_path).encode(), N.dptr(pose), b"") == N.MW_OK, L.mw_last_error()
    assert L.mw_initialize(sim) == N.MW_OK, L.mw_last_error()
    kernel, n = ctypes.c_int32(), ctypes.c_int32()
    assert L.mw_float_kernel(sim, ctypes.byref(kernel)) == N.MW_OK and kernel.value == 2
    assert L.mw_dofs(sim, ctypes.byref(n)) == N.MW_OK and n.value == 1
    P = ctypes.create_string_buffer(1 << 16)
    assert L.mw_device_params(sim, P, len(P)) == N.MW_OK
    head = np.frombuffer(P.raw[:8], np.int32)
    assert head[0] == 1 and head[1] == 0                      # ChainF::n, ChainF::flags: no kHas* bit
    got = np.zeros((3, 3), np.float32)
    assert L.mw_joint_dynamics(sim, 0, 3, 0, _fp(got)) == N.MW_OK
    np.testing.assert_array_equal(got, np.tile(np.float32([0.0, 0.0, FLT_MAX]), (3, 1)))
    L.mw_destroy(sim)
