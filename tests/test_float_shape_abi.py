"""Shaping rewards, contact termination and episode statistics of the
floating-base env at the C ABI.  Without a GPU: libmwstep.so exports
mw_floatenv_shaping, the ctypes mirror of mw_float_shape_config has the C
struct's size and field offsets (an offsetof printer compiled against
include/mwstep.h, as test_float_noise_abi.py does), the six earlier config
structs keep their sizes, null arguments are refused, and the Python layer
carries the new arguments.  With one (the tests marked gpu: a refusal past the
null test needs an env, and an env needs a device): every refusal the header
lists, and the all-zero config that returns the env as made."""

import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["weights", "base_height_target", "soft_limit", "collision_force_min", "stumble_ratio", "max_contact_force",
          "termination_force", "n_penalised_links", "n_termination_links", "penalised_links", "termination_links"]
OTHERS = {"mw_float_task_config": "MwFloatTaskConfig", "mw_float_rand_config": "MwFloatRandConfig",
          "mw_float_loco_config": "MwFloatLocoConfig", "mw_float_inertia_config": "MwFloatInertiaConfig",
          "mw_float_joint_config": "MwFloatJointConfig", "mw_float_noise_config": "MwFloatNoiseConfig"}
# sizes of the six structs before this feature (LP64)
SIZES_BEFORE = {"mw_float_task_config": 104, "mw_float_rand_config": 24, "mw_float_loco_config": 76,
                "mw_float_inertia_config": 28, "mw_float_joint_config": 32, "mw_float_noise_config": 8}
TERMS = ["torque", "power", "joint_acc", "orientation", "base_height", "joint_limits", "collision", "stumble",
         "contact_force", "stand_still"]


@pytest.fixture(scope="module")
def N():
    from mwstep import native
    native.lib()
    return native


def test_library_exports_the_symbol(N):
    L = ctypes.CDLL(N.LIB_PATH)
    declared = {name: args for name, _, args in N.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "mwstep.h")).read()
    assert hasattr(L, "mw_floatenv_shaping")
    assert len(declared["mw_floatenv_shaping"]) == 7
    assert "int mw_floatenv_shaping(" in header
    assert "#define MW_FLOAT_SHAPE_TERMS 10" in header and N.FLOAT_SHAPE_TERMS == 10
    # the header says what "contact" means for the termination
    assert "LAST physics step" in header


def test_ctypes_mirror_matches_the_c_struct(N, tmp_path):
    src = tmp_path / "layout.c"
    prints = "".join(f'  printf("{f} %zu\\n", offsetof(mw_float_shape_config, {f}));\n' for f in FIELDS)
    prints += "".join(f'  printf("{s} %zu\\n", sizeof({s}));\n' for s in OTHERS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mwstep.h"\n'
                   'int main(void) {\n  printf("sizeof %zu\\n", sizeof(mw_float_shape_config));\n'
                   + prints + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert [name for name, _ in N.MwFloatShapeConfig._fields_] == FIELDS
    assert ctypes.sizeof(N.MwFloatShapeConfig) == int(out["sizeof"]) == 88
    for f in FIELDS:
        assert getattr(N.MwFloatShapeConfig, f).offset == int(out[f]), f
    # no existing struct grew: the feature has its own
    for c_name, py_name in OTHERS.items():
        assert ctypes.sizeof(getattr(N, py_name)) == int(out[c_name]) == SIZES_BEFORE[c_name], c_name


def test_null_arguments_are_refused(N):
    cfg = N.MwFloatShapeConfig()
    assert N.lib().mw_floatenv_shaping(None, ctypes.byref(cfg), None, None, None, None, None) == N.MW_EINVAL
    assert "null" in N.last_error()
    assert N.lib().mw_floatenv_shaping(None, None, None, None, None, None, None) == N.MW_EINVAL
    assert "null" in N.last_error()


def test_python_layer_carries_the_arguments():
    from mwstep import FloatVecEnv
    from mwstep.floatenv import REWARD_TERMS
    assert list(REWARD_TERMS) == TERMS
    params = inspect.signature(FloatVecEnv.__init__).parameters
    for name in ("reward_terms", "termination_links", "base_height_target"):
        assert name in params and params[name].default is None, name
    defaults = dict(termination_force=1.0, penalised_links=(), collision_force_min=0.1, soft_limit=0.9,
                    stumble_ratio=5.0)
    for name, value in defaults.items():
        assert params[name].default == value, name
    assert "max_contact_force" in params
    for make in (FloatVecEnv.quadruped, FloatVecEnv.icub):
        assert "kw" in inspect.signature(make).parameters


# ---- the refusals: these need an env, and so a device ----

def _config(N, weights=None, links=(), pen=(), **fields):
    w = np.zeros(10, np.float32)
    for name, value in (weights or {}).items():
        w[TERMS.index(name)] = value
    values = dict(base_height_target=0.45, soft_limit=0.9, collision_force_min=0.1, stumble_ratio=5.0,
                  max_contact_force=50.0, termination_force=1.0)
    values.update(fields)
    term, penal = np.asarray(links, np.int32), np.asarray(pen, np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if len(a) else None
    cfg = N.MwFloatShapeConfig((ctypes.c_float * 10)(*w.tolist()), values["base_height_target"], values["soft_limit"],
                               values["collision_force_min"], values["stumble_ratio"], values["max_contact_force"],
                               values["termination_force"], len(penal), len(term), ip(penal), ip(term))
    cfg._keep = (term, penal)
    return cfg


def _call(N, env, cfg):
    return N.lib().mw_floatenv_shaping(env._h, ctypes.byref(cfg), None, None, None, None, None)


@pytest.mark.gpu
def test_every_refusal(require_gpu, N):
    from mwstep import FloatVecEnv
    env = FloatVecEnv.quadruped(4)                  # trunk (-1) and the shanks (1, 3, 5, 7) carry shapes, the thighs none
    ok = _config(N, {"torque": 1e-4, "collision": 1.0}, links=(-1,), pen=(-1,))
    refused = [
        (_config(N, {"torque": 1.0}, links=(8,)), N.MW_EINVAL, "termination link 8 out of range"),
        (_config(N, {"torque": 1.0}, links=(-2,)), N.MW_EINVAL, "termination link -2 out of range"),
        (_config(N, {"collision": 1.0}, pen=(9,)), N.MW_EINVAL, "penalised link 9 out of range"),
        (_config(N, {"torque": 1.0}, links=(0,)), N.MW_EINVAL, "termination link 0 owns no contact slot"),
        (_config(N, {"collision": 1.0}, pen=(2,)), N.MW_EINVAL, "penalised link 2 owns no contact slot"),
        (_config(N, {"collision": 1.0}), N.MW_EINVAL, "collision term needs penalised links"),
        (_config(N, {"stand_still": 1.0}), N.MW_ESTATE, "needs the locomotion task"),
        (_config(N, {"power": -1.0}), N.MW_EINVAL, "must be >= 0"),
        (_config(N, {"power": float("nan")}), N.MW_EINVAL, "must be finite"),
        (_config(N, {"power": 1.0}, termination_force=float("inf")), N.MW_EINVAL, "must be finite"),
        (_config(N, {"power": 1.0}, base_height_target=float("nan")), N.MW_EINVAL, "must be finite"),
        (_config(N, {"power": 1.0}, collision_force_min=-1.0), N.MW_EINVAL, "must be >= 0"),
        (_config(N, {"power": 1.0}, soft_limit=0.0), N.MW_EINVAL, "soft_limit must be in (0, 1]"),
        (_config(N, {"power": 1.0}, soft_limit=1.5), N.MW_EINVAL, "soft_limit must be in (0, 1]"),
    ]
    for cfg, code, text in refused:
        assert _call(N, env, cfg) == code, text
        assert text in N.last_error(), (text, N.last_error())
    big = _config(N, {"collision": 1.0}, pen=(-1,) * 9)
    assert _call(N, env, big) == N.MW_EINVAL and "n_penalised_links must be in [0, 8]" in N.last_error()
    assert _call(N, env, ok) == N.MW_OK
    env.reset()
    assert _call(N, env, ok) == N.MW_ESTATE and "before the first mw_vecenv_reset" in N.last_error()
    env.close()
    # stumble / contact_force read the contact links
    bare = FloatVecEnv.quadruped(4, contact_links=())
    assert _call(N, bare, _config(N, {"stumble": 1.0})) == N.MW_EINVAL and "need contact links" in N.last_error()
    bare.close()
    # a fixed-base env is another kind
    from mwstep import VecEnv
    other = VecEnv("CartPoleDiscreteBalancing", 4)
    handle = getattr(other, "_h", None) or getattr(other, "handle", None)
    assert N.lib().mw_floatenv_shaping(handle, ctypes.byref(ok), None, None, None, None, None) == N.MW_ESTATE
    assert "needs an env made by mw_floatenv_create" in N.last_error()
    other.close()
    # the Python layer: unknown names, with the known ones listed
    with pytest.raises(ValueError, match="unknown term 'torques'.*'torque'.*'stand_still'"):
        FloatVecEnv.quadruped(4, reward_terms={"torques": 1.0})
    with pytest.raises(ValueError, match="not found"):
        FloatVecEnv.quadruped(4, termination_links=("no_such_link",))
    with pytest.raises(RuntimeError, match="owns no contact slot"):
        FloatVecEnv.quadruped(4, reward_terms={"collision": 1.0}, penalised_links=("thigh_fl",))
    with pytest.raises(RuntimeError, match="needs the locomotion task"):
        FloatVecEnv.quadruped(4, reward_terms={"stand_still": 1.0})


@pytest.mark.gpu
def test_the_all_zero_config_restores_the_env(require_gpu, N):
    import torch
    from mwstep import FloatVecEnv
    kw = dict(joint_noise=0.05, seed=3, max_episode_steps=6)
    rng = np.random.default_rng(1)
    acts = (np.float32([0.6, -1.2] * 4) + rng.uniform(-0.2, 0.2, (10, 4, 8))).astype(np.float32)
    plain = FloatVecEnv.quadruped(4, **kw)
    env = FloatVecEnv.quadruped(4, **kw)
    terms = torch.full((4, 10), 7.0, device=env.device)
    on = _config(N, {"torque": 1e-3, "orientation": 1.0}, links=(-1,))
    assert N.lib().mw_floatenv_shaping(env._h, ctypes.byref(on), ctypes.c_void_p(terms.data_ptr()), None, None, None,
                                       None) == N.MW_OK
    assert _call(N, env, N.MwFloatShapeConfig()) == N.MW_OK
    a, b = env.reset().cpu().numpy(), plain.reset().cpu().numpy()
    np.testing.assert_array_equal(a, b)
    for k in range(10):
        oa, ra, da, _ = env.step(torch.from_numpy(acts[k]).to(env.device))
        ob, rb, db, _ = plain.step(torch.from_numpy(acts[k]).to(plain.device))
        np.testing.assert_array_equal(oa.cpu().numpy(), ob.cpu().numpy())
        np.testing.assert_array_equal(ra.cpu().numpy(), rb.cpu().numpy())
        np.testing.assert_array_equal(da.cpu().numpy(), db.cpu().numpy())
    assert (terms.cpu().numpy() == 7.0).all()        # the buffer of the cancelled call is never written
    env.close()
    plain.close()
