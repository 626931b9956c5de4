"""Shared by the tests of the per-world joint dynamics and the joint
randomisation (test helper): the host build of the kernel's word function
(tests/host_float_joints/harness.cpp), the host restatement of the env's draws
from the oracle's Philox4x32-10, and the states and per-world parameters of the
one-step oracle tests (CPU and GPU share them)."""

import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "gym-ignition_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "host_float_joints", "harness.cpp")
JOINT_BLOCK = 0x40000200
DAMPING, FRICTION, EFFORT = 1, 2, 4
FLT_MAX = np.finfo(np.float32).max

# the one-step oracle cases: model, worlds, and the joints that are given their
# own words (None = every joint).  The iCub's mask is the knees and ankles, six
# leg joints: random_states sinks the robot into the ground at a tilt, so the
# nominal model already has up to 56 rows there (contact points of several
# links, three rows each, and one row per joint beyond its position limit);
# friction adds one row per moving masked joint, and with these six the largest
# problem has 62 of the kernel's 64 rows (all twelve leg joints: 68).
ICUB_LEGS = [f"{s}_{j}" for s in ("l", "r") for j in ("knee", "ankle_pitch", "ankle_roll")]
ORACLE_CASES = [("quadruped", 70, None), ("icub", 40, ICUB_LEGS)]
STATE_SEED, PARAM_SEED = 11, 71
DAMPING_RANGE, FRICTION_RANGE, EFFORT_RANGE = (0.0, 0.5), (0.0, 2.0), (0.1, 1.0)


def build_harness(directory):
    out = os.path.join(str(directory), "libfj.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DMW_HOST_TEST", "-I", CSRC,
                    HARNESS, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.fj_apply.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    for name in ("fj_joint_block", "fj_scale_block", "fj_payload_block", "fj_episode_block", "fj_push_block",
                 "fj_cmd_block"):
        getattr(L, name).restype = ctypes.c_uint
    L.fj_joint_block.argtypes = L.fj_scale_block.argtypes = [ctypes.c_int]
    L.fj_push_block.argtypes = L.fj_cmd_block.argtypes = [ctypes.c_uint]
    return L


def harness_apply(L, flags, nom, draw):
    """float32 words [..., 3] of the kernel's code on float32 nominal words and draws."""
    nom, draw = (np.ascontiguousarray(a, dtype=np.float32) for a in (nom, draw))
    assert nom.shape == draw.shape and nom.shape[-1] == 3
    out = np.zeros_like(nom)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L.fj_apply(nom.size // 3, flags, ptr(nom), ptr(draw), ptr(out))
    return out


def _unif32(word, lo, hi):
    t = np.float32(np.float32(int(word) >> 8) * np.float32(1.0 / 16777216.0))
    return np.float32(np.float32(lo) + (np.float32(hi) - np.float32(lo)) * t)


def draw_ref(oracle, seed, world, episode, n, damping, friction, effort, dofs=None):
    """The env's draw of (global world, episode) [n, 3]: joint d takes words 0,
    1, 2 of block 0x40000200 | d; the unfused float32 form of U(lo, hi).  A
    range that is None and a joint outside dofs report 0, 0, 1."""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    out = np.tile(np.float32([0.0, 0.0, 1.0]), (n, 1))
    for d in (range(n) if dofs is None else dofs):
        r = oracle.philox_raw([world, episode, JOINT_BLOCK | d, 0], key)
        for e, rng in enumerate((damping, friction, effort)):
            if rng is not None:
                out[d, e] = _unif32(r[e], *rng)
    return out


def nominal_words(cm):
    """float32 [n, 3]: damping, friction, effort of the oracle's model as the simulator holds them."""
    M = cm.model
    eff = np.minimum(np.array(M.effort[:cm.n], dtype=np.float64), float(FLT_MAX))
    return np.column_stack([np.array(M.damping[:cm.n]), np.array(M.friction[:cm.n]), eff]).astype(np.float32)


def per_world_words(nominal, W, dofs):
    """[W, n, 3] float32 words: damping0 + U(0, 0.5), friction0 + U(0, 2) N m,
    U(0.1, 1) effort0 for the joints of dofs (None = all), nominal elsewhere."""
    rng = np.random.default_rng(PARAM_SEED)
    n = nominal.shape[0]
    a = rng.uniform(*DAMPING_RANGE, (W, n)).astype(np.float32)
    f = rng.uniform(*FRICTION_RANGE, (W, n)).astype(np.float32)
    s = rng.uniform(*EFFORT_RANGE, (W, n)).astype(np.float32)
    words = np.tile(nominal, (W, 1, 1))
    sel = list(range(n)) if dofs is None else list(dofs)
    words[:, sel, 0] = nominal[sel, 0] + a[:, sel]
    words[:, sel, 1] = nominal[sel, 1] + f[:, sel]
    scaled = s[:, sel] * nominal[sel, 2]
    words[:, sel, 2] = np.where(nominal[sel, 2] == FLT_MAX, nominal[sel, 2], scaled)
    return words.astype(np.float32)


def apply_words(cm, words):
    """Alter this ChainModel in place to the float32 joint words [n, 3]."""
    for i in range(cm.n):
        cm.model.damping[i] = float(words[i, 0])
        cm.model.friction[i] = float(words[i, 1])
        cm.model.effort[i] = float(words[i, 2])


def model_joint_names(model_file):
    """Joint names in dof order from the simulator's model compiler, without a
    GPU (the model is loaded, the simulator never initialized)."""
    from mwstep import native as N
    L = N.lib()
    sim = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, 1, 0, 0)
    N.check(L.mw_create(ctypes.byref(mc), ctypes.byref(sim)))
    try:
        pose = np.float64([0, 0, 0, 1, 0, 0, 0])
        N.check(L.mw_load_model(sim, model_file.encode(), N.dptr(pose), b""), "mw_load_model")
        n = ctypes.c_int32()
        N.check(L.mw_dofs(sim, ctypes.byref(n)))
        names = []
        for d in range(n.value):
            buf = ctypes.create_string_buffer(256)
            N.check(L.mw_joint_name(sim, d, buf, 256))
            names.append(buf.value.decode())
        return names
    finally:
        L.mw_destroy(sim)


def mask_dofs(joint_names, names):
    return None if names is None else [joint_names.index(j) for j in names]


# A floating two-body model for the instance-choice test: one continuous joint
# without limits and without <dynamics>, so ChainF::flags of the nominal model
# has neither kHasLimits nor kHasFriction and the host would pick the wave
# kernel's instance without joint constraint rows.
TWO_BODY_URDF = """<?xml version="1.0"?>
<robot name="two_body">
  <link name="hub">
    <inertial>
      <origin xyz="0 0 0" rpy="0 0 0"/>
      <mass value="2.0"/>
      <inertia ixx="0.02" ixy="0" ixz="0" iyy="0.03" iyz="0" izz="0.04"/>
    </inertial>
  </link>
  <joint name="spin" type="continuous">
    <parent link="hub"/>
    <child link="arm"/>
    <origin xyz="0.1 0 0" rpy="0 0 0"/>
    <axis xyz="0 1 0"/>
  </joint>
  <link name="arm">
    <inertial>
      <origin xyz="0 0 -0.15" rpy="0 0 0"/>
      <mass value="0.5"/>
      <inertia ixx="0.004" ixy="0" ixz="0" iyy="0.004" iyz="0" izz="0.0005"/>
    </inertial>
  </link>
</robot>
"""


def write_two_body(directory):
    path = os.path.join(str(directory), "two_body.urdf")
    with open(path, "w") as f:
        f.write(TWO_BODY_URDF)
    return path
