"""What the host layer of the floating-base env decides, without a GPU: every
refusal of mw_floatenv_create and of the six configure calls (randomize,
locomotion, inertia, joints, noise, shaping) with its return code and a
distinctive fragment of mw_last_error(), the order rules between the calls, the
"everything off" paths, that a refused call leaves the env as it was, the width
of the observation, and the life of an env from create to destroy.  Through the
host build of host_build.py (the HIP stand-in: device memory is host memory,
the launchers do nothing), on the quadruped at a handful of worlds.

The branches behind MW_HIP(...) need a failing device call and are left out,
as are the return codes handed on from run_impl, mw_set_joint_control_mode, the
alloc_* helpers and set_joint_dynamics_flags, which fail only when a device
call does."""

import ctypes

import numpy as np
import pytest

from host_build import build_host, fp, host_sim

W, NDOF = 5, 8
NAN, INF = float("nan"), float("inf")
FEET = (1, 3, 5, 7)      # the shanks: the links with a collision sphere
THIGH = 0                # a link without a collision shape


@pytest.fixture(scope="module")
def N():
    from mwstep import native
    native.lib()
    return native


@pytest.fixture(scope="module")
def host(N, tmp_path_factory):
    return build_host(N, tmp_path_factory.mktemp("hostlib"))


def _ip(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


class _Rig:
    """A quadruped simulator with ground and contacts, the buffers a task config
    points into kept alive, and the envs it made."""

    def __init__(self, N, L, n_worlds=W, steps_per_run=1):
        self.N, self.L = N, L
        self.sim = host_sim(N, L, "quadruped", n_worlds, steps_per_run)
        assert L.mw_set_ground_plane(self.sim, 1, 1.0) == N.MW_OK and L.mw_enable_contacts(self.sim, 1) == N.MW_OK
        self.home_q = np.float32([0.6, -1.2] * 4)
        self.links, self.links_p = _ip(FEET)
        self.env = None

    def task(self, **kw):
        N = self.N
        f = dict(action_mode=N.FLOAT_ACTION_TORQUE, max_episode_steps=100, world_offset=0, n_contact_links=len(FEET),
                 seed=7, z_min=0.0, cos_tilt_max=-1.0, alive_bonus=1.0, w_forward=1.0, w_action=0.0, w_pose=0.0,
                 joint_noise=0.0, pad_=0.0, home_base=(ctypes.c_float * 7)(0, 0, 0.45, 1, 0, 0, 0),
                 home_q=fp(self.home_q), contact_links=self.links_p)
        f.update(kw)
        return N.MwFloatTaskConfig(**f)

    def create(self, **kw):
        env = ctypes.c_void_p()
        cfg = self.task(**kw)
        rc = self.L.mw_floatenv_create(self.sim, ctypes.byref(cfg), ctypes.byref(env))
        if rc == self.N.MW_OK:
            self.env = env
        else:
            assert not env.value               # a refused create hands out no handle
        return rc

    def obs_dim(self):
        n = ctypes.c_int32(-1)
        assert self.L.mw_vecenv_obs_dim(self.env, ctypes.byref(n)) == self.N.MW_OK
        return n.value

    def reset(self):
        obs = np.zeros((W, self.obs_dim()), np.float32)
        return self.L.mw_vecenv_reset(self.env, obs.ctypes.data_as(ctypes.c_void_p))

    def close(self):
        if self.env is not None:
            self.L.mw_vecenv_destroy(self.env)
            self.env = None
        if self.sim is not None:
            self.L.mw_destroy(self.sim)
            self.sim = None


@pytest.fixture
def rig(N, host):
    r = _Rig(N, host)
    yield r
    r.close()


def _refused(L, rc, code, fragment):
    assert rc == code, (rc, L.mw_last_error())
    assert fragment in L.mw_last_error().decode(), L.mw_last_error()


def _loco(N, **kw):
    f = dict(cmd_lo=(ctypes.c_float * 3)(-1.0, -0.5, -1.0), cmd_hi=(ctypes.c_float * 3)(1.0, 0.5, 1.0), cmd_interval=0,
             cmd_zero_prob=0.1, cmd_min=0.1, action_scale=0.25, w_track_lin=1.0, w_track_yaw=0.5, track_sigma=0.25,
             w_lin_z=0.0, w_ang_xy=0.0, w_action_rate=0.0, w_air_time=0.0, air_time_target=0.3, contact_force_min=1.0)
    for key in ("cmd_lo", "cmd_hi"):
        if key in kw:
            kw[key] = (ctypes.c_float * 3)(*kw[key])
    f.update(kw)
    return N.MwFloatLocoConfig(**f)


def _shape(N, weights=None, pen=(), term=(), **kw):
    """(config, the arrays it points into).  weights: term index -> weight."""
    w = [0.0] * N.FLOAT_SHAPE_TERMS
    for k, v in (weights or {}).items():
        w[k] = v
    pen_a, pen_p = _ip(pen)
    term_a, term_p = _ip(term)
    f = dict(weights=(ctypes.c_float * N.FLOAT_SHAPE_TERMS)(*w), base_height_target=0.45, soft_limit=0.9,
             collision_force_min=0.1, stumble_ratio=5.0, max_contact_force=100.0, termination_force=1.0,
             n_penalised_links=len(pen), n_termination_links=len(term), penalised_links=pen_p if len(pen) else None,
             termination_links=term_p if len(term) else None)
    f.update(kw)
    return N.MwFloatShapeConfig(**f), (pen_a, term_a)


# the terms of mw_float_shape_config::weights the checks name
TORQUE, COLLISION, STUMBLE, CONTACT_FORCE, STAND_STILL = 0, 6, 7, 8, 9

FLOATING_BALL_SDF = """<sdf version='1.7'><model name='ballbody'>
  <link name='trunk'><pose>0 0 1 0 0 0</pose>
    <inertial><mass>3</mass><inertia><ixx>0.05</ixx><iyy>0.05</iyy><izz>0.05</izz><ixy>0</ixy><ixz>0</ixz><iyz>0</iyz></inertia></inertial>
    <collision name='c'><geometry><sphere><radius>0.1</radius></sphere></geometry></collision>
  </link>
  <link name='arm'><pose>0 0 0.8 0 0 0</pose>
    <inertial><mass>1</mass><inertia><ixx>0.01</ixx><iyy>0.01</iyy><izz>0.01</izz><ixy>0</ixy><ixz>0</ixz><iyz>0</iyz></inertia></inertial>
  </link>
  <joint name='shoulder' type='ball'><parent>trunk</parent><child>arm</child></joint>
</model></sdf>"""


def test_create_refusals(N, host, rig):
    L = host
    env = ctypes.c_void_p()
    cfg = rig.task()
    for args in ((None, ctypes.byref(cfg), ctypes.byref(env)), (rig.sim, None, ctypes.byref(env)),
                 (rig.sim, ctypes.byref(cfg), None)):
        _refused(L, L.mw_floatenv_create(*args), N.MW_EINVAL, "null argument")
    # a simulator that was never initialised: check_sim's refusal
    raw = ctypes.c_void_p()
    mc = N.MwConfig(1e-3, 1.0, 1, W, 0, 20)
    assert L.mw_create(ctypes.byref(mc), ctypes.byref(raw)) == N.MW_OK
    assert L.mw_floatenv_create(raw, ctypes.byref(cfg), ctypes.byref(env)) == N.MW_ESTATE
    assert not env.value
    L.mw_destroy(raw)
    cart = host_sim(N, L, "cartpole", 2)
    _refused(L, L.mw_floatenv_create(cart, ctypes.byref(cfg), ctypes.byref(env)), N.MW_EINVAL,
             "the floating-base env needs an articulated model on a floating base")
    L.mw_destroy(cart)
    ball = host_sim(N, L, FLOATING_BALL_SDF, 2)
    _refused(L, L.mw_floatenv_create(ball, ctypes.byref(cfg), ctypes.byref(env)), N.MW_EINVAL,
             "does not take models with ball joints (joint 'shoulder#x')")
    L.mw_destroy(ball)
    long_run = _Rig(N, L, steps_per_run=65)
    _refused(L, long_run.create(), N.MW_EINVAL, "steps_per_run must be <= 64")
    long_run.close()
    for kw, fragment in (
            (dict(action_mode=2), "unknown action mode"),
            (dict(action_mode=-1), "unknown action mode"),
            (dict(max_episode_steps=-1), "max_episode_steps must be >= 0"),
            (dict(world_offset=-1), "world_offset must be >= 0"),
            (dict(home_q=None), "home_q is null (one value per dof)"),
            (dict(n_contact_links=-1), "n_contact_links must be in [0, 8]"),
            (dict(n_contact_links=9), "n_contact_links must be in [0, 8]"),
            (dict(contact_links=None), "contact_links is null"),
            (dict(contact_links=_ip([1, 3, -2, 7])[1]), "contact link -2 out of range [-1, 8)"),
            (dict(contact_links=_ip([1, 3, 5, 8])[1]), "contact link 8 out of range [-1, 8)"),
            (dict(home_base=(ctypes.c_float * 7)(0, 0, 0.45, 0, 0, 0, 0)), "home_base orientation quaternion is zero"),
            (dict(home_base=(ctypes.c_float * 7)(0, 0, 0.45, NAN, 0, 0, 0)),
             "home_base orientation quaternion is zero"),
            (dict(joint_noise=-0.1), "joint_noise must be >= 0"),
            (dict(joint_noise=NAN), "joint_noise must be >= 0")):
        _refused(L, rig.create(**kw), N.MW_EINVAL, fragment)
    # which refusal a doubly wrong config gets: the first check in the call's order
    _refused(L, rig.create(action_mode=5, joint_noise=-1.0), N.MW_EINVAL, "unknown action mode")
    # the refused calls left the simulator free: a host setter of the commands works, and so does a good create
    assert L.mw_set_joint_control_mode(rig.sim, 0, W, None, 0, N.MODE_FORCE) == N.MW_OK, L.mw_last_error()
    assert rig.create() == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 13 + 2 * NDOF + len(FEET)
    second = ctypes.c_void_p()
    _refused(L, L.mw_floatenv_create(rig.sim, ctypes.byref(cfg), ctypes.byref(second)), N.MW_ESTATE,
             "the simulator already has a floating-base env")
    assert not second.value


def _configure_calls(N, L, env):
    """name -> a call with a good config on `env`, for the refusals every configure call opens with."""
    rc = N.MwFloatRandConfig(0, 1, 0.0, 0.0, 0.5, 1.0)
    lc = _loco(N)
    ic = N.MwFloatInertiaConfig(0.8, 1.2, 0.0, 0.0, (ctypes.c_float * 3)(0, 0, 0))
    jc = N.MwFloatJointConfig(0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0)
    nc = N.MwFloatNoiseConfig(0, 2)
    sc, keep = _shape(N, {TORQUE: 1e-4})
    return {
        "mw_floatenv_randomize": lambda e=env, c=ctypes.byref(rc): L.mw_floatenv_randomize(e, c, None, None),
        "mw_floatenv_locomotion": lambda e=env, c=ctypes.byref(lc): L.mw_floatenv_locomotion(e, c, None),
        "mw_floatenv_inertia": lambda e=env, c=ctypes.byref(ic): L.mw_floatenv_inertia(e, c, None, None),
        "mw_floatenv_joints": lambda e=env, c=ctypes.byref(jc): L.mw_floatenv_joints(e, c, None, None),
        "mw_floatenv_noise": lambda e=env, c=ctypes.byref(nc): L.mw_floatenv_noise(e, c, None, None, None, None),
        "mw_floatenv_shaping": lambda e=env, c=ctypes.byref(sc), keep=keep: L.mw_floatenv_shaping(
            e, c, None, None, None, None, None),
    }, (rc, lc, ic, jc, nc, sc)


def test_every_configure_call_opens_with_the_same_three_refusals(N, host, rig):
    L = host
    # null env, null config
    calls, _ = _configure_calls(N, L, None)
    for name, call in calls.items():
        _refused(L, call(), N.MW_EINVAL, "null argument")
    assert rig.create() == N.MW_OK
    for name, call in _configure_calls(N, L, rig.env)[0].items():
        _refused(L, call(c=None), N.MW_EINVAL, "null argument")
    # an env of the fixed-base tasks
    cart = host_sim(N, L, "cartpole", 2)
    tc = N.MwTaskConfig(N.TASK_CARTPOLE_DISCRETE, 200, 0, 0, 7, 0, 0.0, 0.0, 0.0, 0.0, 0)
    fixed = ctypes.c_void_p()
    assert L.mw_vecenv_create(cart, ctypes.byref(tc), ctypes.byref(fixed)) == N.MW_OK, L.mw_last_error()
    calls, _ = _configure_calls(N, L, fixed)
    for name, call in calls.items():
        _refused(L, call(), N.MW_ESTATE, f"{name} needs an env made by mw_floatenv_create")
    L.mw_vecenv_destroy(fixed)
    L.mw_destroy(cart)
    # everything after the first reset; before it the same calls are taken (locomotion ahead of noise)
    calls, _ = _configure_calls(N, L, rig.env)
    order = ["mw_floatenv_locomotion"] + [name for name in calls if name != "mw_floatenv_locomotion"]
    for name in order:
        assert calls[name]() == N.MW_OK, (name, L.mw_last_error())
    dim = rig.obs_dim()
    assert dim == 25 + 3 * NDOF + len(FEET)
    assert rig.reset() == N.MW_OK, L.mw_last_error()
    for name in order:
        _refused(L, calls[name](), N.MW_ESTATE, f"{name} must be called before the first mw_vecenv_reset")
    assert rig.obs_dim() == dim


def test_randomize_refusals(N, host, rig):
    L = host
    assert rig.create() == N.MW_OK
    R = N.MwFloatRandConfig
    for cfg, fragment in (
            (R(-1, 1, 0.0, 0.0, 0.0, 0.0), "push_interval must be >= 0"),
            (R(10, 0, 1.0, 0.0, 0.0, 0.0), "push_steps must be in [1, push_interval]"),
            (R(10, 11, 1.0, 0.0, 0.0, 0.0), "push_steps must be in [1, push_interval]"),
            (R(10, 2, -1.0, 0.0, 0.0, 0.0), "push_force and push_torque must be >= 0"),
            (R(10, 2, 1.0, NAN, 0.0, 0.0), "push_force and push_torque must be >= 0"),
            (R(0, 1, 0.0, 0.0, -0.1, 1.0), "the friction range needs 0 <= friction_lo <= friction_hi"),
            (R(0, 1, 0.0, 0.0, 0.8, 0.5), "the friction range needs 0 <= friction_lo <= friction_hi"),
            (R(0, 1, 0.0, 0.0, 0.5, NAN), "the friction range needs 0 <= friction_lo <= friction_hi"),
            # doubly wrong: the push checks come first
            (R(-1, 1, 0.0, 0.0, 0.8, 0.5), "push_interval must be >= 0")):
        _refused(L, L.mw_floatenv_randomize(rig.env, ctypes.byref(cfg), None, None), N.MW_EINVAL, fragment)
    # the refused calls took neither the wrench buffer nor the friction: the simulator's setters work
    mu = np.full(W, 0.7)
    assert L.mw_set_ground_friction(rig.sim, 0, W, N.dptr(mu)) == N.MW_OK, L.mw_last_error()
    good = R(10, 2, 5.0, 1.0, 0.5, 1.0)
    assert L.mw_floatenv_randomize(rig.env, ctypes.byref(good), None, None) == N.MW_OK, L.mw_last_error()
    _refused(L, L.mw_set_ground_friction(rig.sim, 0, W, N.dptr(mu)), N.MW_ESTATE, "friction randomisation")
    # a second call replaces the first: friction off hands the array back
    off = R(0, 1, 0.0, 0.0, 0.0, 0.0)
    assert L.mw_floatenv_randomize(rig.env, ctypes.byref(off), None, None) == N.MW_OK
    assert L.mw_set_ground_friction(rig.sim, 0, W, N.dptr(mu)) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 13 + 2 * NDOF + len(FEET)


def test_locomotion_refusals_and_order(N, host, rig):
    L = host
    assert rig.create() == N.MW_OK
    forward = rig.obs_dim()
    bad = [(_loco(N, **{name: value}), "every field of mw_float_loco_config must be finite")
           for name, value in (("cmd_zero_prob", NAN), ("cmd_min", INF), ("action_scale", NAN), ("w_track_lin", INF),
                               ("w_track_yaw", NAN), ("track_sigma", INF), ("w_lin_z", NAN), ("w_ang_xy", NAN),
                               ("w_action_rate", -INF), ("w_air_time", NAN), ("air_time_target", NAN),
                               ("contact_force_min", INF), ("cmd_lo", (NAN, 0, 0)), ("cmd_hi", (1, INF, 1)))]
    bad += [(_loco(N, cmd_lo=(0.5, 0, 0), cmd_hi=(0.4, 0, 0)), "the command ranges need cmd_lo <= cmd_hi"),
            (_loco(N, cmd_lo=(0, 0, 0.1), cmd_hi=(0, 0, 0.0)), "the command ranges need cmd_lo <= cmd_hi"),
            (_loco(N, cmd_interval=-1), "cmd_interval must be >= 0"),
            (_loco(N, cmd_zero_prob=-0.1), "cmd_zero_prob must be in [0, 1]"),
            (_loco(N, cmd_zero_prob=1.5), "cmd_zero_prob must be in [0, 1]"),
            (_loco(N, track_sigma=0.0), "track_sigma must be > 0"),
            (_loco(N, track_sigma=-1.0), "track_sigma must be > 0"),
            (_loco(N, action_scale=-0.5), "action_scale must be >= 0"),
            # doubly wrong: the finite test comes first, then the ranges
            (_loco(N, cmd_interval=-1, w_lin_z=NAN), "every field of mw_float_loco_config must be finite"),
            (_loco(N, cmd_interval=-1, cmd_lo=(2, 0, 0)), "the command ranges need cmd_lo <= cmd_hi")]
    for cfg, fragment in bad:
        _refused(L, L.mw_floatenv_locomotion(rig.env, ctypes.byref(cfg), None), N.MW_EINVAL, fragment)
        assert rig.obs_dim() == forward                      # a refused call leaves the rows as they were
    # locomotion after noise is refused, whichever half of the noise call is on
    amp = np.zeros(forward, np.float32)
    amp[:3] = 0.01
    good = _loco(N)
    for nc, a in ((N.MwFloatNoiseConfig(0, 0), fp(amp)), (N.MwFloatNoiseConfig(1, 3), None)):
        assert L.mw_floatenv_noise(rig.env, ctypes.byref(nc), a, None, None, None) == N.MW_OK, L.mw_last_error()
        _refused(L, L.mw_floatenv_locomotion(rig.env, ctypes.byref(good), None), N.MW_ESTATE,
                 "mw_floatenv_locomotion must be called before mw_floatenv_noise")
        assert rig.obs_dim() == forward
    # noise off again: the call is taken
    none = N.MwFloatNoiseConfig(0, 0)
    assert L.mw_floatenv_noise(rig.env, ctypes.byref(none), None, None, None, None) == N.MW_OK
    assert L.mw_floatenv_locomotion(rig.env, ctypes.byref(good), None) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 25 + 3 * NDOF + len(FEET)


def test_air_time_needs_contact_links(N, host, rig):
    L = host
    assert rig.create(n_contact_links=0, contact_links=None) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 13 + 2 * NDOF
    cfg = _loco(N, w_air_time=1.0)
    _refused(L, L.mw_floatenv_locomotion(rig.env, ctypes.byref(cfg), None), N.MW_EINVAL,
             "the air-time term (w_air_time != 0) needs contact links")
    assert rig.obs_dim() == 13 + 2 * NDOF
    cfg = _loco(N)
    assert L.mw_floatenv_locomotion(rig.env, ctypes.byref(cfg), None) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 25 + 3 * NDOF
    # without contact links the stumble and contact_force terms have nothing to read
    for term in (STUMBLE, CONTACT_FORCE):
        sc, keep = _shape(N, {term: 1.0})
        _refused(L, L.mw_floatenv_shaping(rig.env, ctypes.byref(sc), None, None, None, None, None), N.MW_EINVAL,
                 "the stumble and contact_force terms need contact links (mw_float_task_config)")


def test_inertia_refusals_and_everything_off(N, host, rig):
    L = host
    assert rig.create() == N.MW_OK

    def I(slo, shi, plo, phi, box=(0, 0, 0)):
        return N.MwFloatInertiaConfig(slo, shi, plo, phi, (ctypes.c_float * 3)(*box))
    scale_msg = "the mass scale range needs 0 < mass_scale_lo <= mass_scale_hi (or both 0: off)"
    payload_msg = "the payload range needs 0 <= payload_lo <= payload_hi"
    finite_msg = "every field of mw_float_inertia_config must be finite"
    for cfg, fragment in (
            (I(NAN, 1.2, 0, 0), finite_msg), (I(0.8, INF, 0, 0), finite_msg), (I(0, 0, NAN, 1), finite_msg),
            (I(0, 0, 0, INF), finite_msg), (I(0.8, 1.2, 0, 0, (0, NAN, 0)), finite_msg),
            (I(0.0, 1.2, 0, 0), scale_msg), (I(-0.5, 1.2, 0, 0), scale_msg), (I(1.5, 1.2, 0, 0), scale_msg),
            (I(0.5, 0.0, 0, 0), scale_msg), (I(0.0, -1.0, 0, 0), scale_msg),
            (I(0.8, 1.2, -0.5, 1.0), payload_msg), (I(0.8, 1.2, 2.0, 1.0), payload_msg),
            (I(0.8, 1.2, 0, 1.0, (0.1, -0.1, 0.1)), "payload_box must be >= 0"),
            # doubly wrong: the scale range before the payload range before the box
            (I(1.5, 1.2, 2.0, 1.0, (-1, 0, 0)), scale_msg), (I(0.8, 1.2, 2.0, 1.0, (-1, 0, 0)), payload_msg)):
        _refused(L, L.mw_floatenv_inertia(rig.env, ctypes.byref(cfg), None, None), N.MW_EINVAL, fragment)
    # the refused calls left the records with the simulator
    words = np.zeros((1, 10), np.float32)
    assert L.mw_link_params(rig.sim, 0, 1, 2, fp(words)) == N.MW_OK
    assert L.mw_set_link_params(rig.sim, 0, 1, 2, fp(words)) == N.MW_OK, L.mw_last_error()
    # everything off on an env that never had the feature: nothing happens
    off = I(0, 0, 0, 0)
    assert L.mw_floatenv_inertia(rig.env, ctypes.byref(off), None, None) == N.MW_OK
    assert L.mw_set_link_params(rig.sim, 0, 1, 2, fp(words)) == N.MW_OK
    # on: the env owns the records; off again: the env as it was made
    for on in (I(0.8, 1.2, 0, 0), I(0, 0, 0.5, 2.0, (0.1, 0.1, 0.05))):
        assert L.mw_floatenv_inertia(rig.env, ctypes.byref(on), None, None) == N.MW_OK, L.mw_last_error()
        _refused(L, L.mw_set_link_params(rig.sim, 0, 1, 2, fp(words)), N.MW_ESTATE, "inertia randomisation")
        assert L.mw_floatenv_inertia(rig.env, ctypes.byref(off), None, None) == N.MW_OK
        assert L.mw_set_link_params(rig.sim, 0, 1, 2, fp(words)) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 13 + 2 * NDOF + len(FEET)


def test_joints_refusals_and_everything_off(N, host, rig):
    L = host
    assert rig.create() == N.MW_OK
    J = N.MwFloatJointConfig
    finite_msg = "every field of mw_float_joint_config must be finite"
    damping_msg = "the damping range needs 0 <= damping_lo <= damping_hi"
    friction_msg = "the joint friction range needs 0 <= friction_lo <= friction_hi"
    effort_msg = "the effort scale range needs 0 < effort_scale_lo <= effort_scale_hi (or both 0: off)"
    for cfg, fragment in (
            (J(0, NAN, 0, 0, 0, 0, 0), finite_msg), (J(0, 0, 0, INF, 0, 0, 0), finite_msg),
            (J(0, 0, 0, 0, NAN, 1.0, 0), finite_msg),
            (J(-0.1, 0.5, 0, 0, 0, 0, 0), damping_msg), (J(0.6, 0.5, 0, 0, 0, 0, 0), damping_msg),
            (J(0, 0, -1.0, 2.0, 0, 0, 0), friction_msg), (J(0, 0, 2.0, 1.0, 0, 0, 0), friction_msg),
            (J(0, 0, 0, 0, 0.0, 1.0, 0), effort_msg), (J(0, 0, 0, 0, 1.5, 1.0, 0), effort_msg),
            (J(0, 0, 0, 0, -0.5, 1.0, 0), effort_msg), (J(0, 0, 0, 0, 0.5, 0.0, 0), effort_msg),
            (J(0, 0, 0, 0, 0, -1.0, 0), effort_msg),
            (J(0, 0.5, 0, 0, 0, 0, 1 << NDOF), "dof_mask names a joint the model does not have"),
            # doubly wrong: damping before friction before effort before the mask
            (J(0.6, 0.5, 2.0, 1.0, 0, 0, 0), damping_msg), (J(0, 0.5, 2.0, 1.0, 1.5, 1.0, 0), friction_msg),
            (J(0, 0.5, 0, 0, 1.5, 1.0, 1 << NDOF), effort_msg)):
        _refused(L, L.mw_floatenv_joints(rig.env, ctypes.byref(cfg), None, None), N.MW_EINVAL, fragment)
    words = np.float32([[0.1, 0.2, 30.0]])
    assert L.mw_set_joint_dynamics(rig.sim, 0, 1, 0, fp(words)) == N.MW_OK, L.mw_last_error()
    off = J(0, 0, 0, 0, 0, 0, 0)
    assert L.mw_floatenv_joints(rig.env, ctypes.byref(off), None, None) == N.MW_OK      # never on: nothing happens
    assert L.mw_set_joint_dynamics(rig.sim, 0, 1, 0, fp(words)) == N.MW_OK
    on = J(0.0, 0.5, 0.0, 2.0, 0.5, 1.0, 0b00110011)
    assert L.mw_floatenv_joints(rig.env, ctypes.byref(on), None, None) == N.MW_OK, L.mw_last_error()
    _refused(L, L.mw_set_joint_dynamics(rig.sim, 0, 1, 0, fp(words)), N.MW_ESTATE, "joint randomisation owns")
    assert L.mw_floatenv_joints(rig.env, ctypes.byref(off), None, None) == N.MW_OK
    assert L.mw_set_joint_dynamics(rig.sim, 0, 1, 0, fp(words)) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 13 + 2 * NDOF + len(FEET)


def test_noise_refusals(N, host, rig):
    L = host
    assert rig.create() == N.MW_OK
    lc = _loco(N)
    assert L.mw_floatenv_locomotion(rig.env, ctypes.byref(lc), None) == N.MW_OK
    dim = rig.obs_dim()
    C = N.MwFloatNoiseConfig
    for cfg in (C(-1, 2), C(3, 2), C(0, N.FLOAT_MAX_ACTION_DELAY + 1)):
        _refused(L, L.mw_floatenv_noise(rig.env, ctypes.byref(cfg), None, None, None, None), N.MW_EINVAL,
                 "the action delay range needs 0 <= delay_lo <= delay_hi <= 8")
    ok = C(0, 0)
    exact0 = dim - 3 - NDOF                                   # the command and the last action end the rows
    for k, value, fragment in (
            (2, -0.1, "every noise amplitude must be finite and >= 0 (word 2)"),
            (5, NAN, "every noise amplitude must be finite and >= 0 (word 5)"),
            (exact0 - 1, INF, f"every noise amplitude must be finite and >= 0 (word {exact0 - 1})"),
            (exact0, 0.01, f"the command and last-action words take no noise (word {exact0})"),
            (dim - 1, 0.01, f"the command and last-action words take no noise (word {dim - 1})")):
        amp = np.zeros(dim, np.float32)
        amp[k] = value
        _refused(L, L.mw_floatenv_noise(rig.env, ctypes.byref(ok), fp(amp), None, None, None), N.MW_EINVAL, fragment)
    # doubly wrong: the delay range before the amplitudes, a lower word before a higher one
    amp = np.zeros(dim, np.float32)
    amp[1], amp[exact0] = -1.0, 0.5
    _refused(L, L.mw_floatenv_noise(rig.env, ctypes.byref(C(3, 2)), fp(amp), None, None, None), N.MW_EINVAL,
             "the action delay range")
    _refused(L, L.mw_floatenv_noise(rig.env, ctypes.byref(ok), fp(amp), None, None, None), N.MW_EINVAL, "(word 1)")
    assert rig.obs_dim() == dim
    # the last noisy word takes an amplitude; a good call after the refused ones
    amp = np.zeros(dim, np.float32)
    amp[exact0 - 1] = 0.02
    assert L.mw_floatenv_noise(rig.env, ctypes.byref(C(1, N.FLOAT_MAX_ACTION_DELAY)), fp(amp), None, None,
                               None) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == dim
    # in the forward task every word may be noisy
    other = _Rig(N, L)
    assert other.create() == N.MW_OK
    amp = np.full(other.obs_dim(), 0.01, np.float32)
    assert L.mw_floatenv_noise(other.env, ctypes.byref(ok), fp(amp), None, None, None) == N.MW_OK, L.mw_last_error()
    other.close()


def test_shaping_refusals_and_everything_off(N, host, rig):
    L = host
    assert rig.create() == N.MW_OK
    dim = rig.obs_dim()

    def call(cfg_keep):
        return L.mw_floatenv_shaping(rig.env, ctypes.byref(cfg_keep[0]), None, None, None, None, None)
    finite_msg = "every field of mw_float_shape_config must be finite"
    nonneg_msg = "collision_force_min, stumble_ratio, max_contact_force and termination_force must be >= 0"
    null_msg = "a link list of mw_float_shape_config is null"
    feet, feet_p = _ip(FEET)
    cases = [
        (_shape(N, {3: NAN}), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: INF}), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: -1e-4}), N.MW_EINVAL, "the weights of mw_float_shape_config must be >= 0"),
        (_shape(N, {TORQUE: 1.0}, base_height_target=NAN), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: 1.0}, soft_limit=INF), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: 1.0}, collision_force_min=NAN), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: 1.0}, stumble_ratio=NAN), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: 1.0}, max_contact_force=INF), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: 1.0}, termination_force=NAN), N.MW_EINVAL, finite_msg),
        (_shape(N, {TORQUE: 1.0}, n_penalised_links=-1), N.MW_EINVAL, "n_penalised_links must be in [0, 8]"),
        (_shape(N, {TORQUE: 1.0}, n_penalised_links=9, penalised_links=feet_p), N.MW_EINVAL,
         "n_penalised_links must be in [0, 8]"),
        (_shape(N, {TORQUE: 1.0}, n_termination_links=-1), N.MW_EINVAL, "n_termination_links must be >= 0"),
        (_shape(N, {TORQUE: 1.0}, n_penalised_links=2), N.MW_EINVAL, null_msg),
        (_shape(N, {TORQUE: 1.0}, n_termination_links=1), N.MW_EINVAL, null_msg),
        (_shape(N, {TORQUE: 1.0}, soft_limit=0.0), N.MW_EINVAL, "soft_limit must be in (0, 1]"),
        (_shape(N, {TORQUE: 1.0}, soft_limit=1.5), N.MW_EINVAL, "soft_limit must be in (0, 1]"),
        (_shape(N, {TORQUE: 1.0}, collision_force_min=-0.1), N.MW_EINVAL, nonneg_msg),
        (_shape(N, {TORQUE: 1.0}, stumble_ratio=-1.0), N.MW_EINVAL, nonneg_msg),
        (_shape(N, {TORQUE: 1.0}, max_contact_force=-1.0), N.MW_EINVAL, nonneg_msg),
        (_shape(N, {TORQUE: 1.0}, termination_force=-1.0), N.MW_EINVAL, nonneg_msg),
        # stand_still without locomotion: an order rule, so MW_ESTATE
        (_shape(N, {STAND_STILL: 1.0}), N.MW_ESTATE,
         "the stand_still term needs the locomotion task: call mw_floatenv_locomotion first"),
        (_shape(N, {COLLISION: 1.0}), N.MW_EINVAL, "the collision term needs penalised links"),
        (_shape(N, pen=[-2]), N.MW_EINVAL, "penalised link -2 out of range [-1, 8)"),
        (_shape(N, pen=[1, NDOF]), N.MW_EINVAL, "penalised link 8 out of range [-1, 8)"),
        (_shape(N, term=[-1, -3]), N.MW_EINVAL, "termination link -3 out of range [-1, 8)"),
        (_shape(N, term=[NDOF]), N.MW_EINVAL, "termination link 8 out of range [-1, 8)"),
        (_shape(N, pen=[THIGH]), N.MW_EINVAL,
         "penalised link 0 owns no contact slot among the 32 of the contact mask (no collision shape?)"),
        (_shape(N, term=[-1, THIGH + 2]), N.MW_EINVAL, "termination link 2 owns no contact slot among the 32"),
        # doubly wrong: the weights before the scalars before the lists before the ranges before the links
        (_shape(N, {TORQUE: -1.0}, soft_limit=NAN), N.MW_EINVAL, "the weights of mw_float_shape_config must be >= 0"),
        (_shape(N, {TORQUE: 1.0}, soft_limit=2.0, n_termination_links=-1), N.MW_EINVAL,
         "n_termination_links must be >= 0"),
        (_shape(N, {COLLISION: 1.0}, soft_limit=2.0), N.MW_EINVAL, "soft_limit must be in (0, 1]"),
        (_shape(N, {STAND_STILL: 1.0, COLLISION: 1.0}, pen=[THIGH]), N.MW_ESTATE, "the stand_still term needs"),
        (_shape(N, pen=[THIGH], term=[NDOF]), N.MW_EINVAL, "penalised link 0 owns no contact slot"),
    ]
    for cfg_keep, code, fragment in cases:
        _refused(L, call(cfg_keep), code, fragment)
        assert rig.obs_dim() == dim
    # everything off: taken, the env as it was made -- before the feature was ever on, and after
    all_off = _shape(N, base_height_target=0.0, soft_limit=0.0, collision_force_min=0.0, stumble_ratio=0.0,
                     max_contact_force=0.0, termination_force=0.0)
    assert call(all_off) == N.MW_OK, L.mw_last_error()
    on = _shape(N, {TORQUE: 1e-4, COLLISION: 1.0, STUMBLE: 0.5, CONTACT_FORCE: 0.01}, pen=[-1], term=[-1, 1])
    assert call(on) == N.MW_OK, L.mw_last_error()
    assert call(all_off) == N.MW_OK, L.mw_last_error()
    # with the locomotion task the stand_still term is taken
    lc = _loco(N)
    assert L.mw_floatenv_locomotion(rig.env, ctypes.byref(lc), None) == N.MW_OK
    assert call(_shape(N, {STAND_STILL: 1.0})) == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 25 + 3 * NDOF + len(FEET)
    # the envs step with the feature on (the effort word of the shared model, no per-world records)
    assert rig.reset() == N.MW_OK, L.mw_last_error()


def test_create_reset_step_destroy_and_hand_back(N, host, rig):
    """The life of an env with every feature on, in position mode; destroying it
    returns the commands, the friction and the link records to the simulator."""
    L = host
    assert rig.create(action_mode=N.FLOAT_ACTION_POSITION) == N.MW_OK, L.mw_last_error()
    calls, keep = _configure_calls(N, L, rig.env)
    for name in ["mw_floatenv_locomotion"] + [k for k in calls if k != "mw_floatenv_locomotion"]:
        assert calls[name]() == N.MW_OK, (name, L.mw_last_error())
    dim = rig.obs_dim()
    assert dim == 25 + 3 * NDOF + len(FEET)
    # what the env owns while it lives
    mu = np.full(W, 0.7)
    link = np.zeros((1, 10), np.float32)
    joint = np.float32([[0.1, 0.2, 30.0]])
    assert L.mw_link_params(rig.sim, 0, 1, 2, fp(link)) == N.MW_OK
    _refused(L, L.mw_set_joint_control_mode(rig.sim, 0, W, None, 0, N.MODE_FORCE), N.MW_ESTATE, "floating-base env")
    _refused(L, L.mw_set_ground_friction(rig.sim, 0, W, N.dptr(mu)), N.MW_ESTATE, "friction randomisation")
    _refused(L, L.mw_set_link_params(rig.sim, 0, 1, 2, fp(link)), N.MW_ESTATE, "randomisation")
    _refused(L, L.mw_set_joint_dynamics(rig.sim, 0, 1, 0, fp(joint)), N.MW_ESTATE, "joint randomisation owns")
    obs, tobs = np.zeros((W, dim), np.float32), np.zeros((W, dim), np.float32)
    act, rew, done = np.zeros((W, NDOF), np.float32), np.zeros(W, np.float32), np.zeros(W, np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    # null buffers are refused by reset and step alike
    _refused(L, L.mw_vecenv_reset(rig.env, None), N.MW_EINVAL, "null argument")
    assert L.mw_vecenv_reset(rig.env, vp(obs)) == N.MW_OK, L.mw_last_error()
    _refused(L, L.mw_vecenv_step(rig.env, vp(act), vp(obs), vp(rew), None, vp(tobs)), N.MW_EINVAL, "null argument")
    for _ in range(3):
        assert L.mw_vecenv_step(rig.env, vp(act), vp(obs), vp(rew), vp(done), vp(tobs)) == N.MW_OK, L.mw_last_error()
    _refused(L, L.mw_vecenv_rollout(rig.env, 4, vp(act), vp(obs), vp(rew), vp(done), vp(tobs)), N.MW_EINVAL,
             "the fused rollout is not available for floating-base envs")
    assert rig.obs_dim() == dim
    L.mw_vecenv_destroy(rig.env)
    rig.env = None
    L.mw_vecenv_destroy(None)                                  # a null handle is ignored
    # the simulator is no longer env-owned: the setters that were refused work again
    assert L.mw_set_joint_control_mode(rig.sim, 0, W, None, 0, N.MODE_FORCE) == N.MW_OK, L.mw_last_error()
    assert L.mw_set_ground_friction(rig.sim, 0, W, N.dptr(mu)) == N.MW_OK, L.mw_last_error()
    assert L.mw_set_link_params(rig.sim, 0, 1, 2, fp(link)) == N.MW_OK, L.mw_last_error()
    assert L.mw_set_joint_dynamics(rig.sim, 0, 1, 0, fp(joint)) == N.MW_OK, L.mw_last_error()
    got = np.zeros((1, 3), np.float32)
    assert L.mw_joint_dynamics(rig.sim, 0, 1, 0, fp(got)) == N.MW_OK
    np.testing.assert_array_equal(got, joint)
    # ... and it takes a new env
    assert rig.create() == N.MW_OK, L.mw_last_error()
    assert rig.obs_dim() == 13 + 2 * NDOF + len(FEET)
