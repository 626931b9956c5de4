"""Per-world joint dynamics of the simulator (mw_set_joint_dynamics /
mw_joint_dynamics: damping, friction and effort limit in the per-world records
the WPAR instances of the world-per-wavefront kernel read).

  * the mechanism changes nothing by itself: with the storage allocated and
    every joint of every world set to the words mw_joint_dynamics returned, a
    run ends bit-equal in mw_get_state to a simulator that never allocated it
    (70 quadrupeds in contact under random torques, 5 iCubs under position
    targets);
  * the parameters reach the right world: 9 quadruped worlds with nine
    parameter sets end world by world bit-equal to nine one-world simulators
    configured through mw_set_joint_param;
  * the instance choice: the same comparison on a floating two-body model whose
    nominal flags select the kernel's instance without joint constraint rows --
    friction given per world only must still act;
  * the shared setter after a per-world set overwrites that word in every
    world and keeps the others."""

import numpy as np
import pytest

from float_env_harness import _quadruped, _run_quadruped
from float_joints_ref import FLT_MAX, write_two_body

pytestmark = pytest.mark.gpu


def _set_all_to_nominal(sim):
    """Allocate the per-world storage by setting every joint of every world to
    the words the getter returned; returns them [n, W, 3]."""
    words = np.stack([sim.joint_dynamics(d) for d in range(sim.dofs)])
    for d in range(sim.dofs):
        sim.set_joint_dynamics(d, words[d])
        np.testing.assert_array_equal(sim.joint_dynamics(d), words[d])
    return words


def test_nominal_words_change_no_bit_quadruped(require_gpu):
    W, steps = 70, 50
    torques = np.random.default_rng(41).uniform(-8, 8, (steps, W, 8))
    plain, par = _quadruped(W), _quadruped(W)
    words = _set_all_to_nominal(par)
    np.testing.assert_array_equal(words, np.tile(np.float32([0.0, 0.0, 60.0]), (8, W, 1)))
    in_contact = []
    ref = _run_quadruped(plain, torques, watch=in_contact)
    np.testing.assert_array_equal(_run_quadruped(par, torques), ref)
    assert in_contact[0] == 3 and sum(c > 0 for c in in_contact) >= 10     # the runs are contact dynamics
    assert len({ref[w].tobytes() for w in range(W)}) == W                # every world went its own way
    # the getter of the simulator without storage returns the nominal words
    np.testing.assert_array_equal(np.stack([plain.joint_dynamics(d) for d in range(8)]), words)
    plain.close()
    par.close()


def test_nominal_words_change_no_bit_icub(require_gpu):
    """The <32> instance, PID position targets (the effort clip through the world's own body block)."""
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.models import ICUB_POSE, icub_pid_gains, icub_posture
    from mwstep.sim import Simulator
    W, steps = 5, 30
    sims = []
    for _ in range(2):
        sim = Simulator(get_model_file("icub"), n_worlds=W, pgs_iters=50, pose=ICUB_POSE)
        sim.set_ground_plane(True, 1.0)
        sim.enable_contacts(True)
        sim.set_controller_period(1e-3)
        for d, (p, dd) in enumerate(icub_pid_gains(sim.joint_names)):
            sim.set_pid(d, [p, 0.0, dd, -80.0, 80.0, 0.0, 0.0, -1.0])
        sim.set_control_mode(N.MODE_POSITION)
        sims.append(sim)
    plain, par = sims
    words = _set_all_to_nominal(par)
    assert (words[:, :, 2] > 0).all() and np.array_equal(words[:, 0], words[:, -1])
    q0 = np.array(icub_posture(plain.joint_names))
    targets = q0 + np.random.default_rng(42).uniform(-0.15, 0.15, (steps, W, plain.dofs))
    out = []
    for sim in sims:
        sim.set("reset_q", np.tile(q0, (W, 1)))
        sim.run(paused=True)
        for t in targets:
            sim.set("position_target", t)
            sim.run()
        out.append(sim.get_state())
    np.testing.assert_array_equal(out[1], out[0])
    assert len({out[0][w].tobytes() for w in range(W)}) == W
    for sim in sims:
        sim.close()


def _configure_one(sim, dofs, words):
    """A one-world simulator given one world's words [len(dofs), 3] through the shared setters."""
    from mwstep import native as N
    for k, d in enumerate(dofs):
        sim.set_joint_param(d, N.PARAM_VISCOUS_FRICTION, float(words[k, 0]))
        sim.set_joint_param(d, N.PARAM_COULOMB_FRICTION, float(words[k, 1]))
        if words[k, 2] != FLT_MAX:
            sim.set_joint_param(d, N.PARAM_MAX_GENERALIZED_FORCE, float(words[k, 2]))


def test_nine_worlds_are_nine_simulators(require_gpu):
    """Hip of leg 0, knee of leg 1, hip of leg 3: damping, friction and an
    effort limit below the torques, nine sets (more worlds than the 8 XCDs)."""
    W, steps = 9, 50
    rng = np.random.default_rng(47)
    torques = rng.uniform(-20, 20, (steps, W, 8))
    dofs = [0, 3, 6]
    sets = np.stack([rng.uniform(0.05, 0.5, (W, 3)), rng.uniform(0.1, 2.0, (W, 3)), rng.uniform(6.0, 30.0, (W, 3))],
                    axis=2).astype(np.float32)                        # [W, dof, 3]
    many = _quadruped(W)
    for k, d in enumerate(dofs):
        many.set_joint_dynamics(d, sets[:, k])
        np.testing.assert_array_equal(many.joint_dynamics(d), sets[:, k])        # exactly what was set
        np.testing.assert_array_equal(many.joint_dynamics(d, [4, 7]), sets[[4, 7], k])
    nominal = _quadruped(1)
    for d in (1, 2, 4, 5, 7):
        np.testing.assert_array_equal(many.joint_dynamics(d), np.tile(nominal.joint_dynamics(d), (W, 1)))
    rec = _run_quadruped(many, torques)
    rec_nominal = _run_quadruped(nominal, torques, worlds=[0])
    assert not np.array_equal(rec[0], rec_nominal[0])                        # the parameters moved the robot
    nominal.close()
    assert many.constraint_overflow() == 0
    for w in range(W):
        one = _quadruped(1)
        _configure_one(one, dofs, sets[w])
        np.testing.assert_array_equal(_run_quadruped(one, torques, worlds=[w])[0], rec[w], err_msg=f"world {w}")
        one.close()
    assert len({rec[w].tobytes() for w in range(W)}) == W
    many.close()


def _two_body(path, W):
    from mwstep import native as N
    from mwstep.sim import Simulator
    sim = Simulator(path, n_worlds=W, pose=(0, 0, 1.0, 1, 0, 0, 0))
    assert sim.float_kernel() == 2
    sim.set_control_mode(N.MODE_FORCE)
    return sim


def _run_two_body(sim, torques, qd0, worlds=None):
    W = sim.n_worlds
    sel = slice(None) if worlds is None else worlds
    sim.set("reset_q", np.zeros((W, 1)))
    sim.set("reset_qd", qd0[sel])
    sim.run(paused=True)
    for tau in torques:
        sim.set("force_target", tau[sel])
        sim.run()
    return sim.get_state()


def test_friction_given_per_world_only_still_acts(require_gpu, tmp_path):
    """The instance choice: the two-body model has one continuous joint, no
    limits and no <dynamics>, so its nominal flags select the instance without
    joint constraint rows.  Nine worlds with nine friction words (nothing else
    changed) must end bit-equal to nine simulators given the friction through
    mw_set_joint_param, and not where the frictionless model ends."""
    from mwstep import native as N
    path = write_two_body(tmp_path)
    W, steps = 9, 40
    rng = np.random.default_rng(53)
    torques = rng.uniform(-0.3, 0.3, (steps, W, 1))
    qd0 = rng.uniform(-2.0, 2.0, (W, 1))
    friction = rng.uniform(0.05, 0.5, W).astype(np.float32)
    many = _two_body(path, W)
    words = many.joint_dynamics(0)
    np.testing.assert_array_equal(words, np.tile(np.float32([0.0, 0.0, FLT_MAX]), (W, 1)))
    words[:, 1] = friction
    many.set_joint_dynamics(0, words)
    np.testing.assert_array_equal(many.joint_dynamics(0), words)
    rec = _run_two_body(many, torques, qd0)
    plain = _two_body(path, W)
    rec_plain = _run_two_body(plain, torques, qd0)
    plain.close()
    moved = [not np.array_equal(rec[w], rec_plain[w]) for w in range(W)]
    assert all(moved), moved                                             # friction acted in every world
    for w in range(W):
        one = _two_body(path, 1)
        one.set_joint_param(0, N.PARAM_COULOMB_FRICTION, float(friction[w]))
        np.testing.assert_array_equal(_run_two_body(one, torques, qd0, worlds=[w])[0], rec[w], err_msg=f"world {w}")
        one.close()
    many.close()


def test_shared_setter_overwrites_that_word_in_every_world(require_gpu):
    """mw_set_joint_param after a per-world set: the effort limit of dof 1 in
    every world, the per-world damping and friction of dofs 1 and 4 kept.  The
    run equals that of a simulator given the limit first and then the words."""
    from mwstep import native as N
    W = 3
    torques = np.full((20, W, 8), 30.0)
    words = np.float32([[0.1, 0.5, 40.0], [0.3, 1.5, 20.0], [0.0, 0.0, 60.0]])
    a, b = _quadruped(W), _quadruped(W)
    for d in (1, 4):
        a.set_joint_dynamics(d, words)
    a.set_joint_param(1, N.PARAM_MAX_GENERALIZED_FORCE, 5.0)     # a: the storage exists already
    want1 = words.copy()
    want1[:, 2] = 5.0
    np.testing.assert_array_equal(a.joint_dynamics(1), want1)
    np.testing.assert_array_equal(a.joint_dynamics(4), words)
    np.testing.assert_array_equal(a.joint_dynamics(2), np.tile(np.float32([0.0, 0.0, 60.0]), (W, 1)))
    b.set_joint_param(1, N.PARAM_MAX_GENERALIZED_FORCE, 5.0)     # b: the limit first, then the storage
    np.testing.assert_array_equal(b.joint_dynamics(1), np.tile(np.float32([0.0, 0.0, 5.0]), (W, 1)))
    b.set_joint_dynamics(1, want1)
    b.set_joint_dynamics(4, words)
    ra, rb = _run_quadruped(a, torques), _run_quadruped(b, torques)
    np.testing.assert_array_equal(ra, rb)
    assert len({ra[w].tobytes() for w in range(W)}) == W          # the kept words differ between the worlds
    a.close()
    b.close()
