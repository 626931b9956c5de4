"""Per-world link parameters of the simulator (mw_set_link_params /
mw_link_params: the WPAR instances of the world-per-wavefront kernel).

  * the mechanism changes nothing by itself: with the storage allocated and
    every world set to the words mw_link_params returned, a run ends bit-equal
    in mw_get_state to a simulator that never allocated it (70 quadrupeds in
    contact under random torques, 5 iCubs under position targets);
  * the parameters reach the right world: 9 quadruped worlds (more than the 8
    XCDs, not a multiple of them) with nine parameter sets, base and two leg
    links changed, end world by world bit-equal to nine one-world simulators
    given the same words;
  * ranges, the getter, the errors.
"""

import numpy as np
import pytest

from float_env_harness import _quadruped, _run_quadruped

pytestmark = pytest.mark.gpu


def _set_all_to_nominal(sim):
    """Allocate the per-world storage by setting every link of every world to
    the words the getter returned; returns them [n + 1, W, 10]."""
    words = np.stack([sim.link_params(link) for link in range(-1, sim.dofs)])
    for link in range(-1, sim.dofs):
        sim.set_link_params(link, words[link + 1])
        np.testing.assert_array_equal(sim.link_params(link), words[link + 1])
    return words


def test_nominal_words_change_no_bit_quadruped(require_gpu):
    W, steps = 70, 50
    torques = np.random.default_rng(41).uniform(-8, 8, (steps, W, 8))
    plain, par = _quadruped(W), _quadruped(W)
    words = _set_all_to_nominal(par)
    assert (words[:, :, 0] > 0).all() and np.array_equal(words[:, 0], words[:, -1])
    in_contact = []
    ref = _run_quadruped(plain, torques, watch=in_contact)
    np.testing.assert_array_equal(_run_quadruped(par, torques), ref)
    print(f"worlds in contact (of 3 watched) per step: {in_contact}")
    assert in_contact[0] == 3 and sum(c > 0 for c in in_contact) >= 10     # the runs are contact dynamics
    assert len({ref[w].tobytes() for w in range(W)}) == W                # every world went its own way
    # the getter of the simulator without storage returns the nominal words
    np.testing.assert_array_equal(np.stack([plain.link_params(link) for link in range(-1, 8)]), words)
    plain.close()
    par.close()


def test_nominal_words_change_no_bit_icub(require_gpu):
    """The <32> instance, PID position targets (effort and gains through the world's own body block)."""
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
    _set_all_to_nominal(par)
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
    n = plain.dofs
    assert np.abs(out[0][:, 3 * n:6 * n]).max() > 0                       # the PIDs worked
    assert len({out[0][w].tobytes() for w in range(W)}) == W
    for sim in sims:
        sim.close()


def _nine_sets(sim, rng):
    """Nine parameter sets for the base and two leg links (thigh of leg 0,
    shank of leg 2): mass scaled by U(0.5, 2), the centre of mass moved by up to
    3 cm, the inertia scaled with the mass -- physical bodies, float32 words."""
    links = [-1, 0, 5]
    sets = {}
    for link in links:
        nominal = sim.link_params(link, [0])[0].astype(np.float64)
        rows = []
        for _ in range(9):
            s = rng.uniform(0.5, 2.0)
            w = nominal.copy()
            w[0] *= s
            w[4:] *= s
            dc = rng.uniform(-0.03, 0.03, 3)
            c = w[1:4] + dc
            # origin inertia of the same body about its moved centre: Io - m shift(c0) + m shift(c)
            for cc, sign in ((w[1:4], -1.0), (c, 1.0)):
                c2 = cc @ cc
                w[4:7] += sign * w[0] * (c2 - cc * cc)
                w[7] -= sign * w[0] * cc[0] * cc[1]
                w[8] -= sign * w[0] * cc[0] * cc[2]
                w[9] -= sign * w[0] * cc[1] * cc[2]
            w[1:4] = c
            rows.append(w)
        sets[link] = np.float32(rows)
    return sets


def test_nine_worlds_are_nine_simulators(require_gpu):
    W, steps = 9, 50
    rng = np.random.default_rng(43)
    torques = rng.uniform(-8, 8, (steps, W, 8))
    many = _quadruped(W)
    sets = _nine_sets(many, rng)
    for link, words in sets.items():
        many.set_link_params(link, words)
        np.testing.assert_array_equal(many.link_params(link), words)        # exactly what was set
        np.testing.assert_array_equal(many.link_params(link, [4, 7]), words[[4, 7]])
    nominal = _quadruped(1)
    untouched = [l for l in range(-1, 8) if l not in sets]
    for link in untouched:
        np.testing.assert_array_equal(many.link_params(link), np.tile(nominal.link_params(link), (W, 1)))
    rec = _run_quadruped(many, torques)
    rec_nominal = _run_quadruped(nominal, torques, worlds=[0])
    assert not np.array_equal(rec[0], rec_nominal[0])                        # the parameters moved the robot
    nominal.close()
    for w in range(W):
        one = _quadruped(1)
        for link, words in sets.items():
            one.set_link_params(link, words[w])
        np.testing.assert_array_equal(_run_quadruped(one, torques, worlds=[w])[0], rec[w], err_msg=f"world {w}")
        one.close()
    assert len({rec[w].tobytes() for w in range(W)}) == W
    many.close()


def test_ranged_set_and_errors(require_gpu):
    from mwstep import get_model_file
    from mwstep.sim import Simulator
    sim = _quadruped(9)
    nominal = sim.link_params("thigh_fl")
    np.testing.assert_array_equal(nominal, sim.link_params(sim.link_names.index("thigh_fl")))
    assert sim.link_index(sim.base_frame) == -1
    new = nominal[3:7].copy()
    new[:, 0] *= np.float32([1.5, 0.5, 2.0, 0.75])
    sim.set_link_params("thigh_fl", new, worlds=range(3, 7))                 # w0 = 3, nw = 4
    got = sim.link_params("thigh_fl")
    np.testing.assert_array_equal(got[3:7], new)
    np.testing.assert_array_equal(got[[0, 1, 2, 7, 8]], nominal[[0, 1, 2, 7, 8]])
    np.testing.assert_array_equal(sim.link_params(-1), np.tile(sim.link_params(-1, [0]), (9, 1)))
    # set_link_inertial: the fp64 parallel-axis shift, rounded once
    sim.set_link_inertial(-1, 9.0, [0.01, 0.0, 0.02], np.diag([0.2, 0.3, 0.4]), worlds=[8])
    want = Simulator.inertial_words(9.0, [0.01, 0.0, 0.02], np.diag([0.2, 0.3, 0.4]))
    np.testing.assert_array_equal(sim.link_params(-1, [8])[0], want)
    before = np.stack([sim.link_params(l) for l in range(-1, 8)])
    bad = nominal[:1].copy()
    for k, value, msg in ((0, 0.0, "mass must be > 0"), (0, -1.0, "mass must be > 0"),
                          (0, np.nan, "must be finite"), (5, np.inf, "must be finite")):
        w = bad.copy()
        w[0, k] = value
        with pytest.raises(RuntimeError, match=msg):
            sim.set_link_params(0, w, worlds=[2])
    with pytest.raises(RuntimeError, match="world range out of bounds"):
        sim.set_link_params(0, nominal[:2], worlds=[8, 9])
    for link in (-2, 8):
        with pytest.raises(RuntimeError, match="out of range"):
            sim.set_link_params(link, nominal[:1], worlds=[0])
        with pytest.raises(RuntimeError, match="out of range"):
            sim.link_params(link)
    with pytest.raises(ValueError, match="not found"):
        sim.link_params("no_such_link")
    np.testing.assert_array_equal(np.stack([sim.link_params(l) for l in range(-1, 8)]), before)
    # parameters, not state: a state record written back leaves them alone
    sim.run()
    sim.set_state(sim.get_state())
    np.testing.assert_array_equal(np.stack([sim.link_params(l) for l in range(-1, 8)]), before)
    sim.close()
    # a fixed-base chain is not on the world-per-wavefront kernel
    cart = Simulator(get_model_file("cartpole"), n_worlds=2)
    with pytest.raises(RuntimeError, match="need the world-per-wavefront kernel"):
        cart.set_link_params(0, nominal[:1])
    with pytest.raises(RuntimeError, match="need the world-per-wavefront kernel"):
        cart.link_params(0)
    cart.close()


def test_joint_setters_reach_every_copy(require_gpu):
    """A setter of the shared model before the first run (here the effort limit)
    rewrites every world's copy of the body block and keeps its inertial words."""
    from mwstep import native as N
    W = 3
    torques = np.full((20, W, 8), 30.0)
    a, b = _quadruped(W), _quadruped(W)
    words = b.link_params(0)
    words[:, 0] *= np.float32([1.0, 1.5, 0.7])
    b.set_link_params(0, words)
    a.set_joint_param(1, N.PARAM_MAX_GENERALIZED_FORCE, 5.0)
    a.set_link_params(0, words)                      # a: limit first, then the storage
    b.set_joint_param(1, N.PARAM_MAX_GENERALIZED_FORCE, 5.0)   # b: the storage exists already
    np.testing.assert_array_equal(b.link_params(0), words)
    np.testing.assert_array_equal(_run_quadruped(b, torques), _run_quadruped(a, torques))
    a.close()
    b.close()
