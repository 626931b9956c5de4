"""Pin the fp64 floating-tree oracle (or_float_step) before trusting it (CPU).

The dense restatement (CRBA mass matrix + RNEA bias with a free root, dense
contact / joint rows) is checked against the parts already pinned:

  * its joint block and joint bias equal the fixed-base CRBA / RNEA of the
    same tree (or_crba / or_rnea, pinned by the reference's pendulum and
    cartpole KATs), and its base block is the composite rigid-body inertia;
  * heavy-base reduction: a base of 1e9 kg in zero gravity reproduces the
    fixed-base engine step (or_step) of the same tree, limits and all;
  * free fall: with no contacts every body falls with g and the joints see
    no gravity (the relative motion is the zero-gravity fixed-base motion);
  * momentum conservation under internal joint torques (zero gravity, no
    contacts): the world spatial momentum drifts only at first order in dt
    (semi-implicit Euler), i.e. 10x less for a 10x smaller step;
  * the reference's contact KAT transposed to an articulated body
    (tests/test_scenario/test_contacts.py:57-122: the vertical contact forces
    sum to the weight within 0.1 N): the quadruped standing on its four feet
    under a joint PD hold carries its 16 kg on exactly its feet;
  * world wrenches (or_float_step_ext, FloatWorld.wrench): against the scene
    oracle's (or_scene_step) on contact states of the quadruped and the iCub
    at five friction coefficients from 0 to 1.2, and against p = F t in zero
    gravity.
"""

import numpy as np
import pytest

G = 9.8


@pytest.fixture(scope="module")
def quad_file():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "gym-ignition_amd", "models", "quadruped.urdf")


STAND = np.array([0.6, -1.2] * 4)


def chain_urdf(n=2, floating=True, cylinder_tip=False, mesh_tip=None):
    """A floating box base with an n-link revolute chain (links: 0.3 m rods,
    alternating y / x axes), a sphere (or a tilted cylinder, or the mesh file
    mesh_tip, tilted) at the tip."""
    links = ['<link name="base"><inertial><mass value="3.0"/>'
             '<inertia ixx="0.02" iyy="0.03" izz="0.04" ixy="0.001" ixz="0" iyz="0"/></inertial>'
             '<collision><geometry><box size="0.3 0.2 0.1"/></geometry></collision></link>']
    if not floating:
        links.insert(0, '<link name="world"/><joint name="fix" type="fixed"><parent link="world"/>'
                        '<child link="base"/></joint>')
    parent = "base"
    for i in range(n):
        axis = "0 1 0" if i % 2 == 0 else "1 0 0"
        z = "-0.05" if i == 0 else "-0.3"
        geo = ('<origin xyz="0 0 -0.3" rpy="0.4 1.1 0"/><geometry><cylinder radius="0.04" length="0.12"/>'
               '</geometry>' if cylinder_tip else
               f'<origin xyz="0 0 -0.3" rpy="0.3 -0.5 0.2"/><geometry><mesh filename="{mesh_tip}" scale="0.5 0.5 0.5"/>'
               '</geometry>' if mesh_tip else
               '<origin xyz="0 0 -0.3"/><geometry><sphere radius="0.04"/></geometry>')
        tip = f'<collision>{geo}</collision>' if i == n - 1 else ""
        links.append(f'<joint name="j{i}" type="revolute"><parent link="{parent}"/><child link="l{i}"/>'
                     f'<origin xyz="0.1 0 {z}" rpy="0 0 0"/><axis xyz="{axis}"/>'
                     f'<limit lower="-2.0" upper="2.0" effort="50" velocity="30"/></joint>'
                     f'<link name="l{i}"><inertial><origin xyz="0 0.01 -0.15"/><mass value="{0.8 - 0.2 * i}"/>'
                     f'<inertia ixx="0.006" iyy="0.007" izz="0.001" ixy="0.0002" ixz="0" iyz="0"/></inertial>'
                     f'{tip}</link>')
        parent = f"l{i}"
    return '<robot name="fchain">' + "".join(links) + "</robot>"


def momentum(fw):
    M, _ = fw.dynamics()
    nu = np.concatenate([fw.V, fw.qd])
    hb = M[:6] @ nu
    L = fw.R @ hb[3:]
    return np.concatenate([fw.R @ hb[:3] + np.cross(fw.p, L), L])


def test_dense_blocks_match_fixed_base(oracle, quad_file):
    cm = oracle.load_urdf(quad_file, pose_xyz=(0.1, -0.2, 0.5), pose_wxyz=(0.9, 0.1, -0.2, 0.3))
    fw = oracle.FloatWorld(cm, ground=False)
    rng = np.random.default_rng(1)
    q = rng.uniform(-1, 1, 8)
    fw.set_joints(q, np.zeros(8))
    M, h = fw.dynamics()
    assert np.abs(M - M.T).max() < 1e-12
    assert np.linalg.eigvalsh(M).min() > 0
    assert M[3, 3] == pytest.approx(16.0) and M[4, 4] == pytest.approx(16.0)
    # fixed-base routines with gravity expressed in the base frame
    cm.model.gravity_base[:] = list(fw.R.T @ np.array([0, 0, -G]))
    np.testing.assert_allclose(M[6:, 6:], oracle.crba(cm, q), atol=1e-12)
    np.testing.assert_allclose(h[6:], oracle.rnea(cm, q, np.zeros(8), np.zeros(8)), atol=1e-12)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_heavy_base_reduces_to_fixed_base_step(oracle, n):
    text = chain_urdf(n)
    cmf = oracle.load_urdf(text, gravity=(0, 0, 0))
    cmf.free.mass = 1e9
    for k in range(3):
        cmf.free.Ic[k] = 1e9
    fw = oracle.FloatWorld(cmf, ground=False, pgs_iters=50)
    cmx = oracle.load_urdf(chain_urdf(n, floating=False), gravity=(0, 0, 0))
    rng = np.random.default_rng(n)
    q = rng.uniform(-1.9, 1.9, n)
    q[0] = 2.05  # beyond the upper limit: a limit row is active
    qd = rng.uniform(-2, 2, n)
    tau = rng.uniform(-5, 5, n)
    fw.set_joints(q, qd)
    mode = np.full(n, oracle.FORCE, np.int32)
    for _ in range(50):
        fw.step(mode, tau)
    qx, qdx = q.copy(), qd.copy()
    for _ in range(50):
        qx, qdx, _, _, _ = oracle.step(cmx, 1e-3, qx, qdx, mode, tau, 50)
    np.testing.assert_allclose(fw.q, qx, atol=1e-7)
    np.testing.assert_allclose(fw.qd, qdx, atol=1e-6)
    assert np.abs(fw.V).max() < 1e-6


def test_free_fall_leaves_joints_weightless(oracle):
    text = chain_urdf(2)
    a = oracle.FloatWorld(oracle.load_urdf(text, pose_xyz=(0, 0, 5.0)), ground=False)
    b = oracle.FloatWorld(oracle.load_urdf(text, pose_xyz=(0, 0, 5.0), gravity=(0, 0, 0)), ground=False)
    for w in (a, b):
        w.set_joints([0.4, -0.3], [1.0, -0.5])
        w.set_twist([0.1, 0.2, -0.1], [0.0, 0.0, 0.0])
    for _ in range(300):
        a.step()
        b.step()
    np.testing.assert_allclose(a.q, b.q, atol=1e-10)
    np.testing.assert_allclose(a.qd, b.qd, atol=1e-10)
    # the base falls with g on top of the weightless motion (semi-implicit
    # Euler), up to the O(dt^2 |w| |v|) rotation-translation coupling of the
    # SE(3) exponential (the base spins)
    t_steps = 300
    dz = -G * 1e-3 * 1e-3 * t_steps * (t_steps + 1) / 2
    assert a.p[2] - b.p[2] == pytest.approx(dz, abs=1e-5)


def test_momentum_drift_is_first_order(oracle, quad_file):
    drifts = []
    for dt in (1e-3, 1e-4):
        cm = oracle.load_urdf(quad_file, pose_xyz=(0, 0, 1.0), gravity=(0, 0, 0))
        fw = oracle.FloatWorld(cm, dt=dt, ground=False)
        rng = np.random.default_rng(0)
        fw.set_joints(np.array([0.3, -0.8] * 4), rng.uniform(-1, 1, 8))
        fw.set_twist(rng.uniform(-.5, .5, 3), rng.uniform(-.5, .5, 3))
        h0 = momentum(fw)
        steps = int(round(0.1 / dt))
        mode = np.full(8, oracle.FORCE, np.int32)
        for k in range(steps):
            fw.step(mode, 2 * np.sin(10 * k * dt + np.arange(8)))
        drifts.append(np.abs(momentum(fw) - h0).max())
    assert drifts[0] < 0.05
    assert 7.0 < drifts[0] / drifts[1] < 13.0


def test_standing_quadruped_carries_its_weight(oracle, quad_file):
    cm = oracle.load_urdf(quad_file, pose_xyz=(0, 0, 0.45))
    fw = oracle.FloatWorld(cm, pgs_iters=50)
    fw.set_joints(STAND, np.zeros(8))
    mode = np.full(8, oracle.FORCE, np.int32)
    heights = []
    for k in range(2000):
        fw.step(mode, -400 * (fw.q - STAND) - 10 * fw.qd)
        heights.append(fw.p[2])
    assert len(fw.contacts) == 4
    assert sorted(c[3] for c in fw.contacts) == [1, 3, 5, 7]     # the shanks (feet)
    fz = sum(c[1][2] for c in fw.contacts)
    assert fz == pytest.approx(16.0 * G, abs=0.1)
    for c in fw.contacts:
        assert c[1][2] > 0 and c[2] > 0                           # pushing up, penetrating
    assert np.ptp(heights[-500:]) < 1e-4                           # at rest
    assert abs(heights[-1] - 0.4408) < 2e-3                        # feet 3 cm spheres, small sag


def test_warm_started_pgs_mode(oracle):
    """or_float_step_warm (the wave kernel's mw_set_pgs_options twin): without
    options it is or_float_step bit for bit; the warm record holds the step's
    impulses by contact slot (3 slot + d) and joint row; on the standing
    humanoid the normal impulses of the record carry the weight (m g dt), and
    the velocity-tolerance exit runs fewer sweeps than the budget while staying
    within 1e-4 of the fixed-count step."""
    import ctypes
    from mwstep import get_model_file
    from mwstep.models import ICUB_POSE, icub_pid_gains, icub_posture
    cm = oracle.load_urdf(get_model_file("icub"), pose_xyz=ICUB_POSE[:3], pose_wxyz=ICUB_POSE[3:])
    n = cm.n
    q0 = np.array(icub_posture(cm.joint_names))
    kp, kd = np.array(icub_pid_gains(cm.joint_names)).T
    hold = lambda w: np.clip(-kp * (w.q - q0) - kd * w.qd, -80, 80)
    mode = np.full(n, oracle.FORCE, np.int32)
    a = oracle.FloatWorld(cm, pgs_iters=50)
    b = oracle.FloatWorld(cm, pgs_iters=50, warm_start=True)
    for w in (a, b):
        w.set_joints(q0, np.zeros(n))
    for _ in range(600):           # lands (4 mm) and settles on its feet
        a.step(mode, hold(a))
        b.warm[:] = 0.0            # cold every step: identical arithmetic
        b.step(mode, hold(b))
    assert np.array_equal(a.q, b.q) and np.array_equal(a.V, b.V)
    # the record: normal impulses at 3 slot, their sum m g dt
    normals = b.warm[0:3 * oracle.OR_MAXFC:3]
    mass = cm.free.mass + sum(cm.model.mass[i] for i in range(n))
    assert np.count_nonzero(normals) == len(b.contacts)
    assert normals.sum() == pytest.approx(mass * 9.8 * 1e-3, rel=0.02)
    # tolerance exit
    c = oracle.FloatWorld(cm, pgs_iters=50, pgs_tol=1e-6, warm_start=True)
    c.s = oracle.OrFloatState()
    ctypes.pointer(c.s)[0] = b.s
    c.warm[:] = b.warm
    sweeps = []
    for _ in range(50):
        tau = hold(b)
        c.step(mode, tau)
        s = ctypes.c_int()
        oracle.lib().or_pgs_stats(ctypes.byref(s), None)
        sweeps.append(s.value)
        b.step(mode, tau)
    assert np.mean(sweeps) < 50
    assert np.abs(c.q - b.q).max() <= 1e-4 and np.abs(c.p - b.p).max() <= 1e-5


@pytest.mark.parametrize("name, link", [("quadruped", 3), ("icub", 20)])
def test_world_wrench_matches_the_scene_oracle(oracle, name, link):
    """or_float_step_ext against or_scene_step (whose wrench input
    test_gpu_scenario_scene.py pins with v = F t / m) on one model: the
    contact states of the one-step GPU tests (feet and trunk in the ground,
    joints beyond their limits, random torques), wrenches on the base and on
    one other link, the same friction coefficient and the converged solve on
    both sides.  The two dense formulations differ only in summation order:
    the state within 1e-9 (measured 2e-15 quadruped, 5e-11 iCub) and the
    contact forces within 1e-9 of the world's largest contact force,
    |df| / (1 + max |f|) (measured 7e-16, 1.2e-10).  The iCub's absolute force
    gap is 3e-8 N, on a 242 N corner force in a world whose largest is 1612 N:
    its soles' redundant corners make the Delassus matrix conditioned 1.3e8,
    so how a foot's load splits between its corners is determined to 1e-8
    relative at best, while the motion is not affected."""
    from float_oracle_check import quat_to_R, random_states
    from mwstep import get_model_file
    W = 24
    cm = oracle.load_urdf(get_model_file(name))
    rng = np.random.default_rng(11)
    q, qd, pose, vel, tau = random_states(cm, W, rng)
    mus = [0.0, 0.05, 0.3, 0.8, 1.2]
    worst_state = worst_force = 0.0
    n_contact = n_pts = 0
    for w in range(W):
        wr = {-1: np.concatenate([rng.uniform(-60, 60, 3), rng.uniform(-5, 5, 3)]),
              link: np.concatenate([rng.uniform(-20, 20, 3), rng.uniform(-2, 2, 3)])}
        mu = mus[w % 5]
        fw = oracle.FloatWorld(cm, mu=mu, pgs_iters=oracle.PGS_CONVERGED)
        sw = oracle.SceneWorld([cm], mu=mu, pgs_iters=oracle.PGS_CONVERGED)
        # a float32 quaternion is a unit one only to 1e-8: normalised here, since the two
        # oracles treat a rotation matrix that is not orthonormal differently (a body
        # point kept in the body frame / taken back with R^T), a 1e-8 effect on the rows
        R0 = quat_to_R(pose[w, 3:] / np.linalg.norm(pose[w, 3:]))
        fw.set_pose(pose[w, :3], R0)
        fw.set_twist(R0.T @ vel[w, 3:], R0.T @ vel[w, :3])
        fw.set_joints(q[w], qd[w])
        sw.set_pose(0, pose[w, :3], R0)
        sw.set_twist(0, R0.T @ vel[w, 3:], R0.T @ vel[w, :3])
        sw.set_joints(0, q[w], qd[w])
        for b, f in wr.items():
            fw.wrench[1 + b] = f
            sw.wrench[0, 1 + b] = f
        sw.mode[0, :cm.n] = oracle.FORCE
        sw.cmd[0, :cm.n] = tau[w]
        fw.step(np.full(cm.n, oracle.FORCE, np.int32), tau[w])
        _, res_f = oracle.pgs_stats()
        sw.step()
        _, res_s = oracle.pgs_stats()
        if not (0.0 <= res_f <= 1e-6 and 0.0 <= res_s <= 1e-6):
            continue   # an exact solve that missed its complementarity conditions is no reference
        e = max(np.abs(fw.q - sw.q(0)).max(), np.abs(fw.qd - sw.qd(0)).max(), np.abs(fw.V - sw.V(0)).max(),
                np.abs(fw.p - sw.p(0)).max(), np.abs(fw.R - sw.R(0)).max())
        worst_state = max(worst_state, float(e))
        assert len(fw.contacts) == len(sw.contacts)
        n_contact += len(fw.contacts) > 0
        f_max = max([float(np.abs(c[1]).max()) for c in fw.contacts], default=0.0)
        for (p, f, d, b) in fw.contacts:
            match = [c for c, who in sw.contacts if np.abs(c[:3] - p).max() <= 1e-12 and who[1] == b]
            assert len(match) == 1
            worst_force = max(worst_force, float(np.abs(match[0][6:9] - f).max()) / (1.0 + f_max))
            n_pts += 1
    print(f"{name}: FloatWorld vs SceneWorld with wrenches, {n_contact}/{W} worlds in contact, {n_pts} points: "
          f"state {worst_state:.2e}, contact force {worst_force:.2e}")
    assert n_contact > W // 4
    assert worst_state <= 1e-9 and worst_force <= 1e-9


def test_base_force_gives_linear_momentum(oracle, quad_file):
    """Zero gravity, no ground, a world force F (and a torque) on the base of
    the tilted quadruped at rest, joints free.
      * One step is exact: the scheme solves M (nu' - nu) = dt (f - bias) with
        the bias zero at rest, so the base rows of M nu', taken to the world
        frame with the start pose, are dt [torque about the base origin; F].
      * After t = 0.2 s the world linear momentum is F t up to the first-order
        drift of the semi-implicit scheme (the base spins and the legs swing:
        test_momentum_drift_is_first_order): the error falls 10x with a 10x
        smaller step, and at dt = 1e-4 it is below 1e-4 |F t| (measured
        1.9e-4 of 6.0 kg m/s; 1.9e-3 at dt = 1e-3)."""
    cm = oracle.load_urdf(quad_file, pose_xyz=(0.2, -0.1, 1.0), pose_wxyz=(0.9, 0.1, -0.2, 0.3), gravity=(0, 0, 0))
    F, torque, t = np.array([30.0, -12.0, 7.0]), np.array([1.0, -2.0, 0.5]), 0.2
    errs = []
    for dt in (1e-3, 1e-4):
        fw = oracle.FloatWorld(cm, dt=dt, ground=False)
        fw.set_joints(np.array([0.3, -0.8] * 4), np.zeros(8))
        fw.wrench[0] = np.concatenate([F, torque])
        M0, R0 = fw.dynamics()[0], fw.R
        fw.step()
        hb = M0[:6] @ np.concatenate([fw.V, fw.qd])
        np.testing.assert_allclose(R0 @ hb[3:], F * dt, rtol=0, atol=1e-12)
        np.testing.assert_allclose(R0 @ hb[:3], torque * dt, rtol=0, atol=1e-12)
        np.testing.assert_allclose(M0[6:] @ np.concatenate([fw.V, fw.qd]), 0.0, atol=1e-12)   # no joint torque
        for _ in range(int(round(t / dt)) - 1):
            fw.step()
        errs.append(float(np.abs(momentum(fw)[3:] - F * t).max()))
    print(f"linear momentum after {t} s under a base force: |p - F t| {errs[0]:.2e} (dt 1e-3), {errs[1]:.2e} (dt 1e-4)")
    assert 7.0 < errs[0] / errs[1] < 13.0
    assert errs[1] <= 1e-4 * np.abs(F * t).max()
