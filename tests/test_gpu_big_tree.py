"""The wave kernel's 48-body instances (wave_run_kernel<48, CONS, WMU, WPAR>,
every floating or welded tree of 33..48 joints) against the fp64 oracle, on
the models of big_tree_cases.py -- tree33, tree40, tree48 and tree48's damped
(d), frictional (f), unlimited (u: the CONS = false instances) and welded (w)
variants.  tests/test_big_tree_cases.py shows on the CPU that these inputs
fit the kernel and that a kernel which forgot the bodies >= 32 could not pass.

  * one step of the PGS-50 arithmetic and of the exact LCP: the procedures of
    test_gpu_float_tree.py (one_step_parity, one_step_exact_lcp), unchanged;
  * the WMU instance (a ground friction per world), the WPAR instance (link
    parameters and joint dynamics per world, also on the links and dofs
    >= 32), world wrenches on bodies >= 32: each world against the oracle on
    its own model, accepted as exact_lcp_acceptance accepts;
  * closed loop under the JointController PID on all 48 joints against the
    oracle's pid_update loop, one and two substeps per run; the warm-started
    PGS against the oracle's warm mode;
  * plumbing at n > 32: run_device, get_state / set_state, contact_bodies,
    effort clamping, joint resets.
"""

import numpy as np
import pytest

import big_tree_cases as C
from float_oracle_check import Q_TOL, QD_TOL, RES_TOL, exact_lcp_acceptance, oracle_step
from test_gpu_float_tree import one_step_exact_lcp, one_step_parity

pytestmark = pytest.mark.gpu
W = C.W
MUS = [0.0, 0.05, 0.3, 0.8, 1.2]          # test_gpu_float_rand_oracle.MUS
HIGH_LINKS = (31, 39, 47)                 # the 32nd, 40th and 48th link


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _sim(monkeypatch, name, n_worlds=W, ground=True, mu=C.MU, **kw):
    from mwstep.sim import Simulator
    monkeypatch.setenv("MWSTEP_WAVE_TREE", "1")
    sim = Simulator(C.urdf(name), n_worlds=n_worlds, pgs_iters=50, **kw)
    assert sim.float_kernel() == 2 and sim.dofs > 32
    assert sim.dofs == len(C.parents(name))
    if sim.floating:
        sim.set_ground_plane(ground, mu)
        sim.enable_contacts(ground)
    return sim


def _start(sim, name, worlds=None):
    """Reset to the start states of `worlds` (default: the first n_worlds);
    returns (start as the simulator reports it, tau)."""
    q, qd, pose, vel, tau = C.states(name)
    ws = np.arange(sim.n_worlds) if worlds is None else np.asarray(worlds)
    sim.set("reset_q", q[ws])
    sim.set("reset_qd", qd[ws])
    if sim.floating:
        sim.reset_base_pose(pose[ws])
        sim.reset_base_velocity(vel[ws])
    sim.run(paused=True)
    return (sim.base_pose(), sim.base_velocity(), sim.get("q"), sim.get("qd")), tau[ws]


def _step(sim, tau):
    from mwstep import native as N
    sim.set_control_mode(N.MODE_FORCE)
    sim.set("force_target", tau)
    sim.run()
    return sim.base_pose(), sim.get("q"), sim.get("qd"), sim.get_state()


@pytest.mark.parametrize("name", C.PGS_MODELS)
def test_one_step_pgs50(require_gpu, oracle, monkeypatch, name):
    """test_one_step_parity_with_contacts on the 48-body instance"""
    assert len(C.parents(name)) > 32          # the helper asserts float_kernel() == 2 and the dof count
    one_step_parity(oracle, monkeypatch, C.urdf(name), name, "wave", states=C.states(name))


@pytest.mark.parametrize("name", C.EXACT_MODELS)
def test_one_step_exact_lcp(require_gpu, oracle, monkeypatch, name):
    """test_one_step_exact_lcp_random_states on the 48-body instance; tree48u
    has no joint row in any world (CONS = false).

    tree48f exposed a bug of the exact solve (not of the 48-body instance): a
    joint beyond its limit that also has Coulomb friction has one Jacobian row
    twice, the pair's Schur pivot (DART's joint CFM, 1e-9) is rounding noise in
    fp32, and with the noise's sign the friction row moved the wrong way, was
    frozen at the wrong bound and the world-step ended unconverged: 8 of 256
    worlds here at any budget from 48 to 192 solves (all within 4.8e-5 of the
    oracle: the pair's impulses only swap), 4 and 9 of 256 on a 16- and a
    32-joint tree with the same friction.  wave_lcp.hpp spd_pivot takes the
    pivot's magnitude; none is left unconverged on any of the three."""
    assert len(C.parents(name)) > 32
    res = one_step_exact_lcp(oracle, monkeypatch, C.urdf(name), name, states=C.states(name))
    assert len(res["no_ref"]) <= W // 20


def test_one_step_welded_tree(require_gpu, oracle, monkeypatch):
    """tree48w, the fixed-base tree on the wave kernel (FloatF::fixed), against
    the oracle's fixed-tree step with the converged LCP: the acceptance of
    exact_lcp_acceptance without the base -- q-dot within QD_TOL, q within
    Q_TOL; the fixed-tree oracle keeps no problem to judge a second answer by,
    so any other world differs, and none may."""
    name = C.WELDED
    cm = oracle.load_urdf(C.urdf(name))
    sim = _sim(monkeypatch, name)
    assert not sim.floating
    (_, _, q0, qd0), tau = _start(sim, name)
    _, q1, qd1, _ = _step(sim, tau)
    mode = np.full(cm.n, oracle.FORCE, np.int32)
    agree, no_ref, differ, worst_q, worst_qd = 0, [], [], 0.0, 0.0
    for w in range(W):
        oq, oqd, *_ = oracle.step(cm, 1e-3, q0[w], qd0[w], mode, tau[w], oracle.PGS_CONVERGED)
        _, res = oracle.pgs_stats()
        if not 0.0 <= res <= RES_TOL:
            no_ref.append(w)
            continue
        e_q, e_qd = float(np.abs(q1[w] - oq).max()), float(np.abs(qd1[w] - oqd).max())
        if e_qd <= QD_TOL and e_q <= Q_TOL:
            agree += 1
            worst_q, worst_qd = max(worst_q, e_q), max(worst_qd, e_qd)
        else:
            differ.append((w, f"{e_qd:.1e}", f"{e_q:.1e}"))
    n_ref = W - len(no_ref)
    print(f"{name}: {agree}/{n_ref} worlds agree with the converged oracle (worst qd {worst_qd:.2e}, q {worst_q:.2e}); "
          f"differ {differ}; oracle unconverged {no_ref}; GPU unconverged {sim.lcp_unconverged()}")
    assert sim.constraint_overflow() == 0 and sim.lcp_unconverged() == 0
    assert np.allclose(sim.base_pose()[:, :3], cm.base_p) and np.allclose(sim.base_velocity(), 0.0)
    sim.close()
    assert len(no_ref) <= W // 20 and not differ and agree >= 0.85 * n_ref


def test_one_step_friction_per_world(require_gpu, oracle, monkeypatch):
    """WMU: tree48 with a ground friction per world cycling through 0, 0.05,
    0.3, 0.8, 1.2, every world against the oracle with its own coefficient
    (test_one_step_wrench_and_friction_exact_lcp's procedure)."""
    name = "tree48"
    cm = oracle.load_urdf(C.urdf(name))
    mus = np.array([MUS[w % len(MUS)] for w in range(W)])
    sim = _sim(monkeypatch, name)
    sim.set_ground_friction(mus)
    np.testing.assert_array_equal(sim.ground_friction(), _f32(mus))
    start, tau = _start(sim, name)
    end = _step(sim, tau)
    res = exact_lcp_acceptance(sim, oracle, cm, mus, tau, start, end, label=f"{name}, mu per world")
    sim.close()
    assert len(res["no_ref"]) <= W // 20
    # the coefficient decides: the same result against the oracle at the nominal 0.8
    miss = sum(float(np.abs(end[2][w] - oracle_step(oracle, cm, start[0][w], start[1][w], start[2][w], start[3][w],
                                                    tau[w], C.MU, oracle.PGS_CONVERGED).qd).max()) > QD_TOL
               for w in range(W) if mus[w] != C.MU)
    print(f"{name}, mu per world: against mu = {C.MU} everywhere {miss} worlds miss QD_TOL")
    assert miss >= C.friction_signal(oracle, name, mus) // 2 > 0


def _own_model_acceptance(sim, oracle, name, alter, start, end, tau, label, mu=C.MU, wrench=None):
    """exact_lcp_acceptance restated per world, every world on its own copy of
    the model (alter(cm, w) edits it in place), as test_gpu_float_inertia_oracle.py
    and test_gpu_float_joints_oracle.py restate it; also counts the worlds
    that miss QD_TOL against the nominal model."""
    from lcp_validity import judge
    cm, nominal_cm = oracle.load_urdf(C.urdf(name)), oracle.load_urdf(C.urdf(name))
    p0, v0, gq0, gqd0 = start
    p1, gq1, gqd1, state = end
    n_worlds = sim.n_worlds
    no_ref, agree, valid, differ, miss_nominal = [], 0, [], [], 0
    worst_qd = worst_q = 0.0
    for w in range(n_worlds):
        wr = wrench(w) if wrench else None
        plain = oracle_step(oracle, nominal_cm, p0[w], v0[w], gq0[w], gqd0[w], tau[w], mu, oracle.PGS_CONVERGED)
        miss_nominal += float(np.abs(gqd1[w] - plain.qd).max()) > QD_TOL
        alter(cm, w)
        ow = oracle_step(oracle, cm, p0[w], v0[w], gq0[w], gqd0[w], tau[w], mu, oracle.PGS_CONVERGED, wr)
        _, res = oracle.pgs_stats()
        if not 0.0 <= res <= RES_TOL:
            no_ref.append(w)
            continue
        prob = oracle.lcp_last()
        e_qd = float(np.abs(gqd1[w] - ow.qd).max())
        e_q = max(float(np.abs(gq1[w] - ow.q).max()), float(np.abs(p1[w, :3] - ow.p).max()))
        if e_qd <= QD_TOL and e_q <= Q_TOL:
            agree += 1
            worst_qd, worst_q = max(worst_qd, e_qd), max(worst_q, e_q)
            continue
        ok, ratio, _ = judge(prob, ow.contacts, sim.contacts(w), state[w])
        rec = (w, f"{e_qd:.1e}", f"ratio {ratio:.2f}")
        (valid if ok and e_q <= 2e-3 * e_qd + 1e-5 else differ).append(rec)
    unconv, overflow = sim.lcp_unconverged(), sim.constraint_overflow()
    n_ref = n_worlds - len(no_ref)
    print(f"{label}: {agree}/{n_ref} worlds agree with the converged oracle on their own model (worst of them qd "
          f"{worst_qd:.2e}, q / pose {worst_q:.2e}); other valid fp64 solutions {valid}; differ {differ}; oracle "
          f"unconverged {len(no_ref)}; GPU unconverged {unconv}, overflow {overflow}; against the nominal model "
          f"{miss_nominal}/{n_worlds} worlds miss QD_TOL")
    assert overflow == 0 and unconv == 0
    assert n_ref >= 0.9 * n_worlds
    assert not differ
    assert agree >= 0.85 * n_ref
    return miss_nominal


def _link_words(sim, oracle, name):
    from test_gpu_float_inertia_oracle import _draw_words, _nominal_words
    nominal = np.stack([sim.link_params(link, [0])[0] for link in range(-1, sim.dofs)])
    np.testing.assert_allclose(nominal, _nominal_words(oracle.load_urdf(C.urdf(name))), rtol=1e-5, atol=1e-7)
    return nominal, _draw_words(nominal, W, C.PAYLOAD_MAX)


def test_one_step_link_parameters_per_world(require_gpu, oracle, monkeypatch):
    """WPAR: every link of tree48 -- the 32nd, 40th and 48th among them --
    scaled by U(0.5, 2) per world and a payload of up to 5 kg on the base
    (test_gpu_float_inertia_oracle.py's draw and acceptance)."""
    from test_gpu_float_inertia_oracle import _apply_words
    name = "tree48"
    sim = _sim(monkeypatch, name)
    nominal, words = _link_words(sim, oracle, name)
    for link in range(-1, sim.dofs):
        sim.set_link_params(link, words[:, link + 1])
    for link in HIGH_LINKS:
        np.testing.assert_array_equal(sim.link_params(link), words[:, link + 1])
        assert (words[:, link + 1, 0] != nominal[link + 1, 0]).all()
    start, tau = _start(sim, name)
    end = _step(sim, tau)
    miss = _own_model_acceptance(sim, oracle, name, lambda cm, w: _apply_words(cm, words[w]), start, end, tau,
                                 f"{name}, per-world masses and payload")
    sim.close()
    assert miss > W // 2


def test_nine_worlds_are_nine_simulators(require_gpu, oracle, monkeypatch):
    """tree48 with per-world link parameters and friction: worlds 0..8 of one
    simulator step bit for bit like nine one-world simulators, three steps."""
    name = "tree48"
    many = _sim(monkeypatch, name, n_worlds=9)
    _, words = _link_words(many, oracle, name)
    mus = np.array([MUS[w % len(MUS)] for w in range(9)])
    in_contact = np.flatnonzero(C.survey_contacts(oracle, name))[:9]      # nine worlds that touch the ground
    sims = [many] + [_sim(monkeypatch, name, n_worlds=1) for _ in range(9)]
    for k, sim in enumerate(sims):
        ws = slice(0, 9) if k == 0 else slice(k - 1, k)
        for link in range(-1, sim.dofs):
            sim.set_link_params(link, words[ws, link + 1])
        sim.set_ground_friction(mus[ws])
        _, tau = _start(sim, name, in_contact[ws])
        _step(sim, tau)
        sim.run()
        sim.run()
    state = many.get_state()
    assert sum(len(many.contacts(w)) > 0 for w in range(9)) >= 5
    for w in range(9):
        np.testing.assert_array_equal(sims[1 + w].get_state()[0], state[w], err_msg=f"world {w}")
        np.testing.assert_array_equal(sims[1 + w].contacts(0), many.contacts(w))
    for sim in sims:
        sim.close()


@pytest.mark.parametrize("name, dofs", [("tree48", C.JOINT_DOFS), ("tree48u", (47,))])
def test_one_step_joint_dynamics_per_world(require_gpu, oracle, monkeypatch, name, dofs):
    """WPAR: damping, friction and effort limit per world on dofs that include
    32..47 (test_gpu_float_joints_oracle.py's draw and acceptance); on tree48u,
    which has no row of its own, friction per world on dof 47 alone switches
    the CONS instance on.

    The tree48 case exposed two bugs of the exact solve, neither particular to
    the 48-body instance (5 of 256 worlds differed, 4 unconverged).  Worlds 20,
    95 and 189 (|dqd| up to 1e-2) have a joint with both its limit row and its
    friction row, the singular pair described at test_one_step_exact_lcp.
    Worlds 15 and 180 (|dqd| 4.0e-4, 5.3e-4; world 180 has 9 rows, no contact,
    cond(A) 7e2) drew a friction of 2.2e-3 and 9.1e-4 N m: a box of 2 f dt <
    4.5e-6 N m s is narrower than the solve's impulse tolerance 2e-6 (1 + max
    |x|), inside which lcp_row_residual counted any impulse as converged; on
    these light links (A_rr = 96 and 294 rad/s per N m s) that was worth A_rr
    2 f dt = 4.3e-4 and 5.3e-4 rad/s.  It now does so only where crossing the
    box stays within the row's velocity tolerance."""
    from float_joints_ref import apply_words, nominal_words
    cm = oracle.load_urdf(C.urdf(name))
    sim = _sim(monkeypatch, name)
    nominal = np.stack([sim.joint_dynamics(d, [0])[0] for d in range(sim.dofs)])
    np.testing.assert_array_equal(nominal, nominal_words(cm))
    words = C.joint_words(nominal, name, dofs)
    for d in dofs:
        sim.set_joint_dynamics(d, words[:, d])
    for d in range(sim.dofs):
        np.testing.assert_array_equal(sim.joint_dynamics(d), words[:, d])
    start, tau = _start(sim, name)
    end = _step(sim, tau)
    miss = _own_model_acceptance(sim, oracle, name, lambda m, w: apply_words(m, words[w]), start, end, tau,
                                 f"{name}, per-world joint dynamics on dofs {list(dofs)}")
    sim.close()
    assert miss > W // 2


def test_one_step_world_wrenches(require_gpu, oracle, monkeypatch):
    """World wrenches on body 33 (link index 32), on the last body and on the
    base in the same step, against the oracle's wrench rows."""
    name = "tree48"
    cm = oracle.load_urdf(C.urdf(name))
    wrenches = C.wrenches()
    assert sorted(wrenches) == [-1, 32, 47]
    sim = _sim(monkeypatch, name)
    start, tau = _start(sim, name)
    for link, wr in wrenches.items():
        sim.apply_world_wrench(link, wr, sim.step_size)
    end = _step(sim, tau)
    of = lambda w: {b: wr[w] for b, wr in wrenches.items()}
    res = exact_lcp_acceptance(sim, oracle, cm, C.MU, tau, start, end, wrench=of, label=f"{name}, wrenches")
    assert len(res["no_ref"]) <= W // 20
    # each of the three wrenches decides: the GPU result misses the oracle that lacks it
    for link in wrenches:
        miss = 0
        for w, ow in res["worlds"].items():
            less = oracle_step(oracle, cm, start[0][w], start[1][w], start[2][w], start[3][w], tau[w], C.MU,
                               oracle.PGS_CONVERGED, {b: f for b, f in of(w).items() if b != link})
            miss += max(float(np.abs(end[2][w] - less.qd).max()),
                        float(np.abs(ow.V - less.V).max())) > QD_TOL
        print(f"{name}: without the wrench on link {link} the oracle misses {miss}/{len(res['worlds'])} worlds")
        assert miss >= 0.9 * len(res["worlds"])
    # the wrenches (and the force targets) last one step: the next is that of a simulator without them
    from mwstep import native as N
    sim.run()
    ref = _sim(monkeypatch, name)
    ref.set_control_mode(N.MODE_FORCE)
    ref.set_state(end[3])
    ref.run()
    np.testing.assert_array_equal(sim.get_state(), ref.get_state())
    assert not np.array_equal(end[2], sim.get("qd"))
    sim.close()
    ref.close()


def _closed_loop_sim(monkeypatch, oracle, substeps):
    from mwstep import native as N
    cm, post, tgt = C.closed_loop_inputs(oracle)
    nw = C.CL_WORLDS
    sim = _sim(monkeypatch, "tree48", n_worlds=nw, ground=False, pose=(0, 0, 1.0, 1, 0, 0, 0), steps_per_run=substeps)
    p, i, d, lim, ilim = C.CL_PID
    sim.set("reset_q", post)
    sim.run(paused=True)
    np.testing.assert_array_equal(sim.get("q"), post)
    sim.set_controller_period(1e-3)
    for dof in range(sim.dofs):
        sim.set_pid(dof, [p, i, d, -lim, lim, 0.0, -ilim, ilim])
    sim.set_control_mode(N.MODE_POSITION)
    sim.set("position_target", tgt)
    return sim, cm, post, tgt


@pytest.mark.parametrize("substeps", [1, 2])
def test_closed_loop_pid_on_48_joints(require_gpu, oracle, monkeypatch, substeps):
    """tree48 in free fall under the JointController PID (P, I and D, clamped)
    on all 48 joints, position mode, from a random posture at rest to targets
    up to 0.3 rad away: C.CL_STEPS physics steps (one or two per run), every
    world against the oracle's pid_update loop, teacher-free, as smoke() does
    for the iCub-class model.  q within 1e-4 (the bound of
    test_humanoid_standing_closed_loop_parity), base position within 1e-5;
    the horizon is where the oracle's own sensitivity to a 3e-7 perturbation
    stays under a tenth of that (test_big_tree_cases.test_closed_loop_horizon)."""
    sim, cm, post, tgt = _closed_loop_sim(monkeypatch, oracle, substeps)
    checks = sorted({C.CL_STEPS // 4, C.CL_STEPS // 2, C.CL_STEPS})
    got = {}
    for k in range(1, C.CL_STEPS // substeps + 1):
        sim.run()
        if k * substeps in checks:
            got[k * substeps] = (sim.get("q"), sim.base_pose()[:, :3])
    worst_q = worst_p = 0.0
    for w in range(C.CL_WORLDS):
        ref, ow = C.closed_loop_reference(oracle, cm, post[w], tgt[w], C.CL_STEPS)
        for k, (q, p) in got.items():
            worst_q = max(worst_q, float(np.abs(q[w] - ref[k]).max()))
        worst_p = max(worst_p, float(np.abs(got[C.CL_STEPS][1][w] - ow.p).max()))
    print(f"tree48 closed loop, {C.CL_STEPS} steps, {substeps} per run: max|dq| {worst_q:.2e}, base position "
          f"{worst_p:.2e}")
    assert sim.constraint_overflow() == 0 and sim.lcp_unconverged() == 0
    sim.close()
    assert worst_q <= C.CL_BOUND and worst_p <= 1e-5


def test_warm_started_pgs_with_joint_friction(require_gpu, oracle, monkeypatch):
    """tree48f landing from 5 mm under a PD hold applied as joint forces, the
    PGS sweeps with tolerance exit and warm start (mw_set_pgs_options) against
    the oracle's same mode, as test_humanoid_warm_started_pgs: q within 1e-3,
    base within 1e-4 over C.WARM_STEPS steps.  The Coulomb rows of the joints
    >= 32 (every second joint) carry impulses in the warm record of the
    snapshot, and a simulator continued from that snapshot steps bit for bit
    like the one that made it."""
    from mwstep import native as N
    name, nw, tol = "tree48f", 4, 1e-6
    cm, post, z = C.warm_inputs(oracle, name)
    sims = []
    for _ in range(2):
        sim = _sim(monkeypatch, name, n_worlds=nw, mu=1.0)
        sim.set_lcp_solver(False)
        sim.set_pgs_options(tol, True)
        assert sim.pgs_options() == (tol, True)
        sims.append(sim)
    sim, twin = sims
    sim.reset_base_pose(np.column_stack([np.zeros((nw, 2)), z, np.tile([1.0, 0, 0, 0], (nw, 1))]))
    sim.set("reset_q", post)
    sim.run(paused=True)
    sim.set_control_mode(N.MODE_FORCE)
    twin.set_control_mode(N.MODE_FORCE)
    kp, kd = C.WARM_PD
    ows = []
    for w in range(nw):
        ow = oracle.FloatWorld(cm, pgs_iters=50, pgs_tol=tol, warm_start=True)
        ow.set_pose([0, 0, z[w]], np.eye(3))
        ow.set_joints(post[w], np.zeros(cm.n))
        ows.append(ow)
    mode = np.full(cm.n, oracle.FORCE, np.int32)
    worst_q = worst_p = 0.0
    touched = np.zeros(nw, bool)
    for k in range(C.WARM_STEPS):
        gq, gqd = sim.get("q"), sim.get("qd")
        tau = _f32(np.clip(-kp * (gq - post) - kd * gqd, -50, 50))
        sim.set("force_target", tau)
        if k == C.WARM_STEPS - 5:
            twin.set_state(sim.get_state())
        if k >= C.WARM_STEPS - 5:
            twin.set("force_target", tau)
            twin.run()
        sim.run()
        for w, ow in enumerate(ows):
            ow.step(mode, np.clip(-kp * (ow.q - post[w]) - kd * ow.qd, -50, 50))
            touched[w] |= len(sim.contacts(w)) > 0
        if k % 10 == 9 or k == C.WARM_STEPS - 1:
            gq, p = sim.get("q"), sim.base_pose()
            for w, ow in enumerate(ows):
                worst_q = max(worst_q, float(np.abs(gq[w] - ow.q).max()))
                worst_p = max(worst_p, float(np.abs(p[w, :3] - ow.p).max()))
    state = sim.get_state()
    np.testing.assert_array_equal(twin.get_state(), state)
    slots, words = 32, 3 * 32 + 3 * 48            # kMaxFloatSlots, kWaveWarmWords (wave_tree.hpp)
    joint_rows = state[:, -2 * words:-words][:, 3 * slots:].reshape(nw, 48, 3)
    coulomb_high = joint_rows[:, 32::2, 2]        # the friction rows of the even joints >= 32
    print(f"{name} warm-started PGS, {C.WARM_STEPS} steps: q {worst_q:.2e}, base {worst_p:.2e}; worlds that touched "
          f"{int(touched.sum())}/{nw}; loaded Coulomb rows of joints >= 32: {int((coulomb_high != 0).sum())}/"
          f"{coulomb_high.size}")
    assert touched.all() and sim.constraint_overflow() == 0
    assert (coulomb_high != 0).sum() >= coulomb_high.size // 2
    assert not joint_rows[:, 33::2, 2].any()      # the odd joints have no friction
    assert worst_q <= 1e-3 and worst_p <= 1e-4
    for s in sims:
        s.close()


def test_run_device_and_snapshot(require_gpu, oracle, monkeypatch):
    """run_device equals repeated run, and a fresh simulator continued from
    get_state / set_state is bit-equal, over 30 steps from eight start states
    with a contact on a body >= 32, which contact_bodies reports."""
    name = "tree48"
    nw, steps = 8, 30
    worlds = np.flatnonzero(C.survey_contacts(oracle, name, high=True))[:nw]
    sims = []
    for _ in range(3):
        sim = _sim(monkeypatch, name, n_worlds=nw)
        _, tau = _start(sim, name, worlds)
        from mwstep import native as N
        sim.set_control_mode(N.MODE_FORCE)
        sim.set("force_target", 0.1 * tau)
        sims.append(sim)
    a, b, c = sims
    a.run()
    bodies = [a.contact_bodies(w) for w in range(nw)]
    assert all((bd >= 32).any() for bd in bodies), bodies
    for w in range(nw):                     # every reported body carries a sphere: a leaf of the tree or the base
        assert set(bodies[w].tolist()) <= set(C.leaves(name)) | {-1}
    for _ in range(steps - 1):
        a.run()
    b.run_device(steps)
    for _ in range(steps // 2):
        c.run()
    snap = c.get_state()
    c.close()
    c = sims[2] = _sim(monkeypatch, name, n_worlds=nw)
    c.set_control_mode(N.MODE_FORCE)          # the force targets acted in the first run alone
    c.set_state(snap)
    for _ in range(steps - steps // 2):
        c.run()
    for other in (b, c):
        np.testing.assert_array_equal(a.get_state(), other.get_state())
        np.testing.assert_array_equal(a.get("q"), other.get("q"))
        np.testing.assert_array_equal(a.base_pose(), other.base_pose())
    assert np.isfinite(a.get_state()).all()
    for s in sims:
        s.close()


def test_force_mode_clamps_effort_on_dof_47(require_gpu, oracle, monkeypatch):
    """MODE_FORCE: a force target beyond the effort limit of dof 47 (50 N m)
    acts as the limit -- bit-equal to a target at the limit, unlike a target
    below it -- and as the oracle's clamp."""
    name = "tree48"
    cm = oracle.load_urdf(C.urdf(name))
    assert cm.model.effort[47] == 50.0
    worlds = np.flatnonzero(~C.survey_contacts(oracle, name))[:4]      # in the air: one answer, no LCP to judge
    ends = []
    for t47 in (200.0, 50.0, 40.0, -200.0, -50.0):
        sim = _sim(monkeypatch, name, n_worlds=4)
        start, tau = _start(sim, name, worlds)
        tau = tau.copy()
        tau[:, 47] = t47
        ends.append(_step(sim, tau))
        assert not any(len(sim.contacts(w)) for w in range(4))
        sim.close()
    np.testing.assert_array_equal(ends[0][3], ends[1][3])
    np.testing.assert_array_equal(ends[3][3], ends[4][3])
    assert not np.array_equal(ends[1][2], ends[2][2])
    worst = 0.0
    for w in range(4):
        t = tau[w].copy()
        t[47] = 200.0
        ow = oracle_step(oracle, cm, start[0][w], start[1][w], start[2][w], start[3][w], t, C.MU, oracle.PGS_CONVERGED)
        worst = max(worst, float(np.abs(ends[0][2][w] - ow.qd).max()))
    print(f"{name}: a force target of 200 N m on dof 47 against the oracle's clamp: qd {worst:.2e}")
    assert worst <= QD_TOL


def test_joint_reset_of_high_dofs_is_consumed_once(require_gpu, oracle, monkeypatch):
    """Joint::resetPosition / resetVelocity on the dofs 32..47 alone, in the
    middle of the closed loop: the simulator steps exactly like one that was
    handed the same full state by one reset of every joint (so every PID
    is fresh in both), and goes on moving -- the reset acts in one run, not in
    the next.  Both simulators take the same reset path, so the PID reset flag
    is checked directly: the four steps after the reset against the oracle's
    pid_update loop from the same state with fresh PID states, q within
    C.CL_BOUND.  On the oracle alone, PID states that were not reset (those of
    its own first 20 steps) and PID states reset again at every step each move
    q by more than 100 C.CL_BOUND within those four steps."""
    a, cm, post, tgt = _closed_loop_sim(monkeypatch, oracle, 1)
    b, *_ = _closed_loop_sim(monkeypatch, oracle, 1)
    nw, n = C.CL_WORLDS, a.dofs
    high = np.arange(32, n, dtype=np.int32)
    for _ in range(20):
        a.run()
    rng = np.random.default_rng(5)
    q_new = _f32(post[:, 32:] + rng.uniform(-0.1, 0.1, (nw, n - 32)))
    qd_new = _f32(rng.uniform(-0.5, 0.5, (nw, n - 32)))
    # both are handed the same state by resets: a, after 20 steps, joint by joint in two
    # calls (the dofs >= 32 to new values, the others to where they are); b, fresh, in one
    qa, qda = a.get("q"), a.get("qd")
    low = np.arange(32, dtype=np.int32)
    a.set("reset_q", qa[:, :32], dofs=low)
    a.set("reset_qd", qda[:, :32], dofs=low)
    a.set("reset_q", q_new, dofs=high)
    a.set("reset_qd", qd_new, dofs=high)
    qa[:, 32:], qda[:, 32:] = q_new, qd_new
    b.set("reset_q", qa)
    b.set("reset_qd", qda)
    pose, vel = a.base_pose(), a.base_velocity()
    for s in (a, b):
        s.reset_base_pose(pose)
        s.reset_base_velocity(vel)
    trail, full = [], []
    for _ in range(4):
        a.run()
        b.run()
        np.testing.assert_array_equal(a.get("q"), b.get("q"))
        np.testing.assert_array_equal(a.get("qd"), b.get("qd"))
        np.testing.assert_array_equal(a.base_pose(), b.base_pose())
        trail.append(a.get("q")[:, 32:])
        full.append(a.get("q"))
    # one step from the reset state -- at most dt (|qd| + dt 50 N m / 9e-4 kg m^2, the lightest leaf
    # under the PID's limit) = 0.06 from it -- then on: not held at it
    first = float(np.abs(trail[0] - q_new).max())
    assert first <= 0.06
    assert all((trail[k + 1] != trail[k]).all() for k in range(3))
    a.close()
    b.close()
    # the PIDs after the reset: the oracle's loop from the reset state with fresh PID states
    from float_oracle_check import quat_to_R
    p, i, d, lim, ilim = C.CL_PID
    gains = oracle.pid_gains(p, i, d, imax=ilim, imin=-ilim, cmdmax=lim, cmdmin=-lim)
    mode = np.full(n, oracle.FORCE, np.int32)

    def loop(w, steps, states=None, start=None, again=False):
        ow = oracle.FloatWorld(cm, ground=False, pgs_iters=oracle.PGS_CONVERGED)
        if start is None:
            ow.set_joints(post[w], np.zeros(n))
        else:
            R = quat_to_R(pose[w, 3:])
            ow.set_pose(pose[w, :3], R)
            ow.set_twist(R.T @ vel[w, 3:], R.T @ vel[w, :3])
            ow.set_joints(*start)
        st = states or [oracle.OrPidState() for _ in range(n)]
        out = []
        for _ in range(steps):
            if again:
                st = [oracle.OrPidState() for _ in range(n)]
            q = ow.q
            ow.step(mode, np.array([oracle.pid_update(gains, st[j], q[j] - tgt[w, j], 1e-3) for j in range(n)]))
            out.append(ow.q)
        return np.array(out), st

    worst, stale, again = 0.0, [], []
    for w in range(nw):
        ref, _ = loop(w, 4, start=(qa[w], qda[w]))
        worst = max(worst, max(float(np.abs(full[k][w] - ref[k]).max()) for k in range(4)))
        _, old = loop(w, 20)
        stale.append(float(np.abs(loop(w, 4, states=old, start=(qa[w], qda[w]))[0] - ref).max()))
        again.append(float(np.abs(loop(w, 4, start=(qa[w], qda[w]), again=True)[0] - ref).max()))
    print(f"joint reset of dofs 32..47: bit-equal to a simulator reset to the same state over 4 steps; the first "
          f"step leaves the reset positions by {first:.1e}; against the oracle with fresh PIDs max|dq| {worst:.2e}; "
          f"on the oracle alone stale PID states move q by {min(stale):.1e}, PIDs reset every step by {min(again):.1e}")
    assert min(stale) > 100 * C.CL_BOUND and min(again) > 100 * C.CL_BOUND
    assert worst <= C.CL_BOUND
