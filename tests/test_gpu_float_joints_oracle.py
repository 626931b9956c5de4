"""Per-world joint dynamics against the fp64 oracle: one step of the wave
kernel from the adversarial contact states of float_oracle_check.random_states,
every world with its own damping (nominal + U(0, 0.5) N m s/rad), Coulomb
friction (nominal + U(0, 2) N m) and effort limit (U(0.1, 1) of the nominal, so
that the U(-20, 20) N m torques exceed some limits) -- on every joint of the
quadruped and on the knees and ankles of the iCub (float_joints_ref.ICUB_LEGS:
the row budget) -- compared with oracle_step on that world's own copy of the
ChainModel: cm.model.damping / friction / effort are altered here, the oracle
is not edited.

The acceptance is that of test_gpu_float_inertia_oracle.py: q-dot within
QD_TOL = 1e-4 and q / pose within Q_TOL = 1e-5; any other world is accepted only
through lcp_validity.judge; no unconverged GPU solve, no overflow; agreement in
>= 85 % of the worlds that have a reference.

What keeps it honest, checked without a GPU: the oracle alone has a reference
(complementarity residual <= RES_TOL) in >= 90 % of the worlds; its answer on
the perturbed model differs from its answer on the nominal model by more than
QD_TOL in more than half the worlds; at least one torque is clipped in at least
half the worlds; contact rows plus joint rows stay <= 64 in every world.  On
the GPU the same result compared with the nominal model must miss QD_TOL in
more than half the worlds."""

import numpy as np
import pytest

from float_joints_ref import ORACLE_CASES, STATE_SEED, apply_words, mask_dofs, nominal_words, per_world_words
from float_oracle_check import Q_TOL, QD_TOL, RES_TOL, oracle_step, random_states

MAX_ROWS = 64  # kWaveMaxRows


def _load(oracle, name):
    from mwstep import get_model_file
    return oracle.load_urdf(get_model_file(name))


def _joint_names(name):
    """Joint names in dof order, without a GPU: the simulator's model compiler."""
    from float_joints_ref import model_joint_names
    from mwstep import get_model_file
    return model_joint_names(get_model_file(name))


@pytest.mark.parametrize("name, W, masked", ORACLE_CASES)
def test_oracle_alone_has_a_reference(oracle, name, W, masked):
    cm = _load(oracle, name)
    nominal_cm = _load(oracle, name)
    dofs = mask_dofs(_joint_names(name), masked)
    nominal = nominal_words(cm)
    q, qd, pose, vel, tau = random_states(cm, W, np.random.default_rng(STATE_SEED))
    words = per_world_words(nominal, W, dofs)
    sel = list(range(cm.n)) if dofs is None else dofs
    assert (words[:, sel, 0] >= nominal[sel, 0]).all() and (words[:, sel, 1] >= nominal[sel, 1]).all()
    rest = [d for d in range(cm.n) if d not in sel]
    np.testing.assert_array_equal(words[:, rest], np.tile(nominal[rest], (W, 1, 1)))
    n_ref = differ = clipped = 0
    most_rows = 0
    for w in range(W):
        plain = oracle_step(oracle, nominal_cm, pose[w], vel[w], q[w], qd[w], tau[w], 1.0, oracle.PGS_CONVERGED)
        apply_words(cm, words[w])
        ow = oracle_step(oracle, cm, pose[w], vel[w], q[w], qd[w], tau[w], 1.0, oracle.PGS_CONVERGED)
        _, res = oracle.pgs_stats()
        n_ref += 0.0 <= res <= RES_TOL
        prob = oracle.lcp_last()
        rows = 0 if prob is None else len(prob["b"])
        most_rows = max(most_rows, rows)
        assert rows <= MAX_ROWS, (w, rows)
        differ += float(np.abs(ow.qd - plain.qd).max()) > QD_TOL
        clipped += bool((np.abs(tau[w]) > words[w, :, 2]).any())
    print(f"{name} x{W}: the oracle has a reference in {n_ref} worlds; its answer moves by more than QD_TOL in "
          f"{differ}; a torque is clipped in {clipped}; most LCP rows {most_rows}")
    assert n_ref >= 0.9 * W
    assert differ > W // 2
    assert clipped >= W / 2


@pytest.mark.gpu
@pytest.mark.parametrize("name, W, masked", ORACLE_CASES)
def test_one_step_with_per_world_joint_dynamics(require_gpu, oracle, monkeypatch, name, W, masked):
    from lcp_validity import judge
    from mwstep import get_model_file
    from mwstep import native as N
    from mwstep.sim import Simulator
    monkeypatch.setenv("MWSTEP_WAVE_TREE", "1")
    cm = _load(oracle, name)
    q, qd, pose, vel, tau = random_states(cm, W, np.random.default_rng(STATE_SEED))
    sim = Simulator(get_model_file(name), n_worlds=W, pgs_iters=50)
    assert sim.float_kernel() == 2 and sim.lcp_solver() == (True, 48)
    sim.set_ground_plane(True, 1.0)
    sim.enable_contacts(True)
    nominal = np.stack([sim.joint_dynamics(d, [0])[0] for d in range(sim.dofs)])
    # the simulator's nominal words are the oracle's model, rounded to float32
    np.testing.assert_array_equal(nominal, nominal_words(cm))
    dofs = mask_dofs(sim.joint_names, masked)
    assert dofs is None or dofs == mask_dofs(_joint_names(name), masked)
    words = per_world_words(nominal, W, dofs)
    for d in (range(sim.dofs) if dofs is None else dofs):
        sim.set_joint_dynamics(d, words[:, d])
    for d in range(sim.dofs):
        np.testing.assert_array_equal(sim.joint_dynamics(d), words[:, d])
    sim.set("reset_q", q)
    sim.set("reset_qd", qd)
    sim.reset_base_pose(pose)
    sim.reset_base_velocity(vel)
    sim.run(paused=True)
    p0, v0, gq0, gqd0 = sim.base_pose(), sim.base_velocity(), sim.get("q"), sim.get("qd")
    sim.set_control_mode(N.MODE_FORCE)
    sim.set("force_target", tau)
    sim.run()
    p1, gq1, gqd1, state = sim.base_pose(), sim.get("q"), sim.get("qd"), sim.get_state()

    nominal_cm = _load(oracle, name)
    no_ref, agree, valid, differ, miss_nominal = [], 0, [], [], 0
    worst_qd = worst_q = 0.0
    for w in range(W):
        plain = oracle_step(oracle, nominal_cm, p0[w], v0[w], gq0[w], gqd0[w], tau[w], 1.0, oracle.PGS_CONVERGED)
        miss_nominal += float(np.abs(gqd1[w] - plain.qd).max()) > QD_TOL
        apply_words(cm, words[w])
        ow = oracle_step(oracle, cm, p0[w], v0[w], gq0[w], gqd0[w], tau[w], 1.0, oracle.PGS_CONVERGED)
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
        ok, ratio, graze = judge(prob, ow.contacts, sim.contacts(w), state[w])
        rec = (w, f"{e_qd:.1e}", f"ratio {ratio:.2f}")
        (valid if ok and e_q <= 2e-3 * e_qd + 1e-5 else differ).append(rec)
    unconv, overflow = sim.lcp_unconverged(), sim.constraint_overflow()
    n_ref = W - len(no_ref)
    print(f"{name} x{W}, per-world damping, friction and effort: {agree}/{n_ref} worlds agree with the converged "
          f"oracle on their own model (worst of them qd {worst_qd:.2e}, q / pose {worst_q:.2e}); other valid fp64 "
          f"solutions {valid}; differ {differ}; oracle unconverged {len(no_ref)}; GPU unconverged {unconv}; GPU "
          f"overflow {overflow}; against the nominal model {miss_nominal}/{W} worlds miss QD_TOL")
    sim.close()
    assert overflow == 0 and unconv == 0
    assert n_ref >= 0.9 * W
    assert not differ
    assert agree >= 0.85 * n_ref
    assert miss_nominal > W // 2
