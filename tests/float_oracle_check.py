"""One step of the floating-base wave kernel against the fp64 oracle's
converged LCP (test helper, shared by test_gpu_float_tree.py and
test_gpu_float_rand_oracle.py).

  * random_states: the adversarial start states of the one-step tests (bodies
    sunk into the ground at random tilts, joints beyond their limits, random
    torques), rounded to float32;
  * oracle_step: one FloatWorld step from a start state the simulator
    reported, with a friction coefficient and world wrenches of its own;
  * exact_lcp_acceptance: the acceptance procedure of
    test_one_step_exact_lcp_random_states -- agreement is q-dot within 1e-4
    and q / pose within 1e-5; any other world is accepted only when the GPU's
    own impulses solve the oracle's fp64 two-stage problem
    (tests/lcp_validity.py judge) and its positions moved by what those
    velocities integrate; worlds where the oracle's own exact solve missed the
    complementarity conditions (residual > 1e-6) have no reference and are
    counted, not compared.
"""

import numpy as np

QD_TOL, Q_TOL = 1e-4, 1e-5   # north star: the wave kernel's exact solve against DART's LCP
RES_TOL = 1e-6               # the oracle's own complementarity residual: above it, no reference


def quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_states(cm, W, rng):
    n = cm.n
    lo = np.array(cm.model.lower[:n])
    hi = np.array(cm.model.upper[:n])
    q = rng.uniform(lo, hi, size=(W, n))
    beyond = rng.uniform(size=(W, n)) < 0.1
    q[beyond] = np.where(rng.uniform(size=(W, n)) < 0.5, lo - 1e-3, hi + 1e-3)[beyond]
    qd = rng.uniform(-2, 2, size=(W, n))
    # base: half the worlds near standing height, half low and tilted
    axis = rng.normal(size=(W, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.5, W)
    quat = np.column_stack([np.cos(ang / 2), axis * np.sin(ang / 2)[:, None]])
    z = np.where(np.arange(W) % 2 == 0, rng.uniform(0.30, 0.48, W), rng.uniform(0.02, 0.25, W))
    pos = np.column_stack([rng.uniform(-1, 1, W), rng.uniform(-1, 1, W), z])
    lin = rng.uniform(-0.5, 0.5, (W, 3))
    angv = rng.uniform(-1, 1, (W, 3))
    tau = rng.uniform(-20, 20, size=(W, n))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    return f32(q), f32(qd), f32(np.column_stack([pos, quat])), f32(np.column_stack([lin, angv])), f32(tau)


def oracle_step(oracle, cm, pose, vel, q, qd, tau, mu, pgs_iters, wrench=None, jig=None):
    """A FloatWorld stepped once from the simulator's start state: pose [7]
    (xyz, wxyz), vel [6] (world linear, world angular), joint q / qd, joint
    torques tau; wrench: {link (-1 = base): [force 3, torque 3]} in the world
    frame, or None; jig: a perturbation applied to every input but the
    orientation (the conditioning probe), or None."""
    jig = jig or (lambda a: a)
    R0 = quat_to_R(pose[3:])
    ow = oracle.FloatWorld(cm, ground=True, mu=float(mu), pgs_iters=pgs_iters)
    ow.set_pose(jig(pose[:3]), R0)
    ow.set_twist(jig(R0.T @ vel[3:]), jig(R0.T @ vel[:3]))
    ow.set_joints(jig(q), jig(qd))
    for link, f in (wrench or {}).items():
        ow.wrench[1 + link] = jig(np.asarray(f, dtype=np.float64))
    ow.step(np.full(cm.n, oracle.FORCE, np.int32), tau)
    return ow


def exact_lcp_acceptance(sim, oracle, cm, mu, tau, start, end, wrench=None, label="", dump=None):
    """start = (base_pose, base_velocity, q, qd) before the run, end =
    (base_pose, q, qd, get_state()) after it, all as the simulator returned
    them; mu: one coefficient or one per world; wrench: None or a function
    world -> {link: [6]}.  Asserts the acceptance conditions and returns
    dict(agree, n_ref, no_ref, valid, differ, worlds: the oracle's FloatWorld
    of every world with a reference)."""
    from lcp_validity import contact_set_gap, judge, oracle_ratio, validity
    p0, v0, gq0, gqd0 = start
    p1, gq1, gqd1, state = end
    W = sim.n_worlds
    mus = np.broadcast_to(np.asarray(mu, dtype=np.float64), (W,))
    no_ref, agree, valid, differ = [], 0, [], []
    ratios_agree = []
    worlds = {}
    worst_qd = worst_q = 0.0
    for w in range(W):
        ow = oracle_step(oracle, cm, p0[w], v0[w], gq0[w], gqd0[w], tau[w], mus[w], oracle.PGS_CONVERGED,
                         wrench(w) if wrench else None)
        _, res = oracle.pgs_stats()
        if not 0.0 <= res <= RES_TOL:
            no_ref.append(w)
            continue
        worlds[w] = ow
        prob = oracle.lcp_last()
        e_qd = float(np.abs(gqd1[w] - ow.qd).max())
        e_q = max(float(np.abs(gq1[w] - ow.q).max()), float(np.abs(p1[w, :3] - ow.p).max()))
        if e_qd <= QD_TOL and e_q <= Q_TOL:
            agree += 1
            worst_qd, worst_q = max(worst_qd, e_qd), max(worst_q, e_q)
            if prob is not None and not any(contact_set_gap(ow.contacts, sim.contacts(w))):
                ratios_agree.append(validity(prob, state[w])["ratio"])
            continue
        ok, ratio, graze = judge(prob, ow.contacts, sim.contacts(w), state[w])
        rec = (w, f"{e_qd:.1e}", f"ratio {ratio:.2f}", f"oracle {oracle_ratio(prob) if prob is not None else 0:.2f}",
               f"grazing {[f'{who} {dep:.1e}' for who, dep in graze]}" if graze else "")
        if ok and e_q <= 2e-3 * e_qd + 1e-5:
            valid.append(rec)
        else:
            differ.append(rec)
            if dump is not None:
                dump(dict(prob, gpu_state=state[w]), w)
    unconv = sim.lcp_unconverged()
    n_ref = W - len(no_ref)
    ra = np.array(ratios_agree) if ratios_agree else np.zeros(1)
    print(f"exact LCP, random states, {label}: {agree}/{n_ref} worlds agree with the converged oracle "
          f"(qd <= 1e-4, q / pose <= 1e-5; worst of them qd {worst_qd:.2e}, q / pose {worst_q:.2e}; their GPU "
          f"impulses' fp64 complementarity / tolerance: "
          f"median {np.median(ra):.2f}, max {ra.max():.2f}); other valid fp64 solutions {valid}; "
          f"differ {differ}; oracle unconverged {len(no_ref)}; GPU unconverged {unconv}/{W}")
    assert sim.constraint_overflow() == 0
    assert unconv == 0
    assert not differ
    assert agree >= 0.85 * n_ref
    return dict(agree=agree, n_ref=n_ref, no_ref=no_ref, valid=valid, differ=differ, worlds=worlds,
                worst_qd=worst_qd, worst_q=worst_q)
