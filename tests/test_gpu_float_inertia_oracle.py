"""Per-world link parameters against the fp64 oracle: one step of the wave
kernel's WPAR instances from the adversarial contact states of
float_oracle_check.random_states, every world with link masses scaled by
U(0.5, 2) (mass and origin inertia, the centre of mass kept) and a point
payload on the base (up to 10 kg on the quadruped, 5 kg on the iCub, within
+-0.1 m), compared with oracle_step on that world's own copy of the
ChainModel -- cm.model.mass / com / Ic and cm.free are altered here, with Ic
from the float32 origin words by the fp64 parallel-axis shift; the oracle is
not edited.

The acceptance is that of exact_lcp_acceptance, restated per world because
every world has its own model: q-dot within QD_TOL = 1e-4 and q / pose within
Q_TOL = 1e-5; any other world is accepted only through lcp_validity.judge; no
unconverged GPU solve, no overflow; agreement in >= 85 % of the worlds that have
a reference.

What keeps it honest: the seed is chosen so that the oracle alone has a
reference (complementarity residual <= RES_TOL) in >= 90 % of the worlds,
checked without a GPU; and the same GPU result compared with the nominal
model must miss QD_TOL in most worlds, else the parameters did nothing."""

import numpy as np
import pytest

from float_inertia_ref import PAYLOAD, SCALE, apply_ref, inertia_about_com
from float_oracle_check import Q_TOL, QD_TOL, RES_TOL, oracle_step, random_states

CASES = [("quadruped", 70, 10.0), ("icub", 40, 5.0)]
STATE_SEED, PARAM_SEED = 11, 61


def _apply_words(cm, words):
    """Alter this ChainModel in place to the float32 origin words [n + 1, 10], base first."""
    m, c, Ic = inertia_about_com(words)
    six = lambda I: [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
    cm.free.mass = m[0]
    for k in range(3):
        cm.free.com[k] = c[0][k]
    for k, v in enumerate(six(Ic[0])):
        cm.free.Ic[k] = v
    for i in range(cm.n):
        cm.model.mass[i] = m[1 + i]
        for k in range(3):
            cm.model.com[i][k] = c[1 + i][k]
        for k, v in enumerate(six(Ic[1 + i])):
            cm.model.Ic[i][k] = v


def _nominal_words(cm):
    """The float32 origin words of the oracle's own model [n + 1, 10]."""
    from mwstep.sim import Simulator
    F, M = cm.free, cm.model
    sym = lambda v: np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]])
    rows = [Simulator.inertial_words(F.mass, list(F.com), sym(list(F.Ic)))]
    rows += [Simulator.inertial_words(M.mass[i], list(M.com[i]), sym(list(M.Ic[i]))) for i in range(cm.n)]
    return np.stack(rows)


def _draw_words(nominal, W, payload_max):
    """[W, n + 1, 10] float32 words: every link scaled, the payload on the base."""
    rng = np.random.default_rng(PARAM_SEED)
    k = nominal.shape[0]
    s = rng.uniform(0.5, 2.0, (W, k)).astype(np.float32)
    mp = rng.uniform(0.0, payload_max, W).astype(np.float32)
    p = rng.uniform(-0.1, 0.1, (W, 3)).astype(np.float32)
    words = np.empty((W, k, 10), np.float32)
    for w in range(W):
        words[w] = apply_ref(SCALE, nominal, s[w], np.zeros(k), np.zeros((k, 3))).astype(np.float32)
        words[w, :1] = apply_ref(PAYLOAD, words[w, :1], s[w, :1], mp[w:w + 1], p[w:w + 1]).astype(np.float32)
    return words


def _load(oracle, name):
    from mwstep import get_model_file
    return oracle.load_urdf(get_model_file(name))


@pytest.mark.parametrize("name, W, payload_max", CASES)
def test_oracle_alone_has_a_reference(oracle, name, W, payload_max):
    """No GPU: from the same states and parameters the oracle's own exact solve
    meets its complementarity conditions in >= 90 % of the worlds."""
    cm = _load(oracle, name)
    nominal = _nominal_words(cm)
    q, qd, pose, vel, tau = random_states(cm, W, np.random.default_rng(STATE_SEED))
    words = _draw_words(nominal, W, payload_max)
    n_ref = 0
    for w in range(W):
        _apply_words(cm, words[w])
        oracle_step(oracle, cm, pose[w], vel[w], q[w], qd[w], tau[w], 1.0, oracle.PGS_CONVERGED)
        _, res = oracle.pgs_stats()
        n_ref += 0.0 <= res <= RES_TOL
    print(f"{name} x{W}: the oracle has a reference in {n_ref} worlds")
    assert n_ref >= 0.9 * W
    # a model altered to its own nominal words is the model (the shift and its inverse, fp64 of float32 words)
    fresh = _load(oracle, name)
    _apply_words(cm, nominal)
    assert abs(cm.free.mass - fresh.free.mass) <= 1e-6 * fresh.free.mass
    assert max(abs(cm.model.Ic[i][k] - fresh.model.Ic[i][k]) for i in range(cm.n) for k in range(6)) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("name, W, payload_max", CASES)
def test_one_step_with_per_world_parameters(require_gpu, oracle, monkeypatch, name, W, payload_max):
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
    nominal = np.stack([sim.link_params(link, [0])[0] for link in range(-1, sim.dofs)])
    # the simulator's nominal words are the oracle's model, rounded to float32
    np.testing.assert_allclose(nominal, _nominal_words(cm), rtol=1e-5, atol=1e-7)
    words = _draw_words(nominal, W, payload_max)
    for link in range(-1, sim.dofs):
        sim.set_link_params(link, words[:, link + 1])
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
        _apply_words(cm, words[w])
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
    print(f"{name} x{W}, per-world masses and payload: {agree}/{n_ref} worlds agree with the converged oracle on "
          f"their own model (worst of them qd {worst_qd:.2e}, q / pose {worst_q:.2e}); other valid fp64 solutions "
          f"{valid}; differ {differ}; oracle unconverged {len(no_ref)}; GPU unconverged {unconv}; against the "
          f"nominal model {miss_nominal}/{W} worlds miss QD_TOL")
    sim.close()
    assert overflow == 0 and unconv == 0
    assert n_ref >= 0.9 * W
    assert not differ
    assert agree >= 0.85 * n_ref
    assert miss_nominal > W // 2
