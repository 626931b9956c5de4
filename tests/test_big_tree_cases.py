"""The inputs of tests/test_gpu_big_tree.py in the fp64 oracle alone (CPU):
they are admissible for the wave kernel, and its tests can fail on them.

Per model and variant, one converged oracle step of each of the 256 worlds
from its start state (big_tree_cases.survey).  Conditions, not measurements:

  * no world needs more than 64 LCP rows (the kernel would drop rows, and the
    GPU tests assert constraint_overflow() == 0);
  * the oracle's own unconverged worlds (no reference) stay within W / 20;
  * more than W / 4 worlds are in contact, and at least W / 8 have a contact
    on a body >= 32;
  * over the exact-LCP models, each of the solve's three row widths (<= 16,
    17..32, 33..64 rows; wave_lcp.hpp) is met by at least 16 worlds;
  * tree48 has 48 joints at depth exactly 12, every tree a three-way branch
    point and leaf spheres on both sides of body 32.

Sensitivity (tree40, tree48): an oracle that treats the model as if it ended
at body 32 -- tau[32:] = 0, qd[32:] = 0, or (almost) no mass on the bodies
>= 32 -- moves the first 32 dofs' q-dot by more than 10 QD_TOL in at least
90 % of the worlds, so a kernel that forgot lanes 32..47 anywhere could not
agree within QD_TOL.  tree33 has one body past 32 and is reported, not
counted.  An oracle stepping world w + 1's state misses every world.

The counts every test here prints are recorded in DESIGN.md 3.4b.
"""

import numpy as np
import pytest

import big_tree_cases as C

W = C.W


@pytest.fixture(scope="module")
def surveys(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = C.survey(oracle, name)
        return cache[name]
    return get


def test_tree_shapes():
    for name, n in (("tree33", 33), ("tree40", 40), ("tree48", 48)):
        pa = C.parents(name)
        assert len(pa) == n and all(p < i for i, p in enumerate(pa))
        kids = np.bincount(np.array(pa) + 1, minlength=n + 1)      # [0]: the base
        assert kids.max() >= 3
        leaves = [i for i in range(n) if kids[i + 1] == 0]
        assert any(i >= 32 for i in leaves) and any(i < 32 for i in leaves)
        assert len(leaves) + 1 <= 16                               # the oracle's shape table (OR_MAXFS)
    assert C.depth_of(C.parents("tree48")) == 12
    # the variants draw nothing: same frames, axes and masses
    assert C.urdf("tree48u").count("continuous") == 48 and "prismatic" not in C.urdf("tree48u")
    assert C.urdf("tree48f").count('friction="0.3"') == 24
    strip = lambda t: t.replace('<dynamics friction="0.3"/>', "")
    assert strip(C.urdf("tree48f")) == C.urdf("tree48")
    assert C.urdf("tree48w").endswith(C.urdf("tree48")[len('<robot name="ftree">'):])


def test_existing_trees_keep_their_bits():
    """tree_urdf's new options are keyword-only additions: the 16-joint
    models of test_gpu_float_tree.py are what they were (CRC of the text)."""
    import zlib
    from test_gpu_float_tree import tree_urdf
    got = [zlib.crc32(t.encode()) for t in (tree_urdf(), tree_urdf(damping=2.0), tree_urdf(cylinders=True))]
    assert got == TREE16_CRC


TREE16_CRC = [2987449200, 16687768, 3581149518]   # of the texts before the options were added


@pytest.mark.parametrize("name", C.FLOATING)
def test_inputs_are_admissible(surveys, name):
    s = surveys(name)
    in_contact, high = int((s["n_contacts"] > 0).sum()), int(s["high"].sum())
    buckets, unconv = C.row_buckets(s["rows"]), C.unconverged(s["res"])
    print(f"{name}: {in_contact}/{W} worlds in contact, {high} on a body >= 32, rows at most {s['rows'].max()}, "
          f"worlds in <= 16 / 17..32 / 33..64 / > 64 rows {buckets}, oracle unconverged {unconv}")
    assert s["cm"].n == len(C.parents(name)) > 32
    assert buckets[3] == 0 and s["rows"].max() <= 64
    assert unconv <= W // 20
    assert in_contact > W // 4
    assert high >= W // 8


def test_every_row_width_is_met(surveys):
    total = np.zeros(3, int)
    for name in C.EXACT_MODELS:
        total = np.maximum(total, C.row_buckets(surveys(name)["rows"])[:3])
    print(f"most worlds of one exact-LCP model in <= 16 / 17..32 / 33..64 rows: {total.tolist()}")
    assert (total >= 16).all()


def test_unlimited_variant_has_no_joint_rows(oracle, surveys):
    """tree48u: no limit, no friction -- every LCP row is a contact's"""
    s = surveys("tree48u")
    assert (s["rows"] == 3 * s["n_contacts"]).all()
    m = s["cm"].model
    assert not any(m.limited[:48]) and not any(m.friction[:48])


def _moved(s, qd):
    return int((np.abs(qd[:, :32] - s["qd"][:, :32]).max(axis=1) > C.SENSITIVE_BY).sum())


@pytest.mark.parametrize("name", ["tree33", "tree40", "tree48"])
def test_a_model_cut_at_body_32_is_noticeable(oracle, surveys, name):
    s = surveys(name)
    cm = s["cm"]
    q, qd0, _, _, tau0 = C.states(name)
    light = oracle.load_urdf(C.urdf(name))
    for i in range(32, cm.n):
        light.model.mass[i] *= 1e-6
        for k in range(6):
            light.model.Ic[i][k] *= 1e-6
    cut = lambda a: np.concatenate([a[:32], np.zeros(cm.n - 32)])
    got = {}
    for what in ("tau", "qd", "mass"):
        qd = np.array([C.oracle_world(oracle, light if what == "mass" else cm, name, w, oracle.PGS_CONVERGED,
                                      tau=cut(tau0[w]) if what == "tau" else None,
                                      qd=cut(qd0[w]) if what == "qd" else None).qd for w in range(W)])
        got[what] = _moved(s, qd)
    print(f"{name}: worlds whose first 32 q-dot move by > {C.SENSITIVE_BY:g} when the model ends at body 32: "
          + ", ".join(f"{k} {v}/{W}" for k, v in got.items()))
    if name != "tree33":
        assert min(got.values()) >= 0.9 * W


@pytest.mark.parametrize("name", ["tree33", "tree40", "tree48"])
def test_wrong_world_misses_every_world(oracle, surveys, name):
    s = surveys(name)
    qd = np.array([C.oracle_world(oracle, s["cm"], name, w, oracle.PGS_CONVERGED, world=(w + 1) % W).qd
                   for w in range(W)])
    miss = int((np.abs(qd - s["qd"]).max(axis=1) > C.SENSITIVE_BY).sum())
    print(f"{name}: world w + 1's state misses {miss}/{W} worlds")
    assert miss == W


def test_closed_loop_horizon(oracle):
    """The closed loop of test_gpu_big_tree.py is compared at C.CL_STEPS steps
    with q within C.CL_BOUND: there the oracle's own trajectory must move by
    less than a tenth of the bound when posture and target are perturbed by
    3e-7 relative (four seeds, every world), and the joints must really move."""
    cm, post, tgt = C.closed_loop_inputs(oracle)
    assert cm.n == 48 and C.CL_STEPS <= 200
    sens, moved = 0.0, []
    for w in range(C.CL_WORLDS):
        ref, _ = C.closed_loop_reference(oracle, cm, post[w], tgt[w], C.CL_STEPS)
        moved.append(float(np.abs(ref[-1] - ref[0])[32:].max()))
        for k in range(4):
            jig, _ = C.closed_loop_reference(oracle, cm, post[w], tgt[w], C.CL_STEPS, 3e-7, k)
            sens = max(sens, float(np.abs(jig - ref).max()))
    print(f"closed loop, {C.CL_STEPS} steps: the oracle moves by {sens:.2e} under a 3e-7 perturbation (bound "
          f"{C.CL_BOUND:g}); the joints >= 32 travel {min(moved):.2f} .. {max(moved):.2f}")
    assert sens < C.CL_BOUND / 10
    assert min(moved) > 1000 * C.CL_BOUND


def test_welded_tree(oracle):
    """tree48w: the same 48 joints on a fixed base (the oracle's fixed-tree step)"""
    cm = oracle.load_urdf(C.urdf(C.WELDED))
    assert cm.n == 48 and not cm.floating
    free = oracle.load_urdf(C.urdf("tree48"))
    assert list(cm.model.parent[:48]) == list(free.model.parent[:48])
    assert np.allclose(cm.base_p, [0, 0, 1.5])
    q, qd, _, _, tau = C.states(C.WELDED)
    mode = np.full(48, oracle.FORCE, np.int32)
    right = np.array([oracle.step(cm, 1e-3, q[w], qd[w], mode, tau[w], oracle.PGS_CONVERGED)[1] for w in range(W)])
    cut = np.array([oracle.step(cm, 1e-3, q[w], qd[w], mode, np.concatenate([tau[w, :32], np.zeros(16)]),
                                oracle.PGS_CONVERGED)[1] for w in range(W)])
    moved = int((np.abs(cut[:, :32] - right[:, :32]).max(axis=1) > C.SENSITIVE_BY).sum())
    print(f"{C.WELDED}: tau[32:] = 0 moves the first 32 q-dot of {moved}/{W} worlds")
    assert moved >= 0.9 * W


def _own_model_survey(oracle, name, alter=None, mus=None, wrench=None):
    """(worlds with a reference, worlds whose q-dot differs from the plain
    model's step by more than QD_TOL, most LCP rows) of the converged oracle,
    every world on its own model / coefficient / wrenches."""
    cm, plain_cm = oracle.load_urdf(C.urdf(name)), oracle.load_urdf(C.urdf(name))
    n_ref = differ = most = 0
    for w in range(W):
        plain = C.oracle_world(oracle, plain_cm, name, w, oracle.PGS_CONVERGED)
        if alter:
            alter(cm, w)
        q, qd, pose, vel, tau = C.states(name)
        ow = C.oracle_step(oracle, cm, pose[w], vel[w], q[w], qd[w], tau[w], C.MU if mus is None else mus[w],
                           oracle.PGS_CONVERGED, wrench(w) if wrench else None)
        prob = oracle.lcp_last()
        n_ref += prob is None or 0.0 <= oracle.pgs_stats()[1] <= C.RES_TOL
        most = max(most, 0 if prob is None else len(prob["b"]))
        differ += float(np.abs(ow.qd - plain.qd).max()) > C.QD_TOL
    return n_ref, differ, most


def test_per_world_inputs_are_admissible(oracle):
    """The per-world tests of test_gpu_big_tree.py on the oracle alone: a
    reference in >= 90 % of the worlds, at most 64 rows, and parameters that
    move more than half the worlds by more than QD_TOL."""
    from float_joints_ref import apply_words, nominal_words
    from test_gpu_float_inertia_oracle import _apply_words, _draw_words, _nominal_words
    got = {}
    link_words = _draw_words(_nominal_words(oracle.load_urdf(C.urdf("tree48"))), W, C.PAYLOAD_MAX)
    got["link parameters"] = _own_model_survey(oracle, "tree48", lambda cm, w: _apply_words(cm, link_words[w]))
    for name, dofs in (("tree48", C.JOINT_DOFS), ("tree48u", (47,))):
        nominal = nominal_words(oracle.load_urdf(C.urdf(name)))
        words = C.joint_words(nominal, name, dofs)
        rest = [d for d in range(48) if d not in dofs]
        np.testing.assert_array_equal(words[:, rest], np.tile(nominal[rest], (W, 1, 1)))
        assert (words[:, list(dofs), 1] > 0).all() and any(d >= 32 for d in dofs)
        got[f"joint dynamics, {name}"] = _own_model_survey(oracle, name, lambda cm, w: apply_words(cm, words[w]))
        if name == "tree48":
            clipped = int((np.abs(C.states(name)[4]) > words[:, :, 2]).any(axis=1).sum())
            print(f"a torque is clipped in {clipped}/{W} worlds")
            assert clipped >= W / 2
    wr = C.wrenches()
    got["wrenches"] = _own_model_survey(oracle, "tree48", wrench=lambda w: {b: f[w] for b, f in wr.items()})
    mus = np.array([[0.0, 0.05, 0.3, 0.8, 1.2][w % 5] for w in range(W)])
    got["ground friction"] = _own_model_survey(oracle, "tree48", mus=mus)
    for what, (n_ref, differ, most) in got.items():
        print(f"{what}: a reference in {n_ref}/{W} worlds, {differ} moved by more than QD_TOL, at most {most} rows")
        assert n_ref >= 0.9 * W and most <= 64
        assert differ > (W // 8 if what == "ground friction" else W // 2)
    signal = C.friction_signal(oracle, "tree48", mus)
    print(f"ground friction: {signal} worlds moved by more than 10 QD_TOL")
    assert signal >= W // 8


def test_warm_landing(oracle):
    """tree48f lands within C.WARM_STEPS steps in every world, and the warm
    record of the oracle's warm mode carries Coulomb impulses on the joints
    >= 32 that have friction (the even ones), none on the odd ones."""
    cm, post, z = C.warm_inputs(oracle)
    kp, kd = C.WARM_PD
    mode = np.full(cm.n, oracle.FORCE, np.int32)
    for w in range(len(z)):
        ow = oracle.FloatWorld(cm, pgs_iters=50, pgs_tol=1e-6, warm_start=True)
        ow.set_pose([0, 0, z[w]], np.eye(3))
        ow.set_joints(post[w], np.zeros(cm.n))
        hold = lambda: np.clip(-kp * (ow.q - post[w]) - kd * ow.qd, -50, 50)
        landed = [k for k in range(C.WARM_STEPS) if ow.step(mode, hold())]
        rows = ow.warm[3 * oracle.OR_MAXFC:].reshape(48, 3)
        print(f"world {w}: base at {z[w]:.3f}, first contact at step {landed[0]}, in contact for {len(landed)} steps")
        assert landed and landed[0] < C.WARM_STEPS // 2
        assert (rows[32::2, 2] != 0).sum() >= 4 and not rows[33::2, 2].any()


@pytest.mark.parametrize("name", ["tree16f", "tree48f"])
def test_friction_trees_have_twin_rows(oracle, name):
    """What the friction trees are for (test_gpu_float_tree.py tree16f, tree48f
    here): in many worlds a joint carries its limit row and its Coulomb row,
    one Jacobian row twice -- A is singular up to the joint CFM, beyond fp32
    (cond(A) > 1e9) -- within 64 rows and with a reference in every world."""
    from float_oracle_check import random_states
    from test_gpu_float_tree import tree_urdf
    text = tree_urdf(friction=0.3) if name == "tree16f" else C.urdf(name)
    cm = oracle.load_urdf(text)
    q, qd, pose, vel, tau = random_states(cm, W, np.random.default_rng(C.STATE_SEED))
    twins = worst = most = unconv = 0
    for w in range(W):
        C.oracle_step(oracle, cm, pose[w], vel[w], q[w], qd[w], tau[w], C.MU, oracle.PGS_CONVERGED)
        p = oracle.lcp_last()
        unconv += not 0.0 <= oracle.pgs_stats()[1] <= C.RES_TOL
        dofs = [(int(i) - 3 * oracle.OR_MAXFC) // 3 for i in p["wid"] if i >= 3 * oracle.OR_MAXFC]
        most = max(most, len(p["b"]))
        if len(dofs) > len(set(dofs)):
            twins += 1
            worst = max(worst, float(np.linalg.cond(p["A"])))
    print(f"{name}: {twins}/{W} worlds with a joint of two rows (cond(A) up to {worst:.1e}), at most {most} rows, "
          f"oracle unconverged {unconv}")
    assert twins > W // 4 and worst > 1e9 and most <= 64 and unconv <= W // 20
