"""GPU tests of the scene kernel's large-contact path at its edges
(scene_kernel.hip sc_step use_big / sc_big_constraints; scene.cpp size_big /
ensure_big) against the fp64 scene oracle, exact mode, teacher-forced, one
step from the GPU's own start state.  The cases are those of
tests/scene_big_cases.py; tests/test_scene_big_cases.py asserts on the CPU
that every world takes the stated path, stays clear of the contact detection
threshold and that at most W / 8 worlds of a case are ill-conditioned.

Bounds (as tests/test_gpu_scene_big.py): pose, contact points and joint q
1e-5, base and joint velocities 1e-4, overflow() == 0, lcp_unconverged() ==
0, contact count and (model, link) identities equal to the oracle's.  A world
beyond 1e-4 in velocity passes only if the GPU's own impulses (large-contact
workspace, joint rows included) solve the oracle's fp64 two-stage problem
within lcp_validity.ACCEPT, at most W / 8 worlds per case; a compact step
offers no impulses and fails.  No world is excused by the oracle's
sensitivity.

  case                          points  rows     nv  W
  a  four cubes (rows only)       28     84      24  16   kernel instance 32
  b  five cubes                   36    108      30  16   kernel instance 32
  c  three cubes + welded limb    20   64 / 65   24   8   K = 4 / 5 joints beyond a limit;
                                                          K = 3 / 4 plus a Coulomb row
  d  five cubes + floating chain  36    109      39  16   kernel instance 64, 1 limit row
  e  mixed batch of (b)        28/20/36 84/60/108 30 12   cube 5 absent / spread / as (b);
                                                          each world bit-identical to itself alone
  f  transitions, 40 steps      0..36   0..108   30   4   none -> ground -> large (frictionless worlds), and
                                                          compact -> large -> compact where the faces part

Worst errors measured on the MI355X (pose, point, velocity; q / qd where the
case has joints; worlds accepted as LCP solutions):

  a  7.5e-7  2.4e-8  2.2e-7                     1 of 16 (gap 7.5e-4, ratio 0.49)
  b  9.6e-8  2.4e-8  9.6e-5                     0
  c  1.4e-8  1.2e-8  1.1e-7   5.7e-8 / 3.4e-7   0 (all four parametrisations)
  d  4.9e-8  3.6e-8  4.9e-5   5.0e-8 / 5.0e-7   0
  e  2.8e-8  2.4e-8  1.6e-7                     0
  f  3.0e-8  8.5e-8  5.8e-6                     0 at every step

In (f) the worlds whose cubes close in on each other are frictionless: their
faces meet while the cubes slide on the ground (the sequence none -> ground
-> large needs that), and with friction such an impact is ill-conditioned.
Measured with friction 0.8 in all four worlds: worlds 0 and 2 differ from the
oracle by 2.8e-4 .. 2.3e-3 m/s at the three impact steps 19, 20, 23, as
solutions of the oracle's fp64 LCP (ratio 0.23 .. 0.82 against
lcp_validity.ACCEPT = 4) -- the oracle's own velocities move by 1e-3 .. 1e-2
at exactly those steps under a 1e-6 relative perturbation of its Delassus
matrix (pyoracle.set_lcp_perturbation) -- but with W = 4 no world may be
accepted that way.  The separating worlds keep friction 0.8, the sliding
landing included.  Large-path worlds of (c) and (d) with joint rows: the
GPU's impulses in the fp64 LCP reach ratio 0.92 (c) and 1.01 (d).

Contact readback across a capacity change (scene.cpp ensure_big): the last
step's contacts stay readable through a paused run after an insertion that
reallocates the contact block, whether or not they were read before it.
"""

import numpy as np
import pytest

import lcp_validity as LV
import scene_big_cases as C
from scene_models import cube_urdf
from test_gpu_scene import _scene
from test_gpu_scene_big import _gpu_impulses, _one_step, _validity

pytestmark = pytest.mark.gpu

POS_TOL, VEL_TOL = 1e-5, 1e-4


def _build(case, world=None):
    """the exact-mode Scene of a case at its start state (world: that world
    alone in a scene of one world)"""
    ws = np.arange(case.W) if world is None else np.array([world])
    sc = _scene([(t, (*b, 1, 0, 0, 0), n) for t, b, n in zip(case.texts, case.base, case.names)], len(ws), 50, C.MU,
                exact=True)
    for i, w in enumerate(ws):
        if case.mu[w] != C.MU:
            sc.set_world_friction(float(case.mu[w]), i, 1)
    for m in range(len(case.texts)):
        if case.pose[m] is not None:
            sc.reset_base_pose(m, case.pose[m][ws])
            sc.reset_base_velocity(m, case.vel[m][ws])
        if case.q[m] is not None:
            sc.set("reset_q", case.q[m][ws], m=m)
            sc.set("reset_qd", case.qd[m][ws], m=m)
    for i, w in enumerate(ws):
        for m in range(len(case.texts)):
            if not case.present[w, m]:
                sc.set_present(m, 0, i, 1)
    sc.run(paused=True)
    return sc


def _step_and_check(oracle, sc, case, cms, label, failures=None):
    """one teacher-forced step of every world within the bounds (failures: a
    list that collects what is out of bounds instead of stopping at the first);
    returns the contact and row counts per world"""
    W = case.W
    worst, ill, ncs, info = _one_step(oracle, sc, cms, W, -1, case.mu, VEL_TOL, case.models_of, sensitivity=False)
    print(f"{label} x{W}: contacts {min(ncs)}..{max(ncs)}, rows {min(info['rows'])}..{max(info['rows'])}, one-step " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f", accepted as LCP solutions {info['valid']}")
    bad = []
    if ill:                                         # the sensitivity excuse is off
        bad.append(f"excused by sensitivity {ill}")
    if len(info["valid"]) > W // 8:
        bad.append(f"{len(info['valid'])} worlds accepted as LCP solutions (cap {W // 8}): {info['valid']}")
    if not (worst["pose"] <= POS_TOL and worst["point"] <= POS_TOL and worst["q"] <= POS_TOL):
        bad.append(f"positions {worst}")
    if not (worst["vel"] <= VEL_TOL and worst["qd"] <= VEL_TOL):
        bad.append(f"velocities {worst}")
    if sc.overflow() != 0 or sc.lcp_unconverged() != 0:
        bad.append(f"overflow {sc.overflow()}, unconverged {sc.lcp_unconverged()}")
    if failures is None:
        assert not bad, (label, bad)
    else:
        failures.extend((label, b) for b in bad)
    return ncs, info


@pytest.mark.parametrize("key", [k for k in C.ONE_STEP if k != "e"])
def test_edge_one_step(require_gpu, oracle, key):
    build, big = C.ONE_STEP[key]
    case = build()
    cms = case.compile(oracle)
    sc = _build(case)
    ncs, info = _step_and_check(oracle, sc, case, cms, case.name)
    for w in range(case.W):
        assert (ncs[w], info["rows"][w]) == case.expect[w], (w, ncs[w], info["rows"][w])
        assert C.path(ncs[w], info["rows"][w]) == big(w)
    if key == "a":
        assert all(22 <= nc <= 32 for nc in ncs)    # large by the rows alone
    if big(0) and any(r > 3 * nc for nc, r in case.expect.values()):
        # joint rows inside the large-contact LCP: the GPU's impulses, joint rows
        # by identity, solve the oracle's fp64 two-stage problem in every world
        ratios = [_validity(info["p"][w], *_gpu_impulses(sc, w, info["p"][w], ncs[w])) for w in range(case.W)]
        print(f"{case.name}: GPU impulses in the fp64 LCP, residual ratio {max(ratios):.2f} (accepted up to {LV.ACCEPT})")
        assert max(ratios) <= LV.ACCEPT
    if key.startswith("c"):
        # the limb touches nothing: its joints follow the oracle on either path, accepted or not
        qd = max(e["qd"] for e in info["raw"])
        print(f"{case.name}: limb qd {qd:.2e}")
        assert qd <= VEL_TOL
    sc.close()


def _state(sc, w, models):
    return [(sc.base_pose(m, w, 1), sc.base_velocity(m, w, 1)) for m in models]


def test_mixed_batch_and_batch_identity(require_gpu, oracle):
    """e: large-path worlds (by points, by rows with a model absent) next to
    compact ones in one launch; every world within the bounds of its own
    oracle world and bit-identical to the same world stepped alone."""
    build, big = C.ONE_STEP["e"]
    case = build()
    cms = case.compile(oracle)
    sc = _build(case)
    solo = [_build(case, world=w) for w in range(case.W)]
    ncs, info = _step_and_check(oracle, sc, case, cms, case.name)
    for w in range(case.W):
        assert (ncs[w], info["rows"][w]) == case.expect[w], (w, ncs[w], info["rows"][w])
        assert C.path(ncs[w], info["rows"][w]) == big(w)
        s1 = solo[w]
        s1.run()
        ms = case.models_of(w)
        for (pa, va), (pb, vb) in zip(_state(sc, w, ms), _state(s1, 0, ms)):
            assert np.array_equal(pa, pb) and np.array_equal(va, vb), w
        assert np.array_equal(sc.contacts(w), s1.contacts(0)), w
        assert s1.overflow() == 0 and s1.lcp_unconverged() == 0
        s1.close()
    assert {big(w) for w in range(case.W)} == {True, False}
    sc.close()


def test_path_transitions(require_gpu, oracle):
    """f: 40 teacher-forced steps through no contact, ground contact
    (compact), more than 32 points (large) and, where the faces part again,
    back to the compact path; the bounds at every step."""
    case = C.TRANSITIONS()
    cms = case.compile(oracle)
    sc = _build(case)
    paths, failures = [], []
    for k in range(C.TRANSITION_STEPS):
        ncs, info = _step_and_check(oracle, sc, case, cms, f"{case.name}, step {k}", failures)
        paths.append([C.path(nc, r) for nc, r in zip(ncs, info["rows"])])
    paths = np.array(paths)
    up = {w: [k for k in range(1, len(paths)) if paths[k, w] and not paths[k - 1, w]] for w in range(case.W)}
    down = {w: [k for k in range(1, len(paths)) if not paths[k, w] and paths[k - 1, w]] for w in range(case.W)}
    print(f"{case.name}: compact -> large at steps {up}, large -> compact at steps {down}")
    assert any(up.values()) and any(down.values())
    assert not failures, failures
    sc.close()


# ------------------------------------------------ readback across a capacity change
def _contacts_close(a, b):
    """count and identities equal; points within 1e-5; forces within 0.5 N
    (the velocity bound 1e-4 m/s as a force on a 5 kg cube over 1 ms)"""
    assert len(a) == len(b), (len(a), len(b))
    assert np.array_equal(a[:, 10:14], b[:, 10:14])
    assert np.abs(a[:, 0:3] - b[:, 0:3]).max() <= POS_TOL and np.abs(a[:, 3:6] - b[:, 3:6]).max() <= POS_TOL
    assert np.abs(a[:, 6:9] - b[:, 6:9]).max() <= 0.5


def _valid_identities(sc, rows):
    n = len(sc.models)
    for r in rows:
        ids = [int(v) for v in r[10:14]]
        assert r[10:14].tolist() == ids and ids[0] >= 0
        for mo, li in (ids[0:2], ids[2:4]):
            assert -1 <= mo < n
            assert li == -1 if mo < 0 else -1 <= li < sc.models[mo]["dofs"]


@pytest.mark.parametrize("read_before", [True, False])
def test_contacts_survive_capacity_change(require_gpu, read_before):
    """Two cubes at rest, 50 steps; a third cube inserted 1 m up takes the
    scene's worst case from 20 to 36 points, so ensure_big reallocates the
    contact block.  The paused run that applies the insertion reports the last
    step's contacts of the two cubes unchanged -- read before the insertion
    (the host mirror was current) or not (it was stale) -- and the next step
    matches a twin scene that held all three cubes from the start."""
    c = cube_urdf()
    at = [(0, -0.15, 0.101, 1, 0, 0, 0), (0, 0.15, 0.101, 1, 0, 0, 0), (0, 0, 1.0, 1, 0, 0, 0)]
    sc = _scene([(c, at[0], "cube1"), (c, at[1], "cube2")], 1, 50, 1.0, exact=True)
    twin = _scene([(c, at[0], "cube1"), (c, at[1], "cube2"), (c, at[2], "cube3")], 1, 50, 1.0, exact=True)
    twin.set_present(2, 0)
    for _ in range(50):
        sc.run()
        twin.run()
    want = twin.contacts(0)
    assert len(want) == 8
    if read_before:
        before = sc.contacts(0)
        assert len(before) == 8
        _contacts_close(before, want)
    pose = [sc.base_pose(m) for m in range(2)]
    sc.insert_model(c, at[2], "cube3")
    sc.run(paused=True)
    assert all(np.array_equal(sc.base_pose(m), pose[m]) for m in range(2))   # a paused run advances nothing
    after = sc.contacts(0)
    _valid_identities(sc, after)
    assert len(after) == 8
    if read_before:
        assert np.array_equal(after, before)
    _contacts_close(after, want)
    assert {int(r[10]) for r in after} == {0, 1} and all(int(r[12]) == -1 for r in after)
    # one step on: the twin places its third cube now
    twin.set_present(2, 1)
    twin.run(paused=True)
    sc.run()
    twin.run()
    got, want = sc.contacts(0), twin.contacts(0)
    _valid_identities(sc, got)
    assert len(got) == 8
    _contacts_close(got, want)
    for m in range(3):
        assert np.abs(sc.base_pose(m) - twin.base_pose(m)).max() <= POS_TOL
        assert np.abs(sc.base_velocity(m) - twin.base_velocity(m)).max() <= VEL_TOL
    assert sc.overflow() == 0 and twin.overflow() == 0
    sc.close()
    twin.close()
