"""The cases of tests/test_gpu_scene_big_edges.py in the fp64 scene oracle
alone (CPU): what the GPU tests rely on, so that they cannot pass vacuously.

Per case and world, one exact-mode oracle step (oracle.SceneWorld,
oracle.lcp_last) from the case's start state:

  * the path: nc oracle contacts, len(p["b"]) rows (tj = rows - 3 nc joint
    rows); sc_step leaves the compact path for nc > 32 or rows > 64.  Every
    world takes the path its case is built for, with the point and row counts
    the case states;
  * clear of the detection threshold: no contact depth within
    lcp_validity.GRAZE (1e-6 m) of zero, no cube corner or face within that
    distance above the ground or its neighbour's face, so fp32 and fp64
    detect the same set;
  * the conditioning cap: a world is ill-conditioned when the oracle's own
    velocities move by more than 1e-4 under a 3e-7 relative perturbation of
    its inputs (four seeds); at most W / 8 worlds of a case are.  The GPU
    tests accept at most that many worlds as different solutions of the LCP.

The transition case runs free for its 40 steps: the same clearance at every
step, both transitions (compact -> large, large -> compact) in some world.
"""

import numpy as np
import pytest

import lcp_validity as LV
import scene_big_cases as C

SENS = 1e-4


def _clearance(case, w, poses, Rs, contacts):
    """cubes only (the chains touch nothing, or only what the contact depths show)"""
    cubes = [m for m in case.models_of(w) if case.names[m].startswith("c")]
    ground, pair = C.cube_gaps([poses[m] for m in cubes], [Rs[m] for m in cubes])
    depth = np.array([c[9] for c, _ in contacts]) if contacts else np.array([1.0])
    assert np.abs(ground).min() >= LV.GRAZE and depth.min() >= LV.GRAZE, (case.name, w)
    assert len(pair) == 0 or np.abs(pair).min() >= LV.GRAZE, (case.name, w)
    return min(float(np.abs(ground).min()), float(depth.min()), float(np.abs(pair).min()) if len(pair) else 1.0)


def _sensitivity(oracle, cms, ow, make):
    sens = 0.0
    for k in range(4):
        ow2 = make(3e-7, k)
        ow2.step()
        for m, cm in enumerate(cms):
            if cm.floating:
                sens = max(sens, float(np.abs(ow2.V(m) - ow.V(m)).max()))
            if cm.n:
                sens = max(sens, float(np.abs(ow2.qd(m) - ow.qd(m)).max()))
    return sens


@pytest.mark.parametrize("key", list(C.ONE_STEP))
def test_one_step_case(oracle, key):
    build, big = C.ONE_STEP[key]
    case = build()
    cms = case.compile(oracle)
    ill, clear, tjs = [], 1.0, set()
    for w in range(case.W):
        ms = case.models_of(w)
        here = [cms[m] for m in ms]
        ow = C.oracle_world(oracle, cms, case, w, case)
        poses, Rs = [ow.p(m) for m in ms], [ow.R(m) for m in ms]
        ow.step()
        nc, rows, p = C.counts(oracle, ow)
        tjs.add(rows - 3 * nc)
        assert (nc, rows) == case.expect[w], (key, w, nc, rows)
        assert C.path(nc, rows) == big(w), (key, w, nc, rows)
        if rows - 3 * nc:
            # the joint rows carry their identities (the GPU tests map them by these)
            assert (p["wid"][3 * nc:] >= LV.OR_WARM_JOINT0).all() and (p["kind"][3 * nc:] == 2).all()
        clear = min(clear, _clearance(case, w, poses, Rs, ow.contacts))
        sens = _sensitivity(oracle, here, ow, lambda eps, k: C.oracle_world(oracle, cms, case, w, case, eps, k))
        if sens > SENS:
            ill.append((w, round(sens, 6)))
    print(f"{case.name}: W {case.W}, joint rows {sorted(tjs)}, least clearance {clear:.2e}, ill-conditioned {ill}")
    assert len(ill) <= case.W // 8, ill


def test_case_a_is_rows_only_and_c_straddles_64(oracle):
    """the counts the cases are built for: 22..32 points on the large path (a), and 64
    / 65 rows from states that differ only in the joints beyond a limit (c)"""
    a = C.ONE_STEP["a"][0]()
    assert all(22 <= nc <= 32 and C.path(nc, rows) for nc, rows in a.expect.values())
    for lo, hi in (("c-K4", "c-K5"), ("c-K3-friction", "c-K4-friction")):
        c4, c5 = C.ONE_STEP[lo][0](), C.ONE_STEP[hi][0]()
        assert {r for _, r in c4.expect.values()} == {64} and {r for _, r in c5.expect.values()} == {65}
        same = c4.q[3] == c5.q[3]
        assert same.sum() == same.size - c4.W and np.array_equal(c4.qd[3], c5.qd[3])
        assert all(np.array_equal(c4.pose[m], c5.pose[m]) and np.array_equal(c4.vel[m], c5.vel[m]) for m in range(3))


def test_transition_case(oracle):
    case = C.TRANSITIONS()
    cms = case.compile(oracle)
    up, down, ill, clear = {}, {}, [], 1.0
    K = len(cms)
    for w in range(case.W):
        ow = C.oracle_world(oracle, cms, case, w, case)
        paths, ncs = [], []
        for k in range(C.TRANSITION_STEPS):
            poses, Rs, Vs = [ow.p(m) for m in range(K)], [ow.R(m) for m in range(K)], [ow.V(m) for m in range(K)]

            def twin(eps, seed):
                r = np.random.default_rng(seed)
                o2 = oracle.SceneWorld(cms, pgs_iters=-1, mu=float(case.mu[w]))
                for m in range(K):
                    o2.set_pose(m, poses[m] * (1 + eps * r.uniform(-1, 1, 3)), Rs[m])
                    o2.set_twist(m, Vs[m][:3] * (1 + eps * r.uniform(-1, 1, 3)), Vs[m][3:] * (1 + eps * r.uniform(-1, 1, 3)))
                return o2

            ow.step()
            nc, rows, _ = C.counts(oracle, ow)
            clear = min(clear, _clearance(case, w, poses, Rs, ow.contacts))
            if nc and _sensitivity(oracle, cms, ow, twin) > SENS:
                ill.append((w, k))
            paths.append(C.path(nc, rows))
            ncs.append(nc)
        up[w] = [k for k in range(1, len(paths)) if paths[k] and not paths[k - 1]]
        down[w] = [k for k in range(1, len(paths)) if not paths[k] and paths[k - 1]]
        print(f"{case.name}: world {w} points per step {ncs}, compact -> large at {up[w]}, large -> compact at {down[w]}")
    print(f"least clearance {clear:.2e}, ill-conditioned (world, step) {ill}")
    assert any(up.values()) and any(down.values())
    assert len(ill) <= case.W // 8, ill
