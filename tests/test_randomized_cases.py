"""The randomised matrix's tests must be able to fail (CPU, fp64 oracle alone).

tests/test_gpu_randomized_matrix.py bounds the kernel's next observation by
1e-4 against the oracle.  That says something about the mass and the gravity
the kernel steps with only if another mass or gravity would move the
observation by more.  For every (task, mask, pose, substeps) combination that
the GPU file counts as a check of mass or of gravity, the oracle is run against
a WRONG oracle, teacher-forced on the same states, counters and actions:

  * wrong world: world0 = 1, the neighbouring world's physics (what a kernel
    with an off-by-one in its physics arrays, or one that ignores them, does);
  * wrong gravity direction (tilted base): gdir = e_z.

Pass condition: over the live (not done) worlds of the 8 steps, at least 40 %
have a next observation more than 1e-3 away from the right one, ten times the
GPU bound.  This is a condition on the inputs, not a measurement of a kernel.
Measured at W = 65: wrong world 49 % (gravity on the tilted balancing tasks)
to 95 %; wrong gdir 93 % (pendulum) to 99 %.  Gravity on an upright balancing
task gives 0 % (asserted below: that is why those cases do not count).

Also here: the conditions behind the GPU file's exclusion caps, on the oracle
runs of every case at every world count.
"""

import numpy as np
import pytest

import randomized_cases as C

W = 65

# (kind, model, mask name, tilted, substeps) of every combination counted as a check
_COMBOS = sorted({(kind, model, mname, False, 1) for _, kind, model, _, mname in C.ONE_STEP}
                 | {(kind, model, mname, True, 1) for _, kind, model, _, mname in C.TILT}
                 | {(kind, model, "both", False, 2) for _, kind, model, _ in C.TWO_SUBSTEPS})
CHECKS = [c for c in _COMBOS
          if C.counts_as_mass_check(C.MASKS[c[2]]) or C.counts_as_gravity_check(c[0], C.MASKS[c[2]], c[3])]
NOT_COUNTED = [c for c in _COMBOS if c not in CHECKS]
_id = lambda c: f"kind{c[0]}-{c[2]}-{'tilted' if c[3] else 'upright'}-{c[4]}substeps"


def _share(tr, wrong):
    obs, done = C.teacher_forced_obs(tr, wrong)
    live = ~(tr.done | done)
    assert live.sum() >= 4 * W                      # the two TimeLimit steps have no live world
    err = np.abs(obs - tr.obs).max(axis=2)[live]
    return float(np.mean(err > C.SENSITIVE_BY)), float(np.median(err))


@pytest.mark.parametrize("combo", CHECKS, ids=_id)
def test_wrong_world_is_noticeable(oracle, combo):
    kind, model, mname, tilted, substeps = combo
    tr = C.trajectory(kind, model, W, C.MASKS[mname], tilted, substeps)
    _, wrong = C.make_ref(kind, model, W, C.MASKS[mname], tilted, substeps, world0=1)
    share, median = _share(tr, wrong)
    print(f"{_id(combo)}: wrong world moves {100 * share:.0f} % of the live worlds by > 1e-3 (median {median:.1e})")
    assert share >= C.SENSITIVE_SHARE


@pytest.mark.parametrize("combo", [c for c in CHECKS if c[3]], ids=_id)
def test_wrong_gravity_direction_is_noticeable(oracle, combo):
    kind, model, mname, tilted, substeps = combo
    tr = C.trajectory(kind, model, W, C.MASKS[mname], tilted, substeps)
    assert not np.allclose(list(tr.task.gdir), [0.0, 0.0, 1.0], atol=0.04)
    _, wrong = C.make_ref(kind, model, W, C.MASKS[mname], tilted, substeps, gdir=(0.0, 0.0, 1.0))
    share, median = _share(tr, wrong)
    print(f"{_id(combo)}: gdir = e_z moves {100 * share:.0f} % of the live worlds by > 1e-3 (median {median:.1e})")
    assert share >= C.SENSITIVE_SHARE


def test_what_is_not_counted():
    """Exactly gravity alone on the upright balancing tasks; there another
    world's gravity moves no world by 1e-3, so the case could not fail."""
    assert NOT_COUNTED == [(0, "cartpole", "gravity", False, 1), (1, "cartpole", "gravity", False, 1)]
    for kind, model, mname, tilted, substeps in NOT_COUNTED:
        tr = C.trajectory(kind, model, W, C.MASKS[mname], tilted, substeps)
        _, wrong = C.make_ref(kind, model, W, C.MASKS[mname], tilted, substeps, world0=1)
        share, _ = _share(tr, wrong)
        assert share < C.SENSITIVE_SHARE


def test_expected_physics_is_sample_physics(oracle):
    """The table behind `expected_physics` holds oracle.sample_physics(cm, task,
    w, episode[w]), and neighbouring worlds draw different physics."""
    tr = C.trajectory(1, "cartpole", W, C.MASKS["both"])
    assert oracle.sample_physics(tr.cm, tr.task, 7, 0)[1] != oracle.sample_physics(tr.cm, tr.task, 8, 0)[1]
    m, g = C.expected_physics(tr, "cartpole", C.MASKS["both"], np.full(W, 1))
    m1, g1 = oracle.sample_physics(tr.cm, tr.task, 9, 1)
    assert np.array_equal(m[:, 9], m1) and g[9] == g1
    late = np.arange(W) % 5                          # episodes past the table are drawn one by one
    m, g = C.expected_physics(tr, "cartpole", C.MASKS["both"], late)
    for w in (3, 4, 64):
        mw, gw = oracle.sample_physics(tr.cm, tr.task, w, int(late[w]))
        assert np.array_equal(m[:, w], mw) and g[w] == gw


_ALL_RUNS = sorted({(kind, model, Wn, mname, False, 1) for _, kind, model, Wn, mname in C.ONE_STEP}
                   | {(kind, model, Wn, mname, True, 1) for _, kind, model, Wn, mname in C.TILT}
                   | {(kind, model, Wn, "both", False, 2) for _, kind, model, Wn in C.TWO_SUBSTEPS})


@pytest.mark.parametrize("Wn", C.WORLDS)
def test_oracle_stays_within_the_exclusion_cap(oracle, Wn):
    """The GPU file lets a done flag differ only where the oracle's observation
    is within 1e-4 of a threshold, and excludes at most 0.2 % of the (world,
    step) pairs.  With these seeds the oracle's own near-threshold pairs stay
    within that cap at every world count, and there is none at W <= 65, where
    the done comparison is therefore exact.  Every world also steps with the
    physics of episodes 0, 1 and 2."""
    for kind, model, Wc, mname, tilted, substeps in _ALL_RUNS:
        if Wc != Wn:
            continue
        tr = C.trajectory(kind, model, Wn, C.MASKS[mname], tilted, substeps)
        near = sum(int(C.near_threshold(kind, tr.terminal_obs[t] * tr.done[t][:, None]
                                        + tr.obs[t] * ~tr.done[t][:, None]).sum()) for t in range(C.T))
        assert near <= C.MAX_EXCLUDED * Wn * C.T, (kind, mname, tilted, substeps, near)
        if Wn <= 65:
            assert near == 0
        assert tr.episode[C.T].min() >= 2 and tr.steps[C.T].max() <= 2
