"""The conditions tests/test_gpu_panda_variants.py relies on, asserted in the
fp64 oracle alone (and, for the wrong-factor mistake, in the host build of
chain_dyn.hpp): no GPU.

  * discrimination: on every state set used with a damped or frictional
    variant the coefficients move the oracle's answer by >= 10x the bound the
    GPU test asserts, and an impulse factor taken from the damped matrix (the
    mistake a wrong second Cholesky factor in the group kernel would make) is
    >= 10x the bound away on states with a limit row;
  * friction row coverage: rows that end strictly inside their box, rows that
    end on its bound, dofs with a velocity of exactly 0 after the update;
  * PID coverage of the rollout: both integral clamps, both command clamps, the
    effort clip where no command clamp binds;
  * threshold clearance of every start state.
The counts are printed (pytest -s)."""

import numpy as np
import pytest

import panda_cases as pc

STEP_SEEDS = (21, 22, 23, 24)   # the four rounds of the GPU one-step tests
W_STEP = 64


@pytest.fixture(scope="module")
def step_sets(oracle):
    return [pc.step_states(oracle, W_STEP, s) for s in STEP_SEEDS]


def test_variants_load_and_dispatch(oracle):
    """The library takes every variant, reports the flags the dispatch reads
    (needs_cons / needs_dual through the uploaded parameter block) and keeps
    the Panda topology for the limit-free model."""
    import ctypes
    from mwstep import native as N
    for name in pc.VARIANTS:
        model, params, cm = pc.variant(oracle, name)
        cfg = N.MwConfig(1e-3, 1.0, 1, 1, 0, 0)
        h = ctypes.c_void_p()
        N.check(N.lib().mw_create(ctypes.byref(cfg), ctypes.byref(h)))
        try:
            pose = np.array([0, 0, 0, 1, 0, 0, 0.0])
            N.check(N.lib().mw_load_model(h, model.encode(), N.dptr(pose), b""))
            for (dof, which), v in params.items():
                N.check(N.lib().mw_set_joint_param(h, dof, which, v))
            n = ctypes.c_int32()
            N.check(N.lib().mw_dofs(h, ctypes.byref(n)))
            assert n.value == 9 == cm.n
            buf = (ctypes.c_int32 * (8 + 40 * 48))()   # ChainF: 8 header words, 48 bodies of 40
            N.check(N.lib().mw_device_params(h, buf, ctypes.sizeof(buf)))
            words = np.frombuffer(buf, dtype=np.int32).copy()
            blk = np.frombuffer(buf, dtype=np.float32).copy()
        finally:
            N.lib().mw_destroy(h)
        damping, friction = pc.coefficients(name)
        # ChainF.flags: damping 1 (needs_dual), limits 2 | friction 4 (needs_cons)
        assert words[1] == (1 if any(damping) else 0) | (0 if name == "free" else 2) | (4 if any(friction) else 0)
        for i in range(9):
            body = 8 + 40 * i
            assert blk[body + 26] == np.float32(damping[i]) and blk[body + 27] == np.float32(friction[i])
            assert words[body + 32] == (0 if name == "free" else 1) == cm.model.limited[i]
            assert words[body + 36] == [-1, 0, 1, 2, 3, 4, 5, 6, 6][i]   # the Panda tree


def test_threshold_clearance(oracle, step_sets):
    """No start state has a joint within 1e-4 rad of a limit: at least 1e-4
    inside or at least 1e-3 beyond, so fp32 and fp64 agree on every limit row
    and no disagreement has to be excused."""
    for q, _, tgt in step_sets:
        inside, beyond = pc.clearance(oracle, q)
        assert inside >= pc.INSIDE and beyond >= pc.BEYOND, (inside, beyond)
    inside, beyond = pc.clearance(oracle, pc.rollout_start(oracle))
    assert inside >= pc.INSIDE and beyond >= pc.BEYOND
    q = np.concatenate(pc.wave_sharing_worlds(oracle))
    inside, beyond = pc.clearance(oracle, q)
    assert inside >= pc.INSIDE and beyond >= pc.BEYOND
    print(f"clearance: one-step sets ok; rollout start {pc.clearance(oracle, pc.rollout_start(oracle))}")


def _moved(a, b):
    """(median, smallest) over the states of the largest |dqd| per state."""
    per_state = np.abs(a - b).max(axis=1)
    return float(np.median(per_state)), float(per_state.min())


@pytest.mark.parametrize("gains", ["force", "kat"])
def test_coefficients_move_the_answer(oracle, step_sets, gains):
    """Per variant and round of states: the median over the 64 states of the
    largest |dqd| the coefficients cause is >= 10 x the 1e-4 the GPU test
    asserts, so in every round at least half of the worlds would each fail it
    by that factor if a kernel dropped the coefficients (the smallest single
    state is printed: a state whose damped joints are all slow moves less)."""
    g = pc.force_gains(oracle) if gains == "force" else pc.kat_gains()
    _, _, plain = pc.variant(oracle, "shipped")
    for name in ("damped", "frictional", "both") + (("partial",) if gains == "force" else ()):
        _, _, cm = pc.variant(oracle, name)
        med, low = np.inf, np.inf
        for q, qd, tgt in step_sets:
            m, lo = _moved(pc.oracle_one_step(oracle, cm, q, qd, tgt, g)[1],
                           pc.oracle_one_step(oracle, plain, q, qd, tgt, g)[1])
            med, low = min(med, m), min(low, lo)
        print(f"{gains} gains, {name}: |dqd| from the coefficients, median over states {med:.2e}, "
              f"smallest state {low:.2e}")
        assert med >= 10 * pc.QD_STEP, (name, med)


def test_free_variant_damping_moves_the_answer(oracle, step_sets):
    """The limit-free model: dropping the implicit damping (what a !CONS
    dispatch that forgot it would do) moves qd by >= 10 x the bound."""
    _, _, cm = pc.variant(oracle, "free")
    _, _, und = pc.variant(oracle, "free")
    for i in range(9):
        und.model.damping[i] = 0.0
    g = pc.force_gains(oracle)
    med, low = np.inf, np.inf
    for q, qd, tgt in step_sets:
        m, lo = _moved(pc.oracle_one_step(oracle, cm, q, qd, tgt, g)[1],
                       pc.oracle_one_step(oracle, und, q, qd, tgt, g)[1])
        med, low = min(med, m), min(low, lo)
    print(f"free: |dqd| from the damping, median over states {med:.2e}, smallest state {low:.2e}")
    assert med >= 10 * pc.QD_STEP


def test_friction_row_coverage(oracle, step_sets):
    """The constant-force case on `frictional` and `both`: friction rows that
    stick, rows that slide, and -- in the zero-gravity rest worlds of
    test_rest_without_gravity -- dofs whose velocity is exactly 0 after the
    update, which get no row."""
    for name in ("frictional", "both", "partial"):
        _, _, cm = pc.variant(oracle, name)
        stick = slide = none = limit = both_rows = 0
        for q, qd, _ in step_sets:
            _, _, lim, fric = pc.force_step_rows(oracle, cm, q, qd)
            stick += int((fric == oracle.ROW_STICK).sum())
            slide += int((fric == oracle.ROW_SLIDE).sum())
            none += int((fric == oracle.ROW_NONE).sum())
            limit += int((lim != oracle.ROW_NONE).sum())
            both_rows += int(((lim != oracle.ROW_NONE) & (fric != oracle.ROW_NONE)).sum())
        print(f"{name}: friction rows sticking {stick}, sliding {slide}, none {none}; limit rows {limit}, "
              f"dofs with both rows {both_rows}")
        assert stick >= 20 and slide >= 200 and limit >= 200 and both_rows >= 100
        # under gravity no velocity is exactly 0: only a dof without friction has no row
        assert none == (4 * 4 * W_STEP if name == "partial" else 0)
    # at rest without gravity and without force every velocity stays exactly 0
    _, _, cm = pc.variant(oracle, "both")
    g = [cm.model.gravity_base[k] for k in range(3)]
    for k in range(3):
        cm.model.gravity_base[k] = 0.0
    q, _, _ = step_sets[0]
    inside = np.all((q > pc.shipped_limits(oracle)[0]) & (q < pc.shipped_limits(oracle)[1]), axis=1)
    n0 = 0
    for w in np.flatnonzero(inside)[:8]:
        oq, oqd, lim, fric = oracle.step_rows(cm, 1e-3, q[w].astype(float), np.zeros(9), [oracle.FORCE] * 9,
                                              np.zeros(9), 20)
        assert np.all(oqd == 0.0) and np.all(oq == q[w].astype(float)) and np.all(fric == oracle.ROW_NONE)
        n0 += 9
    for k in range(3):
        cm.model.gravity_base[k] = g[k]
    print(f"rest without gravity: {n0} dofs with qd == 0 after the update, no row")
    assert n0 >= 9


def test_wrong_impulse_factor_is_visible(oracle, step_sets, panda_file):
    """The host build of chain_dyn.hpp with dual=False on the damped models
    takes the impulse columns from M + dt D instead of M: on the states with a
    limit row that is >= 10 x the GPU test's bound from the oracle, while the
    right factor (dual=True) is inside it."""
    from test_host_dyn import build_harness, _params, _substep
    hd = build_harness()
    for name in ("damped", "both"):
        _, params, cm = pc.variant(oracle, name)
        P = _params(hd, panda_file, [(d, which, v) for (d, which), v in params.items()])
        wrong = right = 0.0
        q, qd, _ = step_sets[0]
        oq, oqd, lim, _ = pc.force_step_rows(oracle, cm, q, qd)
        for w in range(len(q)):
            if not (lim[w] != oracle.ROW_NONE).any():
                continue
            z = np.zeros(9)
            a = _substep(hd, P, q[w], qd[w], pc.TAU, z, z, cons=True, dual=False)[1]
            b = _substep(hd, P, q[w], qd[w], pc.TAU, z, z, cons=True, dual=True)[1]
            wrong = max(wrong, float(np.abs(a - oqd[w]).max()))
            right = max(right, float(np.abs(b - oqd[w]).max()))
        print(f"{name}: host harness max|dqd| vs oracle on limit-row states: dual=False {wrong:.2e}, "
              f"dual=True {right:.2e}")
        assert wrong >= 10 * pc.QD_STEP and right <= pc.QD_STEP


def test_rollout_pid_coverage(oracle):
    """The rollout case in the oracle, steps_per_run 1 and 2: the integral
    clamp and the command clamp bind on both sides, the effort clip binds on
    the joint that has no command clamp; the coefficients move q by >= 10 x the
    free-running bound."""
    _, _, eff = pc.shipped_limits(oracle)
    for spr in (1, 2):
        r = pc.oracle_rollout(oracle, "both", spr)
        g = r["gains"]
        imax = np.array([x.imax for x in g])
        imin = np.array([x.imin for x in g])
        clamp = np.array([x.cmdmax >= x.cmdmin for x in g])
        cmax = np.array([x.cmdmax for x in g])
        cmin = np.array([x.cmdmin for x in g])
        n_imax = int((r["ierr"] == imax).sum())
        n_imin = int((r["ierr"] == imin).sum())
        n_cmax = int(((r["cmd"] == cmax) & clamp).sum())
        n_cmin = int(((r["cmd"] == cmin) & clamp).sum())
        n_eff = int(((np.abs(r["cmd"]) > eff) & ~clamp).sum())
        total = r["cmd"].size
        print(f"rollout spr={spr}: integral at max {n_imax}, at min {n_imin}; command at max {n_cmax}, at min {n_cmin}; "
              f"effort clip alone {n_eff}; of {total} (step, world, dof)")
        assert min(n_imax, n_imin, n_cmax, n_cmin, n_eff) >= 20
        plain = pc.oracle_rollout(oracle, "shipped", spr)
        moved = float(np.abs(r["obs"][:, :, :9] - plain["obs"][:, :, :9]).max())
        print(f"rollout spr={spr}: the coefficients move q by up to {moved:.2e}")
        assert moved >= 10 * pc.Q_FREE
        # joint 4 is driven into its upper limit in the first episode
        hi4 = pc.shipped_limits(oracle)[1][3]
        assert int((r["obs"][:pc.ROLL_TLIM, :, 3] >= hi4).sum()) >= 50


def test_nan_target_applies_zero_force(oracle):
    """ScenarioWorld.run with a non-finite target: PID::Update returns 0 and
    leaves the state (JointController.cpp:308-315 applies that 0), where the
    stale command would have been re-applied."""
    _, _, cm = pc.variant(oracle, "shipped")
    q0 = pc.rollout_start(oracle)[0]
    a = pc.oracle_world(oracle, cm, q0, np.zeros(9), pc.kat_gains())
    b = pc.oracle_world(oracle, cm, q0, np.zeros(9), pc.kat_gains())
    tgt = q0.astype(float) + 0.01
    for ow in (a, b):
        ow.ptgt[:] = tgt
        ow.run()
    assert a.state[1].cmd != 0.0
    before = (a.state[1].cmd, a.state[1].ierr, a.state[1].perr_last)
    a.ptgt[1] = np.nan
    a.run()
    assert (a.state[1].cmd, a.state[1].ierr, a.state[1].perr_last) == before
    # b: the same step with joint 2 switched to zero force by hand
    mode = [oracle.FORCE] * 9
    cmd = np.array([b.state[d].cmd for d in range(9)])
    for d in range(9):
        cmd[d] = oracle.pid_update(b.gains[d], b.state[d], b.q[d] - tgt[d], 1e-3)
    cmd[1] = 0.0
    bq, bqd, *_ = oracle.step(cm, 1e-3, b.q, b.qd, mode, cmd, 20)
    assert np.array_equal(a.q, bq) and np.array_equal(a.qd, bqd)
    assert np.isfinite(a.q).all()
