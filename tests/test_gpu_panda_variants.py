"""The three Panda implementations on damped, frictional, limit-free models
and clamped PIDs, against per-world fp64 oracle ScenarioWorlds (20 sweeps on
both sides, float32-rounded inputs; cases and their CPU-checked conditions:
tests/panda_cases.py, tests/test_panda_cases.py).

  sim    Simulator in Position mode: scenario_run_kernel<9, DUAL, CONS, kPandaTopo>
  lane   VecEnv, MWSTEP_PANDA_KERNEL=lane: vecenv_pid_step_kernel (chain_dyn.hpp)
  group  VecEnv, the default: vecenv_pid_group_kernel<9, DUAL, CONS> (group_tree.hpp)

What each test runs that the shipped-model tests do not:
  one_step_constant_force  DUAL (second factor Cn / dual ABA), friction rows
                           (box +-friction dt, stick and slide), !CONS with
                           implicit damping, the PID's offset word
  one_step_kat_gains       the same rows under the KAT gains
  rollout_clamped_pid      integral clamp, command clamp, offset, empty command
                           range + effort clip, live integral / derivative
                           state, steps_per_run 2 (PID every substep), TimeLimit
                           reset of the PID state, limit row held for many steps
  gains_changed            the group path's re-upload of GLaneTask; the PID
                           reset mw_set_joint_pid asks for
  wave_sharing             rows_of(ballot) union, a0m / a2m masks, wave-wide
                           PGS exit, padding rows
  group_matches_lane       DUAL / !CONS over 300 steps and TimeLimit resets
  nan_target               pid_update's non-finite branch beside live worlds
  rest_without_gravity     the qd != 0 trigger of the friction rows

Bounds are the project's own: one step q <= 1e-5 and qd <= 1e-4, free-running
obs <= 1e-4, reward <= 1e-4 relative.  Measured on the MI355X (max|dq| is
1.2e-7 to 1.3e-7 in every one-step case: half an ulp of a float32 q near 2):

  one step, constant force, max|dqd|     sim      lane     group    host build
    damped                             3.6e-7   3.6e-7   5.7e-6     5.4e-7
    frictional                         8.3e-7   8.3e-7   5.6e-6     6.0e-7
    both                               4.7e-7   4.7e-7   5.6e-6     4.7e-7
    free                               1.4e-7   1.4e-7   2.9e-6     1.1e-7
    partial                            2.8e-7   2.8e-7   5.6e-6     4.0e-7
  one step, KAT gains, max|dqd|
    damped                             4.0e-6   4.0e-6   1.9e-5
    frictional                         3.3e-6   3.6e-6   1.5e-5
    both                               4.1e-6   4.1e-6   1.9e-5
  rollout, clamped PID, max|obs err| (reward <= 1.4e-6 relative)
    steps_per_run 1                    1.6e-5   3.6e-5   3.5e-5
    steps_per_run 2                    6.4e-5   5.2e-5   7.1e-5
  gains changed (before / after)       1.6e-5 / 8.0e-6 (group: 7.4e-6 after)
  NaN target, max|obs err|             2.2e-5   2.2e-5   2.2e-5
  group vs lane, 300 steps: both 1.1e-5 (W = 1), 1.3e-5 (W = 6); free 1.3e-5

(host build: chain_dyn.hpp compiled for the CPU, the lane path's code, on the
same states.  The group kernel's one-step qd error is ten times the lane
path's: its CRBA + Cholesky in a common frame)
"""
import numpy as np
import pytest

import panda_cases as pc

pytestmark = pytest.mark.gpu

IMPLS = ("sim", "lane", "group")
STEP_SEEDS = (21, 22, 23, 24)
W_STEP = 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Rig:
    """One of the three implementations behind the same four calls."""

    def __init__(self, impl, oracle, name, W, gains, monkeypatch, spr=1, tlim=100_000):
        model, params, self.cm = pc.variant(oracle, name)
        self.impl, self.W, self.env = impl, W, None
        if impl == "sim":
            from mwstep.sim import Simulator
            self.sim = Simulator(model, n_worlds=W, step_size=1e-3 / spr, steps_per_run=spr, pgs_iters=20,
                                 joint_params=params)
            self.sim.set_controller_period(1e-3 / spr)
            self._position = False
        else:
            from mwstep.vecenv import VecEnv
            monkeypatch.setenv("MWSTEP_PANDA_KERNEL", impl)
            self.env = VecEnv("PandaPositionTracking", n_worlds=W, seed=pc.ROLL_SEED, max_episode_steps=tlim,
                              model_file=model, physics_rate=1000.0 * spr, pgs_iters=20)
            self.sim = self.env.sim
            assert self.sim.steps_per_run == spr
            for (d, which), v in params.items():
                self.sim.set_joint_param(d, which, v)
        self.set_gains(gains)

    def set_gains(self, gains):
        for d, g in enumerate(gains):
            self.sim.set_pid(d, g.words())

    def load(self, q, qd):
        """Teacher-force the state of every world; the PID state resets."""
        import torch
        q, qd = np.asarray(q, np.float32), np.asarray(qd, np.float32)
        if self.env is not None:
            self.env.reset()   # PID state, low words of q and the counters back to zero
            self.env.set_state(torch.from_numpy(q.T.copy()), torch.from_numpy(qd.T.copy()))
            return
        self.sim.set("reset_q", q.astype(np.float64))
        self.sim.set("reset_qd", qd.astype(np.float64))
        if not self._position:
            self.sim.run(paused=True)
            self.sim.set_control_mode(5)   # Position on every joint
            self._position = True

    def step(self, tgt):
        """-> (obs [W, 18], reward [W] or None, done [W] or None, terminal obs or None)."""
        import torch
        tgt = np.ascontiguousarray(tgt, np.float32)
        if self.env is not None:
            o, r, d, info = self.env.step(torch.from_numpy(tgt).to(self.env.device))
            return (o.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().astype(bool),
                    info["terminal_obs"].cpu().numpy().copy())
        self.sim.set("position_target", tgt.astype(np.float64))
        self.sim.run()
        return np.concatenate([self.sim.get("q"), self.sim.get("qd")], axis=1), None, None, None

    def close(self):
        (self.env or self.sim).close()


# ------------------------------------------------------------ one step -----

_refs = {}


def _one_step_ref(oracle, name, kind):
    """The oracle's answers of the four rounds, computed once per (variant,
    gains) and shared by the three implementations."""
    if (name, kind) not in _refs:
        _, _, cm = pc.variant(oracle, name)
        gains = pc.force_gains(oracle) if kind == "force" else pc.kat_gains()
        rounds = []
        for seed in STEP_SEEDS:
            q, qd, tgt = pc.step_states(oracle, W_STEP, seed)
            rounds.append((q, qd, tgt, *pc.oracle_one_step(oracle, cm, q, qd, tgt, gains)))
        _refs[(name, kind)] = (gains, rounds)
    return _refs[(name, kind)]


def _host_figure(oracle, name):
    """max|dqd| of the host build of chain_dyn.hpp on the constant-force rounds."""
    from test_host_dyn import build_harness, _params, _substep
    if ("host", name) not in _refs:
        hd = build_harness()
        model, params, cm = pc.variant(oracle, name)
        P = _params(hd, model, [(d, which, v) for (d, which), v in params.items()])
        z = np.zeros(9)
        worst = 0.0
        for q, qd, _, _, oqd in _one_step_ref(oracle, name, "force")[1]:
            for w in range(len(q)):
                got = _substep(hd, P, q[w], qd[w], pc.TAU, z, z, cons=name != "free", dual=name != "frictional")
                worst = max(worst, float(np.abs(got[1] - oqd[w]).max()))
        _refs[("host", name)] = worst
    return _refs[("host", name)]


def _one_step(impl, oracle, name, kind, monkeypatch):
    gains, rounds = _one_step_ref(oracle, name, kind)
    rig = Rig(impl, oracle, name, W_STEP, gains, monkeypatch)
    wq = wqd = 0.0
    for q, qd, tgt, oq, oqd in rounds:
        rig.load(q, qd)
        obs = rig.step(tgt)[0]
        wq = max(wq, float(np.abs(obs[:, :9] - oq).max()))
        wqd = max(wqd, float(np.abs(obs[:, 9:] - oqd).max()))
    rig.close()
    return wq, wqd


@pytest.mark.parametrize("name", ["damped", "frictional", "both", "free", "partial"])
@pytest.mark.parametrize("impl", IMPLS)
def test_one_step_constant_force(require_gpu, oracle, monkeypatch, impl, name):
    """Dynamics isolated from the PID: p = i = d = 0 and offset = tau per dof
    (inside the effort and the command clamp), so the controller applies a
    known constant force.  4 rounds of 64 states: a fifth of the joints 2 mrad
    beyond a limit, 30 % of the velocities inside +-2e-3 (friction rows that
    stick and that slide: counts in test_panda_cases.py); `partial` has
    friction on every other dof only, so neighbouring dofs differ in their row
    masks.  Measured: see the module docstring; the host build of the lane
    path's code is printed beside."""
    wq, wqd = _one_step(impl, oracle, name, "force", monkeypatch)
    print(f"one step, constant force, {impl}, {name}: max|dq| {wq:.2e}, max|dqd| {wqd:.2e} "
          f"(host build of chain_dyn.hpp: max|dqd| {_host_figure(oracle, name):.2e})")
    assert wq <= pc.Q_STEP and wqd <= pc.QD_STEP


@pytest.mark.parametrize("name", ["damped", "frictional", "both"])
@pytest.mark.parametrize("impl", IMPLS)
def test_one_step_kat_gains(require_gpu, oracle, monkeypatch, impl, name):
    """The same states and rows under the reference's KAT gains (targets within
    +-0.05 rad of the state), fresh controller."""
    wq, wqd = _one_step(impl, oracle, name, "kat", monkeypatch)
    print(f"one step, KAT gains, {impl}, {name}: max|dq| {wq:.2e}, max|dqd| {wqd:.2e}")
    assert wq <= pc.Q_STEP and wqd <= pc.QD_STEP


@pytest.mark.parametrize("impl", IMPLS)
def test_rest_without_gravity(require_gpu, oracle, monkeypatch, impl):
    """`both` at rest with no gravity and no force: every velocity is exactly 0
    after the velocity update, so no friction row exists (the qd != 0 trigger)
    and the state does not change by a bit -- as in the oracle
    (test_friction_row_coverage)."""
    gains = [pc.Gain(0.0, 0.0, 0.0) for _ in range(9)]
    rig = Rig(impl, oracle, "both", 8, gains, monkeypatch)
    rig.sim.set_gravity([0.0, 0.0, 0.0])
    q = pc.wave_sharing_worlds(oracle, k=8)[0]
    rig.load(q, np.zeros_like(q))
    for _ in range(3):
        obs = rig.step(q)[0]
    assert np.array_equal(obs[:, :9].astype(np.float32), q) and np.all(obs[:, 9:] == 0.0)
    rig.close()


# ------------------------------------------------------------- rollouts ----

def _follow(rig, ref, H, reset_at=True):
    """Run the rig along a precomputed oracle rollout: worst obs error
    (terminal observations at the TimeLimit) and worst relative reward error."""
    rig.load(ref["q0"], np.zeros_like(ref["q0"]))
    worst_o = worst_r = 0.0
    for k in range(H):
        obs, r, done, term = rig.step(ref["tgt"][k])
        cmp_ = obs
        if rig.env is not None:
            assert bool(done.all()) == bool(ref["done"][k]) and bool(done.any()) == bool(done.all())
            if ref["done"][k]:
                cmp_ = term
                assert np.abs(obs[:, :9] - ref["reset"][k]).max() <= 1e-6 and np.all(obs[:, 9:] == 0)
            worst_r = max(worst_r, float((np.abs(r - ref["reward"][k]) / (1.0 + np.abs(ref["reward"][k]))).max()))
        elif ref["done"][k]:
            rig.load(ref["reset"][k], np.zeros_like(ref["q0"]))   # what the env's TimeLimit does
        worst_o = max(worst_o, float(np.abs(cmp_ - ref["obs"][k]).max()))
    return worst_o, worst_r


@pytest.mark.parametrize("spr", [1, 2])
@pytest.mark.parametrize("impl", IMPLS)
def test_rollout_clamped_pid(require_gpu, oracle, monkeypatch, impl, spr):
    """300 free-running steps of 16 worlds of `both` under the asymmetric
    clamped gains (every one of the eight words differs per dof, joint 4 has an
    empty command range), KAT sinusoids on joints 1 and 6 and a 1 Hz, 0.3 rad
    one that drives joint 4 into its upper limit; physics at 1000 and 2000 Hz
    (the PID runs every substep); TimeLimit reset at step 150.  In the oracle
    both integral clamps, both command clamps and the effort clip bind
    (test_rollout_pid_coverage).  After the reset the fingers' targets are
    mid-range (panda_cases.oracle_rollout says why).  Measured: module docstring."""
    ref = pc.oracle_rollout(oracle, "both", spr)
    rig = Rig(impl, oracle, "both", pc.ROLL_W, ref["gains"], monkeypatch, spr=spr, tlim=pc.ROLL_TLIM)
    worst_o, worst_r = _follow(rig, ref, pc.ROLL_H)
    print(f"rollout, clamped PID, {impl}, steps_per_run {spr}: max|obs err| {worst_o:.2e}, reward rel {worst_r:.2e}")
    assert worst_o <= pc.Q_FREE and worst_r <= pc.R_REL
    rig.close()


@pytest.mark.parametrize("impl", IMPLS)
def test_gains_changed_between_steps(require_gpu, oracle, monkeypatch, impl):
    """After 50 steps every dof gets other gains (mw_set_joint_pid on the
    simulator, set_pid on the oracle: a new PID, whose state starts from zero,
    Joint.cpp:479-525); the next 50 steps still match.  The group path copies
    the gains into its own device block and re-uploads it when they change."""
    g2 = pc.clamped_gains(oracle, scale=0.6)
    ref = pc.oracle_rollout(oracle, "both", 1, regain=(50, g2), H=100)
    rig = Rig(impl, oracle, "both", pc.ROLL_W, pc.clamped_gains(oracle), monkeypatch)
    rig.load(ref["q0"], np.zeros_like(ref["q0"]))
    worst = [0.0, 0.0]
    for k in range(100):
        if k == 50:
            rig.set_gains(g2)
        obs = rig.step(ref["tgt"][k])[0]
        worst[k >= 50] = max(worst[k >= 50], float(np.abs(obs - ref["obs"][k]).max()))
    print(f"gains changed at step 50, {impl}: max|obs err| before {worst[0]:.2e}, after {worst[1]:.2e}")
    assert max(worst) <= pc.Q_FREE
    rig.close()


def free_gains():
    """KAT gains for the limit-free model: its fingers turn about their axis
    with an inertia of 1e-5 kg m^2, where the KAT finger gains (a discrete
    derivative gain of 50) are unstable; theirs are scaled to that inertia."""
    g = pc.kat_gains()
    g[7] = g[8] = pc.Gain(0.1, 0.0, 0.002)
    return g


@pytest.mark.parametrize("W", [1, 6])
@pytest.mark.parametrize("name", ["both", "free"])
def test_group_matches_lane_kernel_variants(require_gpu, oracle, monkeypatch, name, W):
    """test_group_matches_lane_kernel on `both` (DUAL, friction rows) and `free`
    (!CONS with implicit damping): 300 steps, TimeLimit resets at 120 and 240."""
    import math
    H = 300
    gains = free_gains() if name == "free" else pc.kat_gains()
    a = Rig("group", oracle, name, W, gains, monkeypatch, tlim=120)
    b = Rig("lane", oracle, name, W, gains, monkeypatch, tlim=120)
    qa, qb = a.env.reset()[:, :9].cpu().numpy().copy(), b.env.reset()[:, :9].cpu().numpy().copy()
    assert np.array_equal(bits(qa), bits(qb))
    worst = worst_r = 0.0
    for k in range(H):
        tgt = qa.copy()
        tgt[:, 0] += 0.9 * 2.8973 * math.sin(2 * math.pi * 0.33 * k * 1e-3)
        tgt[:, 5] += 0.9 * 1.885 * math.sin(2 * math.pi * 0.33 * k * 1e-3)
        monkeypatch.setenv("MWSTEP_PANDA_KERNEL", "group")
        oa, ra, da, ta = a.step(tgt)
        monkeypatch.setenv("MWSTEP_PANDA_KERNEL", "lane")
        ob, rb, db, tb = b.step(tgt)
        assert np.array_equal(da, db) and bool(da.all()) == ((k + 1) % 120 == 0)
        worst = max(worst, float(np.abs(oa - ob).max()))
        worst_r = max(worst_r, float((np.abs(ra - rb) / (1 + np.abs(rb))).max()))
        if da.any():
            assert float(np.abs(ta - tb).max()) <= 1e-4
    print(f"group vs lane kernel, {name}, W={W}, H={H}: max|obs diff| {worst:.2e}, reward rel {worst_r:.2e}")
    assert worst <= 1e-4 and worst_r <= 1e-4
    a.close()
    b.close()


# --------------------------------------------------------- wave sharing ----

def _run_batch(oracle, name, rows, monkeypatch, steps=3):
    """The group kernel on a batch of worlds given as rows [q | qd | target]:
    obs [steps, W, 18] and reward [steps, W] of `steps` free-running steps."""
    W = len(rows)
    rig = Rig("group", oracle, name, W, pc.kat_gains(), monkeypatch)
    rig.load(rows[:, :9], rows[:, 9:18])
    obs, rew = [], []
    for _ in range(steps):
        o, r, _, _ = rig.step(rows[:, 18:])
        obs.append(o)
        rew.append(r)
    rig.close()
    return np.stack(obs), np.stack(rew)


@pytest.mark.parametrize("name", ["shipped", "both"])
def test_wave_sharing_is_bit_exact(require_gpu, oracle, monkeypatch, name):
    """Four worlds share a wave of the group kernel.  The LCP set-up loops over
    the union of their active rows and masks per world (a0m, a2m: a masked row
    moves its impulse by (xn - x) * 0), the sweeps end when no world of the
    wave moved, and a world that has converged repeats a sweep that moves
    nothing; a wave with no row at all skips the LCP, which adds 0 to qd.  So a
    world's answer does not depend on its neighbours by a bit.  Quiet worlds
    (no limit row; on `shipped` no row at all) alternate with loaded ones
    (three to five limit rows): every world at each of the four row positions,
    in batches of 8, 1, 5 and 7 worlds (padding rows copy the last world),
    against the same world in a batch of its own kind.  On `both` every world
    also has nine friction rows."""
    quiet, loaded = pc.wave_sharing_rows(oracle)
    ref = {}
    for kind, rows in (("q", quiet), ("l", loaded)):
        o, r = _run_batch(oracle, name, rows, monkeypatch)
        for i in range(len(rows)):
            ref[(kind, i)] = (bits(o[:, i]), bits(r[:, i]))
    if name == "shipped":
        # the quiet worlds really are quiet and the loaded ones loaded (oracle)
        _, _, cm = pc.variant(oracle, name)
        for rows, want in ((quiet, False), (loaded, True)):
            for row in rows:
                lim = oracle.step_rows(cm, 1e-3, row[:9].astype(float), row[9:18].astype(float), [oracle.FORCE] * 9,
                                       np.zeros(9), 20)[2]
                assert bool((lim != oracle.ROW_NONE).sum() >= 3) == want and (want or not lim.any())
    order = [(k, i) for i in range(4) for k in ("q", "l")]   # q0 l0 q1 l1 ...
    checked = 0
    for shift in range(4):
        mixed = order[shift:] + order[:shift]
        for W in (8, 1, 5, 7):
            ids = mixed[:W]
            rows = np.stack([(quiet if k == "q" else loaded)[i] for k, i in ids])
            o, r = _run_batch(oracle, name, rows, monkeypatch)
            for pos, wid in enumerate(ids):
                assert np.array_equal(bits(o[:, pos]), ref[wid][0]), (name, shift, W, pos, wid)
                assert np.array_equal(bits(r[:, pos]), ref[wid][1]), (name, shift, W, pos, wid)
                checked += 1
    # every world has been at every row position of a wave
    assert checked == 4 * (8 + 1 + 5 + 7)


# ------------------------------------------------------------ NaN target ---

@pytest.mark.parametrize("impl", IMPLS)
def test_nan_target_for_one_step(require_gpu, oracle, monkeypatch, impl):
    """World 2 gets a NaN target on joint 2 for one step: PID::Update returns 0
    and leaves its state (JointController.cpp:308-315 applies that 0;
    pid.hpp).  Every world, the one with the NaN included, follows the oracle
    within the free-running bound, and the other worlds -- worlds 0, 1 and 3
    share its wave in the group kernel -- are bit-identical to a run without
    the NaN.  Input handling: nothing here makes a kernel fault."""
    W, H, K, WN, DN = 8, 12, 5, 2, 1
    _, _, cm = pc.variant(oracle, "shipped")
    q0 = pc.rollout_start(oracle)[:W]
    base = q0.copy()
    gains = pc.kat_gains()
    runs = {}
    for nan in (False, True):
        rig = Rig(impl, oracle, "shipped", W, gains, monkeypatch)
        rig.load(q0, np.zeros_like(q0))
        ows = [pc.oracle_world(oracle, cm, q0[w], np.zeros(9), gains) for w in range(W)] if nan else None
        out, worst = [], 0.0
        for k in range(H):
            tgt = pc.rollout_targets(base, k)
            if nan and k == K:
                tgt[WN, DN] = np.nan
            obs, r, _, _ = rig.step(tgt)
            out.append((obs, r))
            if nan:
                for w, ow in enumerate(ows):
                    ow.ptgt[:] = tgt[w]
                    ow.run()
                    worst = max(worst, float(np.abs(obs[w] - np.concatenate([ow.q, ow.qd])).max()))
                    if r is not None and not (k == K and w == WN):
                        ref_r = -float(np.sum((ow.q - tgt[w].astype(np.float64)) ** 2))
                        assert abs(r[w] - ref_r) <= pc.R_REL * (1 + abs(ref_r))
        runs[nan] = out
        rig.close()
        if nan:
            print(f"NaN target, {impl}: max|obs err| vs oracle over all worlds {worst:.2e}")
            assert np.isfinite(worst) and worst <= pc.Q_FREE
    others = [w for w in range(W) if w != WN]
    for (oa, ra), (ob, rb) in zip(runs[False], runs[True]):
        assert np.array_equal(bits(oa[others]), bits(ob[others]))
        if ra is not None:
            assert np.array_equal(bits(ra[others]), bits(rb[others]))
    # the world with the NaN did take another path from that step on
    assert not np.array_equal(bits(runs[False][K][0][WN]), bits(runs[True][K][0][WN]))
