"""The randomised-physics step kernels (vecenv_step_kernel<..., RAND=true>)
over their whole matrix, against the fp64 oracle.

Cases, seeds and oracle helpers: tests/randomized_cases.py.  That these inputs
are sensitive enough -- another world's mass or gravity, or a wrong gravity
direction, moves the next observation by ten times the bound used here on at
least 40 % of the worlds -- is asserted on the CPU by
tests/test_randomized_cases.py.

  a. one step, teacher-forced to the oracle at every one of 8 steps: 4 tasks x
     {baked, generic} x W in {1, 65, 16449} x {mass, gravity, both};
  b. the same on a base tilted 0.3 rad about y (gdir != e_z);
  c. the same with two substeps per step;
  d. the fused rollout: bit-equal to closed-loop stepping, and against the
     free-running oracle;
  e. a shard with a world_offset is bit-equal to the same worlds of one env.

Bounds, all the project's own (tests/test_gpu_vecenv_parity.py,
tests/test_randomization.py): one-step obs <= 1e-4 on live, not-done worlds;
free-running obs <= 1e-3; reward <= 1e-3; reset obs <= 1e-6; drawn mass <= 1e-6
and gravity <= 2e-5 on EVERY world after every step; counters equal.  A done
flag may differ from the oracle's only where the oracle's observation is within
1e-4 of a threshold; such a world is left out from then on, and at most 0.2 %
of the (world, step) pairs may be left out (none at W <= 65).

With gravity alone on an upright base, only the swing-up and the pendulum cases
say anything about the gravity the dynamics use (randomized_cases.
counts_as_gravity_check); the balancing tasks run anyway and check gravity in (b).
"""

import numpy as np
import pytest

import randomized_cases as C

pytestmark = pytest.mark.gpu

KERNELS = (("baked", False), ("generic", True))


def _env(monkeypatch, task, W, mask, generic=False, **kw):
    from mwstep.vecenv import VecEnv
    if generic:
        monkeypatch.setenv("MWSTEP_DISABLE_BAKED", "1")    # read at every launch: stays set for the test
    else:
        monkeypatch.delenv("MWSTEP_DISABLE_BAKED", raising=False)
    return VecEnv(task, n_worlds=W, seed=C.SEED, randomize=mask, max_episode_steps=C.MAX_EPISODE_STEPS,
                  mass_range=C.MASS_RANGE, gravity_normal=C.GRAVITY_NORMAL, **kw)


def _np(*tensors):
    return [x.cpu().numpy() for x in tensors]


class _Worst:
    def __init__(self):
        self.v = {}

    def add(self, key, err, where=None):
        if where is not None:
            err = err[where]
        if err.size:
            self.v[key] = max(self.v.get(key, 0.0), float(np.max(err)))
        return self.v.get(key, 0.0)

    def __str__(self):
        return ", ".join(f"{k} {v:.2e}" for k, v in self.v.items())


def _check_physics(env, tr, model, mask, episode, alive, worst):
    """physics() of EVERY world against oracle.sample_physics(cm, task, w, episode[w])."""
    m, gz = _np(*env.physics())
    em, egz = C.expected_physics(tr, model, mask, episode)
    if mask & C.RAND_MASS:
        assert worst.add("mass", np.abs(m - em).max(axis=0), alive) <= C.MASS
    else:
        assert not m.any()                  # not drawn: the array keeps its zero fill
    assert worst.add("gravity", np.abs(gz - egz), alive) <= C.GRAVITY
    if mask & C.RAND_GRAVITY and tr.W > 1:
        assert np.unique(gz).size > tr.W // 2


def _done_agreement(kind, tr, t, done, alive):
    """Leaves out the worlds whose done flag differs from the oracle's; that is
    allowed only where the oracle's observation is within 1e-4 of a threshold."""
    pre = np.where(tr.done[t][:, None], tr.terminal_obs[t], tr.obs[t])   # the observation `done` was computed from
    differ = (done != tr.done[t]) & alive
    assert not (differ & ~C.near_threshold(kind, pre)).any(), \
        f"step {t}: done differs from the oracle's away from every threshold in worlds {np.nonzero(differ)[0][:8]}"
    return alive & ~differ


def _one_step_teacher_forced(env, kind, model, mask, tr, label):
    import torch
    W, worst = tr.W, _Worst()
    og, = _np(env.reset())
    assert worst.add("reset obs", np.abs(og - tr.reset_obs)) <= C.RESET_OBS
    alive = np.ones(W, dtype=bool)
    _check_physics(env, tr, model, mask, tr.episode[0], alive, worst)
    left_out = 0
    for t in range(C.T):
        # teacher forcing: the GPU starts every step from the oracle's state; the
        # counters stay in step through the shared TimeLimit
        env.set_state(torch.tensor(tr.q[t]), torch.tensor(tr.qd[t]))
        o, r, d, info = env.step(torch.tensor(tr.actions[t]).to(env.device))
        o, r, d, to = _np(o, r, d, info["terminal_obs"])
        alive = _done_agreement(kind, tr, t, d.astype(bool), alive)
        left_out += int((~alive).sum())
        dref = tr.done[t]
        assert worst.add("obs", np.abs(o - tr.obs[t]).max(axis=1), alive & ~dref) <= C.OBS_ONE_STEP
        assert worst.add("reward", np.abs(r - tr.reward[t]), alive) <= C.REWARD
        assert worst.add("terminal obs", np.abs(to - tr.terminal_obs[t]).max(axis=1), alive & dref) <= C.OBS_ONE_STEP
        assert worst.add("reset obs", np.abs(o - tr.obs[t]).max(axis=1), alive & dref) <= C.RESET_OBS
        ep, st = _np(*env.counters())
        assert np.array_equal(ep[alive], tr.episode[t + 1][alive]) and np.array_equal(st[alive], tr.steps[t + 1][alive])
        _check_physics(env, tr, model, mask, tr.episode[t + 1], alive, worst)
    print(f"{label}: {worst}; (world, step) pairs left out {left_out}")
    assert left_out <= C.MAX_EXCLUDED * W * C.T
    if W <= 65:
        assert left_out == 0
    assert tr.episode[C.T].min() >= 2           # every world stepped with the physics of episodes 0, 1 and 2


# ------------------------------------------------------------ a. one step ---
@pytest.mark.parametrize("kernel,generic", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("case", C.ONE_STEP, ids=C.case_id)
def test_one_step(require_gpu, oracle, monkeypatch, case, kernel, generic):
    task, kind, model, W, mname = case
    mask = C.MASKS[mname]
    env = _env(monkeypatch, task, W, mask, generic)
    assert bool(env.sim.baked_model()) != generic
    tr = C.trajectory(kind, model, W, mask)
    _one_step_teacher_forced(env, kind, model, mask, tr, f"{C.case_id(case)}-{kernel}")
    env.close()


# ---------------------------------------------------------- b. tilted base ---
@pytest.mark.parametrize("case", C.TILT, ids=C.case_id)
def test_one_step_tilted_base(require_gpu, oracle, monkeypatch, case):
    """The base rotated 0.3 rad about y.  The tilted model's parameter block
    (its gravity in the base frame) is not a shipped model's, so it gets the
    GENERIC kernel; gdir = R_base^T e_z reaches it through the task block."""
    task, kind, model, W, mname = case
    mask = C.MASKS[mname]
    env = _env(monkeypatch, task, W, mask, pose=C.TILTED)
    assert env.sim.baked_model() == 0
    tr = C.trajectory(kind, model, W, mask, True)
    assert abs(tr.task.gdir[0] + np.sin(0.3)) < 1e-12 and abs(tr.task.gdir[2] - np.cos(0.3)) < 1e-12
    _one_step_teacher_forced(env, kind, model, mask, tr, f"{C.case_id(case)}-tilted")
    env.close()


# --------------------------------------------------------- c. two substeps ---
@pytest.mark.parametrize("case", C.TWO_SUBSTEPS, ids=C.case_id)
def test_one_step_two_substeps(require_gpu, oracle, monkeypatch, case):
    """physics_rate = 2 x agent_rate: dt = 5e-4, the action acts on the first substep."""
    task, kind, model, W = case
    mask = C.MASKS["both"]
    env = _env(monkeypatch, task, W, mask, physics_rate=2000.0)
    assert env.sim.baked_model() != 0 and env.sim.steps_per_run == 2
    tr = C.trajectory(kind, model, W, mask, False, 2)
    _one_step_teacher_forced(env, kind, model, mask, tr, f"{C.case_id(case)}-2substeps")
    env.close()


# -------------------------------------------------------------- d. rollout ---
@pytest.mark.parametrize("kernel,generic", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("case", C.ROLLOUT, ids=C.case_id)
def test_rollout_equals_stepping(require_gpu, monkeypatch, case, kernel, generic):
    """One fused T-step launch against T closed-loop launches on a twin: every
    output, the final state, the counters and the draws bit for bit.  (Two
    instantiations of the same arithmetic; each is compared with the oracle by
    test_one_step and test_rollout_vs_oracle.)"""
    import torch
    task, kind, model, W = case
    mask = C.MASKS["both"]
    a, b = (_env(monkeypatch, task, W, mask, generic) for _ in range(2))
    assert bool(a.sim.baked_model()) != generic
    assert torch.equal(a.reset(), b.reset())
    acts = torch.tensor(C.actions(kind, C.T, W)).to(a.device)
    obs, rew, done, term = a.rollout(acts)
    for t in range(C.T):
        o, r, d, info = b.step(acts[t].contiguous())
        assert torch.equal(d, done[t]), f"done differs at step {t}"
        rows = d.bool()
        assert torch.equal(info["terminal_obs"][rows], term[t][rows]), f"terminal_obs differs at step {t}"
        assert torch.equal(o, obs[t]), f"obs differs at step {t}: {(o - obs[t]).abs().max().item():.3e}"
        assert torch.equal(r, rew[t]), f"reward differs at step {t}: {(r - rew[t]).abs().max().item():.3e}"
    for x, y in zip(a.counters() + a.state() + a.physics(), b.counters() + b.state() + b.physics()):
        assert torch.equal(x, y)
    assert int(a.counters()[0].min()) >= 2
    a.close()
    b.close()


@pytest.mark.parametrize("kernel,generic", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("case", C.ROLLOUT, ids=C.case_id)
def test_rollout_vs_oracle(require_gpu, oracle, monkeypatch, case, kernel, generic):
    """The fused rollout cannot be teacher-forced: it free-runs beside the
    oracle through the same TimeLimit resets, under the free-running bound."""
    import torch
    task, kind, model, W = case
    mask = C.MASKS["both"]
    env = _env(monkeypatch, task, W, mask, generic)
    assert bool(env.sim.baked_model()) != generic
    tr = C.trajectory(kind, model, W, mask)
    worst = _Worst()
    og, = _np(env.reset())
    assert worst.add("reset obs", np.abs(og - tr.reset_obs)) <= C.RESET_OBS
    obs, rew, done, term = _np(*env.rollout(torch.tensor(tr.actions).to(env.device)))
    alive = np.ones(W, dtype=bool)
    left_out = 0
    for t in range(C.T):
        alive = _done_agreement(kind, tr, t, done[t].astype(bool), alive)
        left_out += int((~alive).sum())
        assert worst.add("obs", np.abs(obs[t] - tr.obs[t]).max(axis=1), alive) <= C.OBS_FREE_RUNNING
        assert worst.add("reward", np.abs(rew[t] - tr.reward[t]), alive) <= 10 * C.OBS_FREE_RUNNING
        assert worst.add("terminal obs", np.abs(term[t] - tr.terminal_obs[t]).max(axis=1),
                         alive & tr.done[t]) <= C.OBS_FREE_RUNNING
    ep, st = _np(*env.counters())
    assert np.array_equal(ep[alive], tr.episode[C.T][alive]) and np.array_equal(st[alive], tr.steps[C.T][alive])
    _check_physics(env, tr, model, mask, tr.episode[C.T], alive, worst)
    print(f"{C.case_id(case)}-rollout-{kernel}: {worst}; (world, step) pairs left out {left_out}")
    assert left_out <= C.MAX_EXCLUDED * W * C.T
    if W <= 65:
        assert left_out == 0
    env.close()


# ------------------------------------------------------- e. shard identity ---
# (shard worlds, its world_offset, worlds of the whole env): both envs of a pair
# run the same instantiation -- 64-thread blocks (<= 16384 worlds) or 256-thread
SHARDS = ((65, 1000, 1065), (16449, 64, 16513))


@pytest.mark.parametrize("WA,offset,WB", SHARDS, ids=[f"W{s[0]}-offset{s[1]}" for s in SHARDS])
@pytest.mark.parametrize("task,kind,model", C.TASKS, ids=[t[0] for t in C.TASKS])
def test_shard_identity(require_gpu, monkeypatch, task, kind, model, WA, offset, WB):
    """A shard is its worlds of the whole env, bit for bit: the draws are keyed
    by world_offset + w.  (Two shards drawing the same physics would differ
    from the whole env here.)"""
    import torch
    mask = C.MASKS["both"]
    A = _env(monkeypatch, task, WA, mask, world_offset=offset)
    B = _env(monkeypatch, task, WB, mask)
    sl = slice(offset, offset + WA)

    def same(what, x, y):
        assert torch.equal(x, y), f"{what} differs in {int((x != y).sum())} places"

    def same_stored(when):
        for name, xs, ys in (("counters", A.counters(), B.counters()), ("state", A.state(), B.state()),
                             ("physics", A.physics(), B.physics())):
            for x, y in zip(xs, ys):
                same(f"{name} {when}", x, y[..., sl])

    same("reset obs", A.reset(), B.reset()[sl])
    same_stored("after reset")
    acts = torch.tensor(C.actions(kind, C.T, WB)).to(B.device)
    for t in range(C.T):
        oa, ra, da, ia = A.step(acts[t, sl].contiguous())
        ob, rb, db, ib = B.step(acts[t].contiguous())
        same(f"done at step {t}", da, db[sl])
        same(f"obs at step {t}", oa, ob[sl])
        same(f"reward at step {t}", ra, rb[sl])
        rows = da.bool()
        same(f"terminal_obs at step {t}", ia["terminal_obs"][rows], ib["terminal_obs"][sl][rows])
        same_stored(f"after step {t}")
    m, gz = A.physics()
    assert int(A.counters()[0].min()) >= 2 and torch.unique(gz).numel() > WA // 2
    A.close()
    B.close()
