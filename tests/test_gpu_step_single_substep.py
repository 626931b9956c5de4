"""The single-substep step kernels against the loop kernels, bit for bit.

With one physics substep per env step the launcher takes a straight-line
instantiation of the closed-loop 64-world-block kernels (vecenv_kernel.hip,
template argument ONE); MWSTEP_FORCE_SUBSTEP_LOOP=1 makes it take the loop
instantiation, which serves every other substep count.  Both run the same
arithmetic, so everything they return and leave behind must be EQUAL: obs,
reward, done, terminal_obs of every step, and q, qd, episode, steps at the end.

  * 1, 63, 65 and 130 worlds: a partial last block, lanes past W working on
    world W - 1;
  * CartPole kinds 0, 1, 2 and Pendulum, on the constant-folded (baked) and the
    generic kernels;
  * 300 steps with max_episode_steps = 7.  Every world runs into the TimeLimit;
    at six steps a third of the worlds is pushed beyond a task bound through
    the state setter (the same push in both runs), so task resets fall between
    the TimeLimit resets and the lanes of a wave stop being in step.  Both
    kinds of reset are asserted to have occurred;
  * one case with worlds placed beyond the cart's position limit, so the limit
    row and its PGS loop run in the first step; the fp64 oracle says for which
    worlds the row is active;
  * one case with two substeps per env step: the launcher takes the loop kernel
    whatever the switch says.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS, MAX_EPISODE_STEPS = 300, 7
PUSH_AT = (9, 33, 76, 121, 200, 261)     # t % 3 = 0, 0, 1, 1, 2, 0: world 0 is pushed too
TASKS = ("CartPoleDiscreteBalancing", "CartPoleContinuousBalancing", "CartPoleContinuousSwingup",
         "PendulumSwingUp")
# a joint velocity beyond the task's bound on it (cart: |dx| <= 20; pendulum: |dq| <= 10)
PUSH_QD0 = {"PendulumSwingUp": 12.0}
SWITCH = "MWSTEP_FORCE_SUBSTEP_LOOP"


def actions_for(task, T, W, seed=5):
    rng = np.random.default_rng(seed)
    if task == "CartPoleDiscreteBalancing":
        return rng.integers(0, 2, size=(T, W), dtype=np.int32)
    return rng.uniform(-50.0, 50.0, size=(T, W)).astype(np.float32)


def run(monkeypatch, task, W, generic, force_loop, steps=STEPS, push_at=PUSH_AT, physics_rate=1000.0, start=None):
    """One closed loop; returns every step's outputs, the final state and
    counters (host tensors) and the number of task / TimeLimit resets."""
    import torch
    from mwstep.vecenv import VecEnv
    if generic:
        monkeypatch.setenv("MWSTEP_DISABLE_BAKED", "1")
    else:
        monkeypatch.delenv("MWSTEP_DISABLE_BAKED", raising=False)
    if force_loop:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    env = VecEnv(task, n_worlds=W, seed=42, max_episode_steps=MAX_EPISODE_STEPS, physics_rate=physics_rate)
    assert bool(env.sim.baked_model()) != generic
    env.reset()
    if start is not None:
        env.set_state(*start(env))
    acts = torch.from_numpy(actions_for(task, steps, W)).to(env.device)
    dev = env.device
    obs = torch.empty((steps, W, env.obs_dim), device=dev)
    term = torch.empty((steps, W, env.obs_dim), device=dev)
    rew = torch.empty((steps, W), device=dev)
    done = torch.empty((steps, W), dtype=torch.uint8, device=dev)
    count = torch.zeros((W,), dtype=torch.int32, device=dev)      # the env's own step counter, redone here
    n_task = torch.zeros((), dtype=torch.int64, device=dev)
    n_limit = torch.zeros((), dtype=torch.int64, device=dev)
    world = torch.arange(W, device=dev)
    for t in range(steps):
        if t in push_at:
            q, qd = env.state()
            qd[0] = torch.where(world % 3 == t % 3, torch.full_like(qd[0], PUSH_QD0.get(task, 25.0)), qd[0])
            env.set_state(q, qd)
        o, r, d, info = env.step(acts[t])
        obs[t].copy_(o)
        rew[t].copy_(r)
        done[t].copy_(d)
        term[t].copy_(info["terminal_obs"])
        count += 1
        n_task += ((d != 0) & (count < MAX_EPISODE_STEPS)).sum()
        n_limit += ((d != 0) & (count == MAX_EPISODE_STEPS)).sum()
        count *= (d == 0)
    q, qd = env.state()
    episode, nsteps = env.counters()
    assert torch.equal(nsteps, count), "the test's step counter is not the env's"
    out = {"obs": obs, "reward": rew, "done": done, "terminal_obs": term, "q": q, "qd": qd,
           "episode": episode, "steps": nsteps}
    out = {k: v.cpu() for k, v in out.items()}
    env.close()
    return out, int(n_task), int(n_limit)


def assert_bit_equal(a, b):
    import torch
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)), k


@pytest.mark.parametrize("generic", [False, True], ids=["baked", "generic"])
@pytest.mark.parametrize("W", [1, 63, 65, 130])
@pytest.mark.parametrize("task", TASKS)
def test_single_substep_equals_loop(require_gpu, monkeypatch, task, W, generic):
    one, n_task, n_limit = run(monkeypatch, task, W, generic, force_loop=False)
    loop, m_task, m_limit = run(monkeypatch, task, W, generic, force_loop=True)
    assert n_task > 0, "no task reset in the case"
    assert n_limit > 0, "no TimeLimit reset in the case"
    assert (n_task, n_limit) == (m_task, m_limit)
    assert_bit_equal(one, loop)


@pytest.mark.parametrize("generic", [False, True], ids=["baked", "generic"])
def test_limit_row_in_first_step(require_gpu, monkeypatch, oracle, cartpole_file, generic):
    """Worlds 0, 5, 10, ... start beyond the cart's upper position limit and
    worlds 1, 6, ... beyond the lower one: the limit row is active and its PGS
    loop runs in the first step of the single-substep kernel."""
    import torch
    task, W = "CartPoleDiscreteBalancing", 130
    x0 = np.zeros(W, np.float32)
    x0[0::5], x0[1::5] = 4.9, -4.85
    moved = x0 != 0
    kept = {}

    def start(env):
        q, qd = env.state()
        q[0] = torch.where(torch.from_numpy(moved).to(env.device), torch.from_numpy(x0).to(env.device), q[0])
        kept["q"], kept["qd"] = q.cpu().numpy().astype(np.float64), qd.cpu().numpy().astype(np.float64)
        return q, qd

    one, _, _ = run(monkeypatch, task, W, generic, force_loop=False, steps=20, push_at=(), start=start)
    q0, qd0 = kept["q"].copy(), kept["qd"].copy()
    loop, _, _ = run(monkeypatch, task, W, generic, force_loop=True, steps=20, push_at=(), start=start)
    assert np.array_equal(q0, kept["q"]) and np.array_equal(qd0, kept["qd"])
    assert_bit_equal(one, loop)

    # the oracle's rows of the first step, from the state both runs started in
    cm = oracle.load_urdf(cartpole_file)
    a0 = actions_for(task, 20, W)[0]
    mode = np.full(cm.n, oracle.FORCE, np.int32)
    rows = np.empty(W, np.int32)
    for w in range(W):
        cmd = np.array([20.0 if a0[w] == 1 else -20.0, 0.0])
        rows[w] = oracle.step_rows(cm, 1e-3, q0[:, w], qd0[:, w], mode, cmd)[2][0]
    assert (rows[0::5] == oracle.ROW_UPPER).all() and (rows[1::5] == oracle.ROW_LOWER).all()
    assert (rows[~moved] == oracle.ROW_NONE).all()
    # beyond the limit is beyond the task's |x| <= 2.4 as well: those worlds are done in the first step
    assert np.array_equal(one["done"][0].numpy() != 0, moved)


def test_two_substeps_take_the_loop_kernel(require_gpu, monkeypatch):
    """steps_per_run == 2 (physics at twice the agent rate): the switch changes
    nothing, the launcher is on the loop kernel either way."""
    a, n_task, n_limit = run(monkeypatch, "CartPoleDiscreteBalancing", 130, False, force_loop=False,
                             physics_rate=2000.0)
    b, _, _ = run(monkeypatch, "CartPoleDiscreteBalancing", 130, False, force_loop=True, physics_rate=2000.0)
    assert n_task > 0 and n_limit > 0
    assert_bit_equal(a, b)
