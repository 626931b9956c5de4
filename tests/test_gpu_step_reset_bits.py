"""Bit-identity of the step kernels where worlds reset one by one.

tests/golden/step_reset_bits.json holds sha256 digests written by
tests/golden/make_step_reset_bits.py on the GPU from the build that preceded
the step kernel's helper wave: CartPole (discrete) and Pendulum, 1500
closed-loop steps with max_episode_steps=5000, so every reset is a task `done`
and wavefronts hold done and not-done lanes together (the generator asserts
it).  The reset state is a function of (seed, world, episode) alone; who
computes it and when (a helper wave beside the physics, through LDS, on the
64-world blocks; inline on the 256-thread path) may not move one bit, so the
digests must be EQUAL.  Worlds 1, 63, 65, 130, 16384, 16385; baked and generic.

test_steps_equal_rollout needs no fixture: T closed-loop steps and one fused
rollout of the same actions return the same arrays bit for bit.  The rollout
kernel resets inline, the step kernel takes the reset state from its helper
wave.  (The two were bit-equal before the helper wave existed as well.)
"""

import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_step_reset_bits",
                                               os.path.join(_GOLDEN, "make_step_reset_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module")
def recorded():
    with open(bits.FIXTURE) as f:
        doc = json.load(f)
    assert (doc["steps"], doc["max_episode_steps"]) == (bits.STEPS, bits.MAX_EPISODE_STEPS)
    assert sorted(doc["digests"]) == sorted(c[0] for c in bits.CASES)
    return doc["digests"]


@pytest.mark.parametrize("case", bits.CASES, ids=[c[0] for c in bits.CASES])
def test_step_reset_bits(require_gpu, recorded, monkeypatch, case):
    if case[3]:
        monkeypatch.setenv("MWSTEP_DISABLE_BAKED", "1")
    else:
        monkeypatch.delenv("MWSTEP_DISABLE_BAKED", raising=False)
    got = bits.run_case(case)
    want = recorded[case[0]]
    differing = sorted(k for k in want if got.get(k) != want[k])
    assert not differing and sorted(got) == sorted(want), f"{case[0]}: digests differ for {differing}"


@pytest.mark.parametrize("task", ["CartPoleDiscreteBalancing", "PendulumSwingUp"])
@pytest.mark.parametrize("W", [65, 130])
def test_steps_equal_rollout(require_gpu, monkeypatch, task, W):
    import torch
    from mwstep.vecenv import VecEnv
    monkeypatch.delenv("MWSTEP_DISABLE_BAKED", raising=False)
    T = bits.STEPS
    acts = torch.from_numpy(bits.actions_for(task, T, W)).cuda()

    def make():
        env = VecEnv(task, n_worlds=W, seed=42, max_episode_steps=bits.MAX_EPISODE_STEPS)
        env.reset()
        return env

    a = make()
    obs = torch.empty((T, W, a.obs_dim), device=a.device)
    term = torch.zeros((T, W, a.obs_dim), device=a.device)
    rew = torch.empty((T, W), device=a.device)
    done = torch.empty((T, W), dtype=torch.uint8, device=a.device)
    for t in range(T):
        o, r, d, info = a.step(acts[t])
        obs[t].copy_(o)
        rew[t].copy_(r)
        done[t].copy_(d)
        # step() leaves terminal_obs of a not-done world as it was; rollout() leaves it zero
        term[t].copy_(torch.where(d[:, None] != 0, info["terminal_obs"], term[t]))
    b = make()
    robs, rrew, rdone, rterm = b.rollout(acts)
    assert int(done.sum()) > 0 and 0 < int(done[:, :64].sum(1).max()) < 64, "no partly done wave"
    for name, x, y in (("obs", obs, robs), ("reward", rew, rrew), ("done", done, rdone),
                       ("terminal_obs", term, rterm)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    for x, y in zip(a.state() + a.counters(), b.state() + b.counters()):
        assert torch.equal(x, y)
    a.close()
    b.close()
