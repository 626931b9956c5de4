"""Writes tests/golden/step_reset_bits.json: sha256 digests of closed-loop runs
in which the task itself ends episodes, so that worlds reset at different steps
and a wavefront holds done and not-done lanes side by side.  For
tests/test_gpu_step_reset_bits.py (which imports the cases and the runner from
here).  Needs a GPU.

    python tests/golden/make_step_reset_bits.py [path/to/libmwstep.so [out.json]]

tests/golden/step_bits.json resets every world at the same step (TimeLimit 40):
a wave there is all done or all not done.  Here max_episode_steps is 5000 and
the run is STEPS long, so every reset is a task `done` (CartPole: the pole or
the cart leaves its bounds under random actions after some hundred steps;
Pendulum: |dq| > 10).  The committed fixture comes from the build of the commit
BEFORE the step kernel got its helper wave (which draws the reset state beside
the physics and hands it over through LDS), so the test demands bit-identical
results of that change and of every later one.

Digests: obs, reward, done, terminal_obs, q, qd, steps and episode after the
last step, and one running sha256 over `done` and `terminal_obs` of EVERY step.
Worlds: 1; 63; 65 (a second block whose helper has one live lane); 130; 16384
and 16385, the two sides of the switch from 64-world blocks (with helper wave)
to 256-thread blocks (inline reset).  Each on the constant-folded (baked) kernel
and, with MWSTEP_DISABLE_BAKED=1, on the generic one.
"""

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "step_reset_bits.json")

STEPS, MAX_EPISODE_STEPS, CHUNK = 1500, 5000, 100
WORLDS = (1, 63, 65, 130, 16384, 16385)
ACTION_RANGE = {"PendulumSwingUp": 50.0}
VARIANTS = (("discrete", "CartPoleDiscreteBalancing"), ("pendulum", "PendulumSwingUp"))
CASES = [(f"{name}-W{W}-{'generic' if generic else 'baked'}", task, W, generic)
         for name, task in VARIANTS for W in WORLDS for generic in (False, True)]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def actions_for(task, T, W, seed=11):
    """Seeded actions on the device, [T, W] (drawn on the host: the same on every machine)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    if task == "CartPoleDiscreteBalancing":
        return rng.integers(0, 2, size=(T, W), dtype=np.int32)
    a = ACTION_RANGE[task]
    return rng.uniform(-a, a, size=(T, W)).astype(np.float32)


def run_steps(env, acts):
    """Closed loop over acts [T, W]; returns the last step's outputs, the
    running digest of every step's done / terminal_obs, and what the resets
    looked like: (steps with 0 < done.sum() < W, steps with a wave of 64 worlds
    holding done and not-done lanes)."""
    import numpy as np
    import torch
    T, W = acts.shape
    running = hashlib.sha256()
    dbuf = torch.empty((CHUNK, W), dtype=torch.uint8, device=env.device)
    tbuf = torch.empty((CHUNK, W, env.obs_dim), dtype=torch.float32, device=env.device)
    mixed_steps = mixed_waves = 0
    wave = np.arange(W) // 64
    lanes = np.bincount(wave)
    for t in range(T):
        obs, reward, done, info = env.step(acts[t])
        dbuf[t % CHUNK].copy_(done)
        tbuf[t % CHUNK].copy_(info["terminal_obs"])
        if (t + 1) % CHUNK == 0 or t + 1 == T:
            n = t % CHUNK + 1
            d = dbuf[:n].cpu().numpy()
            running.update(d.tobytes())
            running.update(tbuf[:n].cpu().numpy().tobytes())
            for row in d:
                k = int(row.sum())
                mixed_steps += 0 < k < W
                per_wave = np.bincount(wave, weights=row, minlength=len(lanes))
                mixed_waves += bool(((per_wave > 0) & (per_wave < lanes)).any())
    return obs, reward, done, info["terminal_obs"], running.hexdigest(), (mixed_steps, mixed_waves)


def run_case(case):
    """Digests of one case on the library mwstep.native has loaded.  The caller
    sets MWSTEP_DISABLE_BAKED for the generic cases (read at env creation)."""
    import torch
    from mwstep.vecenv import VecEnv
    _, task, W, generic = case
    assert bool(os.environ.get("MWSTEP_DISABLE_BAKED") == "1") == generic
    env = VecEnv(task, n_worlds=W, seed=42, max_episode_steps=MAX_EPISODE_STEPS)
    assert bool(env.sim.baked_model()) != generic
    env.reset()
    acts = torch.from_numpy(actions_for(task, STEPS, W)).to(env.device)
    obs, reward, done, term, running, (mixed_steps, mixed_waves) = run_steps(env, acts)
    q, qd = env.state()
    episode, steps = env.counters()
    out = {"obs": _sha(obs), "reward": _sha(reward), "done": _sha(done), "terminal_obs": _sha(term),
           "q": _sha(q), "qd": _sha(qd), "steps": _sha(steps), "episode": _sha(episode),
           "done_terminal_obs_all_steps": running}
    # the case has to exercise what it is there for: task-done resets, at
    # different steps in different worlds, inside one wave
    assert int(episode.max()) >= 1, "no auto-reset in the case"
    if W > 1:
        assert mixed_steps > 0, "no step with 0 < done.sum() < W"
        assert mixed_waves > 0, "no wave with done and not-done lanes"
    env.close()
    return out


def main():
    if len(sys.argv) > 1:
        os.environ["MWSTEP_LIB"] = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.join(ROOT, "gym-ignition_amd", "python"))
    from mwstep import native
    digests = {}
    for case in CASES:
        if case[3]:
            os.environ["MWSTEP_DISABLE_BAKED"] = "1"
        else:
            os.environ.pop("MWSTEP_DISABLE_BAKED", None)
        digests[case[0]] = run_case(case)
    os.environ.pop("MWSTEP_DISABLE_BAKED", None)
    doc = {"library_version": native.lib().mw_version().decode(), "steps": STEPS,
           "max_episode_steps": MAX_EPISODE_STEPS, "digests": digests}
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(digests)} cases from {native.LIB_PATH}")


if __name__ == "__main__":
    main()
