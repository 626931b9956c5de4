"""Writes tests/golden/step_bits.json: sha256 digests of what the batched env's
step kernels produce, for tests/test_gpu_step_bits.py (which imports the cases
and the runner from here).  Needs a GPU.

    python tests/golden/make_step_bits.py [--add-missing] [path/to/libmwstep.so [out.json]]

Run it against the library whose results are the reference.  The first 48
cases of the committed fixture (the variants up to `discrete_rollout`) come
from the build of the commit BEFORE the step kernel took flat, preloaded
arguments, so the test demands bit-identical results of that change and of
every later one.  The 36 cases of the randomised kernels (`*_randomized` of
the other three tasks, and `discrete_randomized_` rollout / offset1000 /
2substeps) were added with --add-missing from the build of the commit that
added them, whose kernels still reproduce the first 48 bit for bit.
(MWSTEP_LIB, or the path argument, selects the library; the default is the
in-tree build.)

--add-missing runs every case, refuses to write anything if a digest already
in the fixture would change, and otherwise adds the cases the fixture lacks:
the entries it had come out byte for byte as they were.

A case is 120 closed-loop steps with max_episode_steps=40 and seeded actions,
so TimeLimit, auto-reset, terminal_obs and the episode counter all act (the
last step is itself a TimeLimit step); or one fused 50-step rollout.  Every
case runs on the constant-folded (baked) kernel and, with
MWSTEP_DISABLE_BAKED=1, on the generic one.
"""

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "step_bits.json")

STEPS, MAX_EPISODE_STEPS, ROLLOUT_STEPS = 120, 40, 50
# 1 world; a partial second wave; the 256-thread path with a partial last block
WORLDS = (1, 65, 16449)
ACTION_RANGE = {"CartPoleContinuousBalancing": 50.0, "CartPoleContinuousSwingup": 200.0, "PendulumSwingUp": 50.0}
# (variant name, task, VecEnv keyword arguments, fused rollout?)
VARIANTS = (
    ("discrete", "CartPoleDiscreteBalancing", {}, False),
    ("balancing", "CartPoleContinuousBalancing", {}, False),
    ("swingup", "CartPoleContinuousSwingup", {}, False),
    ("pendulum", "PendulumSwingUp", {}, False),
    ("discrete_randomized", "CartPoleDiscreteBalancing", {"randomize": True}, False),
    ("discrete_offset1000", "CartPoleDiscreteBalancing", {"world_offset": 1000}, False),
    ("discrete_2substeps", "CartPoleDiscreteBalancing", {"physics_rate": 2000.0}, False),
    ("discrete_rollout", "CartPoleDiscreteBalancing", {}, True),
    ("balancing_randomized", "CartPoleContinuousBalancing", {"randomize": True}, False),
    ("swingup_randomized", "CartPoleContinuousSwingup", {"randomize": True}, False),
    ("pendulum_randomized", "PendulumSwingUp", {"randomize": True}, False),
    ("discrete_randomized_rollout", "CartPoleDiscreteBalancing", {"randomize": True}, True),
    ("discrete_randomized_offset1000", "CartPoleDiscreteBalancing", {"randomize": True, "world_offset": 1000}, False),
    ("discrete_randomized_2substeps", "CartPoleDiscreteBalancing", {"randomize": True, "physics_rate": 2000.0}, False),
)
CASES = [(f"{name}-W{W}-{'generic' if generic else 'baked'}", task, kw, rollout, W, generic)
         for name, task, kw, rollout in VARIANTS for W in WORLDS for generic in (False, True)]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def actions_for(task, T, W, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    if task == "CartPoleDiscreteBalancing":
        return rng.integers(0, 2, size=(T, W)).astype(np.int32)
    a = ACTION_RANGE[task]
    return rng.uniform(-a, a, size=(T, W)).astype(np.float32)


def run_case(case):
    """Digests of one case on the library mwstep.native has loaded.  The caller
    sets MWSTEP_DISABLE_BAKED for the generic cases (read at env creation)."""
    import torch
    from mwstep.vecenv import VecEnv
    _, task, kw, rollout, W, generic = case
    assert bool(os.environ.get("MWSTEP_DISABLE_BAKED") == "1") == generic
    env = VecEnv(task, n_worlds=W, seed=42, max_episode_steps=MAX_EPISODE_STEPS, **kw)
    assert bool(env.sim.baked_model()) != generic
    env.reset()
    T = ROLLOUT_STEPS if rollout else STEPS
    acts = torch.from_numpy(actions_for(task, T, W)).to(env.device)
    if rollout:
        obs, reward, done, term = env.rollout(acts)
    else:
        for t in range(T):
            obs, reward, done, info = env.step(acts[t])
        term = info["terminal_obs"]
    q, qd = env.state()
    episode, steps = env.counters()
    out = {"obs": _sha(obs), "reward": _sha(reward), "done": _sha(done), "terminal_obs": _sha(term),
           "q": _sha(q), "qd": _sha(qd), "steps": _sha(steps), "episode": _sha(episode)}
    if kw.get("randomize"):
        m, gz = env.physics()
        out["mass"], out["gravity_z"] = _sha(m), _sha(gz)
    # every world went through three auto-resets (closed loop) / one (rollout)
    assert int(episode.min()) >= (1 if rollout else 3), "the case did not exercise the auto-reset"
    env.close()
    return out


def main():
    argv = [a for a in sys.argv[1:] if a != "--add-missing"]
    add_missing = len(argv) != len(sys.argv) - 1
    if len(argv) > 0:
        os.environ["MWSTEP_LIB"] = os.path.abspath(argv[0])
    sys.path.insert(0, os.path.join(ROOT, "gym-ignition_amd", "python"))
    from mwstep import native
    digests = {}
    for case in CASES:
        if case[5]:
            os.environ["MWSTEP_DISABLE_BAKED"] = "1"
        else:
            os.environ.pop("MWSTEP_DISABLE_BAKED", None)
        digests[case[0]] = run_case(case)
    os.environ.pop("MWSTEP_DISABLE_BAKED", None)
    doc = {"library_version": native.lib().mw_version().decode(), "steps": STEPS,
           "max_episode_steps": MAX_EPISODE_STEPS, "rollout_steps": ROLLOUT_STEPS, "digests": digests}
    out = argv[1] if len(argv) > 1 else FIXTURE
    if add_missing:
        with open(FIXTURE) as f:
            old = json.load(f)
        changed = sorted(k for k, v in old["digests"].items() if digests.get(k) != v)
        if changed or any(old[k] != doc[k] for k in ("steps", "max_episode_steps", "rollout_steps")):
            sys.exit(f"nothing written: this build does not reproduce {len(changed)} recorded cases: {changed}")
        added = sorted(set(digests) - set(old["digests"]))
        doc = dict(old, digests=dict(digests, **old["digests"]))   # the header and the old entries as they were
        print(f"{len(old['digests'])} recorded cases reproduced; adding {len(added)}: {added}")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(doc['digests'])} cases from {native.LIB_PATH}")


if __name__ == "__main__":
    main()
