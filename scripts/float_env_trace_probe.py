#!/usr/bin/env python3
"""Workload for a kernel trace of the floating-base env's two task kernels:
300 eager steps of a plain FloatVecEnv and of one with the locomotion task on
(the configuration of bench_float_env.py --task locomotion), alternating, for
the iCub at 512 worlds and the quadruped at 4,096.  Both hold the home
posture, so the run kernel does the same work in either.

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python3 scripts/float_env_trace_probe.py

The dispatches of float_env_action_kernel<LOCO> and float_env_post_kernel<RAND,
PUSH, LOCO> in OUT/run_kernel_trace.csv, grouped by kernel name and grid size
(2,048 threads: the iCub's 8 blocks; 16,384: the quadruped's 64), give the
cost of each kernel with and without the task (profiles/float_loco/).

--init runs, instead of the locomotion env, the two envs of bench_float_env.py
--init beside the plain one: episodes of 20 steps that reset to the home state,
and the same with the initial-state randomisation and a 256-row bank on.  Every
20th dispatch of float_env_post_kernel of either is a launch in which all
worlds reset (profiles/float_init/).

--tracking runs the env of bench_float_env.py --tracking beside the plain one:
two looping clips of the home state followed at 2 / 3 frames per step.  Both
post kernels are the same instance; the dispatches of the tracking env are the
ones with the larger dynamic LDS (LDS_Block_Size in the trace)."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-ignition_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def init_probe(np, torch, FloatVecEnv):
    from bench_float_env import INIT, INIT_EPISODE, init_bank
    for model, W in (("icub", 512), ("quadruped", 4096)):
        plain = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0)
        ibase = getattr(FloatVecEnv, model)(W, max_episode_steps=INIT_EPISODE, z_min=-10.0)
        started = getattr(FloatVecEnv, model)(W, max_episode_steps=INIT_EPISODE, z_min=-10.0,
                                              init_states=init_bank(torch, plain), **INIT)
        envs = (plain, ibase, started)
        for env in envs:
            env.reset()
        hold = torch.from_numpy(np.tile(plain.home_q, (W, 1))).to(plain.device)
        for _ in range(300):
            for env in envs:
                env.step_raw(hold.data_ptr())
        torch.cuda.synchronize()
        for env in envs:
            env.close()


def tracking_probe(np, torch, FloatVecEnv):
    from bench_float_env import TRACK, home_clips
    for model, W in (("icub", 512), ("quadruped", 4096)):
        plain = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0)
        fps = 2.0 / 3.0 / (plain.sim.step_size * plain.sim.steps_per_run)
        tracked = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, clip_fps=fps,
                                              motion_clips=home_clips(torch, plain), **TRACK)
        plain.reset()
        tracked.reset()
        hold = torch.from_numpy(np.tile(plain.home_q, (W, 1))).to(plain.device)
        for _ in range(300):
            plain.step_raw(hold.data_ptr())
            tracked.step_raw(hold.data_ptr())
        torch.cuda.synchronize()
        plain.close()
        tracked.close()


def main():
    import numpy as np
    import torch
    from mwstep import FloatVecEnv
    if not torch.cuda.is_available():
        sys.exit("float_env_trace_probe.py needs the GPU")
    if "--init" in sys.argv[1:]:
        return init_probe(np, torch, FloatVecEnv)
    if "--tracking" in sys.argv[1:]:
        return tracking_probe(np, torch, FloatVecEnv)
    from bench_float_env import LOCOMOTION
    for model, W in (("icub", 512), ("quadruped", 4096)):
        plain = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0)
        loco = getattr(FloatVecEnv, model)(W, max_episode_steps=0, z_min=-10.0, **LOCOMOTION)
        plain.reset()
        loco.reset()
        hold = torch.from_numpy(np.tile(plain.home_q, (W, 1))).to(plain.device)
        zeros = torch.zeros((W, loco.action_dim), dtype=torch.float32, device=loco.device)
        for _ in range(300):
            plain.step_raw(hold.data_ptr())
            loco.step_raw(zeros.data_ptr())
        torch.cuda.synchronize()
        plain.close()
        loco.close()


if __name__ == "__main__":
    main()
