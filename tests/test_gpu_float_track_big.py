"""FloatVecEnv's motion-clip tracking task on the 48-joint tree
(big_tree_cases.tree48) with the reference joint positions in the observation:
65 worlds (one full tile and a single row), rows of 109 words per frame, dofs
beyond 32 in every sum, and a post launch whose tiles no longer fit the 64 KB a
block gets without asking.

DESIGN.md ("Motion-clip tracking", LDS budget) records the outcome on gfx950:
the plain task with tracking needs 78,144 B per block and the locomotion task
with shaping and tracking 110,400 B, both inside the 163,840 B (160 KiB) a block
may use once the kernel's dynamic-LDS attribute is raised, so both configure and
run.  The tests assert that outcome -- the per-step checks of
test_gpu_float_track.py hold -- and not merely either one."""

import numpy as np
import pytest

import big_tree_cases as C
from float_env_harness import FREE, _dev
from float_track_check import TrackCheck, synthetic_clip
from test_float_track_host import build_harness

pytestmark = pytest.mark.gpu

NAME, N, W = "tree48", 48, 65
NS = 13 + 2 * N
FRAMES, NUM, DEN = 7, 5, 2
WEIGHTS = dict(pose=0.5, velocity=0.05, root_pos=0.2, root_rot=0.15, root_vel=0.1)
SCALES = dict(pose=2.0, velocity=0.01, root_pos=10.0, root_rot=5.0, root_vel=1.0, ang_scale=0.1)


@pytest.fixture(scope="module")
def ftk(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("ftk"))


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("everything", [False, True], ids=["plain", "locomotion+shaping"])
def test_48_joints_with_reference_words(require_gpu, oracle, ftk, everything):
    import torch
    from mwstep import FloatVecEnv
    seed, H, steps = 41, 6, 9
    base, links = C.env_home(oracle, NAME)
    rng = np.random.default_rng(9)
    clips = [synthetic_clip(base, np.zeros(N), FRAMES, True, rng, amp=0.03),
             synthetic_clip(base, np.zeros(N), FRAMES + 3, False, rng, amp=0.03)]
    wj = rng.uniform(0.5, 1.5, N).astype(np.float32)
    extra = {}
    if everything:
        extra = dict(task="locomotion", command_ranges=((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)), cmd_interval=3,
                     reward_terms=dict(torque=2e-5, orientation=1.0, joint_acc=2.5e-7))
    env = FloatVecEnv(C.urdf(NAME), W, action_mode="torque", home_base=base, contact_links=links, pgs_iters=50,
                      pid_gains=None, seed=seed, max_episode_steps=H, w_forward=0.0,
                      motion_clips=[torch.from_numpy(c).cuda() for c in clips], clip_loop=(True, False),
                      clip_fps=NUM / DEN / 1e-3, track_weights=WEIGHTS, track_scales=SCALES, track_joint_weights=wj,
                      obs_reference=True, **FREE, **extra)
    assert env.sim.dofs == N and env.obs_slices["reference"] == slice(env.obs_dim - N, env.obs_dim)
    assert env.obs_dim == (25 + 3 * N if everything else NS) + len(links) + 3 + N
    both = np.concatenate(clips)
    check = TrackCheck(env, oracle, ftk, both, seed, NUM, DEN, WEIGHTS, SCALES, wj=wj, max_steps=H,
                       worlds=list(range(0, W, 5)) + [63, 64])
    obs = _np(env.reset())
    check.start(obs)
    n_done = 0
    for k in range(steps):
        a = rng.uniform(-5, 5, (W, N)).astype(np.float32)
        o, r, d, info = env.step(_dev(env, a))
        obs, r, d = _np(o), _np(r), _np(d).astype(bool)
        check.step(obs, r, d, info, check_reward=not everything)
        n_done += int(d.sum())
    check.report(f"tracking on tree48 ({'locomotion + shaping' if everything else 'plain'})")
    assert n_done >= W and check.seen["wraps"] > 0 and check.seen["clip_end"] > 0
    assert check.bit_mismatch.tolist() == [0, 0, 0, 0, 0]
    if everything:
        # the LDS a kernel may be launched with is the kernel's, not the env's: a second env of the same
        # instances that needs less (no shaping tiles) must not take away what this one was granted
        extra.pop("reward_terms")
        other = FloatVecEnv(C.urdf(NAME), 4, action_mode="torque", home_base=base, contact_links=links, pgs_iters=50,
                            pid_gains=None, seed=seed, motion_clips=[torch.from_numpy(c).cuda() for c in clips],
                            clip_loop=(True, False),
                            clip_fps=NUM / DEN / 1e-3, obs_reference=True, **FREE, **extra)
        other.reset()
        other.step(_dev(other, np.zeros((4, N))))
        o, r, d, info = env.step(_dev(env, rng.uniform(-5, 5, (W, N)).astype(np.float32)))
        check.step(_np(o), _np(r), _np(d).astype(bool), info, check_reward=False)
        torch.cuda.synchronize()
        other.close()
    env.close()
