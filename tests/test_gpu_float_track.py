"""FloatVecEnv's motion-clip tracking task (mw_floatenv_tracking) on the GPU, on
the quadruped: 70 worlds (one full tile and one of 6 rows, where the staging of
the reference rows would go wrong), two synthetic clips of 12 frames around the
stand posture -- one looping, one not -- at 2 / 3 frames per control step, and
episodes short enough that every world resets several times.

Every step of every world is held to the fp64 restatement of
tests/float_track_ref.py from the rows of obs / terminal_obs and the clips,
within the bounds that module derives (see test_float_track_host.py), and the
five errors and the reference words of obs to the host build of the kernel's own
arithmetic bit for bit (float_track_check.TrackCheck)."""

import numpy as np
import pytest

import float_init_ref as RI
import float_track_ref as R
from float_env_harness import FREE, LOCO, STAND, _dev, _make
from float_track_check import TrackCheck, synthetic_clip
from test_float_track_host import build_harness

pytestmark = pytest.mark.gpu

W, NQ = 70, 8
NS = 13 + 2 * NQ
HOME = (0.0, 0.0, 0.45, 1.0, 0.0, 0.0, 0.0)
FRAMES, NUM, DEN = 12, 2, 3
ENV_DT = 1e-3                                           # step_size 1e-3, one physics step per control step
FPS = NUM / DEN / ENV_DT
WEIGHTS = dict(pose=0.5, velocity=0.05, root_pos=0.2, root_rot=0.15, root_vel=0.1)
SCALES = dict(pose=2.0, velocity=0.1, root_pos=10.0, root_rot=5.0, root_vel=1.0, ang_scale=0.1)


@pytest.fixture(scope="module")
def ftk(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("ftk"))


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(3)
    return [synthetic_clip(HOME, STAND, FRAMES, True, rng), synthetic_clip(HOME, STAND, FRAMES, False, rng, step=(0.01, -0.02))]


def _np(t):
    return t.cpu().numpy()


def _env(clips, seed, **kw):
    import torch
    dev = [torch.from_numpy(c).cuda() for c in clips]
    args = dict(motion_clips=dev, clip_loop=(True, False), clip_fps=FPS, track_weights=WEIGHTS, track_scales=SCALES,
                seed=seed, w_forward=0.0, **FREE)
    args.update(kw)
    return _make("quadruped", W, **args)


def _actions(env, rng, obs, spread=0.05):
    """Follow the reference joint positions, a little off."""
    return (obs[:, env.obs_slices["reference"]] + rng.uniform(-spread, spread, (W, NQ))).astype(np.float32)


def test_resets_steps_clip_end_and_loop(require_gpu, oracle, ftk, clips):
    """(a) resets, (b) every step, (c) the clip's end and the loop's wrap."""
    seed, H, steps = 31, 20, 45
    env = _env(clips, seed, max_episode_steps=H)
    both = np.concatenate(clips)
    assert env.obs_dim == NS + 4 + 3 + NQ and env.clip_fraction == (NUM, DEN)
    assert env.clip_table == ((0, FRAMES, True), (FRAMES, FRAMES, False))
    assert env.tracking_terms.shape == env.tracking_errors.shape == (W, 5)
    assert env.obs_slices["phase"] == slice(NS + 4, NS + 6) and env.obs_slices["clip"] == slice(NS + 6, NS + 7)
    assert env.obs_slices["reference"] == slice(NS + 7, NS + 7 + NQ)
    check = TrackCheck(env, oracle, ftk, both, seed, NUM, DEN, WEIGHTS, SCALES, max_steps=H)
    obs = _np(env.reset())
    check.start(obs)
    assert set(check.clip.tolist()) == {0, 1} and len(set(check.f0.tolist())) >= FRAMES - 3
    assert check.f0.max() == FRAMES - 2 and check.f0.min() == 0
    rng = np.random.default_rng(5)
    n_done = np.zeros(W, int)
    loop_x = []
    for k in range(steps):
        o, r, d, info = env.step(_dev(env, _actions(env, rng, obs)))
        assert info["tracking_terms"] is env.tracking_terms and info["track_frame"] is env.track_frame
        obs, r, d = _np(o), _np(r), _np(d).astype(bool)
        # the loop's wrap: the reference base position moves on by the clip's displacement per period
        for w in check.worlds:
            if check.clip[w] == 0 and not d[w]:
                ck = R.clock(int(check.f0[w]), int(check.t[w]) + 1, NUM, DEN, FRAMES, True)
                if ck[3] > 0:
                    loop_x.append(R.reference_row(both, env.clip_table[0], ck)[0] - both[ck[0], 0])
        check.step(obs, r, d, info)
        n_done += d
    check.report("tracking on the quadruped")
    assert n_done.min() >= 2                               # every world reset several times
    ep, st = env.counters()
    np.testing.assert_array_equal(_np(ep), check.episode)
    np.testing.assert_array_equal(_np(st), check.t)
    # both ways an episode ends here, and the wrap, were met, and the nlerp had to flip a sign
    assert check.seen["clip_end"] > W and check.seen["time_limit"] > 10 and check.seen["failed"] == 0
    assert check.seen["wraps"] > 50 and check.seen["flips"] > 50
    disp = float(both[FRAMES - 1, 0]) - float(both[0, 0])
    assert len(loop_x) > 50 and min(loop_x) > 0.9 * disp   # the accumulated root displacement is in the reference
    assert check.bit_mismatch.tolist() == [0, 0, 0, 0, 0]
    env.close()


def test_early_termination(require_gpu, oracle, ftk, clips):
    """(d) a tight max_pose ends episodes as terminated, without the alive bonus."""
    seed = 32
    bounds = dict(pose=2e-2, root_rot=0.5)
    env = _env(clips, seed, max_episode_steps=0, track_termination=bounds, rsi_prob=0.5)
    both = np.concatenate(clips)
    check = TrackCheck(env, oracle, ftk, both, seed, NUM, DEN, WEIGHTS, SCALES, bounds=(2e-2, 0.0, 0.5), rsi_prob=0.5)
    obs = _np(env.reset())
    check.start(obs)
    assert (check.f0 == 0).sum() > W // 3 and (check.f0 > 0).sum() > W // 5       # rsi_prob: half start at frame 0
    rng = np.random.default_rng(6)
    bonus_free = 0
    for k in range(12):
        o, r, d, info = env.step(_dev(env, _actions(env, rng, obs, spread=0.3)))
        obs, r, d = _np(o), _np(r), _np(d).astype(bool)
        pose = _np(env.tracking_errors)[:, 0]
        ended = np.array([R.clock(int(check.f0[w]), int(check.t[w]) + 1, NUM, DEN, FRAMES, bool(env.clip_table[int(check.clip[w])][2]))[4]
                          for w in range(W)])
        np.testing.assert_array_equal(d, (pose > np.float32(2e-2)) | ended)
        terms = _np(env.tracking_terms).astype(np.float64).sum(axis=1)
        over = pose > np.float32(2e-2)
        assert (np.abs(r[over] - terms[over]) <= 1e-6).all()                # terminated: no alive bonus
        assert (np.abs(r[~over] - 1.0 - terms[~over]) <= 1e-6).all()        # truncated or running: the bonus is kept
        bonus_free += int(over.sum())
        check.step(obs, r, d, info)
    check.report("early termination")
    assert check.seen["failed"] == bonus_free > W // 2
    env.close()


def test_graph_replay_matches_eager_steps(require_gpu, clips):
    """(e) one captured step, replayed with resets inside, is the eager steps bit for bit."""
    import torch
    K = 10
    kw = dict(max_episode_steps=4, joint_noise=0.02)
    rng = np.random.default_rng(8)
    acts = (np.float32(STAND) + rng.uniform(-0.2, 0.2, (K + 1, W, NQ))).astype(np.float32)
    plain = _env(clips, 33, **kw)
    plain.reset()
    plain.step(torch.from_numpy(acts[0]).to(plain.device))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = _env(clips, 33, **kw)
        env.reset()
        a = torch.from_numpy(acts[0]).to(env.device)
        env.step(a)                                  # warm-up
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            env.step(a)
        n_done = 0
        for k in range(K):
            a.copy_(torch.from_numpy(acts[k + 1]).to(env.device))
            graph.replay()
            side.synchronize()
            plain.step(torch.from_numpy(acts[k + 1]).to(plain.device))
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"replay {k + 1}")
            for name in ("obs", "reward", "done", "terminal_obs", "tracking_terms", "tracking_errors", "track_clip",
                         "track_frame", "init_state"):
                np.testing.assert_array_equal(_np(getattr(env, name)), _np(getattr(plain, name)), err_msg=name)
            n_done += int(env.done.sum())
    assert n_done >= 2 * W
    env.close()
    plain.close()


def test_combined_with_locomotion_shaping_noise_and_init_offsets(require_gpu, oracle, ftk, clips):
    """(f) everything on together: the tracking words carry no noise, the slices
    tile the row, the per-step checks hold on the clean rows, the start state is
    the clip row plus the reported offsets, and episode_return includes the terms."""
    seed, H = 34, 9
    pos, lin = ((-0.05, 0.05), (-0.05, 0.05), (0.0, 0.05)), ((-0.2, 0.2), (-0.2, 0.2), (0.0, 0.0))
    noise = dict(base_position=0.01, joint_positions=0.02, joint_velocities=0.5, gravity=0.05)
    env = _env(clips, seed, max_episode_steps=H, obs_noise=noise, action_scale=0.25,
               reward_terms=dict(torque=2e-5, orientation=1.0, joint_acc=2.5e-7), termination_links=(),
               init_pos_range=pos, init_lin_vel_range=lin, **LOCO)
    both = np.concatenate(clips)
    sl = env.obs_slices
    nb = NS + 4
    assert sl["last_action"].stop == nb + 12 + NQ == sl["phase"].start and sl["reference"].stop == env.obs_dim
    covered = sorted((s.start, s.stop) for s in sl.values())
    assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:])) and covered[-1][1] == env.obs_dim
    amp = _np(env.obs_noise)
    assert (amp[sl["phase"].start:] == 0).all() and (amp[:3] > 0).all()
    for name in ("phase", "clip", "reference"):
        with pytest.raises(ValueError, match="take no noise"):
            env._noise_vector({name: 0.1})
    check = TrackCheck(env, oracle, ftk, both, seed, NUM, DEN, WEIGHTS, SCALES, max_steps=H, worlds=range(0, W, 3))
    obs = _np(env.reset())
    clean = _np(env.clean_obs)
    check.start(clean, exact_state=False)
    track = slice(sl["phase"].start, env.obs_dim)
    np.testing.assert_array_equal(obs[:, track].view(np.uint32), clean[:, track].view(np.uint32))
    assert (obs[:, :3] != clean[:, :3]).any()

    def check_start(worlds):
        # the clip row plus the reported draws, one rounding each; joint words the row's
        state, draws = _np(env.init_state), _np(env.init_draws)
        for w in worlds:
            row = both[env.clip_table[int(check.clip[w])][0] + int(check.f0[w])]
            want = RI.base_words32(row, draws[w], RI.POS | RI.LIN)
            np.testing.assert_array_equal(state[w, :13].view(np.uint32), want.view(np.uint32))
            np.testing.assert_array_equal(state[w, 13:].view(np.uint32), row[13:].view(np.uint32))
            assert draws[w, 12] == -1.0
    check_start(range(W))
    assert np.abs(_np(env.init_draws)[:, :3]).max() > 0.03
    rng = np.random.default_rng(7)
    finished = 0
    for k in range(2 * H + 2):
        a = rng.uniform(-0.3, 0.3, (W, NQ)).astype(np.float32)
        o, r, d, info = env.step(_dev(env, a))
        obs, r, d = _np(o), _np(r), _np(d).astype(bool)
        clean, clean_term = _np(env.clean_obs), _np(env.clean_terminal_obs)
        np.testing.assert_array_equal(obs[:, track].view(np.uint32), clean[:, track].view(np.uint32))
        term_obs = _np(info["terminal_obs"])
        np.testing.assert_array_equal(term_obs[d][:, track].view(np.uint32), clean_term[d][:, track].view(np.uint32))
        check.step(obs, r, d, info, exact_state=False, check_reward=False, clean=clean, clean_term=clean_term)
        if d.any():
            check_start(np.flatnonzero(d))
            # the finished episodes' return is the sum of their rewards, the tracking terms among them
            got = _np(env.episode_return)[d].astype(np.float64)
            want, part = check.last_return[d], check.last_terms[d]
            tol = 2.0 ** -23 * (H + 1) * np.maximum(1.0, np.abs(want))
            assert (np.abs(got - want) <= tol).all(), (got, want)
            assert (part > 100 * tol).all()                              # ... which the sum would miss by far
            finished += int(d.sum())
    check.report("tracking with locomotion, shaping, noise and init offsets")
    assert finished >= 2 * W
    env.close()


def test_refusals(require_gpu, clips):
    """(g) what the env refuses, through the Python layer."""
    import torch
    from mwstep import FloatVecEnv
    from mwstep import native as N
    dev = [torch.from_numpy(c).cuda() for c in clips]
    quad = lambda **kw: _make("quadruped", 4, **FREE, **kw)
    with pytest.raises(RuntimeError, match="cannot be combined with mw_floatenv_tracking"):
        quad(motion_clips=dev, init_states=torch.zeros((3, NS), device="cuda"))
    with pytest.raises(RuntimeError, match="the length of a clip must be >= 2"):
        quad(motion_clips=[dev[0], dev[1][:1].contiguous()])
    with pytest.raises(ValueError, match="1 to 16 clips"):
        quad(motion_clips=[dev[0]] * 17)
    with pytest.raises(ValueError, match="no ratio of whole numbers"):
        quad(motion_clips=dev, clip_fps=1000.0 / np.pi)
    with pytest.raises(ValueError, match="unknown name"):
        quad(motion_clips=dev, track_weights=dict(hands=1.0))
    with pytest.raises(TypeError, match="shape"):
        quad(motion_clips=torch.zeros((5, NS + 1), device="cuda"))
    # at the C layer: the denominator, the 17th clip, the call order
    env = quad()
    assert env.tracking_terms is None and env.track_clip is None and env.motion_clips is None
    assert "phase" not in env.obs_slices and "tracking_terms" not in env._info

    def call(cfg):
        return N.lib().mw_floatenv_tracking(env._h, cfg, dev[0].data_ptr(), None, None, None, None)
    i16 = lambda *v: (N.ctypes.c_int32 * 16)(*v)
    f5 = (N.ctypes.c_float * 5)()
    base = dict(n_frames=FRAMES, n_clips=1, clip_first=i16(0), clip_length=i16(FRAMES), clip_loop=i16(1), frame_num=1,
                frame_den=1, weights=f5, scales=f5, rsi_prob=1.0)
    for change, fragment in ((dict(frame_den=0), "frame_num and frame_den must be >= 1"),
                             (dict(n_clips=17), "n_clips must be in [1, 16]"),
                             (dict(clip_length=i16(1)), "the length of a clip must be >= 2")):
        cfg = N.MwFloatTrackConfig(**{**base, **change})
        assert call(N.ctypes.byref(cfg)) == N.MW_EINVAL and fragment in N.last_error()
    nc = N.MwFloatNoiseConfig(0, 2)
    assert N.lib().mw_floatenv_noise(env._h, N.ctypes.byref(nc), None, None, None, None) == N.MW_OK
    cfg = N.MwFloatTrackConfig(**base)
    assert call(N.ctypes.byref(cfg)) == N.MW_ESTATE and "before mw_floatenv_noise" in N.last_error()
    env.close()
    env = quad()
    env.reset()
    assert call(N.ctypes.byref(cfg)) == N.MW_ESTATE and "before the first mw_vecenv_reset" in N.last_error()
    env.close()
