"""Inertia randomisation of the floating-base env (mw_floatenv_inertia: per-world
link masses and a base payload drawn on the device into the simulator's
per-world link parameters).

The yardstick of the parity tests is the one of test_gpu_float_env.py: a
host-commanded twin Simulator given what the env reports -- here also
env.inertial[w] through Simulator.set_link_params at every reset -- must end
with a bit-identical mw_get_state record.  The draws are restated on the host
from the oracle's Philox4x32-10 within the fused / unfused rounding bound of
U(lo, hi), 4 * 2^-23 * (hi - lo) (test_gpu_float_rand.py), and the ten words
from the reported draws within the derived bound of
tests/host_float_inertia/harness.cpp."""

import ctypes

import numpy as np
import pytest

from float_env_harness import FREE, LOCO, PUSH, STAND, _captured_step_graph, _make, _parity, _twin
from float_inertia_ref import PAYLOAD, SCALE, apply_ref, build_harness, draw_ref, harness_apply, inertia_about_com

pytestmark = pytest.mark.gpu

SCALES, PAYLOADS, BOX = (0.5, 2.0), (0.0, 10.0), (0.1, 0.08, 0.05)
INERTIA = dict(mass_scale_range=SCALES, payload_range=PAYLOADS, payload_box=BOX)


def test_twin_parity_torque_quadruped(require_gpu):
    """W = 70: two tiles of the env kernels, the second partial; episodes of 7
    steps, so the draws of 8 resets of every world interleave with the run."""
    W, steps, H = 70, 60, 7
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=11, joint_noise=0.05,
              max_episode_steps=H, action_scale=0.5, friction_range=(0.3, 1.2), **FREE, **PUSH, **LOCO, **INERTIA)
    env = _make("quadruped", W, **kw)
    assert env.inertial.shape == (W, 9, 10) and env.inertia_draws.shape == (W, 13)
    twin = _twin(env, "quadruped")
    rng = np.random.default_rng(3)
    acts = rng.uniform(-5, 5, (steps + 1, W, 8)).astype(np.float32)
    seen = _parity(env, twin, lambda k: acts[k], steps, H,
                   lambda t, a: t.set("force_target", (np.float32(0.5) * a).astype(np.float64)),
                   carry=("inertial",))["inertial"]
    masses = np.stack([s[:, :, 0] for s in seen])                     # [episodes, W, links]
    nominal = twin.link_params(0, [0])[0, 0]
    print(f"quadruped: {len(seen)} episodes, thigh mass {masses[:, :, 1].min():.3f} .. {masses[:, :, 1].max():.3f} "
          f"(nominal {nominal:.3f}), base mass {masses[:, :, 0].min():.2f} .. {masses[:, :, 0].max():.2f}")
    assert len(np.unique(masses[:, :, 1])) > 0.9 * masses[:, :, 1].size   # differ across worlds and episodes
    env.close()
    twin.close()


def test_twin_parity_position_icub(require_gpu):
    """The <32> instance: 33 links per world, nine Philox blocks of scales."""
    from mwstep.models import icub_pid_gains
    W, steps, H = 5, 60, 20
    kw = dict(max_episode_steps=H, seed=12, action_scale=0.25, friction_range=(0.5, 1.2), joint_noise=0.02,
              mass_scale_range=(0.8, 1.25), payload_range=(0.0, 5.0), payload_box=BOX, **FREE, **PUSH, **LOCO)
    env = _make("icub", W, **kw)
    assert env.inertial.shape == (W, 33, 10)
    gains = [[p, 0.0, d, -80.0, 80.0, 0.0, 0.0, -1.0] for p, d in icub_pid_gains(env.sim.joint_names)]
    twin = _twin(env, "icub", gains)
    rng = np.random.default_rng(5)
    acts = rng.uniform(-0.4, 0.4, (steps + 1, W, 32)).astype(np.float32)
    seen = _parity(env, twin, lambda k: acts[k], steps, H,
                   lambda t, a: t.set("position_target", env.sim.get("position_target")),
                   carry=("inertial",))["inertial"]
    assert len(seen) == 4 and not np.array_equal(seen[0], seen[1])
    env.close()
    twin.close()


def test_draw_restatement(require_gpu, oracle, tmp_path):
    import torch
    W, seed, H, steps = 70, 21, 6, 20
    kw = dict(action_mode="torque", pid_gains=None, seed=seed, max_episode_steps=H, **FREE, **INERTIA)
    env = _make("quadruped", W, **kw)
    part = _make("quadruped", 35, world_offset=35, **kw)
    fi = build_harness(tmp_path)
    n = env.action_dim
    nominal = np.stack([env.sim.link_params(link, [0])[0] for link in range(-1, n)])
    env.reset()
    part.reset()
    # sharding: worlds 35..69 of the big env are the small env's, bit for bit
    np.testing.assert_array_equal(part.inertial.cpu().numpy(), env.inertial.cpu().numpy()[35:])
    np.testing.assert_array_equal(part.inertia_draws.cpu().numpy(), env.inertia_draws.cpu().numpy()[35:])
    tol_s = 4 * 2.0 ** -23 * (SCALES[1] - SCALES[0])
    tol_m = 4 * 2.0 ** -23 * (PAYLOADS[1] - PAYLOADS[0])
    tol_p = [4 * 2.0 ** -23 * 2 * b for b in BOX]
    worlds = list(range(0, W, 7))
    zero = torch.zeros((W, n), dtype=torch.float32, device=env.device)
    worst = dict(scale=0.0, payload=0.0, position=0.0, words=0.0)
    host_equal = True
    history = []

    def check(episode):
        nonlocal host_equal
        draws, words = env.inertia_draws.cpu().numpy(), env.inertial.cpu().numpy()
        s, mp, p = draws[:, :n + 1], draws[:, n + 1], draws[:, n + 2:]
        assert SCALES[0] - tol_s <= s.min() and s.max() <= SCALES[1] + tol_s
        assert PAYLOADS[0] - tol_m <= mp.min() and mp.max() <= PAYLOADS[1] + tol_m
        assert (np.abs(p) <= np.float32(BOX) + np.float32(tol_p)).all()
        assert len(np.unique(s)) > 0.9 * s.size and len(np.unique(mp)) > 0.9 * W
        for w in worlds:
            rs, rm, rp = draw_ref(oracle, seed, w, episode, n, SCALES, PAYLOADS, BOX)
            worst["scale"] = max(worst["scale"], float(np.abs(s[w].astype(np.float64) - rs).max()) / tol_s)
            worst["payload"] = max(worst["payload"], abs(float(mp[w]) - float(rm)) / tol_m)
            worst["position"] = max(worst["position"], float((np.abs(p[w].astype(np.float64) - rp) / tol_p).max()))
        # the ten words from the reported draws: the kernel's code on the host, and fp64 within its bound
        for w in range(W):
            zeros = np.zeros(n + 1, np.float32)
            got, bound = harness_apply(fi, SCALE, nominal, s[w], zeros, np.zeros((n + 1, 3), np.float32))
            ref = apply_ref(SCALE, nominal, s[w], zeros, np.zeros((n + 1, 3)))
            b_got, b_bound = harness_apply(fi, SCALE | PAYLOAD, nominal[:1], s[w, :1], mp[w:w + 1], p[w:w + 1])
            got[0], bound[0] = b_got[0], b_bound[0]
            ref[0] = apply_ref(SCALE | PAYLOAD, nominal[:1], s[w, :1], mp[w:w + 1], p[w:w + 1])[0]
            err = np.abs(words[w].astype(np.float64) - ref)
            worst["words"] = max(worst["words"], float((err / np.maximum(bound, 1e-300))[bound > 0].max()))
            assert (err <= bound).all(), (w, np.argwhere(err > bound))
            host_equal = host_equal and np.array_equal(got, words[w])
        m, _, Ic = inertia_about_com(words)
        assert (m > 0).all() and (np.linalg.eigvalsh(Ic)[..., 0] > 0).all()
        for link in range(-1, n):
            np.testing.assert_array_equal(env.sim.link_params(link), words[:, link + 1])
        history.append(words.copy())

    check(0)
    for i in range(steps):
        _, _, d, _ = env.step(zero)
        assert bool(d.all()) == ((i + 1) % H == 0)
        if d.all():
            check((i + 1) // H)      # the post launch has already drawn the new episode's words
    assert len(history) == 1 + steps // H
    assert all(not np.array_equal(history[0][w], history[1][w]) for w in range(W))
    print("draw restatement (error / bound): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; the host build of the kernel's code gives the reported words bit for bit: {host_equal}")
    assert all(v <= 1.0 for v in worst.values())
    env.close()
    part.close()


def test_unit_scale_is_no_scale(require_gpu):
    """mass_scale_range (1, 1), no payload: the per-world instances run, every
    reset rewrites the records, and no bit of 60 steps differs from an env
    without the feature.  While the env exists the simulator's setter is
    refused and its getter reads the drawn words; afterwards it works again."""
    import torch
    from mwstep import native as N
    W, steps, H = 70, 60, 7
    kw = dict(action_mode="torque", home_base=(0, 0, 0.47, 1, 0, 0, 0), pid_gains=None, seed=9, joint_noise=0.05,
              max_episode_steps=H, **FREE)
    env = _make("quadruped", W, mass_scale_range=(1.0, 1.0), **kw)
    plain = _make("quadruped", W, **kw)
    assert plain.inertial is None and plain.inertia_draws is None and env.inertial is not None
    nominal = np.stack([plain.sim.link_params(link) for link in range(-1, 8)], axis=1)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), plain.reset().cpu().numpy())
    rng = np.random.default_rng(13)
    n_done = 0
    for k in range(1, steps + 1):
        a = torch.from_numpy(rng.uniform(-5, 5, (W, 8)).astype(np.float32)).to(env.device)
        o, r, d, info = env.step(a)
        po, pr, pd, plain_info = plain.step(a)
        assert set(plain_info) == {"terminal_obs"} and set(info) == {"terminal_obs", "inertial", "inertia_draws"}
        n_done += int(d.sum())
        if k % 10 == 0 or k == steps:
            np.testing.assert_array_equal(env.sim.get_state(), plain.sim.get_state(), err_msg=f"state after step {k}")
            for x, y in ((o, po), (r, pr), (d, pd)):
                np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
            np.testing.assert_array_equal(env.inertial.cpu().numpy(), nominal)
    assert n_done == W * (steps // H)
    plain.close()
    sim = env.sim
    with pytest.raises(RuntimeError, match="a floating-base env with inertia randomisation owns"):
        sim.set_link_params(0, nominal[0, 1])
    np.testing.assert_array_equal(sim.link_params(0), nominal[:, 1])
    h, env._h = env._h, None
    N.lib().mw_vecenv_destroy(h)
    words = nominal[:2, 1].copy()
    words[:, 0] *= np.float32(1.5)
    sim.set_link_params(0, words, worlds=[3, 4])
    np.testing.assert_array_equal(sim.link_params(0, [2, 3, 4]), np.vstack([nominal[2:3, 1], words]))
    sim.run()
    env.close()


def test_owner_reads_the_drawn_words_and_errors(require_gpu):
    from mwstep import native as N
    from mwstep.vecenv import VecEnv
    L = N.lib()
    box = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    env = _make("quadruped", 4)
    bad = [N.MwFloatInertiaConfig(0.0, 1.2, 0.0, 0.0, box), N.MwFloatInertiaConfig(1.5, 1.2, 0.0, 0.0, box),
           N.MwFloatInertiaConfig(-0.5, 1.2, 0.0, 0.0, box), N.MwFloatInertiaConfig(0.0, 0.0, 2.0, 1.0, box),
           N.MwFloatInertiaConfig(0.0, 0.0, -1.0, 1.0, box), N.MwFloatInertiaConfig(0.8, float("nan"), 0.0, 0.0, box),
           N.MwFloatInertiaConfig(0.8, 1.2, 0.0, 1.0, (ctypes.c_float * 3)(0.1, -0.1, 0.1))]
    for cfg in bad:
        assert L.mw_floatenv_inertia(env._h, ctypes.byref(cfg), None, None) == N.MW_EINVAL
    # the refused calls left the env without the feature: the simulator's setter works
    env.sim.set_link_params(0, env.sim.link_params(0))
    good = N.MwFloatInertiaConfig(0.8, 1.2, 0.0, 5.0, box)
    env.reset()
    assert L.mw_floatenv_inertia(env._h, ctypes.byref(good), None, None) == N.MW_ESTATE
    assert "before the first mw_vecenv_reset" in N.last_error()
    env.close()
    cart = VecEnv("CartPoleDiscreteBalancing", n_worlds=4)
    assert L.mw_floatenv_inertia(cart._h, ctypes.byref(good), None, None) == N.MW_ESTATE
    assert "mw_floatenv_create" in N.last_error()
    cart.close()
    with pytest.raises(RuntimeError, match="0 < mass_scale_lo <= mass_scale_hi"):
        _make("quadruped", 4, mass_scale_range=(1.5, 1.2))
    # null output buffers are allowed; payload alone leaves the legs nominal and the getter reads the draw
    env = _make("quadruped", 4)
    nominal = np.stack([env.sim.link_params(link) for link in range(-1, 8)], axis=1)
    only_payload = N.MwFloatInertiaConfig(0.0, 0.0, 1.0, 5.0, box)
    assert L.mw_floatenv_inertia(env._h, ctypes.byref(only_payload), None, None) == N.MW_OK
    env.reset()
    got = np.stack([env.sim.link_params(link) for link in range(-1, 8)], axis=1)
    np.testing.assert_array_equal(got[:, 1:], nominal[:, 1:])
    added = got[:, 0, 0] - nominal[:, 0, 0]
    assert (added >= 1.0 - 1e-5).all() and (added <= 5.0 + 1e-5).all() and len(set(added.tolist())) == 4
    env.close()


def test_graph_capture_with_inertia(require_gpu):
    """One captured step with the draws on: 20 replays with resets inside are 20 eager steps."""
    import torch
    W, K = 70, 20
    kw = dict(joint_noise=0.05, seed=4, max_episode_steps=6, friction_range=(0.3, 1.2), **FREE, **PUSH, **INERTIA)
    rng = np.random.default_rng(8)
    acts = (np.float32(STAND) + rng.uniform(-0.2, 0.2, (K + 1, W, 8))).astype(np.float32)
    plain = _make("quadruped", W, **kw)
    plain.reset()
    plain.step(torch.from_numpy(acts[0]).to(plain.device))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        env = _make("quadruped", W, **kw)
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
            np.testing.assert_array_equal(env.obs.cpu().numpy(), plain.obs.cpu().numpy())
            np.testing.assert_array_equal(env.inertial.cpu().numpy(), plain.inertial.cpu().numpy())
            n_done += int(env.done.sum())
        types, _ = _captured_step_graph(env, a)
        side.synchronize()
    assert types == [0, 0, 0], types                 # the step stays three kernel nodes
    assert n_done == 3 * W                           # steps 6, 12, 18 of 21 end an episode
    env.close()
    plain.close()
