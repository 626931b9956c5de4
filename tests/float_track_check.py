"""What the GPU tests of the motion-clip tracking task (test_gpu_float_track.py,
test_gpu_float_track_big.py) share: synthetic clips, and a lockstep checker
that follows every world's clip, start frame and step count on the host and
holds each step's errors, terms, reward, done flag and observation words to the
fp64 restatement (float_track_ref.py, with its bounds) and to the host build of
the kernel's own arithmetic (tests/host_float_track/harness.cpp), bit for bit
where no expf, sinf or cosf is involved.  A plain module: no tests, no
fixtures."""

import ctypes

import numpy as np

import float_track_ref as R


def synthetic_clip(home_base, home_q, frames, loop, rng, step=(0.02, 0.01), amp=0.15):
    """`frames` rows [13 + 2 n] around the home posture: sinusoidal joint offsets,
    a base that moves on, sways in height and yaws a little.  A looping clip's
    last row is its first pose again, moved on by the base's displacement."""
    n = len(home_q)
    period = frames - 1
    rows = np.zeros((frames, 13 + 2 * n), np.float64)
    phase = rng.uniform(0, 2 * np.pi, n)
    for k in range(frames):
        s = 2 * np.pi * k / period
        yaw = 0.2 * np.sin(s)
        rows[k, :3] = [home_base[0] + step[0] * k, home_base[1] + step[1] * k, home_base[2] + 0.01 * np.sin(s)]
        rows[k, 3:7] = [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]
        rows[k, 7:13] = [step[0], step[1], 0.01 * np.cos(s), 0.0, 0.0, 0.2 * np.cos(s)]
        rows[k, 13:13 + n] = np.asarray(home_q) + amp * np.sin(s + phase)
        rows[k, 13 + n:] = amp * np.cos(s + phase)
    if not loop:
        rows[-1, 13:13 + n] += 0.05                   # no need to close
    rows[frames // 2, 3:7] *= -1.0                     # the same rotation with the other sign: the nlerp must flip it
    return rows.astype(np.float32)


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


class TrackCheck:
    def __init__(self, env, oracle, ftk, clips, seed, num, den, weights, scales, bounds=(0.0, 0.0, 0.0), rsi_prob=1.0,
                 wj=None, world_offset=0, max_steps=0, alive_bonus=1.0, worlds=None):
        self.env, self.oracle, self.ftk, self.clips, self.seed = env, oracle, ftk, clips, seed
        self.n = env.action_dim
        self.NS = 13 + 2 * self.n
        self.table = env.clip_table
        self.num, self.den, self.prob, self.offset = num, den, rsi_prob, world_offset
        self.w32 = np.float32([weights[k] for k in R.TERMS])
        self.s32 = np.float32([scales[k] for k in R.TERMS])
        self.ang = np.float32(scales["ang_scale"])
        self.bounds = np.float32(bounds)
        self.wj = np.ones(self.n, np.float32) if wj is None else np.float32(wj)
        self.max_steps, self.alive = max_steps, alive_bonus
        W = env.n_worlds
        self.worlds = list(range(W)) if worlds is None else list(worlds)
        self.episode = np.zeros(W, np.int64)
        self.t = np.zeros(W, np.int64)
        self.clip = np.zeros(W, np.int64)
        self.f0 = np.zeros(W, np.int64)
        self.worst = dict(errors=0.0, terms=0.0, reward=0.0, phase=0.0, reference=0.0)
        self.seen = dict(wraps=0, clip_end=0, failed=0, time_limit=0, steps=0, flips=0)
        self.bit_mismatch = np.zeros(5, np.int64)
        self.return_sums = np.zeros(W)               # fp64 sum of the current episode's rewards / tracking terms
        self.term_sums = np.zeros(W)
        self.last_return = np.zeros(W)               # ... of every world's last finished episode
        self.last_terms = np.zeros(W)

    # -- the float32 reference row as the device forms it, through the host build of the same functions --
    def _lerp32(self, p0, p1, a):
        out = np.zeros(len(p0), np.float32)
        self.ftk.ftk_lerp(len(p0), _p(np.ascontiguousarray(p0)), _p(np.ascontiguousarray(p1)),
                          _p(np.full(len(p0), a, np.float32)), _p(out))
        return out

    def _reference32(self, entry, ck):
        first, length, _ = entry
        i, i1, a, wraps, _ = ck
        a32 = np.float32(a.numerator) / np.float32(a.denominator)
        p0, p1 = self.clips[first + i], self.clips[first + i1]
        ref = self._lerp32(p0, p1, a32)
        if wraps:
            out = np.zeros(2, np.float32)
            self.ftk.ftk_wrapped(2, _p(ref[:2].copy()), _p(np.full(2, wraps, np.uint32)),
                                 _p(self.clips[first + length - 1, :2].copy()), _p(self.clips[first, :2].copy()), _p(out))
            ref[:2] = out
        qr = np.zeros(4, np.float32)
        self.ftk.ftk_nlerp(1, _p(p0[3:7].copy()), _p(p1[3:7].copy()), _p(np.float32([a32])), _p(qr))
        if float(p0[3:7].astype(np.float64) @ p1[3:7]) < 0:
            self.seen["flips"] += 1
        return ref, qr

    def _obs_words(self, w, row, entry, t, what):
        """The tracking block of a row of obs of world w whose episode has taken t steps."""
        sl = self.env.obs_slices
        c, f0 = int(self.clip[w]), int(self.f0[w])
        length = entry[1]
        i, _, a, _, _ = R.clock(f0, t, self.num, self.den, length, bool(entry[2]))
        s, co = R.phase_words(i, float(a), length)
        err = max(abs(float(row[sl["phase"]][0]) - s), abs(float(row[sl["phase"]][1]) - co))
        self.worst["phase"] = max(self.worst["phase"], err / R.PHASE_TOL)
        assert err <= R.PHASE_TOL, (what, w, t, err)
        assert row[sl["clip"]][0] == c, (what, w)
        if "reference" in sl:
            nxt = R.clock(f0, t + 1, self.num, self.den, length, bool(entry[2]))
            first = entry[0]
            a32 = np.float32(nxt[2].numerator) / np.float32(nxt[2].denominator)
            q = slice(13, 13 + self.n)
            want = self._lerp32(self.clips[first + nxt[0], q], self.clips[first + nxt[1], q], a32)
            np.testing.assert_array_equal(row[sl["reference"]].view(np.uint32), want.view(np.uint32),
                                          err_msg=f"{what}: reference words of world {w} at t = {t}")
            ref = R.reference_row(self.clips, entry, nxt)[q]
            tol = R.reference_tol(self.clips, entry, nxt)[q]
            self.worst["reference"] = max(self.worst["reference"], float((np.abs(row[sl["reference"]] - ref) / tol).max()))

    def _draw(self, w):
        c, f0 = R.draw_ref(self.oracle, self.seed, self.offset + w, int(self.episode[w]), self.table, self.prob)
        self.clip[w], self.f0[w], self.t[w] = c, f0, 0

    def start(self, obs, exact_state=True):
        """After env.reset(): every world's draw, start state and reset row."""
        env = self.env
        clip, frame, state = env.track_clip.cpu().numpy(), env.track_frame.cpu().numpy(), env.init_state.cpu().numpy()
        for w in range(env.n_worlds):
            self._draw(w)
        np.testing.assert_array_equal(clip, self.clip)
        np.testing.assert_array_equal(frame, self.f0)
        for w in self.worlds:
            self._reset_row(w, obs[w], state[w], exact_state, "reset")

    def _reset_row(self, w, row, state, exact_state, what):
        entry = self.table[int(self.clip[w])]
        if exact_state:
            want = self.clips[entry[0] + int(self.f0[w])]
            np.testing.assert_array_equal(state.view(np.uint32), want.view(np.uint32), err_msg=f"{what}: world {w}")
        self._obs_words(w, row, entry, 0, what)

    def step(self, obs, reward, done, info, exact_state=True, check_reward=True, clean=None, clean_term=None):
        """After env.step(): all arguments numpy; clean / clean_term: the rows before the noise, where there is any."""
        env, n, NS = self.env, self.n, self.NS
        term_obs = info["terminal_obs"].cpu().numpy() if clean_term is None else clean_term
        now = obs if clean is None else clean
        rows = np.where(done[:, None], term_obs, now)
        errs, terms = env.tracking_errors.cpu().numpy(), env.tracking_terms.cpu().numpy()
        clip, frame, state = env.track_clip.cpu().numpy(), env.track_frame.cpu().numpy(), env.init_state.cpu().numpy()
        self.t += 1
        self.seen["steps"] += 1
        self.return_sums += reward
        self.term_sums += terms.sum(axis=1)
        for w in range(env.n_worlds):
            entry = self.table[int(self.clip[w])]
            ck = R.clock(int(self.f0[w]), int(self.t[w]), self.num, self.den, entry[1], bool(entry[2]))
            limit = self.max_steps > 0 and self.t[w] >= self.max_steps
            if w in self.worlds:
                row = rows[w]
                ref64, tol64 = R.reference_row(self.clips, entry, ck), R.reference_tol(self.clips, entry, ck)
                e64 = R.errors(row[:NS], ref64, self.wj, n, self.ang)
                e_tol = R.errors_tol(e64, n) + R.errors_input_tol(row[:NS], ref64, tol64, self.wj, n, self.ang) + 1e-300
                self.worst["errors"] = max(self.worst["errors"], float((np.abs(errs[w] - e64) / e_tol).max()))
                assert (np.abs(errs[w] - e64) <= e_tol).all(), (w, int(self.t[w]), errs[w], e64, e_tol)
                # ... and the same bits as the host build of the kernel's arithmetic
                ref32, qr = self._reference32(entry, ck)
                e32 = np.zeros(5, np.float32)
                self.ftk.ftk_errors(1, n, _p(np.ascontiguousarray(row[:NS])), _p(ref32), _p(qr), _p(self.wj), self.ang,
                                    _p(e32))
                self.bit_mismatch += errs[w].view(np.uint32) != e32.view(np.uint32)
                t64 = R.terms(self.w32, self.s32, e64)
                t_tol = R.terms_tol(self.w32, self.s32, e_tol)
                ok = t_tol > 0
                self.worst["terms"] = max(self.worst["terms"], float((np.abs(terms[w] - t64)[ok] / t_tol[ok]).max()))
                assert (np.abs(terms[w] - t64) <= t_tol).all(), (w, terms[w], t64)
                assert (terms[w][~ok] == 0).all()
                failed = any(self.bounds[k] > 0 and errs[w][j] > self.bounds[k] for k, j in enumerate((0, 2, 3)))
                if check_reward:
                    want = (0.0 if failed else self.alive) + t64.sum()
                    r_tol = t_tol.sum() + 8 * R.U * (abs(self.alive) + np.abs(t64).sum())
                    self.worst["reward"] = max(self.worst["reward"], abs(float(reward[w]) - want) / r_tol)
                    assert abs(float(reward[w]) - want) <= r_tol, (w, float(reward[w]), want)
                    assert bool(done[w]) == bool(failed or ck[4] or limit), (w, int(self.t[w]), failed, ck, limit)
                self.seen["wraps"] += int(ck[3] > 0)
                self.seen["failed"] += int(failed)
                self.seen["clip_end"] += int(ck[4] and not failed)
                self.seen["time_limit"] += int(bool(limit) and not failed and not ck[4])
                self._obs_words(w, row, entry, int(self.t[w]), "step")
            if done[w]:
                self.episode[w] += 1
                self._draw(w)
                self.last_return[w], self.last_terms[w] = self.return_sums[w], self.term_sums[w]
                self.return_sums[w] = self.term_sums[w] = 0.0
                if w in self.worlds:
                    self._reset_row(w, now[w], state[w], exact_state, "auto-reset")
        np.testing.assert_array_equal(clip, self.clip)
        np.testing.assert_array_equal(frame, self.f0)

    def report(self, name):
        print(f"{name}: {self.seen}; worst error / bound {({k: round(v, 3) for k, v in self.worst.items()})}; "
              f"errors differing from the host build's bits {self.bit_mismatch.tolist()}")
