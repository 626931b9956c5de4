// float_env_kernel.hip -- the device layer of the batched env for articulated
// floating-base models on the world-per-wavefront kernel (mw_floatenv_create).
// One env step is three launches on the sim's stream:
//
//   float_env_action_kernel   actions [W, n] -> SimDev::cmd / ptgt [n][W]
//   wave_run_kernel           (kernels.hip, unchanged) one run of every world
//   float_env_post_kernel     obs / reward / done, and for the done worlds the
//                             pending resets the next run's first launch applies
//
// With randomisation on (mw_floatenv_randomize) the launches stay these three:
// the post launch's PUSH instance reports the push the run applied and writes
// the next step's into the run kernel's wrench array, its RAND instance draws
// the friction of every episode it starts into the simulator's per-world
// array (T.rand.mu), its INERT instance (mw_floatenv_inertia) the link masses
// and the base payload into the simulator's per-world link parameters
// (T.inertia.wpar), its JOINT instance (mw_floatenv_joints) the joints'
// damping, friction and effort limit into the same records.
// The locomotion task (mw_floatenv_locomotion) is the LOCO
// instance of both env kernels: the action launch keeps the raw action and the
// action-rate sum and writes the scaled command, the post launch appends the
// body-frame block of the observation, draws the velocity commands and adds
// the tracking / smoothness / air-time terms to the reward.
// Observation noise and action latency (mw_floatenv_noise) stay inside the
// same launches too.  The post launch adds amp[k] u to word k where it writes
// a row of obs or terminal_obs out of its tile (ft_write_noisy; u from a Philox
// stream keyed by the row's world, episode and step count), a block-uniform
// runtime branch on the amplitude pointer rather than a sixth template flag;
// reward, termination and the locomotion bookkeeping read the clean tile, and
// the clean rows go to two optional buffers.  The action launch's DELAY
// instances keep every world's last actions in a ring and hand the run the one
// of d steps ago, d drawn per episode by the post launch that issues the reset.
// Shaping rewards, contact termination and episode statistics
// (mw_floatenv_shaping) are one more block-uniform runtime branch of the post
// launch (T.shape.on): during the gather every wave sums its share of the dofs
// and links into partials in LDS (shape_gather), wave 0 combines them into the
// ten terms, adds them to the reward, ors the termination links' loaded slots
// into the termination and steps the running episode sums (shape_terms,
// ft_shape_stats); the [W, 10] rows leave through two small LDS tiles as
// contiguous spans.  In torque mode the action launch keeps the command it
// stored in an array of the env, through a nullable argument.
// Initial-state randomisation and the reset-state bank (mw_floatenv_init_state)
// are the third such branch (T.init.on), in the post launch's reset block
// alone: a done world starts from a row of the caller's bank or the home row
// plus drawn offsets (init_reset) where the plain reset writes constants, and
// the first words of the reset rows leave once more as T.init.state_out.
// The motion-clip tracking task (mw_floatenv_tracking) is the fourth
// (T.track.on): one wave works out every world's frame clock, the waves then
// blend the worlds' reference rows out of the caller's clips into one more LDS
// tile -- a wave per row, its lanes across the row's words, so the clip is read
// as contiguous spans -- and wave 0 takes the five errors lane-per-world from
// it (track_clock, track_stage); the reset block starts a done world from a row
// of a drawn clip through init_reset.
//
// Both kernels are transposes between the row-major [W, k] tensors of the
// agent and the [k][W] SoA arrays of the simulator.  A block of 256 threads
// owns a tile of 64 worlds and stages it through LDS, so the row side moves
// as contiguous spans and the SoA side with the world index across the lanes:
// both global sides are coalesced.  Rows in LDS are `k | 1` words apart: a
// lane-per-world access then strides an odd number of banks (conflict-free
// for ds_read_b32 / ds_write_b32, whose banks are word address mod 32 within
// each 32-lane half).
#include <hip/hip_runtime.h>

#include <array>
#include <mutex>
#include <utility>

#include "finite.hpp"
#include "float_task.hpp"
#include "kernels.hpp"
#include "rng.hpp"

namespace mw {
namespace dev {

constexpr int kEnvTile = 64;      // worlds per block (lane = world)
constexpr int kEnvThreads = 256;  // 4 waves share the tile's columns / rows
constexpr int kEnvWaves = kEnvThreads / 64;
static_assert(kEnvWaves == kShapeLanes, "a wave of the post kernel owns one partial of the shaping sums");
constexpr int kShapePitch = kShapeTerms | 1;  // rows of the [kEnvTile][10] tiles in LDS
// dynamic LDS of the post kernel's shaping branch: partial sums, two term tiles, hits
constexpr size_t kShapeLds = (kEnvWaves * kShapeSums * kEnvTile + 2 * kEnvTile * kShapePitch) * sizeof(float) +
                             kEnvWaves * kEnvTile;

// dynamic LDS of the post kernel's tracking branch, behind the shaping region
// where there is one: the reference tile [kEnvTile][track_pitch(n)] -- a row is
// the 13 + 2 n blended words, with q0 unblended in the quaternion's place, and
// q1 in four more words, for the nlerp a lane takes per world -- the two
// [kEnvTile][5] tiles of terms_out / errors_out (5 is odd already) and
// kTrackClockWords arrays of one word per world: the clocks.
constexpr int kTrackClockWords = 10;
enum TrackClockWord : int {
    kTcRow0 = 0,  // rows of the caller's buffer the reference of the step's instant x_t lies between
    kTcRow1,
    kTcBlend,     // (float) its blend
    kTcWraps,     // periods of a looping clip gone by
    kTcFirst,     // the clip's first and last row: the displacement of a period
    kTcLast,
    kTcNext0,     // likewise for x_{t+1}, the reference joint positions of the observation
    kTcNext1,
    kTcNextBlend,
    kTcEnded,     // the clip ended: the episode is truncated
};
__host__ __device__ constexpr int track_pitch(int n) { return (13 + 2 * n + 4) | 1; }
__host__ __device__ constexpr size_t track_lds(int n) {
    return (static_cast<size_t>(kEnvTile) * track_pitch(n) + 2 * kEnvTile * kTrackTerms + kTrackClockWords * kEnvTile) *
           sizeof(float);
}

// actions [W, n] -> out [n][W] (SimDev::cmd or ptgt), and sum_i a_i^2 per
// world for the reward (asq [W]).  The value stored is the float32 the host
// setters would upload for that number; the effort limit stays with the run
// kernel's clamp, as on the host-commanded path.  That clamp (a min / max
// pair) turns a NaN torque into -effort without a trace, and the PID drops a
// NaN target: a world whose action holds a non-finite value is therefore
// flagged diverged here (sticky flag + count, as the run kernels flag a
// non-finite state), so that the post kernel ends and resets it.
// LOCO (the locomotion task): the raw action of every world is kept row-major
// in A.prev [W][n] -- the same contiguous span as the input, read and written
// by the thread that stages the word -- after sum_d (a_t - a_{t-1})^2 went to
// A.rate [W] through a second tile of the differences (a reset zeroes the kept
// row, so a_{t-1} = 0 on an episode's first step).  With A.scale > 0 the value
// stored is home_q[d] + scale a_d (position mode, one fused multiply-add) or
// scale a_d (torque mode); sum a^2 and the non-finite test stay on the raw action.
template <bool LOCO>
struct ActLocoArgs {};
template <>
struct ActLocoArgs<true> {
    float scale;
    int32_t position;
    float* prev;
    float* rate;
    float home_q[kMaxBodies];
};

// DELAY (the action latency of mw_floatenv_noise): every world keeps its last
// R = delay_hi + 1 raw actions in L.ring [W][R][n], each row a contiguous span
// of n words.  With t = L.steps[w] steps taken and d = L.delay[w] (the
// episode's delay, left by the post launch that issued its reset), the thread
// that stages word i of the tile stores it in the world's slot t % R and puts
// the same word of slot (t - d) % R -- the action of step t - d, written by an
// earlier launch where d > 0 -- into one more LDS tile, which the scaling and
// the store to `out` then read instead of the raw one (the slots and what is
// applied are worked out once per world into LDS first, and the stores to the
// ring are a loop of their own behind the loads).  While t < d nothing is
// read and the world receives the neutral command, home_q[j] in position mode
// and 0 in torque mode (what action_scale * 0 gives): no slot an earlier
// episode wrote is ever applied, so a reset leaves the ring alone.  sum a^2,
// the action-rate term, A.prev and the non-finite test stay on the raw tile.
template <bool DELAY>
struct ActDelayArgs {};
template <>
struct ActDelayArgs<true> {
    const uint32_t* steps;
    const int32_t* delay;
    float* ring;
    uint32_t R;
    int32_t position;
    float home_q[kMaxBodies];
};

// kept_cmd (mw_floatenv_shaping in torque mode, else null): the value stored
// to `out` goes to this [n][W] array of the env as well -- the run zeroes
// SimDev::cmd at its end, and the post launch's torque and power terms need
// the command the run clamped.  A nullable argument, not another instance.
template <bool LOCO, bool DELAY>
__global__ void __launch_bounds__(kEnvThreads) float_env_action_kernel(const float* __restrict__ actions,
                                                                       float* __restrict__ out,
                                                                       float* __restrict__ asq,
                                                                       uint8_t* __restrict__ div,
                                                                       unsigned long long* __restrict__ ndiv, int n,
                                                                       int W, ActLocoArgs<LOCO> A, ActDelayArgs<DELAY> L,
                                                                       float* __restrict__ kept_cmd) {
    // [kEnvTile][n | 1]; LOCO: then [kEnvTile][n | 1] of a_t - a_{t-1}; DELAY: then [kEnvTile][n | 1] of a_{t-d}
    extern __shared__ float tile[];
    const int pitch = n | 1;
    const int w0 = blockIdx.x * kEnvTile;
    const int rows = min(kEnvTile, W - w0);
    const float* __restrict__ src = actions + static_cast<size_t>(w0) * n;
    constexpr int kApplied = (LOCO ? 2 : 1) * kEnvTile;  // first row of the DELAY tile
    // DELAY, per world of the tile: the ring row the step's action goes to, the
    // row it applies, and what is applied -- 0 the action itself (d = 0), 1 the
    // neutral command (t < d), 2 the ring's row
    __shared__ uint32_t s_store[DELAY ? kEnvTile : 1];
    __shared__ uint32_t s_read[DELAY ? kEnvTile : 1];
    __shared__ uint8_t s_mode[DELAY ? kEnvTile : 1];
    if constexpr (DELAY) {
        if (static_cast<int>(threadIdx.x) < rows) {
            const uint32_t t = L.steps[w0 + threadIdx.x], dl = static_cast<uint32_t>(L.delay[w0 + threadIdx.x]);
            const bool kept = dl && !ft_delay_neutral(t, dl);
            s_store[threadIdx.x] = ft_delay_slot(t, 0u, L.R);
            // where no row is applied, one this launch does not write (R >= 2): the
            // staging loop then loads without a branch and drops the value
            s_read[threadIdx.x] = kept ? ft_delay_slot(t, dl, L.R) : ft_delay_slot(t + 1u, 0u, L.R);
            s_mode[threadIdx.x] = dl ? (kept ? 2 : 1) : 0;
        }
        __syncthreads();
    }
    // the tile's rows are one contiguous span of rows * n words
    for (int i = threadIdx.x; i < rows * n; i += kEnvThreads) {
        const int r = i / n, d = i - r * n;
        const float a = src[i];
        tile[r * pitch + d] = a;
        if constexpr (LOCO) {
            float* prev = A.prev + static_cast<size_t>(w0) * n;
            tile[(kEnvTile + r) * pitch + d] = a - prev[i];
            prev[i] = a;
        }
        if constexpr (DELAY) {
            const float kept = L.ring[(static_cast<size_t>(w0 + r) * L.R + s_read[r]) * n + d];
            tile[(kApplied + r) * pitch + d] = s_mode[r] == 2 ? kept : a;
        }
    }
    __syncthreads();
    if constexpr (DELAY) {
        // the step's own action into its ring row, behind every load of the
        // ring: a loop of stores alone, so neither loop waits on the other's memory
        for (int i = threadIdx.x; i < rows * n; i += kEnvThreads) {
            const int r = i / n, d = i - r * n;
            L.ring[(static_cast<size_t>(w0 + r) * L.R + s_store[r]) * n + d] = tile[r * pitch + d];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane >= rows) return;
    const float* row = tile + lane * pitch;
    const float* applied = DELAY ? tile + (kApplied + lane) * pitch : row;
    bool neutral = false;
    if constexpr (DELAY) neutral = s_mode[lane] == 1;
    for (int d = wave; d < n; d += kEnvWaves) {
        float v = applied[d];
        if constexpr (LOCO) {
            if (A.scale > 0.f) v = A.position ? fmaf(A.scale, v, A.home_q[d]) : A.scale * v;
        }
        if constexpr (DELAY) {
            if (neutral) v = L.position ? L.home_q[d] : 0.f;
        }
        out[static_cast<size_t>(d) * W + w0 + lane] = v;
        // the shaping terms' copy of the command (torque mode: the run clears its own), block-uniform
        if (kept_cmd) kept_cmd[static_cast<size_t>(d) * W + w0 + lane] = v;
    }
    if constexpr (LOCO) {
        if (wave == 1) A.rate[w0 + lane] = ft_sum_sq(tile + (kEnvTile + lane) * pitch, n, 1);
    }
    if (wave == 0) {
        asq[w0 + lane] = ft_sum_sq(row, n, 1);
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || nonfinite_bits(row[d]);
        if (bad && !div[w0 + lane]) {
            div[w0 + lane] = 1;
            atomicAdd(ndiv, 1ull);
        }
    }
}

// The rows of the post kernel's tile written out with observation noise
// (T.noise.amp): one thread per Philox block of four words, the (row, block)
// pairs of the tile spread over the whole block, so a thread runs the ten
// rounds a few times where a lane per word would run them once per row.  Word
// k = 4 b + j leaves as clean + amp[k] u, u the noise unit of word j of block
// b of the counter (global world, episode, b, 1 + t) -- a stream of its own:
// every other draw has 0 in the fourth word -- with (episode, t) =
// (s_episode[r] - back, s_t[r]); a word of amplitude zero keeps the clean
// word's bits, and a block of such words draws nothing.  The clean words go to
// `clean` (may be null); the tile stays clean.  only: the rows to write (null =
// every row).
__device__ __forceinline__ void ft_write_noisy(const FloatTaskF& T, const float* tile, int pitch, int rows, int w0,
                                               float* __restrict__ dst, float* __restrict__ clean,
                                               const uint8_t* only, const uint32_t* s_episode, uint32_t back,
                                               const uint32_t* s_t) {
    const int NO = T.n_obs, nb = (NO + 3) >> 2;
    const float* __restrict__ amp = T.noise.amp;
    for (int i = threadIdx.x; i < rows * nb; i += kEnvThreads) {
        const int r = i / nb, b = i - r * nb;
        if (only && !only[r]) continue;
        const float* src = tile + r * pitch + 4 * b;
        const size_t o = static_cast<size_t>(w0 + r) * NO + 4 * b;
        const int m = min(4, NO - 4 * b);
        float v[4], a[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = a[j] = 0.f;
            if (j < m) {
                v[j] = src[j];
                a[j] = amp[4 * b + j];
                if (clean) clean[o + j] = v[j];
                any = any || a[j] != 0.f;
            }
        }
        if (any) {
            uint32_t x[4];
            philox_ctr(T.seed_lo, T.seed_hi, T.world_offset + static_cast<uint32_t>(w0 + r), s_episode[r] - back,
                       static_cast<uint32_t>(b), 1u + s_t[r], x);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (a[j] != 0.f) v[j] = ft_noisy(v[j], a[j], ft_noise_unit(x[j]));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < m) dst[o + j] = v[j];
    }
}

// The shaping gather of one world (mw_floatenv_shaping; lane = world, called by
// every wave of a live lane): wave v takes the dofs, the contact links, the
// penalised links and the active termination slots v, v + 4, ... into its
// partial of the eight sums (float_task.hpp) and its termination hit, both
// left in LDS for wave 0.  Per dof it reads q, qd, the kept qd of the last step
// and -- where a torque is wanted -- the JointController's output (position
// mode) or the kept command, clamped with the effort word the run clamped with;
// it stores qd for the next step and the torque into the caller's row.  That
// store is the one access here that is strided across the lanes (n words
// apart): the tile's 64 rows are one contiguous span which the four waves
// fill between them, and the torque of a done world must be formed here,
// before the resets below redraw the effort limits (JOINT).  The link forces
// are the sums of the active slots' force vectors in slot order, as the
// observation's z force is.
__device__ __forceinline__ void shape_gather(const FloatTaskF& T, const SimDev& S, const FreeDev& D, int n, size_t Ws,
                                             int w, int wave, int lane, float* s_part, uint8_t* s_hit) {
    const FloatShapeF& H = T.shape;
    float ds[kShapeDofSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float col = 0.f, stu = 0.f, exc = 0.f;
    const float* __restrict__ tsrc = T.action_mode ? S.pid_u : H.cmd_kept;  // null: no torque is wanted
    const float* __restrict__ eff = H.effort + static_cast<size_t>(w) * H.effort_stride;
    float* __restrict__ tout = H.torque_out ? H.torque_out + static_cast<size_t>(w) * n : nullptr;
    for (int d = wave; d < n; d += kEnvWaves) {
        const size_t i = d * Ws + w;
        const float q = S.q[i], qd = S.qd[i], prev = H.qd_prev[i];
        float tau = 0.f;
        if (tsrc) tau = ft_shape_tau(tsrc[i], eff[d * kWparBodyWords]);
        if (tout) tout[d] = tau;
        H.qd_prev[i] = qd;
        ft_shape_dof(tau, q, qd, prev, H.env_dt, H.soft_lo[d], H.soft_hi[d], T.home_q[d], ds);
    }
    const uint32_t cm = D.cmask[w];
    auto slot_force = [&](int slot, float (&f)[3]) {
        const size_t c = (static_cast<size_t>(slot) * 7 + 3) * Ws + w;
#pragma unroll
        for (int e = 0; e < 3; ++e) f[e] += D.cdata[c + e * Ws];
    };
    if (H.w[kShStumble] != 0.f || H.w[kShContactForce] != 0.f) {
        for (int j = wave; j < T.n_links; j += kEnvWaves) {
            float f[3] = {0.f, 0.f, 0.f};
            for (uint32_t m = cm & T.link_slots[j]; m; m &= m - 1u) slot_force(__builtin_ctz(m), f);
            ft_shape_contact(H, f[0], f[1], f[2], stu, exc);
        }
    }
    if (H.w[kShCollision] != 0.f) {
        for (int j = wave; j < H.n_pen; j += kEnvWaves) {
            float f[3] = {0.f, 0.f, 0.f};
            for (uint32_t m = cm & H.pen_slots[j]; m; m &= m - 1u) slot_force(__builtin_ctz(m), f);
            col = col + ft_shape_collision(H, f[0], f[1], f[2]);
        }
    }
    bool hit = false;
    int k = 0;
    for (uint32_t m = cm & H.term_slots; m; m &= m - 1u, ++k) {
        if ((k & (kEnvWaves - 1)) != wave) continue;
        float f[3] = {0.f, 0.f, 0.f};
        slot_force(__builtin_ctz(m), f);
        hit = hit || ft_shape_slot_hit(H, f[0], f[1], f[2]);
    }
    float* part = s_part + wave * kShapeSums * kEnvTile + lane;
#pragma unroll
    for (int e = 0; e < kShapeDofSums; ++e) part[e * kEnvTile] = ds[e];
    part[5 * kEnvTile] = col;
    part[6 * kEnvTile] = stu;
    part[7 * kEnvTile] = exc;
    s_hit[wave * kEnvTile + lane] = hit ? 1 : 0;
}

// Wave 0's half: the partials combined in wave order into the ten terms of
// the world.  pose: the row's first seven words; standing: the command the
// step ran under counts as standing still (LOCO only).
__device__ __forceinline__ void shape_terms(const FloatShapeF& H, const float* pose_row, bool standing, bool diverged,
                                            int lane, const float* s_part, float (&term)[kShapeTerms]) {
    float sum[kShapeSums], x[kShapeTerms];
#pragma unroll
    for (int e = 0; e < kShapeSums; ++e) {
        float p[kShapeLanes];
#pragma unroll
        for (int v = 0; v < kShapeLanes; ++v) p[v] = s_part[(v * kShapeSums + e) * kEnvTile + lane];
        sum[e] = ft_shape_combine(p);
    }
    const float pose[7] = {pose_row[0], pose_row[1], pose_row[2], pose_row[3], pose_row[4], pose_row[5], pose_row[6]};
    ft_shape_x(H, sum, pose, standing, x);
    ft_shape_terms(H, x, diverged, term);
}

// The frame clocks of one world of the tracking task (lane = world, one wave):
// from the steps taken before this launch's update and the kept start frame,
// the instant the step's state is compared at (t = steps + 1) and the next one
// (the reference joint positions of the observation), as rows of the caller's
// buffer and blends in LDS for the staging waves; the phase and clip words go
// straight into the world's row of the obs tile.
__device__ __forceinline__ void track_clock(const FloatTrackF& K, uint32_t steps, int w, int lane, float* row,
                                            uint32_t* s_clock) {
    const int32_t c = K.clip[w], f0 = K.f0[w];
    const int32_t* __restrict__ e = K.table + c * kTrackTableWords;
    const int32_t first = e[0], length = e[1];
    const bool loop = e[2] != 0;
    const TrackClock A = ft_track_clock(f0, steps + 1u, K.frame_num, K.frame_den, length, loop);
    const TrackClock B = ft_track_clock(f0, steps + 2u, K.frame_num, K.frame_den, length, loop);
    s_clock[kTcRow0 * kEnvTile + lane] = static_cast<uint32_t>(first + A.i);
    s_clock[kTcRow1 * kEnvTile + lane] = static_cast<uint32_t>(first + A.i1);
    s_clock[kTcBlend * kEnvTile + lane] = __float_as_uint(A.a);
    s_clock[kTcWraps * kEnvTile + lane] = A.wraps;
    s_clock[kTcFirst * kEnvTile + lane] = static_cast<uint32_t>(first);
    s_clock[kTcLast * kEnvTile + lane] = static_cast<uint32_t>(first + length - 1);
    s_clock[kTcNext0 * kEnvTile + lane] = static_cast<uint32_t>(first + B.i);
    s_clock[kTcNext1 * kEnvTile + lane] = static_cast<uint32_t>(first + B.i1);
    s_clock[kTcNextBlend * kEnvTile + lane] = __float_as_uint(B.a);
    s_clock[kTcEnded * kEnvTile + lane] = A.ended ? 1u : 0u;
    float sn, cs;
    ft_track_phase_words(ft_track_phase(A.i, A.a, length), sn, cs);
    row[K.nb] = sn;
    row[K.nb + 1] = cs;
    row[K.nb + 2] = static_cast<float>(c);
}

// The reference rows of the tile's worlds staged into LDS: a wave takes row r
// with its lanes across the row's words, so every load of the clip is a
// contiguous span of one row (two rows per world, and two words of two more
// where a looping clip has wrapped).  The quaternion's words are kept apart
// (track_lds); the n joint positions of x_{t+1} go straight into the obs tile.
__device__ __forceinline__ void track_stage(const FloatTrackF& K, int n, int rows, int wave, int lane, float* s_ref,
                                            const uint32_t* s_clock, float* tile, int pitch) {
    const int NS = 13 + 2 * n, RP = track_pitch(n);
    const float* __restrict__ clips = K.clips;
    for (int r = wave; r < rows; r += kEnvWaves) {
        const float* __restrict__ c0 = clips + static_cast<size_t>(s_clock[kTcRow0 * kEnvTile + r]) * NS;
        const float* __restrict__ c1 = clips + static_cast<size_t>(s_clock[kTcRow1 * kEnvTile + r]) * NS;
        const float a = __uint_as_float(s_clock[kTcBlend * kEnvTile + r]);
        const uint32_t wraps = s_clock[kTcWraps * kEnvTile + r];
        float* ref = s_ref + r * RP;
        for (int k = lane; k < NS; k += 64) {
            const float p0 = c0[k], p1 = c1[k];
            if (k >= 3 && k < 7) {
                ref[k] = p0;
                ref[NS + k - 3] = p1;
                continue;
            }
            float v = ft_track_lerp(p0, p1, a);
            if (k < 2 && wraps) {
                const float* __restrict__ cl = clips + static_cast<size_t>(s_clock[kTcLast * kEnvTile + r]) * NS;
                const float* __restrict__ cf = clips + static_cast<size_t>(s_clock[kTcFirst * kEnvTile + r]) * NS;
                v = ft_track_wrapped(v, wraps, cl[k], cf[k]);
            }
            ref[k] = v;
        }
        if (K.obs_reference) {
            const float* __restrict__ b0 = clips + static_cast<size_t>(s_clock[kTcNext0 * kEnvTile + r]) * NS + 13;
            const float* __restrict__ b1 = clips + static_cast<size_t>(s_clock[kTcNext1 * kEnvTile + r]) * NS + 13;
            const float b = __uint_as_float(s_clock[kTcNextBlend * kEnvTile + r]);
            for (int k = lane; k < n; k += 64) tile[r * pitch + K.nb + 3 + k] = ft_track_lerp(b0[k], b1[k], b);
        }
    }
}

// The reset of one done world with the initial-state randomisation on
// (mw_floatenv_init_state, T.init.on; lane = world, called by every wave of the
// lane): it takes the place of the plain reset's joint loop and base block and
// leaves the same words -- the pending joint and base resets with their flags,
// the divergence flag re-armed, the reset row in the tile -- from a base row
// plus draws (float_task.hpp).  A wave that has work draws the row choice
// itself (one Philox call, only with a bank) rather than wait for another's
// through LDS: the reset block has no barrier.  The joints go in blocks of four
// round the waves as in the plain reset, the same Philox blocks for the
// position noise and one more call per block for the velocity draws; a wave's
// words of the base row are the block's four q and four qd, the gather of one
// row per done lane split over the waves.  The home row is read the same way,
// from a copy in device memory (T.init.home): a choice between a word of the
// bank and a word of T would make the compiler select between their addresses,
// and a by-value argument whose address is taken is copied to scratch, in
// every instance and with the feature off too.  The base -- the row's 13 words, the
// four groups' draws, the composed orientation, in the locomotion task (loco_nb
// >= 0: the first word of the appended block) the projected gravity and the
// body-frame velocities of the drawn state -- is wave kInitBaseWave's, a wave
// the other reset draws load least.  With shaping on the drawn qd is the kept
// qd of the first step's joint_acc term: written here by the wave that drew
// it, behind the barriers that follow the gather's store of the same word.  A
// non-finite q of a bank row stays non-finite (the clip alone would turn a NaN
// into the lower limit): the run flags the world diverged.
// With the tracking task on (T.track.on) the base row is a row of a clip: every
// wave that has work draws the clip and the start frame from the tracking block
// as it would draw the bank row, and the base wave writes the phase and clip
// words of x_0 and keeps the world's clip and start frame for the clocks of the
// steps to come.  The reference joint positions of x_1 follow in a pass of
// their own (track_reset_reference), which draws once more instead of keeping
// the rows' addresses live across this function.
constexpr int kInitBaseWave = 2;
__device__ __forceinline__ void init_reset(const ChainF* __restrict__ P, const FloatTaskF& T, const SimDev& S,
                                           const FreeDev& D, int n, size_t Ws, int w, int wave, uint32_t episode,
                                           bool shaped, int loco_nb, float* row) {
    const FloatInitF& I = T.init;
    const uint32_t g = T.world_offset + static_cast<uint32_t>(w);
    const int NS = 13 + 2 * n, nblocks = (n + 3) / 4;
    const bool base_wave = wave == kInitBaseWave;
    if (!base_wave && wave >= nblocks) return;
    int32_t k_row = -1;
    if (I.n_states > 0) {
        uint32_t r[4];
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtInitRowBlock);
        k_row = ft_init_row(r[0], r[1], I.n_states, I.state_prob);
    }
    // one pointer for either kind of start: the home row is a row in device memory too (the env's own)
    const float* __restrict__ base_row = k_row >= 0 ? I.states + static_cast<size_t>(k_row) * NS : I.home;
    const FloatTrackF& K = T.track;
    const bool tracked = K.on != 0u;
    int32_t clip = 0, f0 = 0;
    if (tracked) {
        uint32_t r[4];
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtTrackBlock);
        clip = ft_track_clip(r[0], K.n_clips);
        const int32_t* __restrict__ e = K.table + clip * kTrackTableWords;
        f0 = ft_track_start(r[1], r[2], e[1], K.rsi_prob);
        base_row = K.clips + static_cast<size_t>(e[0] + f0) * NS;
    }
    float* __restrict__ draws = I.draws_out ? I.draws_out + static_cast<size_t>(w) * (kInitBaseDraws + n) : nullptr;
    const bool jv = I.joint_vel > 0.f;
    for (int b = wave; b < nblocks; b += kEnvWaves) {
        uint32_t r[4], rv[4] = {0u, 0u, 0u, 0u};
        philox(T.seed_lo, T.seed_hi, g, episode, r, static_cast<uint32_t>(b));
        if (jv) philox(T.seed_lo, T.seed_hi, g, episode, rv, ft_init_qd_block(4 * b));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = 4 * b + k;
            if (d < n) {
                const float q0 = base_row[13 + d], qd0 = base_row[13 + n + d];
                const float x = q0 + unif(r[k], -T.joint_noise, T.joint_noise);
                const float clipped = fminf(fmaxf(x, P->b[d].lower), P->b[d].upper);
                const float q = nonfinite_bits(x) ? x : clipped;  // by the bits: the build assumes finite math
                const float dv = jv ? ft_unif(rv[k], -I.joint_vel, I.joint_vel) : 0.f;
                const float qd = jv ? ft_init_sum(qd0, dv) : qd0;
                const size_t i = d * Ws + w;
                S.rq[i] = q;
                S.rqd[i] = qd;
                S.rflag[i] = 1u | 2u | 4u;  // position, velocity, PID reset
                row[13 + d] = q;
                row[13 + n + d] = qd;
                if (shaped) T.shape.qd_prev[i] = qd;
                if (draws) draws[kInitBaseDraws + d] = dv;
            }
        }
    }
    if (!base_wave) return;
    float rowb[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) rowb[k] = base_row[k];
    float off[4][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    uint32_t r[4];
    if (I.groups & kInitPos) {
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtInitPosBlock);
        ft_init_offsets(r, I.pos_lo, I.pos_hi, off[0]);
    }
    if (I.groups & kInitRpy) {
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtInitRpyBlock);
        ft_init_offsets(r, I.rpy_lo, I.rpy_hi, off[1]);
    }
    if (I.groups & kInitLin) {
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtInitLinBlock);
        ft_init_offsets(r, I.lin_lo, I.lin_hi, off[2]);
    }
    if (I.groups & kInitAng) {
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtInitAngBlock);
        ft_init_offsets(r, I.ang_lo, I.ang_hi, off[3]);
    }
    float base[13], qn[4];
    ft_init_base(I, rowb, off[0], off[1], off[2], off[3], base, qn);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        D.rpose[k * Ws + w] = base[k];
        row[k] = base[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        D.rvel[k * Ws + w] = base[7 + k];
        row[7 + k] = base[7 + k];
    }
    D.rflag[w] = 1u | 2u;
    S.div[w] = 0;  // a reset re-arms the divergence flag (mw_reset_* do)
    if (loco_nb >= 0) {
        const float lin[3] = {base[7], base[8], base[9]}, ang[3] = {base[10], base[11], base[12]};
        float gr[3], v[3], om[3];
        ft_projected_gravity(qn[0], qn[1], qn[2], qn[3], gr);
        ft_init_body_frame(qn, lin, v);
        ft_init_body_frame(qn, ang, om);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            row[loco_nb + k] = gr[k];
            row[loco_nb + 3 + k] = v[k];
            row[loco_nb + 6 + k] = om[k];
        }
    }
    if (draws) {
#pragma unroll
        for (int k = 0; k < 12; ++k) draws[k] = off[k / 3][k % 3];
        draws[12] = static_cast<float>(k_row);
    }
    if (tracked) {
        float sn, cs;
        ft_track_phase_words(ft_track_phase(f0, 0.f, K.table[clip * kTrackTableWords + 1]), sn, cs);
        row[K.nb] = sn;
        row[K.nb + 1] = cs;
        row[K.nb + 2] = static_cast<float>(clip);
        K.clip[w] = clip;
        K.f0[w] = f0;
        if (K.clip_out) K.clip_out[w] = clip;
        if (K.frame_out) K.frame_out[w] = f0;
    }
}

// The reference joint positions of x_1 in the reset row of one done world
// (obs_reference; lane = world, the joints round the waves): the gather of two
// rows' joint words per done lane, as init_reset's of the base row.
__device__ __forceinline__ void track_reset_reference(const FloatTaskF& T, int n, int w, int wave, uint32_t episode,
                                                      float* row) {
    const FloatTrackF& K = T.track;
    if (wave >= n) return;
    uint32_t r[4];
    philox(T.seed_lo, T.seed_hi, T.world_offset + static_cast<uint32_t>(w), episode, r, kFtTrackBlock);
    const int32_t* __restrict__ e = K.table + ft_track_clip(r[0], K.n_clips) * kTrackTableWords;
    const int32_t first = e[0], length = e[1];
    const TrackClock B = ft_track_clock(ft_track_start(r[1], r[2], length, K.rsi_prob), 1u, K.frame_num, K.frame_den,
                                        length, e[2] != 0);
    const int NS = 13 + 2 * n;
    const float* __restrict__ b0 = K.clips + static_cast<size_t>(first + B.i) * NS + 13;
    const float* __restrict__ b1 = K.clips + static_cast<size_t>(first + B.i1) * NS + 13;
    for (int d = wave; d < n; d += kEnvWaves) row[K.nb + 3 + d] = ft_track_lerp(b0[d], b1[d], B.a);
}

// Per world: gather the observation, reward, done, counters; where done, the
// terminal observation, the reset sample written as pending resets (exactly
// the bits and values mw_reset_joint_positions + mw_reset_joint_velocities +
// mw_reset_base_pose + mw_reset_base_velocity leave on the device), the
// divergence flag re-armed, and the reset state's observation.  reset_all:
// every world starts episode 0 (mw_vecenv_reset), only obs is written.
// RAND (friction randomisation, T.rand.friction_hi > 0): a reset also draws
// the friction coefficient of the episode it starts, U(friction_lo,
// friction_hi) from the episode block, into T.rand.mu -- the next run reads
// it together with the pending reset -- and T.rand.friction_out.
// PUSH (T.rand.push_interval > 0): node 0 of the run kernel's wrench array
// [6][wnodes][W] holds the world wrench on the base that the run before this
// launch applied; it goes to T.rand.push_out [W, 6], and the wrench of the
// world's next step takes its place -- zeros where no push is active; the
// other nodes stay zero from allocation.  The schedule is a pure function of
// (seed, global world, episode, steps taken), all known here once the counters
// are updated: the episode's phase from its episode block, push k's (fx, fy,
// tz) from block kFtPushBlock | k (float_task.hpp).
// LOCO (T.loco.on): the row grows by 12 + n words behind the NB = 13 + 2 n +
// n_links of the plain env -- projected gravity, body-frame linear and angular
// velocity (wave 0, from the base words it holds), the command in force for
// the next step (wave 3) and the raw action the step applied (every thread,
// the kept rows of the action launch as one contiguous span).  Wave 3 draws
// the command the step ran under (steps taken t, for the reward) and the one
// of t + 1 (for obs and terminal_obs) during the gather, before the counters
// move, and the new episode's command 0 with the resets; the waves that sum a
// link's contact force also step its air-time counter and leave the touchdown
// payment in LDS for wave 0's reward.  A reset zeroes the kept action row and
// the air counters.
// INERT (mw_floatenv_inertia, T.inertia): a reset also draws the inertial
// words of the episode it starts -- link k (0 = the base, 1 + i = body i)
// scaled by U(mass_lo, mass_hi) from word k % 4 of block kFtScaleBlock | k / 4,
// then the payload of block kFtPayloadBlock added to the base
// (float_task.hpp; a feature that is off is skipped) -- from the nominal words
// (P, the shared ChainF; T.inertia.base0) into the world's record of the run
// kernel's per-world link parameters (T.inertia.wpar: the base's ten words,
// each BodyF's ten from kBodyInertial on), T.inertia.inertial_out and, the draws
// themselves, T.inertia.draw_out; the next run reads the record together with
// the pending reset.  The blocks of four links go round the
// waves starting at wave 1, so wave 0's chain takes one only from the 13th
// link on.
// JOINT (mw_floatenv_joints, T.joints): a reset also draws the joint dynamics
// of the episode it starts -- joint d of T.joints.dof_mask takes a, f, s from
// words 0..2 of block kFtJointBlock | d, damping = damping0 + a, friction =
// friction0 + f, effort = s effort0 (ft_joint_words; the nominal words from P,
// the shared ChainF) -- into those three words of the joint's BodyF in the
// same record (kBodyJointWord): one Philox call and three stores per joint.  A feature that is
// off draws nothing and a joint outside the mask leaves its record alone; both
// report the nominal words and the draws 0, 0, 1 (T.joints.joints_out,
// draw_out).  The joints go round the waves starting at wave 1.
// Tracking (mw_floatenv_tracking, T.track.on; block-uniform like shaping): the
// row grows by 3 words behind everything else -- sin and cos of the phase and
// the clip, written by wave 1 with the clocks -- and, with obs_reference, n
// reference joint positions.  Wave 1 works out the clocks before the counters
// move, a barrier of this branch alone hands them to the staging (track_stage),
// and behind the gather's barrier wave 0 takes the errors from the reference
// tile, ors the early termination into the termination and the clip's end into
// done, and adds the five terms to the reward ahead of the shaping terms, so
// that the episode return of the shaping statistics includes them.
template <bool RAND, bool PUSH, bool LOCO, bool INERT, bool JOINT>
__global__ void __launch_bounds__(kEnvThreads) float_env_post_kernel(const ChainF* __restrict__ P, FloatTaskF T,
                                                                     SimDev S, FreeDev D, VecDev V,
                                                                     const float* __restrict__ asq,
                                                                     float* __restrict__ obs,
                                                                     float* __restrict__ reward,
                                                                     uint8_t* __restrict__ done_out,
                                                                     float* __restrict__ term_obs, int n, int W,
                                                                     int reset_all) {
    extern __shared__ float tile[];  // [kEnvTile][n_obs | 1]: the observation rows
    __shared__ uint8_t s_done[kEnvTile];
    __shared__ uint32_t s_episode[kEnvTile];
    __shared__ uint32_t s_steps[kEnvTile];  // PUSH, noise: steps taken in the episode the next step belongs to
    __shared__ uint32_t s_last[kEnvTile];   // noise: the step count a finished episode ended with
    __shared__ float s_cmd[LOCO ? 3 * kEnvTile : 1];                 // the command the step ran under
    __shared__ float s_pay[LOCO ? kMaxContactLinks * kEnvTile : 1];  // touchdown payment per link
    const int NO = T.n_obs, pitch = NO | 1;
    // shaping (block-uniform; the launcher adds kShapeLds bytes behind the tile
    // only then, so an env without it keeps its LDS footprint): every wave's
    // partial sums [wave][sum][lane] (the dof sums, then the link sums), the
    // [kEnvTile][10 | 1] tiles of terms_out / ep_terms and the waves'
    // termination hits
    const bool shaped = __builtin_expect(T.shape.on != 0u, 0);
    float* const s_part = tile + kEnvTile * pitch;
    float* const s_terms = s_part + kEnvWaves * kShapeSums * kEnvTile;
    float* const s_epterms = s_terms + kEnvTile * kShapePitch;
    uint8_t* const s_hit = reinterpret_cast<uint8_t*>(s_epterms + kEnvTile * kShapePitch);
    // tracking (block-uniform; the launcher adds track_lds(n) bytes behind the
    // shaping region, or behind the tile without one, only then)
    const bool tracked = __builtin_expect(T.track.on != 0u, 0);
    float* const s_ref = s_part + (shaped ? kShapeLds / sizeof(float) : 0);
    float* const s_tterms = s_ref + kEnvTile * track_pitch(n);
    float* const s_terrs = s_tterms + kEnvTile * kTrackTerms;
    uint32_t* const s_clock = reinterpret_cast<uint32_t*>(s_terrs + kEnvTile * kTrackTerms);
    const int NB = 13 + 2 * n + T.n_links;  // LOCO: the appended block starts here
    const int w0 = blockIdx.x * kEnvTile;
    const int rows = min(kEnvTile, W - w0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = w0 + lane;
    const bool live = lane < rows;
    const bool noisy = T.noise.amp != nullptr;  // block-uniform
    const bool starts = __builtin_expect(T.init.on != 0u, 0);  // block-uniform: the reset state is drawn (init_reset)
    float* row = tile + lane * pitch;
    const size_t Ws = static_cast<size_t>(W);
    if (!reset_all) {
        if constexpr (LOCO) {
            const float* __restrict__ kept = T.loco.prev_action + static_cast<size_t>(w0) * n;
            for (int i = threadIdx.x; i < rows * n; i += kEnvThreads) {
                const int r = i / n, d = i - r * n;
                tile[r * pitch + NB + 12 + d] = kept[i];
            }
        }
        if (tracked) {
            if (wave == 1 && live) track_clock(T.track, V.steps[w], w, lane, row, s_clock);
            __syncthreads();
            track_stage(T.track, n, rows, wave, lane, s_ref, s_clock, tile, pitch);
        }
        // gather: lane = world, the waves split the words
        if (live) {
            if (wave == 0) {
                float b[13], lin[3], ang[3];
#pragma unroll
                for (int k = 0; k < 13; ++k) b[k] = D.base[k * Ws + w];
                ft_world_velocity(b, lin, ang);
#pragma unroll
                for (int k = 0; k < 7; ++k) row[k] = b[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) { row[7 + k] = lin[k]; row[10 + k] = ang[k]; }
                if constexpr (LOCO) {
                    float g[3];
                    ft_projected_gravity(b[3], b[4], b[5], b[6], g);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        row[NB + k] = g[k];
                        row[NB + 3 + k] = b[10 + k];
                        row[NB + 6 + k] = b[7 + k];
                    }
                }
            }
            for (int k = wave; k < 2 * n; k += kEnvWaves)
                row[13 + k] = (k < n) ? S.q[k * Ws + w] : S.qd[(k - n) * Ws + w];
            for (int j = wave; j < T.n_links; j += kEnvWaves) {
                // world z force of the link: its active contact slots of the last substep
                float f = 0.f;
                for (uint32_t m = D.cmask[w] & T.link_slots[j]; m; m &= m - 1u)
                    f += D.cdata[(static_cast<size_t>(__builtin_ctz(m)) * 7 + 5) * Ws + w];
                row[13 + 2 * n + j] = f;
                if constexpr (LOCO) {
                    uint32_t air = T.loco.air_steps[j * Ws + w];
                    s_pay[j * kEnvTile + lane] = ft_air_step(T.loco, f, air);
                    T.loco.air_steps[j * Ws + w] = air;
                }
            }
            if (LOCO && wave == 3) {
                const uint32_t g = T.world_offset + static_cast<uint32_t>(w), episode = V.episode[w], t = V.steps[w];
                const uint32_t k0 = ft_cmd_index(t, T.loco.cmd_interval), k1 = ft_cmd_index(t + 1u, T.loco.cmd_interval);
                uint32_t r[4];
                float c[3];
                philox(T.seed_lo, T.seed_hi, g, episode, r, ft_cmd_block(k0));
                ft_command(T.loco, r, c);
#pragma unroll
                for (int k = 0; k < 3; ++k) s_cmd[k * kEnvTile + lane] = c[k];
                if (k1 != k0) {
                    philox(T.seed_lo, T.seed_hi, g, episode, r, ft_cmd_block(k1));
                    ft_command(T.loco, r, c);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) row[NB + 9 + k] = c[k];
            }
            if (shaped) shape_gather(T, S, D, n, Ws, w, wave, lane, s_part, s_hit);
        }
        __syncthreads();
        if (wave == 0) {
            bool done = false;
            uint32_t episode = 0u, last = 0u;
            if (live) {
                bool term = ft_terminated(row[2], ft_tilt(row[4], row[5]), S.div[w] != 0, T.z_min, T.cos_tilt_max);
                if (shaped) {
                    // a termination link's slot under load in the run's last substep
#pragma unroll
                    for (int v = 0; v < kEnvWaves; ++v) term = term || s_hit[v * kEnvTile + lane] != 0;
                }
                float tr_err[kTrackTerms] = {0.f, 0.f, 0.f, 0.f, 0.f};
                bool clip_end = false;
                if (tracked) {
                    const int NS = 13 + 2 * n;
                    const float* ref = s_ref + lane * track_pitch(n);
                    const float q0[4] = {ref[3], ref[4], ref[5], ref[6]};
                    const float q1[4] = {ref[NS], ref[NS + 1], ref[NS + 2], ref[NS + 3]};
                    float qr[4];
                    ft_track_nlerp(q0, q1, __uint_as_float(s_clock[kTcBlend * kEnvTile + lane]), qr);
                    ft_track_errors(row, ref, qr, T.track.wj, n, T.track.ang_scale, tr_err);
                    term = term || ft_track_failed(T.track, tr_err);
                    clip_end = s_clock[kTcEnded * kEnvTile + lane] != 0u;  // truncated, as at the time limit
                }
                uint32_t steps = V.steps[w] + 1u;
                done = term || clip_end || (T.max_steps > 0 && steps >= static_cast<uint32_t>(T.max_steps));
                float rew = ft_reward(T, term, row[7], asq[w], ft_sum_sq_diff(row + 13, 1, T.home_q, n));
                if constexpr (LOCO) {
                    const float cmd[3] = {s_cmd[lane], s_cmd[kEnvTile + lane], s_cmd[2 * kEnvTile + lane]};
                    const float v[3] = {row[NB + 3], row[NB + 4], row[NB + 5]};
                    const float om[3] = {row[NB + 6], row[NB + 7], row[NB + 8]};
                    float pay = 0.f;
                    for (int j = 0; j < T.n_links; ++j) pay += s_pay[j * kEnvTile + lane];
                    rew = ft_loco_reward(T.loco, rew, cmd, v, om, T.loco.action_rate[w], pay);
                }
                if (tracked) {
                    float tr_term[kTrackTerms];
                    ft_track_terms(T.track, tr_err, S.div[w] != 0, tr_term);
                    rew = ft_track_reward(rew, tr_term);
#pragma unroll
                    for (int k = 0; k < kTrackTerms; ++k) {
                        s_tterms[lane * kTrackTerms + k] = tr_term[k];
                        s_terrs[lane * kTrackTerms + k] = tr_err[k];
                    }
                }
                if (shaped) {
                    const FloatShapeF& H = T.shape;
                    const bool diverged = S.div[w] != 0;
                    bool standing = false;
                    if constexpr (LOCO) standing = ft_shape_standing(s_cmd[lane], s_cmd[kEnvTile + lane], T.loco.cmd_min);
                    float term_k[kShapeTerms], acc_t[kShapeTerms], ep_t[kShapeTerms];
                    shape_terms(H, row, standing, diverged, lane, s_part, term_k);
                    rew = ft_shape_reward(rew, term_k);
                    // the episode's running sums; where done, out as the finished episode's and zeroed
                    float acc_r = H.acc_return[w], ep_r = 0.f;
                    int32_t acc_l = H.acc_length[w], ep_l = 0;
#pragma unroll
                    for (int k = 0; k < kShapeTerms; ++k) acc_t[k] = H.acc_terms[k * Ws + w];
                    const bool finished = ft_shape_stats(rew, term_k, diverged, done, acc_r, acc_l, acc_t, ep_r, ep_l, ep_t);
                    H.acc_return[w] = acc_r;
                    H.acc_length[w] = acc_l;
#pragma unroll
                    for (int k = 0; k < kShapeTerms; ++k) {
                        H.acc_terms[k * Ws + w] = acc_t[k];
                        s_terms[lane * kShapePitch + k] = term_k[k];
                        if (finished) s_epterms[lane * kShapePitch + k] = ep_t[k];
                    }
                    if (finished && H.ep_return) H.ep_return[w] = ep_r;
                    if (finished && H.ep_length) H.ep_length[w] = ep_l;
                }
                reward[w] = rew;
                done_out[w] = done ? 1 : 0;
                episode = V.episode[w];
                last = steps;
                if (done) {
                    episode += 1u;
                    steps = 0u;
                    V.episode[w] = episode;
                }
                V.steps[w] = steps;
            }
            s_done[lane] = done ? 1 : 0;
            s_episode[lane] = episode;
            if (PUSH || noisy) s_steps[lane] = live ? V.steps[w] : 0u;
            if (noisy) s_last[lane] = last;
        }
        __syncthreads();
        // the finished episodes' last observation: row r of the tile, lanes across its words
        // (the noise of the finished episode at its final step count)
        if (noisy) {
            ft_write_noisy(T, tile, pitch, rows, w0, term_obs, T.noise.clean_term_obs, s_done, s_episode, 1u, s_last);
        } else {
            for (int r = wave; r < rows; r += kEnvWaves)
                if (s_done[r])
                    for (int k = lane; k < NO; k += 64)
                        term_obs[static_cast<size_t>(w0 + r) * NO + k] = tile[r * pitch + k];
        }
        if (shaped) {
            // the tiles of the terms: [rows, 10] is one contiguous span of either output
            float* __restrict__ terms_out = T.shape.terms_out;
            float* __restrict__ ep_terms = T.shape.ep_terms;
            for (int i = threadIdx.x; i < rows * kShapeTerms; i += kEnvThreads) {
                const int r = i / kShapeTerms, k = i - r * kShapeTerms;
                const size_t o = static_cast<size_t>(w0) * kShapeTerms + i;
                if (terms_out) terms_out[o] = s_terms[r * kShapePitch + k];
                if (ep_terms && s_done[r]) ep_terms[o] = s_epterms[r * kShapePitch + k];
            }
        }
        if (tracked) {
            // likewise [rows, 5]
            float* __restrict__ terms_out = T.track.terms_out;
            float* __restrict__ errors_out = T.track.errors_out;
            for (int i = threadIdx.x; i < rows * kTrackTerms; i += kEnvThreads) {
                const size_t o = static_cast<size_t>(w0) * kTrackTerms + i;
                if (terms_out) terms_out[o] = s_tterms[i];
                if (errors_out) errors_out[o] = s_terrs[i];
            }
        }
        __syncthreads();
    } else {
        if (wave == 0) {
            s_done[lane] = live ? 1 : 0;
            s_episode[lane] = 0u;
            if (PUSH || noisy) s_steps[lane] = 0u;
            if (live) {
                V.episode[w] = 0u;
                V.steps[w] = 0u;
                if (shaped) {
                    // the running sums start over; the finished episodes' buffers stay
                    T.shape.acc_return[w] = 0.f;
                    T.shape.acc_length[w] = 0;
#pragma unroll
                    for (int k = 0; k < kShapeTerms; ++k) T.shape.acc_terms[k * Ws + w] = 0.f;
                }
            }
        }
        __syncthreads();
    }
    if (PUSH && wave == 2 && live) {
        const size_t node = static_cast<size_t>(D.wnodes) * Ws;  // words per wrench component
        if (!reset_all && T.rand.push_out) {
#pragma unroll
            for (int e = 0; e < 6; ++e) T.rand.push_out[static_cast<size_t>(w) * 6 + e] = D.wrench[e * node + w];
        }
        const uint32_t g = T.world_offset + static_cast<uint32_t>(w), episode = s_episode[lane];
        uint32_t r[4], k;
        philox(T.seed_lo, T.seed_hi, g, episode, r, kFtEpisodeBlock);
        float f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (ft_push_active(s_steps[lane], ft_push_phase(r[0], T.rand.push_interval), T.rand.push_interval,
                           T.rand.push_steps, k)) {
            philox(T.seed_lo, T.seed_hi, g, episode, r, ft_push_block(k));
            f[0] = unif(r[0], -T.rand.push_force, T.rand.push_force);
            f[1] = unif(r[1], -T.rand.push_force, T.rand.push_force);
            f[5] = unif(r[2], -T.rand.push_torque, T.rand.push_torque);
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) D.wrench[e * node + w] = f[e];
    }
    // resets: home pose + U(-noise, noise) per joint clipped into the position
    // limits, Philox counter (global world, episode, block of 4 dofs, 0) as
    // pid_task_reset; the base at home_base, everything at rest
    if (live && s_done[lane]) {
        const uint32_t episode = s_episode[lane];
        if (starts) {
            init_reset(P, T, S, D, n, Ws, w, wave, episode, shaped, LOCO ? NB : -1, row);
            if (tracked && T.track.obs_reference) track_reset_reference(T, n, w, wave, episode, row);
        } else {
            for (int b = wave; b < (n + 3) / 4; b += kEnvWaves) {
                uint32_t r[4];
                philox(T.seed_lo, T.seed_hi, T.world_offset + static_cast<uint32_t>(w), episode, r,
                       static_cast<uint32_t>(b));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int d = 4 * b + k;
                    if (d < n) {
                        const float x = T.home_q[d] + unif(r[k], -T.joint_noise, T.joint_noise);
                        const float q = fminf(fmaxf(x, P->b[d].lower), P->b[d].upper);
                        const size_t i = d * Ws + w;
                        S.rq[i] = q;
                        S.rqd[i] = 0.f;
                        S.rflag[i] = 1u | 2u | 4u;  // position, velocity, PID reset
                        row[13 + d] = q;
                        row[13 + n + d] = 0.f;
                    }
                }
            }
        }
        if (!starts && wave == 0) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                D.rpose[k * Ws + w] = T.home_base[k];
                row[k] = T.home_base[k];
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                D.rvel[k * Ws + w] = 0.f;
                row[7 + k] = 0.f;
            }
            D.rflag[w] = 1u | 2u;
            S.div[w] = 0;  // a reset re-arms the divergence flag (mw_reset_* do)
            if constexpr (LOCO) {
                float g[3];
                ft_projected_gravity(T.home_base[3], T.home_base[4], T.home_base[5], T.home_base[6], g);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    row[NB + k] = g[k];
                    row[NB + 3 + k] = 0.f;
                    row[NB + 6 + k] = 0.f;
                }
            }
        }
        if (RAND && wave == 1) {
            uint32_t r[4];
            philox(T.seed_lo, T.seed_hi, T.world_offset + static_cast<uint32_t>(w), episode, r, kFtEpisodeBlock);
            const float mu = unif(r[1], T.rand.friction_lo, T.rand.friction_hi);
            T.rand.mu[w] = mu;
            if (T.rand.friction_out) T.rand.friction_out[w] = mu;
        }
        if (T.noise.ring && wave == 2) {
            // the action delay of the episode this reset starts: the next action launch reads it
            uint32_t r[4];
            philox(T.seed_lo, T.seed_hi, T.world_offset + static_cast<uint32_t>(w), episode, r, kFtEpisodeBlock);
            const int32_t dl = static_cast<int32_t>(ft_delay_draw(r[2], T.noise.delay_lo, T.noise.delay_hi));
            T.noise.delay[w] = dl;
            if (T.noise.delay_out) T.noise.delay_out[w] = dl;
        }
        if constexpr (INERT) {
            const FloatInertiaF& I = T.inertia;
            const uint32_t g = T.world_offset + static_cast<uint32_t>(w);
            const bool scale = I.mass_hi > 0.f, payload = I.payload_hi > 0.f;
            float* __restrict__ rec = I.wpar + static_cast<size_t>(w) * I.stride;
            float* __restrict__ out = I.inertial_out ? I.inertial_out + static_cast<size_t>(w) * (n + 1) * 10 : nullptr;
            float* __restrict__ draw = I.draw_out ? I.draw_out + static_cast<size_t>(w) * (n + 5) : nullptr;
            for (int b = (wave + kEnvWaves - 1) % kEnvWaves; 4 * b <= n; b += kEnvWaves) {
                uint32_t r[4] = {0u, 0u, 0u, 0u};
                if (scale) philox(T.seed_lo, T.seed_hi, g, episode, r, ft_scale_block(4 * b));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = 4 * b + j;
                    if (k <= n) {
                        const float* __restrict__ nom = k ? &P->b[k - 1].mass : I.base0;
                        float w0[10], wd[10];
#pragma unroll
                        for (int e = 0; e < 10; ++e) wd[e] = w0[e] = nom[e];
                        const float s = scale ? unif(r[j], I.mass_lo, I.mass_hi) : 1.f;
                        if (scale) ft_inertia_scale(w0, s, wd);
                        if (draw) draw[k] = s;
                        if (k == 0) {
                            float mp = 0.f, pp[3] = {0.f, 0.f, 0.f};
                            if (payload) {
                                uint32_t rp[4];
                                philox(T.seed_lo, T.seed_hi, g, episode, rp, kFtPayloadBlock);
                                mp = unif(rp[0], I.payload_lo, I.payload_hi);
#pragma unroll
                                for (int e = 0; e < 3; ++e) pp[e] = unif(rp[1 + e], -I.payload_box[e], I.payload_box[e]);
                                ft_inertia_payload(wd, mp, pp);
                            }
                            if (draw) {
                                draw[n + 1] = mp;
#pragma unroll
                                for (int e = 0; e < 3; ++e) draw[n + 2 + e] = pp[e];
                            }
                        }
                        float* __restrict__ dst = k ? rec + kWparBody0 + (k - 1) * kWparBodyWords + kBodyInertial : rec;
#pragma unroll
                        for (int e = 0; e < 10; ++e) {
                            dst[e] = wd[e];
                            if (out) out[k * 10 + e] = wd[e];
                        }
                    }
                }
            }
        }
        if constexpr (JOINT) {
            const FloatJointF& J = T.joints;
            const uint32_t g = T.world_offset + static_cast<uint32_t>(w);
            const bool damp = J.damping_hi > 0.f, fric = J.friction_hi > 0.f, eff = J.effort_hi > 0.f;
            float* __restrict__ rec = J.wpar + static_cast<size_t>(w) * J.stride + kWparBody0;
            float* __restrict__ out = J.joints_out ? J.joints_out + static_cast<size_t>(w) * n * 3 : nullptr;
            float* __restrict__ draw = J.draw_out ? J.draw_out + static_cast<size_t>(w) * n * 3 : nullptr;
            for (int d = (wave + kEnvWaves - 1) % kEnvWaves; d < n; d += kEnvWaves) {
                const BodyF& b0 = P->b[d];
                const float nom[3] = {b0.damping, b0.friction, b0.effort};
                float a[3] = {0.f, 0.f, 1.f}, wd[3] = {nom[0], nom[1], nom[2]};
                if ((J.dof_mask >> d) & 1u) {
                    uint32_t r[4];
                    philox(T.seed_lo, T.seed_hi, g, episode, r, ft_joint_block(d));
                    if (damp) a[0] = unif(r[0], J.damping_lo, J.damping_hi);
                    if (fric) a[1] = unif(r[1], J.friction_lo, J.friction_hi);
                    if (eff) a[2] = unif(r[2], J.effort_lo, J.effort_hi);
                    float wn[3];
                    ft_joint_words(nom, a, wn);
                    if (damp) wd[0] = wn[0];
                    if (fric) wd[1] = wn[1];
                    if (eff) wd[2] = wn[2];
                    float* __restrict__ dst = rec + d * kWparBodyWords;
                    dst[kBodyDamping] = wd[0];
                    dst[kBodyFriction] = wd[1];
                    dst[kBodyEffort] = wd[2];
                }
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    if (out) out[d * 3 + e] = wd[e];
                    if (draw) draw[d * 3 + e] = a[e];
                }
            }
        }
        for (int j = wave; j < T.n_links; j += kEnvWaves) {
            row[13 + 2 * n + j] = 0.f;
            if constexpr (LOCO) T.loco.air_steps[j * Ws + w] = 0u;
        }
        if (shaped && !starts) {
            // joint_acc of an episode's first step is taken from rest (the wave that wrote the word)
            for (int d = wave; d < n; d += kEnvWaves) T.shape.qd_prev[d * Ws + w] = 0.f;
        }
        if constexpr (LOCO) {
            for (int d = wave; d < n; d += kEnvWaves) {
                row[NB + 12 + d] = 0.f;
                T.loco.prev_action[static_cast<size_t>(w) * n + d] = 0.f;
            }
            if (wave == 3) {
                uint32_t r[4];
                float c[3];
                philox(T.seed_lo, T.seed_hi, T.world_offset + static_cast<uint32_t>(w), episode, r, ft_cmd_block(0u));
                ft_command(T.loco, r, c);
#pragma unroll
                for (int k = 0; k < 3; ++k) row[NB + 9 + k] = c[k];
            }
        }
    }
    if (LOCO && wave == 3 && live && T.loco.command_out) {
        // the words this thread wrote itself: the gather's, or the reset's over them
#pragma unroll
        for (int k = 0; k < 3; ++k) T.loco.command_out[static_cast<size_t>(w) * 3 + k] = row[NB + 9 + k];
    }
    __syncthreads();
    if (starts && T.init.state_out) {
        // the state the new episodes start from: the first 13 + 2 n words of their clean reset rows
        const int NS = 13 + 2 * n;
        float* __restrict__ state_out = T.init.state_out;
        for (int r = wave; r < rows; r += kEnvWaves)
            if (s_done[r])
                for (int k = lane; k < NS; k += 64) state_out[static_cast<size_t>(w0 + r) * NS + k] = tile[r * pitch + k];
    }
    // (the noise of the episode and step count the row belongs to: the updated counters)
    if (noisy) {
        ft_write_noisy(T, tile, pitch, rows, w0, obs, T.noise.clean_obs, nullptr, s_episode, 0u, s_steps);
        return;
    }
    for (int r = wave; r < rows; r += kEnvWaves)
        for (int k = lane; k < NO; k += 64) obs[static_cast<size_t>(w0 + r) * NO + k] = tile[r * pitch + k];
}

}  // namespace dev

template <bool LOCO, bool DELAY>
static void launch_action(const FloatTaskF& T, const float* actions, float* out, float* asq, uint8_t* div,
                          unsigned long long* ndiv, int n, int W, hipStream_t st) {
    const dim3 grid((W + dev::kEnvTile - 1) / dev::kEnvTile), block(dev::kEnvThreads);
    // one tile, one more each for LOCO and DELAY: at most 3 x 64 x 49 words = 37 KB
    const size_t lds = (1 + LOCO + DELAY) * static_cast<size_t>(dev::kEnvTile) * (n | 1) * sizeof(float);
    dev::ActLocoArgs<LOCO> A;
    dev::ActDelayArgs<DELAY> L;
    if constexpr (LOCO) {
        A.scale = T.loco.action_scale;
        A.position = T.action_mode;
        A.prev = T.loco.prev_action;
        A.rate = T.loco.action_rate;
        for (int d = 0; d < kMaxBodies; ++d) A.home_q[d] = T.home_q[d];
    }
    if constexpr (DELAY) {
        L.steps = T.noise.steps;
        L.delay = T.noise.delay;
        L.ring = T.noise.ring;
        L.R = T.noise.delay_hi + 1u;
        L.position = T.action_mode;
        for (int d = 0; d < kMaxBodies; ++d) L.home_q[d] = T.home_q[d];
    }
    hipLaunchKernelGGL((dev::float_env_action_kernel<LOCO, DELAY>), grid, block, lds, st, actions, out, asq, div, ndiv, n,
                       W, A, L, T.action_mode == 0 ? T.shape.cmd_kept : nullptr);
}

hipError_t launch_float_env_action(const FloatTaskF& T, const float* actions, float* out, float* asq, uint8_t* div,
                                   unsigned long long* ndiv, int n, int W, hipStream_t st) {
    const bool loco = T.loco.on != 0u, delay = T.noise.ring != nullptr;
    if (loco && delay) launch_action<true, true>(T, actions, out, asq, div, ndiv, n, W, st);
    else if (loco) launch_action<true, false>(T, actions, out, asq, div, ndiv, n, W, st);
    else if (delay) launch_action<false, true>(T, actions, out, asq, div, ndiv, n, W, st);
    else launch_action<false, false>(T, actions, out, asq, div, ndiv, n, W, st);
    return hipGetLastError();
}

// The 32 instances of the post kernel, bit k of the index the k-th template
// argument: RAND, PUSH, LOCO, INERT, JOINT.
using PostKernel = decltype(&dev::float_env_post_kernel<false, false, false, false, false>);
template <size_t... I>
constexpr std::array<PostKernel, sizeof...(I)> post_kernels(std::index_sequence<I...>) {
    return {{dev::float_env_post_kernel<(I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0, (I & 16) != 0>...}};
}
constexpr auto kPostKernels = post_kernels(std::make_index_sequence<32>{});

// dynamic LDS of the post launch: the tile of rows, then the shaping and the tracking region where on
static size_t post_dynamic_lds(const FloatTaskF& T, int n) {
    return static_cast<size_t>(dev::kEnvTile) * (T.n_obs | 1) * sizeof(float) + (T.shape.on ? dev::kShapeLds : 0) +
           (T.track.on ? dev::track_lds(n) : 0);
}

hipError_t reserve_float_env_post_lds(const FloatTaskF& T, int n, int device, size_t* need, size_t* limit) {
    const size_t dynamic = post_dynamic_lds(T, n);
    const size_t loco = T.loco.on ? 4u : 0u;  // the instances with the locomotion arrays in their static LDS
    hipFuncAttributes fa{};
    if (hipError_t err = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kPostKernels[loco]))) return err;
    int per_block = 0;
    if (hipError_t err = hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, device)) return err;
    *need = dynamic + fa.sharedSizeBytes;
    *limit = static_cast<size_t>(per_block);
    if (*need > *limit || *need <= 65536u) return hipSuccess;
    // beyond the default: every instance this env can still become (the other
    // four flags may follow) is told how much dynamic LDS it may be launched
    // with.  The attribute belongs to the kernel, not to the env: it is only
    // ever raised, so that an env configured earlier keeps what it was given.
    static std::mutex guard;
    static size_t granted[2] = {0u, 0u};
    const std::lock_guard<std::mutex> lock(guard);
    if (dynamic <= granted[loco ? 1 : 0]) return hipSuccess;
    for (size_t i = 0; i < kPostKernels.size(); ++i)
        if ((i & 4u) == loco)
            if (hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kPostKernels[i]),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     static_cast<int>(dynamic)))
                return err;
    granted[loco ? 1 : 0] = dynamic;
    return hipSuccess;
}

hipError_t launch_float_env_post(const ChainF* P, const FloatTaskF& T, const SimDev& S, const FreeDev& D,
                                 const VecDev& V, const float* asq, float* obs, float* reward, uint8_t* done,
                                 float* term_obs, int n, int W, int reset_all, hipStream_t st) {
    const size_t lds = post_dynamic_lds(T, n);
    const dim3 grid((W + dev::kEnvTile - 1) / dev::kEnvTile), block(dev::kEnvThreads);
    // The locomotion rows are 25 + 3 n + n_links words: at most (48 dofs, 8
    // links) 64 x 177 words = 45,312 B, with the 14,080 B of the shaping branch
    // (partials, term tiles, hits) and the kernel's 3,648 B of static LDS still
    // inside the 65,536 B a block gets without asking for more.  The tracking
    // task adds its reference tile (track_lds) and can pass that: the configure
    // calls have then run reserve_float_env_post_lds.
    const bool rand = T.rand.friction_hi > 0.f, push = T.rand.push_interval > 0u, loco = T.loco.on != 0u;
    const bool inert = T.inertia.wpar != nullptr, joint = T.joints.wpar != nullptr;
    hipLaunchKernelGGL(kPostKernels[rand | push << 1 | loco << 2 | inert << 3 | joint << 4], grid, block, lds, st, P, T,
                       S, D, V, asq, obs, reward, done, term_obs, n, W, reset_all);
    return hipGetLastError();
}

}  // namespace mw
