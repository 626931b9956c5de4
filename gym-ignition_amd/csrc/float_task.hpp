// float_task.hpp -- task arithmetic of the batched env for articulated
// floating-base models (float_env_kernel.hip): world-frame base velocity from
// the stored body twist, tilt, reward and the termination predicate, float32.
// Plain inline functions: the post kernel calls them per world, and
// tests/host_float_task/harness.cpp builds the same code with g++ against
// numpy fp64.  The Philox reset sampling stays in rng.hpp (device only); the
// integer arithmetic of the push schedule (mw_floatenv_randomize) is here too,
// built by tests/host_float_rand/harness.cpp, the inertial words of the
// inertia randomisation (mw_floatenv_inertia: mass scale, payload), built by
// tests/host_float_inertia/harness.cpp, the joint words of the joint
// randomisation (mw_floatenv_joints: damping, friction, effort), built by
// tests/host_float_joints/harness.cpp, and so is the arithmetic of the
// locomotion task (mw_floatenv_locomotion: commands, projected gravity, the
// air-time counter, the extra reward terms), built by
// tests/host_float_loco/harness.cpp, and that of the observation noise and the
// action latency (mw_floatenv_noise: the noise unit, the noisy word, the delay
// draw and the ring's slots), built by tests/host_float_noise/harness.cpp, and
// that of the shaping rewards, the contact termination and the episode
// statistics (mw_floatenv_shaping: the ten terms, the slot predicate, the
// accumulator step), built by tests/host_float_shape/harness.cpp, and that of
// the initial-state randomisation (mw_floatenv_init_state: the row choice, the
// offsets, the composed orientation, the velocity sums), built by
// tests/host_float_init/harness.cpp, and that of the motion-clip tracking task
// (mw_floatenv_tracking: the frame clock, the clip draw, the blended reference
// row, the five errors and terms), built by tests/host_float_track/harness.cpp.
#pragma once

#ifdef MW_HOST_TEST
#include <cmath>
#ifndef __device__
#define __device__
#endif
#ifndef __host__
#define __host__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#else
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstdint>

#include "chain_params.hpp"
#include "world_params.hpp"

namespace mw {

constexpr int kMaxContactLinks = 8;  // mw_float_task_config::contact_links

// Randomisation of the floating-base env (mw_floatenv_randomize): pushes on
// the base and per-world ground friction, all off when zero.
struct FloatRandF {
    uint32_t push_interval;  // steps between push starts, 0 = no pushes
    uint32_t push_steps;     // steps a push lasts, 1..push_interval
    float push_force;        // fx, fy ~ U(-push_force, push_force) (N)
    float push_torque;       // tz ~ U(-push_torque, push_torque) (N m)
    float friction_lo, friction_hi;  // mu ~ U(lo, hi) per episode; on when hi > 0
    float* push_out;         // [W, 6] the wrench applied this step (caller's, may be null)
    float* friction_out;     // [W] the friction coefficient of the current episode (caller's, may be null)
    float* mu;               // [W] the simulator's per-world friction array (mw_sim::d_mu) when friction_hi > 0
};

// Philox counter blocks of the randomisation draws: the reset draw uses
// blocks 0 .. (n + 3) / 4 - 1 of the same (world, episode) counter.
constexpr uint32_t kFtEpisodeBlock = 0x40000000u;  // r[0]: push phase, r[1]: friction, r[2]: action delay
constexpr uint32_t kFtPushBlock = 0x80000000u;     // | k: push k of the episode (fx, fy, tz)
constexpr uint32_t kFtCmdBlock = 0xC0000000u;      // | k: command k of the episode (v_x, v_y, yaw rate, zero test)

// Locomotion task of the floating-base env (mw_floatenv_locomotion), off when
// `on` is zero: a per-world velocity command, the body-frame block of the
// observation, scaled actions and the tracking / smoothness / air-time terms
// of the reward.
struct FloatLocoF {
    uint32_t on;
    uint32_t cmd_interval;       // steps between command draws, 0 = one per episode
    float cmd_lo[3], cmd_hi[3];  // v_x, v_y (m/s), yaw rate (rad/s), body frame
    float cmd_zero_prob;         // a draw is the zero command with this probability
    float cmd_min;               // v_x^2 + v_y^2 <= cmd_min^2: no air-time term
    float action_scale;          // 0 = raw actions
    float w_track_lin, w_track_yaw, track_sigma, w_lin_z, w_ang_xy, w_action_rate;
    float w_air_time, air_time_target, contact_force_min;
    float env_dt;                // steps_per_run * step_size (s)
    float* prev_action;          // [W][n] the raw action of the last step, zeros after a reset
    uint32_t* air_steps;         // [n_links][W] steps without contact since the last touchdown
    float* action_rate;          // [W] sum_d (a_t - a_{t-1})^2 of the last step
    float* command_out;          // [W, 3] the command in force for the next step (caller's, may be null)
};

// Inertia randomisation of the floating-base env (mw_floatenv_inertia): link
// mass scales and a payload on the base, each off when its `hi` is zero.
struct FloatInertiaF {
    float mass_lo, mass_hi;        // s ~ U(lo, hi) per link and episode; on when hi > 0
    float payload_lo, payload_hi;  // m_p ~ U(lo, hi) kg per episode; on when hi > 0
    float payload_box[3];          // p ~ U(-box, box) m, base frame
    int32_t stride;                // words between two worlds' records in wpar
    float base0[10];               // the base's nominal inertial words (FloatF's first ten)
    float* wpar;                   // the simulator's per-world link parameters (mw_sim::d_wpar, RunArgs::wpar)
    float* inertial_out;           // [W, n + 1, 10] the words of the current episode (caller's, may be null)
    float* draw_out;               // [W, n + 5] the episode's draws: s_0 .. s_n, m_p, p xyz (caller's, may be null)
};
constexpr uint32_t kFtScaleBlock = 0x40000100u;    // | k / 4, word k % 4: scale of link k (0 = the base), k <= 48
constexpr uint32_t kFtPayloadBlock = 0x40000180u;  // r[0]: payload mass, r[1..3]: its position

// Joint randomisation of the floating-base env (mw_floatenv_joints): viscous
// damping and Coulomb friction added to the nominal words, the effort limit
// scaled, each off when its `hi` is zero; off altogether when wpar is null.
struct FloatJointF {
    float damping_lo, damping_hi;    // a ~ U(lo, hi) N m s/rad per joint and episode; on when hi > 0
    float friction_lo, friction_hi;  // f ~ U(lo, hi) N m; on when hi > 0
    float effort_lo, effort_hi;      // s ~ U(lo, hi), a factor; on when hi > 0
    uint64_t dof_mask;               // bit d: joint d is drawn (never 0 here: mw_floatenv_joints fills it)
    int32_t stride;                  // words between two worlds' records in wpar
    float* wpar;                     // the simulator's per-world link parameters (mw_sim::d_wpar, RunArgs::wpar)
    float* joints_out;               // [W, n, 3] damping, friction, effort of the current episode (caller's, may be null)
    float* draw_out;                 // [W, n, 3] the episode's draws a, f, s (caller's, may be null)
};
constexpr uint32_t kFtJointBlock = 0x40000200u;  // | d, words 0..2: damping, friction, effort draw of joint d < 48
constexpr float kFtUnbounded = 3.402823466e+38f;  // FLT_MAX: to_f32 of an infinite effort limit

// Observation noise and action latency of the floating-base env
// (mw_floatenv_noise): the noise is on when amp is set, the latency when ring is.
constexpr int kMaxActionDelay = 8;  // control steps; the ring holds delay_hi + 1 <= 9 rows per world
struct FloatNoiseF {
    const float* amp;          // [n_obs] amplitude of every observation word (device); null = no noise
    float* clean_obs;          // [W, n_obs] the rows of obs before the noise (caller's, may be null)
    float* clean_term_obs;     // [W, n_obs] likewise for terminal_obs, rows of done worlds only
    uint32_t delay_lo, delay_hi;  // d = delay_lo + r[2] % (delay_hi - delay_lo + 1) per episode
    float* ring;               // [W][delay_hi + 1][n] the raw actions of the last steps; null = no latency
    int32_t* delay;            // [W] the delay of the current episode (the env's own: the action launch reads it)
    const uint32_t* steps;     // [W] VecDev::steps for the action launch, whose launcher keeps its signature
    int32_t* delay_out;        // [W] the same words (caller's, may be null)
};

// Shaping rewards, contact termination and episode statistics of the
// floating-base env (mw_floatenv_shaping), off when `on` is zero.  Column k of
// a world's row of terms is -w[k] x_k of the step, x_k as listed; a weight of
// zero skips the term, which then reports 0.
constexpr int kShapeTerms = 10;
enum ShapeTerm : int {
    kShTorque = 0,     // sum_d tau_d^2
    kShPower,          // sum_d |tau_d qd_d|
    kShJointAcc,       // sum_d ((qd_d - qd_prev_d) / env_dt)^2
    kShOrientation,    // g_x^2 + g_y^2 of the projected gravity
    kShBaseHeight,     // (z - base_height_target)^2
    kShJointLimits,    // sum_d max(0, lo_d - q_d) + max(0, q_d - hi_d), lo / hi the soft limits
    kShCollision,      // penalised links whose contact force norm exceeds collision_force_min
    kShStumble,        // contact links with hypot(f_x, f_y) > stumble_ratio |f_z| and |f_z| > 0
    kShContactForce,   // sum over the contact links of max(0, |f| - max_contact_force)
    kShStandStill,     // sum_d |q_d - home_q_d| under a command with v_x^2 + v_y^2 <= cmd_min^2
};
// A sum over dofs or links is taken in kShapeLanes partial sums -- item i goes
// to partial i % kShapeLanes, each partial in index order -- which are then
// added in order: ((p_0 + p_1) + p_2) + p_3.  The post kernel's four waves
// each own one partial; a host build runs the same order.
constexpr int kShapeLanes = 4;
constexpr int kShapeDofSums = 5;   // torque, power, joint_acc, joint_limits, stand_still
constexpr int kShapeLinkSums = 3;  // collision, stumble, contact_force
constexpr int kShapeSums = kShapeDofSums + kShapeLinkSums;  // the dof sums, then the link sums
struct FloatShapeF {
    uint32_t on;
    uint32_t term_slots;           // union of the termination links' contact slots (FreeDev::cmask bits)
    float w[kShapeTerms];          // >= 0
    float base_height_target, collision_force_min, stumble_ratio, max_contact_force, termination_force;
    float env_dt;                  // steps_per_run * step_size (s)
    int32_t n_pen;                 // penalised links
    uint32_t pen_slots[kMaxContactLinks];  // contact slots of every penalised link
    float soft_lo[kMaxBodies], soft_hi[kMaxBodies];  // -/+ kFtUnbounded for a joint without finite limits
    const float* effort;           // the effort word of body 0: the shared ChainF's, or world 0's record (RunArgs::wpar)
    int32_t effort_stride;         // words between two worlds' records, 0 with the shared model
    float* qd_prev;                // [n][W] qd after the last step, zeros after a reset (the env's own)
    float* cmd_kept;               // [n][W] torque mode: the command the action launch stored (the env's own, may be null)
    float* terms_out;              // [W, 10] the step's terms (caller's, may be null)
    float* torque_out;             // [W, n] the torque the terms used (caller's, may be null)
    float* acc_return;             // [W] running sums of the current episode (the env's own)
    int32_t* acc_length;           // [W]
    float* acc_terms;              // [10][W]
    float* ep_return;              // [W] the last finished episode of every world (caller's, each may be null)
    int32_t* ep_length;            // [W]
    float* ep_terms;               // [W, 10]
};

// Initial-state randomisation and the reset-state bank of the floating-base
// env (mw_floatenv_init_state), off when `on` is zero.  An episode starts from
// a base row of 13 + 2 n words in the layout of a row of obs (position,
// quaternion wxyz, world linear and angular velocity, q, qd) -- the home row,
// or a row of the bank -- plus the draws below, each group off when its bit of
// `groups` is clear.
enum InitGroup : uint32_t { kInitPos = 1u, kInitRpy = 2u, kInitLin = 4u, kInitAng = 8u };
constexpr int kInitBaseDraws = 13;  // dpos, roll pitch yaw, dlin, dang, the bank row: then n joint-velocity draws
struct FloatInitF {
    uint32_t on;
    uint32_t groups;               // InitGroup bits
    float pos_lo[3], pos_hi[3];    // added to the base position (m, world frame)
    float rpy_lo[3], rpy_hi[3];    // roll, pitch, yaw (rad): qz(yaw) qy(pitch) qx(roll) q_row
    float lin_lo[3], lin_hi[3];    // added to the world linear velocity (m/s)
    float ang_lo[3], ang_hi[3];    // added to the world angular velocity (rad/s)
    float joint_vel;               // qd_d = row_qd_d + U(-joint_vel, joint_vel); on when > 0
    float state_prob;              // a bank row where U(0, 1) of r[1] < state_prob, else the home row
    int32_t n_states;              // rows of the bank, 0 = none
    const float* states;           // [n_states, 13 + 2 n] the bank (caller's, read at every reset)
    const float* home;             // [13 + 2 n] the home row: home_base, zeros, home_q, zeros (the env's own)
    float* state_out;              // [W, 13 + 2 n] the state the current episode started from (caller's, may be null)
    float* draws_out;              // [W, 13 + n] the episode's draws (caller's, may be null)
};
constexpr uint32_t kFtInitRowBlock = 0x40000300u;  // r[0]: bank row, r[1]: bank or home row
constexpr uint32_t kFtInitPosBlock = 0x40000301u;  // r[0..2]: position offsets
constexpr uint32_t kFtInitRpyBlock = 0x40000302u;  // r[0..2]: roll, pitch, yaw
constexpr uint32_t kFtInitLinBlock = 0x40000303u;  // r[0..2]: linear velocity offsets
constexpr uint32_t kFtInitAngBlock = 0x40000304u;  // r[0..2]: angular velocity offsets
constexpr uint32_t kFtInitQdBlock = 0x40000340u;   // | d / 4, word d % 4: velocity draw of joint d < 48

// Motion-clip tracking task of the floating-base env (mw_floatenv_tracking),
// off when `on` is zero.  A clip is a run of rows of the caller's buffer, each
// 13 + 2 n words in the layout of a row of obs; a world follows one clip per
// episode from a drawn start frame, on an integer frame clock of frame_num /
// frame_den frames per control step.  What a lane indexes by its own clip --
// the table -- and what a loop walks -- the joint weights -- sit in device
// memory, not in this by-value struct: a struct indexed per lane is copied to
// scratch (see init_reset).
constexpr int kMaxClips = 16;
constexpr int kTrackTerms = 5;
constexpr int kTrackTableWords = 4;  // first row, length, loop, 0 per clip
enum TrackTerm : int {
    kTrPose = 0,   // sum_d wj_d (q_d - q^_d)^2
    kTrVelocity,   // sum_d wj_d (qd_d - qd^_d)^2
    kTrRootPos,    // |p - p^|^2
    kTrRootRot,    // 1 - (q . q^)^2
    kTrRootVel,    // |v - v^|^2 + ang_scale |w - w^|^2
};
struct FloatTrackF {
    uint32_t on;
    int32_t n_clips;               // 1 .. kMaxClips
    int32_t frame_num, frame_den;  // frames per control step, both >= 1
    int32_t obs_reference;         // the block of obs carries the n reference joint positions of the next step
    int32_t nb;                    // first word of the block in a row of obs: phase sin, cos, clip id, [reference]
    float rsi_prob;                // a drawn start frame where U(0, 1) of r[2] < rsi_prob, else frame 0
    float ang_scale;               // weight of the angular part of root_vel
    float weight[kTrackTerms], scale[kTrackTerms];  // term k = weight[k] expf(-scale[k] e_k)
    float max_pose, max_root_pos, max_root_rot;     // early termination above it, 0 = off
    const float* clips;            // [F, 13 + 2 n] the clip rows (caller's, read at every step)
    const int32_t* table;          // [n_clips][kTrackTableWords] (the env's own, device)
    const float* wj;               // [n] the per-joint weights (the env's own, device)
    int32_t* clip;                 // [W] the clip of the current episode (the env's own)
    int32_t* f0;                   // [W] its start frame
    float* terms_out;              // [W, 5] the step's signed terms (caller's, may be null)
    float* errors_out;             // [W, 5] the step's errors (caller's, may be null)
    int32_t* clip_out;             // [W] copies of clip / f0 (caller's, each may be null)
    int32_t* frame_out;            // [W]
};
constexpr uint32_t kFtTrackBlock = 0x40000400u;  // r[0]: clip, r[1]: start frame, r[2]: drawn start or frame 0

// Task description of the floating-base env (kernel argument, by value).
struct FloatTaskF {
    int32_t action_mode;     // 0 torque (SimDev::cmd), 1 position (SimDev::ptgt)
    int32_t max_steps;       // 0 = no time limit
    int32_t n_links;         // contact words of the observation
    int32_t n_obs;           // 13 + 2 n + n_links
    uint32_t seed_lo, seed_hi;
    uint32_t world_offset;
    float z_min, cos_tilt_max;
    float alive_bonus, w_forward, w_action, w_pose;
    float joint_noise;
    float home_base[7];      // x y z qw qx qy qz
    uint32_t link_slots[kMaxContactLinks];  // contact slots (FreeDev::cmask bits) of every contact link
    float home_q[kMaxBodies];
    FloatRandF rand;
    FloatLocoF loco;
    FloatInertiaF inertia;
    FloatJointF joints;
    FloatNoiseF noise;
    FloatShapeF shape;
    FloatTrackF track;
    FloatInitF init;
};

namespace dev {

// The push schedule is a pure function of (seed, global world, episode, t), t
// the steps already taken in the episode: the episode's phase shifts a grid
// of period push_interval, push k = (t + phase) / interval is active while
// (t + phase) % interval < push_steps.
__device__ __forceinline__ uint32_t ft_push_phase(uint32_t r0, uint32_t interval) {
    return interval ? r0 % interval : 0u;
}
__device__ __forceinline__ bool ft_push_active(uint32_t t, uint32_t phase, uint32_t interval, uint32_t push_steps,
                                               uint32_t& k) {
    const uint32_t s = t + phase;
    k = s / interval;
    return s % interval < push_steps;
}
__device__ __forceinline__ uint32_t ft_push_block(uint32_t k) { return kFtPushBlock | k; }

// The rotation of the base (row-major, body -> world) from its unit
// quaternion: the matrix mw_get_base_velocity rotates the body twist with.
__device__ __forceinline__ void ft_rotation(float qw, float qx, float qy, float qz, float (&R)[9]) {
    R[0] = 1.f - 2.f * (qy * qy + qz * qz); R[1] = 2.f * (qx * qy - qw * qz); R[2] = 2.f * (qx * qz + qw * qy);
    R[3] = 2.f * (qx * qy + qw * qz); R[4] = 1.f - 2.f * (qx * qx + qz * qz); R[5] = 2.f * (qy * qz - qw * qx);
    R[6] = 2.f * (qx * qz - qw * qy); R[7] = 2.f * (qy * qz + qw * qx); R[8] = 1.f - 2.f * (qx * qx + qy * qy);
}

// World linear velocity of the base origin and world angular velocity from
// the stored base words [13] = p xyz, q wxyz, body twist w xyz, v xyz
// (Model::baseWorldLinearVelocity / baseWorldAngularVelocity).
__device__ __forceinline__ void ft_world_velocity(const float (&base)[13], float (&lin)[3], float (&ang)[3]) {
    float R[9];
    ft_rotation(base[3], base[4], base[5], base[6], R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        lin[r] = R[3 * r] * base[10] + R[3 * r + 1] * base[11] + R[3 * r + 2] * base[12];
        ang[r] = R[3 * r] * base[7] + R[3 * r + 1] * base[8] + R[3 * r + 2] * base[9];
    }
}

// R_zz: the world-z component of the base's z axis (1 upright, 0 on its side).
__device__ __forceinline__ float ft_tilt(float qx, float qy) { return 1.f - 2.f * (qx * qx + qy * qy); }

// Terminated by height, tilt or divergence (the time limit is not a failure).
__device__ __forceinline__ bool ft_terminated(float z, float rzz, bool diverged, float z_min, float cos_tilt_max) {
    return z < z_min || rzz < cos_tilt_max || diverged;
}

// sum_i x_i^2 and sum_i (x_i - h_i)^2 over n values `stride` apart, in index order
__device__ __forceinline__ float ft_sum_sq(const float* x, int n, size_t stride) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += x[i * stride] * x[i * stride];
    return s;
}
__device__ __forceinline__ float ft_sum_sq_diff(const float* x, size_t stride, const float* h, int n) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) {
        const float e = x[i * stride] - h[i];
        s += e * e;
    }
    return s;
}

// alive_bonus [not terminated] + w_forward v_x - w_action sum a^2 - w_pose sum (q - home)^2
__device__ __forceinline__ float ft_reward(const FloatTaskF& T, bool terminated, float vx, float sum_a2,
                                           float sum_pose2) {
    return (terminated ? 0.f : T.alive_bonus) + T.w_forward * vx - T.w_action * sum_a2 - T.w_pose * sum_pose2;
}

// rng.hpp's unif(), restated here so that the host harnesses build it:
// lo + (hi - lo) (x >> 8) 2^-24.
__device__ __forceinline__ float ft_unif(uint32_t x, float lo, float hi) {
    return lo + (hi - lo) * (static_cast<float>(x >> 8) * (1.f / 16777216.f));
}

// ---- observation noise and action latency (FloatNoiseF) ----
// The unit of the noise, ft_unif(x, -1, 1): -1 + (x >> 8) 2^-23, a multiple of
// 2^-23 in [-1, 1).  Every step is exact in float32 (a 24-bit integer, a power
// of two, a difference of multiples of 2^-23 below 2), so the value does not
// depend on whether the compiler fuses the product and the sum.
__device__ __forceinline__ float ft_noise_unit(uint32_t x) { return ft_unif(x, -1.f, 1.f); }
// clean + amp u in one rounding
__device__ __forceinline__ float ft_noisy(float clean, float amp, float u) { return fmaf(amp, u, clean); }

// The delay of an episode from word 2 of its episode block, lo <= hi.
__device__ __forceinline__ uint32_t ft_delay_draw(uint32_t r2, uint32_t lo, uint32_t hi) {
    return lo + r2 % (hi - lo + 1u);
}
// A ring of R rows per world: the step with t steps taken stores its action in
// slot ft_delay_slot(t, 0, R) and applies the row of ft_delay_slot(t, d, R), the
// action of step t - d -- while t < d the neutral command instead.  With d < R
// the applied slot was last written at step t - d of this episode: the slots
// written since are those of t - d + 1 .. t, all others modulo R.
__device__ __forceinline__ bool ft_delay_neutral(uint32_t t, uint32_t d) { return t < d; }
__device__ __forceinline__ uint32_t ft_delay_slot(uint32_t t, uint32_t d, uint32_t R) { return (t - d) % R; }

// ---- inertia randomisation (FloatInertiaF) ----
// A link's ten inertial words: mass, com xyz, Io xx yy zz xy xz yz about the
// link origin.  Every fused operation is an explicit fmaf and every other
// product, sum or quotient is rounded on its own: the device build contracts
// a * b + c wherever it finds one, across statements and inlined calls too, so
// both functions switch contraction off for their own operations.  The words
// are then defined values, the same from hipcc and from a host compiler.
#if defined(__clang__)
#define MW_FT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MW_FT_NO_CONTRACT
#endif

// mass = s mass0, Io[k] = s Io0[k], the centre of mass kept: 7 roundings.
__device__ __forceinline__ void ft_inertia_scale(const float (&w0)[10], float s, float (&w)[10]) {
    MW_FT_NO_CONTRACT
    w[0] = s * w0[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) w[k] = w0[k];
#pragma unroll
    for (int k = 4; k < 10; ++k) w[k] = s * w0[k];
}

// A point mass mp at p (link frame) joins the link, in place:
//   m' = m + mp;  com' = (m com + mp p) / m';  Io' = Io + mp (|p|^2 1 - p p^T)
// with |p|^2 - p_x^2 taken as p_y^2 + p_z^2 (no cancellation).
__device__ __forceinline__ void ft_inertia_payload(float (&w)[10], float mp, const float (&p)[3]) {
    MW_FT_NO_CONTRACT
    const float m = w[0];
    const float m1 = m + mp;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mc = m * w[1 + k];
        const float num = fmaf(mp, p[k], mc);
        w[1 + k] = num / m1;
    }
    const float xx = p[0] * p[0], yy = p[1] * p[1], zz = p[2] * p[2];
    const float xy = p[0] * p[1], xz = p[0] * p[2], yz = p[1] * p[2];
    const float syz = yy + zz, sxz = xx + zz, sxy = xx + yy;
    w[0] = m1;
    w[4] = fmaf(mp, syz, w[4]);
    w[5] = fmaf(mp, sxz, w[5]);
    w[6] = fmaf(mp, sxy, w[6]);
    w[7] = fmaf(-mp, xy, w[7]);
    w[8] = fmaf(-mp, xz, w[8]);
    w[9] = fmaf(-mp, yz, w[9]);
}

// ---- joint randomisation (FloatJointF) ----
// nom: the joint's nominal damping, friction and effort words; draw: a, f, s.
// damping = damping0 + a, friction = friction0 + f, effort = s effort0 with an
// unbounded limit (kFtUnbounded) kept: one rounding per word, none fused.
__device__ __forceinline__ void ft_joint_words(const float (&nom)[3], const float (&draw)[3], float (&w)[3]) {
    MW_FT_NO_CONTRACT
    w[0] = nom[0] + draw[0];
    w[1] = nom[1] + draw[1];
    const float e = draw[2] * nom[2];
    w[2] = nom[2] == kFtUnbounded ? nom[2] : e;
}

// Philox block of joint d's draws (words 0, 1, 2: damping, friction, effort)
__device__ __forceinline__ uint32_t ft_joint_block(int d) { return kFtJointBlock | static_cast<uint32_t>(d); }

// Philox block of link k's scale (k = 0 the base, 1 + i body i); its word is k % 4
__device__ __forceinline__ uint32_t ft_scale_block(int k) { return kFtScaleBlock | static_cast<uint32_t>(k >> 2); }

// ---- locomotion task (FloatLocoF) ----

// The command schedule is a pure function of (seed, global world, episode, t),
// t the steps already taken in the episode: command k = t / cmd_interval (0
// with one command per episode) comes from the Philox block kFtCmdBlock | k
// (k < 2^30).
__device__ __forceinline__ uint32_t ft_cmd_index(uint32_t t, uint32_t interval) { return interval ? t / interval : 0u; }
__device__ __forceinline__ uint32_t ft_cmd_block(uint32_t k) { return kFtCmdBlock | (k & 0x3FFFFFFFu); }
// r[0..2] into the three ranges; the zero command where U(0, 1) of r[3] (an
// exact float32: (r[3] >> 8) 2^-24) is below cmd_zero_prob.
__device__ __forceinline__ bool ft_cmd_is_zero(uint32_t r3, float zero_prob) { return ft_unif(r3, 0.f, 1.f) < zero_prob; }
__device__ __forceinline__ void ft_command(const FloatLocoF& L, const uint32_t (&r)[4], float (&cmd)[3]) {
    const bool zero = ft_cmd_is_zero(r[3], L.cmd_zero_prob);
#pragma unroll
    for (int k = 0; k < 3; ++k) cmd[k] = zero ? 0.f : ft_unif(r[k], L.cmd_lo[k], L.cmd_hi[k]);
}

// World -z in the body frame: minus the last row of the base's rotation.
__device__ __forceinline__ void ft_projected_gravity(float qw, float qx, float qy, float qz, float (&g)[3]) {
    g[0] = -(2.f * (qx * qz - qw * qy));
    g[1] = -(2.f * (qy * qz + qw * qx));
    g[2] = -(1.f - 2.f * (qx * qx + qy * qy));
}

// One step of a link's air-time bookkeeping: without contact the counter
// grows; the first step with contact after a flight is the touchdown, which
// pays (air_steps env_dt - air_time_target) and zeroes the counter.
__device__ __forceinline__ float ft_air_step(const FloatLocoF& L, float fz, uint32_t& air_steps) {
    if (!(fz > L.contact_force_min)) {
        air_steps += 1u;
        return 0.f;
    }
    const uint32_t flown = air_steps;
    air_steps = 0u;
    return flown ? static_cast<float>(flown) * L.env_dt - L.air_time_target : 0.f;
}

// The locomotion terms on top of ft_reward's four: v, w the body-frame linear
// and angular velocity of the base, cmd the command the step ran under, rate
// sum (a_t - a_{t-1})^2, air_pay the links' touchdown payments summed.
__device__ __forceinline__ float ft_loco_reward(const FloatLocoF& L, float base_reward, const float (&cmd)[3],
                                                const float (&v)[3], const float (&w)[3], float rate, float air_pay) {
    const float ex = cmd[0] - v[0], ey = cmd[1] - v[1], ew = cmd[2] - w[2];
    float r = base_reward;
    r += L.w_track_lin * expf(-(ex * ex + ey * ey) / L.track_sigma);
    r += L.w_track_yaw * expf(-(ew * ew) / L.track_sigma);
    r -= L.w_lin_z * (v[2] * v[2]);
    r -= L.w_ang_xy * (w[0] * w[0] + w[1] * w[1]);
    r -= L.w_action_rate * rate;
    if (cmd[0] * cmd[0] + cmd[1] * cmd[1] > L.cmd_min * L.cmd_min) r += L.w_air_time * air_pay;
    return r;
}

// ---- shaping rewards, contact termination, episode statistics (FloatShapeF) ----
// Every product and sum below has a defined rounding, as the inertial words
// above: a fused operation is an explicit fmaf, every other one is rounded on
// its own (contraction off), sums run in the order written.  A term is then
// the same bits from hipcc and from a host compiler.

// The soft limits of a joint: centre -/+ soft_limit * half-range; a joint
// without finite limits (either word at kFtUnbounded) gets -/+ kFtUnbounded
// and never contributes.  mw_floatenv_shaping runs it on the host.
__host__ __device__ __forceinline__ void ft_soft_limits(float lower, float upper, float soft, float& lo, float& hi) {
    MW_FT_NO_CONTRACT
    lo = -kFtUnbounded;
    hi = kFtUnbounded;
    if (!(lower > -kFtUnbounded) || !(upper < kFtUnbounded)) return;
    const float sum = lower + upper, dif = upper - lower;
    const float c = 0.5f * sum, h = 0.5f * dif;
    const float sh = soft * h;
    lo = c - sh;
    hi = c + sh;
}

// The torque the run's substeps used: dof_force's clamp (kernels.hip) of the
// JointController's last output (position mode) or of the stored command.
__device__ __forceinline__ float ft_shape_tau(float u, float effort) { return fminf(fmaxf(u, -effort), effort); }

// One dof into the five dof sums of its partial: torque (one rounding), power
// (two), joint_acc (three), joint_limits (at most three), stand_still (two).
__device__ __forceinline__ void ft_shape_dof(float tau, float q, float qd, float qd_prev, float env_dt, float lo,
                                             float hi, float home, float (&acc)[kShapeDofSums]) {
    MW_FT_NO_CONTRACT
    acc[0] = fmaf(tau, tau, acc[0]);
    const float p = tau * qd;
    acc[1] = acc[1] + fabsf(p);
    const float dv = qd - qd_prev;
    const float a = dv / env_dt;
    acc[2] = fmaf(a, a, acc[2]);
    const float below = lo - q, above = q - hi;
    const float out = fmaxf(0.f, below) + fmaxf(0.f, above);
    acc[3] = acc[3] + out;
    const float e = q - home;
    acc[4] = acc[4] + fabsf(e);
}

// |f| of a force vector: sqrt(fz^2 + (fy^2 + fx^2)), four roundings
__device__ __forceinline__ float ft_force_norm(float fx, float fy, float fz) {
    MW_FT_NO_CONTRACT
    const float xx = fx * fx;
    const float xy = fmaf(fy, fy, xx);
    return sqrtf(fmaf(fz, fz, xy));
}

// A contact slot of a termination link ends the episode when its force norm
// exceeds termination_force (the slot is active in cmask: the caller's test).
__device__ __forceinline__ bool ft_shape_slot_hit(const FloatShapeF& H, float fx, float fy, float fz) {
    return ft_force_norm(fx, fy, fz) > H.termination_force;
}

// A penalised link with the summed force f of its active slots: 1 where |f| > collision_force_min
__device__ __forceinline__ float ft_shape_collision(const FloatShapeF& H, float fx, float fy, float fz) {
    return ft_force_norm(fx, fy, fz) > H.collision_force_min ? 1.f : 0.f;
}

// A contact link with the summed force f of its active slots into the stumble
// count and the excess-force sum of its partial.
__device__ __forceinline__ void ft_shape_contact(const FloatShapeF& H, float fx, float fy, float fz, float& stumble,
                                                 float& excess) {
    MW_FT_NO_CONTRACT
    const float xx = fx * fx;
    const float hxy = sqrtf(fmaf(fy, fy, xx));
    const float az = fabsf(fz);
    const float lim = H.stumble_ratio * az;
    stumble = stumble + ((az > 0.f && hxy > lim) ? 1.f : 0.f);
    const float over = ft_force_norm(fx, fy, fz) - H.max_contact_force;
    excess = excess + fmaxf(0.f, over);
}

// The partials of one sum added in order
__device__ __forceinline__ float ft_shape_combine(const float (&p)[kShapeLanes]) {
    MW_FT_NO_CONTRACT
    float s = p[0];
#pragma unroll
    for (int v = 1; v < kShapeLanes; ++v) s = s + p[v];
    return s;
}

// g_x^2 + g_y^2 of the projected gravity (ft_projected_gravity's first two
// words, here with defined rounding): g_x = -2 (qx qz - qw qy), g_y = -2 (qy qz
// + qw qx); the doublings are exact, six roundings in all.
__device__ __forceinline__ float ft_shape_orientation(float qw, float qx, float qy, float qz) {
    MW_FT_NO_CONTRACT
    const float xz = qx * qz, yz = qy * qz;
    const float hx = fmaf(-qw, qy, xz), hy = fmaf(qw, qx, yz);
    const float gx = -(2.f * hx), gy = -(2.f * hy);
    const float xx = gx * gx;
    return fmaf(gy, gy, xx);
}

// (z - target)^2, two roundings
__device__ __forceinline__ float ft_shape_height(float z, float target) {
    MW_FT_NO_CONTRACT
    const float e = z - target;
    return e * e;
}

// stand_still counts under a command with v_x^2 + v_y^2 <= cmd_min^2
__device__ __forceinline__ bool ft_shape_standing(float cx, float cy, float cmd_min) {
    MW_FT_NO_CONTRACT
    const float xx = cx * cx;
    const float c2 = fmaf(cy, cy, xx), m2 = cmd_min * cmd_min;
    return c2 <= m2;
}

// The ten x of a world from its eight combined sums (kShapeDofSums, then
// kShapeLinkSums), the base's pose words (x y z qw qx qy qz) and whether the
// command counts as standing still.
__device__ __forceinline__ void ft_shape_x(const FloatShapeF& H, const float (&sum)[kShapeSums], const float (&pose)[7],
                                           bool standing, float (&x)[kShapeTerms]) {
    x[kShTorque] = sum[0];
    x[kShPower] = sum[1];
    x[kShJointAcc] = sum[2];
    x[kShOrientation] = ft_shape_orientation(pose[3], pose[4], pose[5], pose[6]);
    x[kShBaseHeight] = ft_shape_height(pose[2], H.base_height_target);
    x[kShJointLimits] = sum[3];
    x[kShCollision] = sum[5];
    x[kShStumble] = sum[6];
    x[kShContactForce] = sum[7];
    x[kShStandStill] = standing ? sum[4] : 0.f;
}

// The ten signed terms from the ten x: -(w x), one rounding; 0 where the
// weight is zero or the world diverged (its state is not finite).
__device__ __forceinline__ void ft_shape_terms(const FloatShapeF& H, const float (&x)[kShapeTerms], bool diverged,
                                               float (&term)[kShapeTerms]) {
    MW_FT_NO_CONTRACT
#pragma unroll
    for (int k = 0; k < kShapeTerms; ++k) {
        const float wx = H.w[k] * x[k];
        term[k] = (H.w[k] != 0.f && !diverged) ? -wx : 0.f;
    }
}

// reward = r_existing + term[0] + ... + term[9], in that order
__device__ __forceinline__ float ft_shape_reward(float r_existing, const float (&term)[kShapeTerms]) {
    MW_FT_NO_CONTRACT
    float r = r_existing;
#pragma unroll
    for (int k = 0; k < kShapeTerms; ++k) r = r + term[k];
    return r;
}

// One step of a world's episode statistics: the running sums take the step
// (nothing from a diverged world); where done they are copied out as the
// finished episode (finished = true, ep_* filled) and zeroed.
__device__ __forceinline__ bool ft_shape_stats(float reward, const float (&term)[kShapeTerms], bool diverged, bool done,
                                               float& acc_return, int32_t& acc_length,
                                               float (&acc_terms)[kShapeTerms], float& ep_return, int32_t& ep_length,
                                               float (&ep_terms)[kShapeTerms]) {
    MW_FT_NO_CONTRACT
    if (!diverged) {
        acc_return = acc_return + reward;
        acc_length += 1;
#pragma unroll
        for (int k = 0; k < kShapeTerms; ++k) acc_terms[k] = acc_terms[k] + term[k];
    }
    if (!done) return false;
    ep_return = acc_return;
    ep_length = acc_length;
    acc_return = 0.f;
    acc_length = 0;
#pragma unroll
    for (int k = 0; k < kShapeTerms; ++k) {
        ep_terms[k] = acc_terms[k];
        acc_terms[k] = 0.f;
    }
    return true;
}

// ---- initial-state randomisation and the reset-state bank (FloatInitF) ----

// The bank row an episode starts from, from words 0 and 1 of its row block:
// r_a % K where U(0, 1) of r_b (an exact float32) is below state_prob, else -1,
// the home row.  state_prob 1 always takes the bank (U < 1), 0 never.
__device__ __forceinline__ int32_t ft_init_row(uint32_t r_a, uint32_t r_b, int32_t n_states, float state_prob) {
    if (n_states <= 0 || !(ft_unif(r_b, 0.f, 1.f) < state_prob)) return -1;
    return static_cast<int32_t>(r_a % static_cast<uint32_t>(n_states));
}
// Philox block of joint d's velocity draw; its word is d % 4
__device__ __forceinline__ uint32_t ft_init_qd_block(int d) { return kFtInitQdBlock | static_cast<uint32_t>(d >> 2); }

// The three offsets of a group from words 0..2 of its block
__device__ __forceinline__ void ft_init_offsets(const uint32_t (&r)[4], const float (&lo)[3], const float (&hi)[3],
                                                float (&d)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = ft_unif(r[k], lo[k], hi[k]);
}

// A row's word plus its draw, one rounding (a position, a velocity)
__device__ __forceinline__ float ft_init_sum(float word, float draw) {
    MW_FT_NO_CONTRACT
    return word + draw;
}

// q / |q|: the square sum ((w^2 + x^2) + y^2) + z^2 in fused steps, one
// square root, one quotient, four products
__device__ __forceinline__ void ft_init_normalise(float (&q)[4]) {
    MW_FT_NO_CONTRACT
    const float ww = q[0] * q[0];
    const float wx = fmaf(q[1], q[1], ww);
    const float wy = fmaf(q[2], q[2], wx);
    const float n2 = fmaf(q[3], q[3], wy);
    const float inv = 1.f / sqrtf(n2);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] * inv;
}

// The reset orientation qz(yaw) qy(pitch) qx(roll) q_row, normalised: three
// world-frame rotations after the row's own, each a Hamilton product with a
// quaternion of two nonzero words (one product and one fused multiply-add per
// component), sinf / cosf of the half angles.  An angle of zero leaves its
// factor exact (c = 1, s = 0).
__device__ __forceinline__ void ft_init_orientation(const float (&rpy)[3], const float (&q_row)[4], float (&q)[4]) {
    MW_FT_NO_CONTRACT
    float h, c, s, a[4], b[4];
    h = 0.5f * rpy[0]; c = cosf(h); s = sinf(h);
    {
        const float cw = c * q_row[0], cx = c * q_row[1], cy = c * q_row[2], cz = c * q_row[3];
        a[0] = fmaf(-s, q_row[1], cw); a[1] = fmaf(s, q_row[0], cx);
        a[2] = fmaf(-s, q_row[3], cy); a[3] = fmaf(s, q_row[2], cz);
    }
    h = 0.5f * rpy[1]; c = cosf(h); s = sinf(h);
    {
        const float cw = c * a[0], cx = c * a[1], cy = c * a[2], cz = c * a[3];
        b[0] = fmaf(-s, a[2], cw); b[1] = fmaf(s, a[3], cx);
        b[2] = fmaf(s, a[0], cy); b[3] = fmaf(-s, a[1], cz);
    }
    h = 0.5f * rpy[2]; c = cosf(h); s = sinf(h);
    {
        const float cw = c * b[0], cx = c * b[1], cy = c * b[2], cz = c * b[3];
        q[0] = fmaf(-s, b[3], cw); q[1] = fmaf(-s, b[2], cx);
        q[2] = fmaf(s, b[1], cy); q[3] = fmaf(s, b[0], cz);
    }
    ft_init_normalise(q);
}

// R^T v with R of the unit quaternion q: a world vector in the body frame (the
// body-frame velocities of the locomotion rows)
__device__ __forceinline__ void ft_init_body_frame(const float (&q)[4], const float (&v)[3], float (&out)[3]) {
    float R[9];
    ft_rotation(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = R[k] * v[0] + R[3 + k] * v[1] + R[6 + k] * v[2];
}

// The base words of a reset from its base row (13 words) and the four groups'
// draws: base[0..12] the words of the reset row (and of D.rpose / D.rvel), qn
// the unit quaternion of the start (base[3..6] itself with the orientation
// group on, else the row's normalised: the row's own words are then written
// as they are and the run normalises what it takes).
__device__ __forceinline__ void ft_init_base(const FloatInitF& I, const float (&row)[13], const float (&dpos)[3],
                                             const float (&rpy)[3], const float (&dlin)[3], const float (&dang)[3],
                                             float (&base)[13], float (&qn)[4]) {
    const float q_row[4] = {row[3], row[4], row[5], row[6]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        base[k] = (I.groups & kInitPos) ? ft_init_sum(row[k], dpos[k]) : row[k];
        base[7 + k] = (I.groups & kInitLin) ? ft_init_sum(row[7 + k], dlin[k]) : row[7 + k];
        base[10 + k] = (I.groups & kInitAng) ? ft_init_sum(row[10 + k], dang[k]) : row[10 + k];
    }
    if (I.groups & kInitRpy) {
        ft_init_orientation(rpy, q_row, qn);
#pragma unroll
        for (int k = 0; k < 4; ++k) base[3 + k] = qn[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) base[3 + k] = qn[k] = q_row[k];
        ft_init_normalise(qn);
    }
}

// ---- motion-clip tracking task (FloatTrackF) ----

// The clip of an episode and the frame it starts at, from words 0..2 of its
// tracking block: clip r0 % n_clips; frame r1 % (length - 1) where U(0, 1) of r2
// (an exact float32) is below rsi_prob, else 0.  A start frame is never the last
// row: a looping clip's last row is its first pose again, a clip that ends has
// nothing to follow from there.
__device__ __forceinline__ int32_t ft_track_clip(uint32_t r0, int32_t n_clips) {
    return static_cast<int32_t>(r0 % static_cast<uint32_t>(n_clips));
}
__device__ __forceinline__ int32_t ft_track_start(uint32_t r1, uint32_t r2, int32_t length, float rsi_prob) {
    if (!(ft_unif(r2, 0.f, 1.f) < rsi_prob)) return 0;
    return static_cast<int32_t>(r1 % static_cast<uint32_t>(length - 1));
}

// The frame clock, integers throughout: with f0 the start frame and t the steps
// taken, x_num = f0 den + t num; the reference of that instant lies between
// rows i and i1 of the clip at blend a = (x_num % den) / den, i = x_num / den.
// A looping clip has the period length - 1 (its last row is its first pose):
// i wraps modulo the period and `wraps` counts the periods gone by.  A clip
// that ends is `ended` at the first instant that would need a row beyond the
// last; the reference then stays the last row (i = i1 = length - 1, a = 0).
// With a == 0 the second row is not needed and i1 = i, so no row beyond the
// clip is ever addressed.
struct TrackClock {
    int32_t i, i1;   // rows of the clip, 0 <= i <= i1 <= length - 1
    float a;         // in [0, 1)
    uint32_t wraps;
    bool ended;
};
__device__ __forceinline__ TrackClock ft_track_clock(int32_t f0, uint32_t t, int32_t num, int32_t den, int32_t length,
                                                     bool loop) {
    const uint64_t d = static_cast<uint64_t>(den);
    const uint64_t x = static_cast<uint64_t>(f0) * d + static_cast<uint64_t>(t) * static_cast<uint64_t>(num);
    const uint64_t last = static_cast<uint64_t>(length - 1);
    // the same quotients in 32 bits where x fits, as it does for all but the longest
    // episodes: a 64-bit division is a long routine on the device
    const bool narrow = (x >> 32) == 0u;
    uint64_t fi = narrow ? static_cast<uint32_t>(x) / static_cast<uint32_t>(den) : x / d;
    const uint32_t rem = static_cast<uint32_t>(x - fi * d);
    TrackClock c;
    c.wraps = 0u;
    c.ended = false;
    c.a = static_cast<float>(rem) / static_cast<float>(den);
    if (loop) {
        const uint64_t w = narrow ? static_cast<uint32_t>(fi) / static_cast<uint32_t>(last) : fi / last;
        c.wraps = static_cast<uint32_t>(w);
        fi -= w * last;
    } else if (fi + (rem ? 1u : 0u) > last) {
        c.ended = true;
        fi = last;
        c.a = 0.f;
    }
    c.i = static_cast<int32_t>(fi);
    c.i1 = c.i + ((rem && !c.ended) ? 1 : 0);
    return c;
}

// phi = x_t / (length - 1), modulo 1 on a looping clip: two roundings
__device__ __forceinline__ float ft_track_phase(int32_t i, float a, int32_t length) {
    MW_FT_NO_CONTRACT
    const float x = static_cast<float>(i) + a;
    return x / static_cast<float>(length - 1);
}
// sin and cos of 2 pi phi: one rounding of the angle, then sinf / cosf
__device__ __forceinline__ void ft_track_phase_words(float phi, float& s, float& c) {
    MW_FT_NO_CONTRACT
    const float ang = 6.283185307179586f * phi;
    s = sinf(ang);
    c = cosf(ang);
}

// One word of the reference row: p0 + a (p1 - p0), the difference rounded, then
// one fused step; a == 0 gives p0's bits.
__device__ __forceinline__ float ft_track_lerp(float p0, float p1, float a) {
    MW_FT_NO_CONTRACT
    const float d = p1 - p0;
    return fmaf(a, d, p0);
}
// The base x or y of a looping clip after `wraps` periods: the word plus wraps
// times the clip's displacement over a period (last row minus first row)
__device__ __forceinline__ float ft_track_wrapped(float word, uint32_t wraps, float p_last, float p_first) {
    MW_FT_NO_CONTRACT
    const float d = p_last - p_first;
    return fmaf(static_cast<float>(wraps), d, word);
}
// The reference orientation: nlerp of q0 and q1 (wxyz) -- q1 negated where the
// dot product is negative (the short way round), every word blended as above,
// the result normalised (ft_init_normalise).
__device__ __forceinline__ void ft_track_nlerp(const float (&q0)[4], const float (&q1)[4], float a, float (&q)[4]) {
    MW_FT_NO_CONTRACT
    const float ww = q0[0] * q1[0];
    const float wx = fmaf(q0[1], q1[1], ww);
    const float wy = fmaf(q0[2], q1[2], wx);
    const float dot = fmaf(q0[3], q1[3], wy);
    const float sgn = dot < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = ft_track_lerp(q0[k], sgn * q1[k], a);
    ft_init_normalise(q);
}

// The five errors of a world: row, the 13 + 2 n first words of its observation
// (the state after the step); ref, the reference row of the same instant with
// its orientation already blended (qr).  Sums run in index order, each item a
// difference, a weighted product and a fused step.
__device__ __forceinline__ void ft_track_errors(const float* row, const float* ref, const float (&qr)[4],
                                                const float* wj, int n, float ang_scale, float (&e)[kTrackTerms]) {
    MW_FT_NO_CONTRACT
    float sp = 0.f, sv = 0.f;
    for (int d = 0; d < n; ++d) {
        const float dq = row[13 + d] - ref[13 + d];
        const float wq = wj[d] * dq;
        sp = fmaf(wq, dq, sp);
        const float dv = row[13 + n + d] - ref[13 + n + d];
        const float wv = wj[d] * dv;
        sv = fmaf(wv, dv, sv);
    }
    e[kTrPose] = sp;
    e[kTrVelocity] = sv;
    const float dx = row[0] - ref[0], dy = row[1] - ref[1], dz = row[2] - ref[2];
    const float xx = dx * dx;
    const float xy = fmaf(dy, dy, xx);
    e[kTrRootPos] = fmaf(dz, dz, xy);
    const float ww = row[3] * qr[0];
    const float wx = fmaf(row[4], qr[1], ww);
    const float wy = fmaf(row[5], qr[2], wx);
    const float dot = fmaf(row[6], qr[3], wy);
    e[kTrRootRot] = fmaf(-dot, dot, 1.f);
    float lin = 0.f, ang = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dl = row[7 + k] - ref[7 + k], da = row[10 + k] - ref[10 + k];
        lin = fmaf(dl, dl, lin);
        ang = fmaf(da, da, ang);
    }
    e[kTrRootVel] = fmaf(ang_scale, ang, lin);
}

// The five signed terms: weight_k expf(-(scale_k e_k)); 0 where the weight is
// zero or the world diverged (its state is not finite).
__device__ __forceinline__ void ft_track_terms(const FloatTrackF& K, const float (&e)[kTrackTerms], bool diverged,
                                               float (&term)[kTrackTerms]) {
    MW_FT_NO_CONTRACT
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) {
        const float x = K.scale[k] * e[k];
        const float v = K.weight[k] * expf(-x);
        term[k] = (K.weight[k] != 0.f && !diverged) ? v : 0.f;
    }
}
// reward = r_existing + term[0] + ... + term[4], in that order
__device__ __forceinline__ float ft_track_reward(float r_existing, const float (&term)[kTrackTerms]) {
    MW_FT_NO_CONTRACT
    float r = r_existing;
#pragma unroll
    for (int k = 0; k < kTrackTerms; ++k) r = r + term[k];
    return r;
}
// Early termination: pose, root_pos or root_rot above its bound (0 = off)
__device__ __forceinline__ bool ft_track_failed(const FloatTrackF& K, const float (&e)[kTrackTerms]) {
    return (K.max_pose > 0.f && e[kTrPose] > K.max_pose) || (K.max_root_pos > 0.f && e[kTrRootPos] > K.max_root_pos) ||
           (K.max_root_rot > 0.f && e[kTrRootRot] > K.max_root_rot);
}

#undef MW_FT_NO_CONTRACT

}  // namespace dev
}  // namespace mw
