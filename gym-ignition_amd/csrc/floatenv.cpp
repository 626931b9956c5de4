// floatenv.cpp -- the floating-base env of the C ABI (include/mwstep.h,
// mw_floatenv_*): mw_floatenv_create, the configure calls that run between it
// and the first mw_vecenv_reset, and what mw_vecenv_reset / _step / _destroy
// (vecenv.cpp) do for such an env.  The kernels are float_env_kernel.hip's; the
// run between the action and the post launch is the simulator's (run_impl).
//
// Every call keeps one rule: a failed call leaves the env as it was.  Nothing
// is assigned into the handle or the simulator until every check and every
// allocation of that call has succeeded.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "errors.hpp"
#include "vecenv_state.hpp"

using mw::fail;

// The refusals every configure call opens with.
static int check_configurable(const mw_vecenv* e, const void* cfg, const char* call) {
    if (!e || !cfg) return fail(MW_EINVAL, "null argument");
    if (!e->fenv) return fail(MW_ESTATE, std::string(call) + " needs an env made by mw_floatenv_create");
    if (e->fenv->was_reset)
        return fail(MW_ESTATE, std::string(call) + " must be called before the first mw_vecenv_reset");
    return MW_OK;
}

// The contact slots of a link (FloatF::shape_body / shape_slot0 order:
// slot_body) among the 32 that the wave kernel's contact mask holds.
static uint32_t link_slots(const mw_sim* s, int32_t link) {
    uint32_t slots = 0u;
    for (int slot = 0; slot < s->n_slots && slot < 32; ++slot)
        if (s->slot_body[slot] == link) slots |= 1u << slot;
    return slots;
}

// The home row [13 + 2 n] in device memory: what init_reset starts an episode
// from where neither a bank row nor a clip row is drawn.
static int make_home_row(const mw_sim* s, const mw::FloatTaskF& T, mw::dev_ptr<float[]>& home) {
    const size_t n = static_cast<size_t>(s->n), words = 13 + 2 * n;
    std::vector<float> home_row(words, 0.f);
    for (int k = 0; k < 7; ++k) home_row[k] = T.home_base[k];
    for (size_t d = 0; d < n; ++d) home_row[13 + d] = T.home_q[d];
    MW_HIP(mw::dev_alloc(home, words * sizeof(float)));
    MW_HIP(hipMemcpy(home.get(), home_row.data(), words * sizeof(float), hipMemcpyHostToDevice));  // complete on return
    return MW_OK;
}

// The local memory of the post launch under the task `T` a configure call is
// about to commit, against the device's (float_env_kernel.hip).  A build of
// this layer without the kernels (the host-only builds of the tests, whose
// launchers do nothing) has no such function and nothing to check.
namespace mw {
__attribute__((weak)) hipError_t reserve_float_env_post_lds(const FloatTaskF& T, int n, int device, size_t* need,
                                                            size_t* limit);
}
static int check_post_lds(const mw_sim* s, const mw::FloatTaskF& T, const char* call) {
    if (!mw::reserve_float_env_post_lds) return MW_OK;
    size_t need = 0, limit = 0;
    const hipError_t err = mw::reserve_float_env_post_lds(T, s->n, s->cfg.device, &need, &limit);
    if (need > limit)
        return fail(MW_ECAPACITY, std::string(call) + ": the post launch would need " + std::to_string(need) +
                                      " bytes of local memory per block, the device allows " + std::to_string(limit));
    MW_HIP(err);
    return MW_OK;
}

extern "C" {

// Batched env of an articulated floating-base model on the wave kernel
// (float_env_kernel.hip): the env's kernels write the run kernel's command
// and pending-reset arrays on the device, the run itself is run_impl's.
int mw_floatenv_create(mw_sim* s, const mw_float_task_config* cfg, mw_vecenv** out) {
    if (!s || !cfg || !out) return fail(MW_EINVAL, "null argument");
    *out = nullptr;
    int rc = check_sim(s);
    if (rc) return rc;
    if (!s->floating || !s->float_tree || !s->wave || s->n == 0)
        return fail(MW_EINVAL, "the floating-base env needs an articulated model on a floating base (joints, "
                               "mw_is_floating) stepped by the world-per-wavefront kernel (mw_float_kernel == 2)");
    if (s->env_owned) return fail(MW_ESTATE, "the simulator already has a floating-base env");
    const int n = s->n;
    for (int d = 0; d < n; ++d)
        if (s->model.bodies[d].ball)
            return fail(MW_EINVAL, "the floating-base env does not take models with ball joints (joint '" +
                                       s->model.bodies[d].joint_name + "')");
    if (s->cfg.steps_per_run > 64) return fail(MW_EINVAL, "steps_per_run must be <= 64");
    if (cfg->action_mode != MW_FLOAT_ACTION_TORQUE && cfg->action_mode != MW_FLOAT_ACTION_POSITION)
        return fail(MW_EINVAL, "unknown action mode");
    if (cfg->max_episode_steps < 0) return fail(MW_EINVAL, "max_episode_steps must be >= 0");
    if (cfg->world_offset < 0) return fail(MW_EINVAL, "world_offset must be >= 0");
    if (!cfg->home_q) return fail(MW_EINVAL, "home_q is null (one value per dof)");
    if (cfg->n_contact_links < 0 || cfg->n_contact_links > mw::kMaxContactLinks)
        return fail(MW_EINVAL, "n_contact_links must be in [0, " + std::to_string(mw::kMaxContactLinks) + "]");
    if (cfg->n_contact_links > 0 && !cfg->contact_links) return fail(MW_EINVAL, "contact_links is null");
    for (int j = 0; j < cfg->n_contact_links; ++j)
        if (cfg->contact_links[j] < -1 || cfg->contact_links[j] >= n)
            return fail(MW_EINVAL, "contact link " + std::to_string(cfg->contact_links[j]) + " out of range [-1, " +
                                       std::to_string(n) + ")");
    {
        const float* hb = cfg->home_base;
        if (!(hb[3] * hb[3] + hb[4] * hb[4] + hb[5] * hb[5] + hb[6] * hb[6] > 0.f))
            return fail(MW_EINVAL, "the home_base orientation quaternion is zero");
    }
    if (!(cfg->joint_noise >= 0.f)) return fail(MW_EINVAL, "joint_noise must be >= 0");
    auto e = std::make_unique<mw_vecenv>();
    e->sim = s;
    e->fenv = std::make_unique<mw::FloatEnv>();
    mw::FloatTaskF& T = e->fenv->ftask;
    T.action_mode = cfg->action_mode;
    T.max_steps = cfg->max_episode_steps;
    T.n_links = cfg->n_contact_links;
    T.n_obs = 13 + 2 * n + cfg->n_contact_links;
    T.seed_lo = static_cast<uint32_t>(cfg->seed);
    T.seed_hi = static_cast<uint32_t>(cfg->seed >> 32);
    T.world_offset = static_cast<uint32_t>(cfg->world_offset);
    T.z_min = cfg->z_min;
    T.cos_tilt_max = cfg->cos_tilt_max;
    T.alive_bonus = cfg->alive_bonus;
    T.w_forward = cfg->w_forward;
    T.w_action = cfg->w_action;
    T.w_pose = cfg->w_pose;
    T.joint_noise = cfg->joint_noise;
    for (int k = 0; k < 7; ++k) T.home_base[k] = cfg->home_base[k];
    for (int d = 0; d < n; ++d) T.home_q[d] = cfg->home_q[d];
    for (int j = 0; j < cfg->n_contact_links; ++j) T.link_slots[j] = link_slots(s, cfg->contact_links[j]);
    e->task.n_obs = T.n_obs;  // mw_vecenv_obs_dim
    MW_HIP(hipSetDevice(s->cfg.device));
    // every dof in Force or Position mode; Position: the JointController runs
    // every physics step (period = step size), as the Panda task sets it
    const bool pos = cfg->action_mode == MW_FLOAT_ACTION_POSITION;
    if ((rc = mw_set_joint_control_mode(s, 0, s->W, nullptr, 0, pos ? MW_MODE_POSITION : MW_MODE_FORCE))) return rc;
    if (pos) s->period_ns = s->dt_ns;
    // flush the modes, targets and gains now: from here on the command block
    // is written on the device only, and a step must find nothing to stage
    if ((rc = run_impl(s, 1, false))) return rc;
    const size_t W = static_cast<size_t>(s->W);
    MW_HIP(mw::dev_alloc_zeroed(e->d_counters, 2 * W * sizeof(uint32_t), s->stream));
    e->dev.episode = static_cast<uint32_t*>(e->d_counters.get());
    e->dev.steps = e->dev.episode + W;
    MW_HIP(mw::dev_alloc_zeroed(e->fenv->d_asq, W * sizeof(float), s->stream));
    s->env_owned = true;
    *out = e.release();
    return MW_OK;
}

// Pushes and friction randomisation of a floating-base env: the post launch
// (and the reset's) fills the wave kernel's wrench array with the next step's
// push, which run_impl then passes on as it is, and draws the friction of
// every episode it resets into the simulator's per-world array.
int mw_floatenv_randomize(mw_vecenv* e, const mw_float_rand_config* cfg, float* push_out, float* friction_out) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_randomize")) return rc;
    if (cfg->push_interval < 0) return fail(MW_EINVAL, "push_interval must be >= 0");
    if (cfg->push_interval > 0 && (cfg->push_steps < 1 || cfg->push_steps > cfg->push_interval))
        return fail(MW_EINVAL, "push_steps must be in [1, push_interval]");
    if (!(cfg->push_force >= 0.f) || !(cfg->push_torque >= 0.f))
        return fail(MW_EINVAL, "push_force and push_torque must be >= 0");
    if (!(cfg->friction_lo >= 0.f) || !(cfg->friction_hi >= cfg->friction_lo))
        return fail(MW_EINVAL, "the friction range needs 0 <= friction_lo <= friction_hi");
    mw_sim* s = e->sim;
    const bool push = cfg->push_interval > 0, friction = cfg->friction_hi > 0.f;
    MW_HIP(hipSetDevice(s->cfg.device));
    if (push && !s->env_wrench)
        if (int rc = alloc_env_wrench(s)) return rc;
    if (friction)
        if (int rc = alloc_ground_friction(s)) return rc;
    mw::FloatRandF& R = e->fenv->ftask.rand;
    R = mw::FloatRandF{};
    if (push) {
        R.push_interval = static_cast<uint32_t>(cfg->push_interval);
        R.push_steps = static_cast<uint32_t>(cfg->push_steps);
        R.push_force = cfg->push_force;
        R.push_torque = cfg->push_torque;
        R.push_out = push_out;
    }
    if (friction) {
        R.friction_lo = cfg->friction_lo;
        R.friction_hi = cfg->friction_hi;
        R.friction_out = friction_out;
        R.mu = s->d_mu.get();
    }
    s->env_wrench = push;
    s->env_friction = friction;
    return MW_OK;
}

// The locomotion task: a per-world velocity command drawn by the post launch,
// the body-frame block of the observation, scaled actions and the tracking /
// smoothness / air-time reward terms, all inside the step's three launches
// (the LOCO instances of float_env_kernel.hip).
int mw_floatenv_locomotion(mw_vecenv* e, const mw_float_loco_config* cfg, float* command_out) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_locomotion")) return rc;
    mw::FloatEnv& F = *e->fenv;
    mw::FloatTaskF& T = F.ftask;
    // it changes the width of the rows, which the noise amplitudes were checked against
    if (T.noise.amp || T.noise.ring)
        return fail(MW_ESTATE, "mw_floatenv_locomotion must be called before mw_floatenv_noise");
    if (T.track.on) return fail(MW_ESTATE, "mw_floatenv_locomotion must be called before mw_floatenv_tracking");
    const float fields[] = {cfg->cmd_lo[0], cfg->cmd_lo[1], cfg->cmd_lo[2], cfg->cmd_hi[0], cfg->cmd_hi[1],
                            cfg->cmd_hi[2], cfg->cmd_zero_prob, cfg->cmd_min, cfg->action_scale, cfg->w_track_lin,
                            cfg->w_track_yaw, cfg->track_sigma, cfg->w_lin_z, cfg->w_ang_xy, cfg->w_action_rate,
                            cfg->w_air_time, cfg->air_time_target, cfg->contact_force_min};
    for (float f : fields)
        if (!std::isfinite(f)) return fail(MW_EINVAL, "every field of mw_float_loco_config must be finite");
    for (int k = 0; k < 3; ++k)
        if (cfg->cmd_hi[k] < cfg->cmd_lo[k]) return fail(MW_EINVAL, "the command ranges need cmd_lo <= cmd_hi");
    if (cfg->cmd_interval < 0) return fail(MW_EINVAL, "cmd_interval must be >= 0");
    if (cfg->cmd_zero_prob < 0.f || cfg->cmd_zero_prob > 1.f) return fail(MW_EINVAL, "cmd_zero_prob must be in [0, 1]");
    if (!(cfg->track_sigma > 0.f)) return fail(MW_EINVAL, "track_sigma must be > 0");
    if (cfg->action_scale < 0.f) return fail(MW_EINVAL, "action_scale must be >= 0");
    if (cfg->w_air_time != 0.f && T.n_links == 0)
        return fail(MW_EINVAL, "the air-time term (w_air_time != 0) needs contact links");
    mw_sim* s = e->sim;
    const size_t W = static_cast<size_t>(s->W), n = static_cast<size_t>(s->n);
    const size_t links = static_cast<size_t>(T.n_links > 0 ? T.n_links : 1);
    MW_HIP(hipSetDevice(s->cfg.device));
    mw::dev_ptr<float[]> prev, rate;
    mw::dev_ptr<uint32_t[]> air;
    MW_HIP(mw::dev_alloc_zeroed(prev, W * n * sizeof(float), s->stream));
    MW_HIP(mw::dev_alloc_zeroed(air, links * W * sizeof(uint32_t), s->stream));
    MW_HIP(mw::dev_alloc_zeroed(rate, W * sizeof(float), s->stream));
    F.d_prev_action = std::move(prev);
    F.d_air_steps = std::move(air);
    F.d_action_rate = std::move(rate);
    mw::FloatLocoF& L = T.loco;
    L = mw::FloatLocoF{};
    L.on = 1u;
    L.cmd_interval = static_cast<uint32_t>(cfg->cmd_interval);
    for (int k = 0; k < 3; ++k) {
        L.cmd_lo[k] = cfg->cmd_lo[k];
        L.cmd_hi[k] = cfg->cmd_hi[k];
    }
    L.cmd_zero_prob = cfg->cmd_zero_prob;
    L.cmd_min = cfg->cmd_min;
    L.action_scale = cfg->action_scale;
    L.w_track_lin = cfg->w_track_lin;
    L.w_track_yaw = cfg->w_track_yaw;
    L.track_sigma = cfg->track_sigma;
    L.w_lin_z = cfg->w_lin_z;
    L.w_ang_xy = cfg->w_ang_xy;
    L.w_action_rate = cfg->w_action_rate;
    L.w_air_time = cfg->w_air_time;
    L.air_time_target = cfg->air_time_target;
    L.contact_force_min = cfg->contact_force_min;
    L.env_dt = static_cast<float>(s->cfg.steps_per_run * s->cfg.step_size);
    L.prev_action = F.d_prev_action.get();
    L.air_steps = F.d_air_steps.get();
    L.action_rate = F.d_action_rate.get();
    L.command_out = command_out;
    T.n_obs = 25 + 3 * s->n + T.n_links;
    e->task.n_obs = T.n_obs;  // mw_vecenv_obs_dim
    return MW_OK;
}

// Inertia randomisation of a floating-base env: the post launch (and the
// reset's) draws the link masses and the base payload of every episode it
// starts into the simulator's per-world link parameters, which the run reads
// (the INERT instances of float_env_kernel.hip).
int mw_floatenv_inertia(mw_vecenv* e, const mw_float_inertia_config* cfg, float* inertial_out, float* draw_out) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_inertia")) return rc;
    const float fields[] = {cfg->mass_scale_lo, cfg->mass_scale_hi, cfg->payload_lo, cfg->payload_hi,
                            cfg->payload_box[0], cfg->payload_box[1], cfg->payload_box[2]};
    for (float f : fields)
        if (!std::isfinite(f)) return fail(MW_EINVAL, "every field of mw_float_inertia_config must be finite");
    const bool scale = cfg->mass_scale_hi > 0.f, payload = cfg->payload_hi > 0.f;
    if (scale ? !(cfg->mass_scale_lo > 0.f && cfg->mass_scale_lo <= cfg->mass_scale_hi)
              : (cfg->mass_scale_lo != 0.f || cfg->mass_scale_hi < 0.f))
        return fail(MW_EINVAL, "the mass scale range needs 0 < mass_scale_lo <= mass_scale_hi (or both 0: off)");
    if (!(cfg->payload_lo >= 0.f) || !(cfg->payload_hi >= cfg->payload_lo))
        return fail(MW_EINVAL, "the payload range needs 0 <= payload_lo <= payload_hi");
    for (int k = 0; k < 3; ++k)
        if (!(cfg->payload_box[k] >= 0.f)) return fail(MW_EINVAL, "payload_box must be >= 0");
    mw_sim* s = e->sim;
    mw::FloatInertiaF& I = e->fenv->ftask.inertia;
    if (!scale && !payload) {  // everything off: the env as it was made
        if (I.wpar) s->env_inertia = false;
        I = mw::FloatInertiaF{};
        return MW_OK;
    }
    MW_HIP(hipSetDevice(s->cfg.device));
    if (int rc = alloc_link_params(s)) return rc;
    I = mw::FloatInertiaF{};
    I.mass_lo = scale ? cfg->mass_scale_lo : 0.f;
    I.mass_hi = scale ? cfg->mass_scale_hi : 0.f;
    I.payload_lo = payload ? cfg->payload_lo : 0.f;
    I.payload_hi = payload ? cfg->payload_hi : 0.f;
    for (int k = 0; k < 3; ++k) I.payload_box[k] = cfg->payload_box[k];
    I.stride = s->wpar_stride;
    std::memcpy(I.base0, &s->h_float.mass, sizeof(I.base0));
    I.wpar = s->d_wpar.get();
    I.inertial_out = inertial_out;
    I.draw_out = draw_out;
    s->env_inertia = true;
    return MW_OK;
}

// Joint randomisation of a floating-base env: the post launch (and the
// reset's) draws the damping, the friction and the effort limit of every
// masked joint for the episode it starts into the same per-world records (the
// JOINT instances of float_env_kernel.hip).  The run kernel's instance follows
// what is drawn: friction needs CONS, damping FloatF::dual (set_joint_dynamics_flags).
int mw_floatenv_joints(mw_vecenv* e, const mw_float_joint_config* cfg, float* joints_out, float* draw_out) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_joints")) return rc;
    const float fields[] = {cfg->damping_lo, cfg->damping_hi, cfg->friction_lo,
                            cfg->friction_hi, cfg->effort_scale_lo, cfg->effort_scale_hi};
    for (float f : fields)
        if (!std::isfinite(f)) return fail(MW_EINVAL, "every field of mw_float_joint_config must be finite");
    if (!(cfg->damping_lo >= 0.f) || !(cfg->damping_hi >= cfg->damping_lo))
        return fail(MW_EINVAL, "the damping range needs 0 <= damping_lo <= damping_hi");
    if (!(cfg->friction_lo >= 0.f) || !(cfg->friction_hi >= cfg->friction_lo))
        return fail(MW_EINVAL, "the joint friction range needs 0 <= friction_lo <= friction_hi");
    const bool damping = cfg->damping_hi > 0.f, friction = cfg->friction_hi > 0.f, effort = cfg->effort_scale_hi > 0.f;
    if (effort ? !(cfg->effort_scale_lo > 0.f && cfg->effort_scale_lo <= cfg->effort_scale_hi)
               : (cfg->effort_scale_lo != 0.f || cfg->effort_scale_hi < 0.f))
        return fail(MW_EINVAL, "the effort scale range needs 0 < effort_scale_lo <= effort_scale_hi (or both 0: off)");
    mw_sim* s = e->sim;
    const uint64_t all = s->n >= 64 ? ~uint64_t{0} : (uint64_t{1} << s->n) - 1u;
    if (cfg->dof_mask & ~all) return fail(MW_EINVAL, "dof_mask names a joint the model does not have");
    mw::FloatEnv& F = *e->fenv;
    mw::FloatJointF& J = F.ftask.joints;
    MW_HIP(hipSetDevice(s->cfg.device));
    if (!damping && !friction && !effort) {  // everything off: the env as it was made
        if (J.wpar) {
            s->env_joints = false;
            J = mw::FloatJointF{};
            return set_joint_dynamics_flags(s, F.joints_saved[0], F.joints_saved[1]);
        }
        return MW_OK;
    }
    if (int rc = alloc_link_params(s)) return rc;
    if (!J.wpar) {
        F.joints_saved[0] = s->wpar_friction;
        F.joints_saved[1] = s->wpar_damping;
    }
    if (int rc = set_joint_dynamics_flags(s, F.joints_saved[0] || friction, F.joints_saved[1] || damping)) return rc;
    J = mw::FloatJointF{};
    J.damping_lo = damping ? cfg->damping_lo : 0.f;
    J.damping_hi = damping ? cfg->damping_hi : 0.f;
    J.friction_lo = friction ? cfg->friction_lo : 0.f;
    J.friction_hi = friction ? cfg->friction_hi : 0.f;
    J.effort_lo = effort ? cfg->effort_scale_lo : 0.f;
    J.effort_hi = effort ? cfg->effort_scale_hi : 0.f;
    J.dof_mask = cfg->dof_mask ? cfg->dof_mask : all;
    J.stride = s->wpar_stride;
    J.wpar = s->d_wpar.get();
    J.joints_out = joints_out;
    J.draw_out = draw_out;
    s->env_joints = true;
    return MW_OK;
}

// Observation noise and action latency of a floating-base env: the post launch
// adds amp[k] u to the words of obs and terminal_obs as it writes them out and
// draws the delay of every episode it starts; the action launch's DELAY
// instance applies the action of that many steps ago from a per-world ring
// (float_env_kernel.hip).
static_assert(mw::kMaxActionDelay == MW_FLOAT_MAX_ACTION_DELAY, "the ring bound of float_task.hpp is the ABI's");
int mw_floatenv_noise(mw_vecenv* e, const mw_float_noise_config* cfg, const float* amplitude, float* clean_obs,
                      float* clean_terminal_obs, int32_t* delay_out) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_noise")) return rc;
    if (cfg->delay_lo < 0 || cfg->delay_hi < cfg->delay_lo || cfg->delay_hi > mw::kMaxActionDelay)
        return fail(MW_EINVAL, "the action delay range needs 0 <= delay_lo <= delay_hi <= " +
                                   std::to_string(mw::kMaxActionDelay));
    mw_sim* s = e->sim;
    mw::FloatEnv& F = *e->fenv;
    mw::FloatTaskF& T = F.ftask;
    const size_t W = static_cast<size_t>(s->W), n = static_cast<size_t>(s->n), NO = static_cast<size_t>(T.n_obs);
    if (amplitude) {
        // the locomotion rows end with the command (3) and the last action (n),
        // the tracking block follows them to the end of the row: never noisy
        const size_t track0 = T.track.on ? static_cast<size_t>(T.track.nb) : NO;
        const size_t exact0 = T.loco.on ? track0 - 3 - n : track0;
        for (size_t k = 0; k < NO; ++k) {
            if (!std::isfinite(amplitude[k]) || amplitude[k] < 0.f)
                return fail(MW_EINVAL, "every noise amplitude must be finite and >= 0 (word " + std::to_string(k) + ")");
            if (k >= track0 && amplitude[k] != 0.f)
                return fail(MW_EINVAL, "the phase, clip and reference words take no noise (word " + std::to_string(k) + ")");
            if (k >= exact0 && amplitude[k] != 0.f)
                return fail(MW_EINVAL, "the command and last-action words take no noise (word " + std::to_string(k) + ")");
        }
    }
    const bool delay = cfg->delay_hi > 0;
    MW_HIP(hipSetDevice(s->cfg.device));
    mw::dev_ptr<float[]> amp, ring;
    mw::dev_ptr<int32_t[]> dl;
    if (amplitude) {
        MW_HIP(mw::dev_alloc(amp, NO * sizeof(float)));
        MW_HIP(hipMemcpy(amp.get(), amplitude, NO * sizeof(float), hipMemcpyHostToDevice));  // complete on return
    }
    if (delay) {
        const size_t words = W * static_cast<size_t>(cfg->delay_hi + 1) * n;
        MW_HIP(mw::dev_alloc_zeroed(ring, words * sizeof(float), s->stream));
        MW_HIP(mw::dev_alloc_zeroed(dl, W * sizeof(int32_t), s->stream));
    }
    F.d_noise_amp = std::move(amp);
    F.d_action_ring = std::move(ring);
    F.d_action_delay = std::move(dl);
    mw::FloatNoiseF& N = T.noise;
    N = mw::FloatNoiseF{};
    if (amplitude) {
        N.amp = F.d_noise_amp.get();
        N.clean_obs = clean_obs;
        N.clean_term_obs = clean_terminal_obs;
    }
    if (delay) {
        N.delay_lo = static_cast<uint32_t>(cfg->delay_lo);
        N.delay_hi = static_cast<uint32_t>(cfg->delay_hi);
        N.ring = F.d_action_ring.get();
        N.delay = F.d_action_delay.get();
        N.steps = e->dev.steps;
        N.delay_out = delay_out;
    }
    return MW_OK;
}

// Shaping rewards, contact termination and episode statistics of a
// floating-base env: one more runtime branch of the post launch
// (float_env_kernel.hip: shape_gather, shape_terms), and in torque mode a
// nullable argument of the action launch.
static_assert(mw::kShapeTerms == MW_FLOAT_SHAPE_TERMS, "the term count of float_task.hpp is the ABI's");
int mw_floatenv_shaping(mw_vecenv* e, const mw_float_shape_config* cfg, float* terms_out, float* torque_out,
                        float* ep_return, int32_t* ep_length, float* ep_terms) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_shaping")) return rc;
    mw_sim* s = e->sim;
    mw::FloatEnv& F = *e->fenv;
    mw::FloatTaskF& T = F.ftask;
    const int n = s->n;
    const float scalars[] = {cfg->base_height_target, cfg->soft_limit,        cfg->collision_force_min,
                             cfg->stumble_ratio,      cfg->max_contact_force, cfg->termination_force};
    bool any = cfg->n_penalised_links != 0 || cfg->n_termination_links != 0;
    for (int k = 0; k < mw::kShapeTerms; ++k) {
        if (!std::isfinite(cfg->weights[k])) return fail(MW_EINVAL, "every field of mw_float_shape_config must be finite");
        if (cfg->weights[k] < 0.f) return fail(MW_EINVAL, "the weights of mw_float_shape_config must be >= 0");
        any = any || cfg->weights[k] != 0.f;
    }
    for (float f : scalars) {
        if (!std::isfinite(f)) return fail(MW_EINVAL, "every field of mw_float_shape_config must be finite");
        any = any || f != 0.f;
    }
    if (cfg->n_penalised_links < 0 || cfg->n_penalised_links > mw::kMaxContactLinks)
        return fail(MW_EINVAL, "n_penalised_links must be in [0, " + std::to_string(mw::kMaxContactLinks) + "]");
    if (cfg->n_termination_links < 0) return fail(MW_EINVAL, "n_termination_links must be >= 0");
    if ((cfg->n_penalised_links > 0 && !cfg->penalised_links) || (cfg->n_termination_links > 0 && !cfg->termination_links))
        return fail(MW_EINVAL, "a link list of mw_float_shape_config is null");
    if (!any) {  // everything off: the env as it was made
        T.shape = mw::FloatShapeF{};
        F.d_shape_qd.reset();
        F.d_shape_cmd.reset();
        F.d_shape_sums.reset();
        F.d_shape_length.reset();
        return MW_OK;
    }
    if (!(cfg->soft_limit > 0.f && cfg->soft_limit <= 1.f)) return fail(MW_EINVAL, "soft_limit must be in (0, 1]");
    if (cfg->collision_force_min < 0.f || cfg->stumble_ratio < 0.f || cfg->max_contact_force < 0.f ||
        cfg->termination_force < 0.f)
        return fail(MW_EINVAL, "collision_force_min, stumble_ratio, max_contact_force and termination_force must be >= 0");
    if (cfg->weights[mw::kShStandStill] != 0.f && !T.loco.on)
        return fail(MW_ESTATE, "the stand_still term needs the locomotion task: call mw_floatenv_locomotion first");
    if (cfg->weights[mw::kShCollision] != 0.f && cfg->n_penalised_links == 0)
        return fail(MW_EINVAL, "the collision term needs penalised links");
    if ((cfg->weights[mw::kShStumble] != 0.f || cfg->weights[mw::kShContactForce] != 0.f) && T.n_links == 0)
        return fail(MW_EINVAL, "the stumble and contact_force terms need contact links (mw_float_task_config)");
    // a link of the lists must exist and own a contact slot: one without could never fire
    auto slots_of = [&](int32_t link, const char* what, uint32_t& slots) {
        if (link < -1 || link >= n)
            return fail(MW_EINVAL, std::string(what) + " link " + std::to_string(link) + " out of range [-1, " +
                                       std::to_string(n) + ")");
        slots = link_slots(s, link);
        if (!slots)
            return fail(MW_EINVAL, std::string(what) + " link " + std::to_string(link) +
                                       " owns no contact slot among the 32 of the contact mask (no collision shape?)");
        return MW_OK;
    };
    uint32_t pen_slots[mw::kMaxContactLinks] = {}, term_slots = 0u;
    for (int j = 0; j < cfg->n_penalised_links; ++j)
        if (int rc = slots_of(cfg->penalised_links[j], "penalised", pen_slots[j])) return rc;
    for (int j = 0; j < cfg->n_termination_links; ++j) {
        uint32_t m = 0u;
        if (int rc = slots_of(cfg->termination_links[j], "termination", m)) return rc;
        term_slots |= m;
    }
    const size_t W = static_cast<size_t>(s->W), nw = static_cast<size_t>(n) * W;
    const bool keep_cmd = T.action_mode == MW_FLOAT_ACTION_TORQUE &&
                          (cfg->weights[mw::kShTorque] != 0.f || cfg->weights[mw::kShPower] != 0.f || torque_out);
    MW_HIP(hipSetDevice(s->cfg.device));
    if (T.track.on && !T.shape.on) {
        // the shaping tiles join the tracking task's in the post launch's local memory
        mw::FloatTaskF grown = T;
        grown.shape.on = 1u;
        if (int rc = check_post_lds(s, grown, "mw_floatenv_shaping")) return rc;
    }
    mw::dev_ptr<float[]> qd, cmd, sums;
    mw::dev_ptr<int32_t[]> len;
    MW_HIP(mw::dev_alloc_zeroed(qd, nw * sizeof(float), s->stream));
    if (keep_cmd) MW_HIP(mw::dev_alloc_zeroed(cmd, nw * sizeof(float), s->stream));
    MW_HIP(mw::dev_alloc_zeroed(sums, (1 + mw::kShapeTerms) * W * sizeof(float), s->stream));
    MW_HIP(mw::dev_alloc_zeroed(len, W * sizeof(int32_t), s->stream));
    F.d_shape_qd = std::move(qd);
    F.d_shape_cmd = std::move(cmd);
    F.d_shape_sums = std::move(sums);
    F.d_shape_length = std::move(len);
    mw::FloatShapeF& H = T.shape;
    H = mw::FloatShapeF{};
    H.on = 1u;
    H.term_slots = term_slots;
    for (int k = 0; k < mw::kShapeTerms; ++k) H.w[k] = cfg->weights[k];
    H.base_height_target = cfg->base_height_target;
    H.collision_force_min = cfg->collision_force_min;
    H.stumble_ratio = cfg->stumble_ratio;
    H.max_contact_force = cfg->max_contact_force;
    H.termination_force = cfg->termination_force;
    H.env_dt = static_cast<float>(s->cfg.steps_per_run * s->cfg.step_size);
    H.n_pen = cfg->n_penalised_links;
    for (int j = 0; j < cfg->n_penalised_links; ++j) H.pen_slots[j] = pen_slots[j];
    for (int d = 0; d < mw::kMaxBodies; ++d) {
        H.soft_lo[d] = -mw::kFtUnbounded;
        H.soft_hi[d] = mw::kFtUnbounded;
        if (d < n) mw::dev::ft_soft_limits(s->h_params.b[d].lower, s->h_params.b[d].upper, cfg->soft_limit, H.soft_lo[d], H.soft_hi[d]);
    }
    H.qd_prev = F.d_shape_qd.get();
    H.cmd_kept = F.d_shape_cmd.get();
    H.terms_out = terms_out;
    H.torque_out = torque_out;
    H.acc_return = F.d_shape_sums.get();
    H.acc_terms = F.d_shape_sums.get() + W;
    H.acc_length = F.d_shape_length.get();
    H.ep_return = ep_return;
    H.ep_length = ep_length;
    H.ep_terms = ep_terms;
    return MW_OK;
}

// Initial-state randomisation and the reset-state bank of a floating-base env:
// one more block-uniform runtime branch of the post launch's reset block
// (float_env_kernel.hip, T.init.on), which draws where an episode starts -- a
// row of the caller's bank or the home row, plus offsets -- into the pending
// resets.  The bank and the two outputs are the caller's; the env's own is a
// copy of the home row in device memory, which the kernel reads as it reads a
// bank row.
int mw_floatenv_init_state(mw_vecenv* e, const mw_float_init_config* cfg, const float* states_dev, float* state_dev,
                           float* draws_dev) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_init_state")) return rc;
    struct Range {
        const float (&lo)[3];
        const float (&hi)[3];
        uint32_t bit;
        const char* name;
    };
    const Range ranges[] = {{cfg->pos_lo, cfg->pos_hi, mw::kInitPos, "pos"},
                            {cfg->rpy_lo, cfg->rpy_hi, mw::kInitRpy, "rpy"},
                            {cfg->lin_vel_lo, cfg->lin_vel_hi, mw::kInitLin, "lin_vel"},
                            {cfg->ang_vel_lo, cfg->ang_vel_hi, mw::kInitAng, "ang_vel"}};
    uint32_t groups = 0u;
    for (const Range& r : ranges)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(r.lo[k]) || !std::isfinite(r.hi[k]))
                return fail(MW_EINVAL, "every field of mw_float_init_config must be finite");
            if (r.lo[k] > r.hi[k])
                return fail(MW_EINVAL, std::string("the ") + r.name + " range needs " + r.name + "_lo <= " + r.name + "_hi");
            if (r.lo[k] != 0.f || r.hi[k] != 0.f) groups |= r.bit;
        }
    if (!std::isfinite(cfg->joint_vel) || !std::isfinite(cfg->state_prob))
        return fail(MW_EINVAL, "every field of mw_float_init_config must be finite");
    if (cfg->joint_vel < 0.f) return fail(MW_EINVAL, "joint_vel must be >= 0");
    if (cfg->state_prob < 0.f || cfg->state_prob > 1.f) return fail(MW_EINVAL, "state_prob must be in [0, 1]");
    if (cfg->n_states < 0) return fail(MW_EINVAL, "n_states must be >= 0");
    if (cfg->n_states > 0 && !states_dev) return fail(MW_EINVAL, "n_states > 0 needs the bank: states_dev is null");
    if (cfg->n_states == 0 && states_dev) return fail(MW_EINVAL, "a bank (states_dev) needs n_states > 0");
    mw_sim* s = e->sim;
    mw::FloatEnv& F = *e->fenv;
    mw::FloatInitF& I = F.ftask.init;
    const bool tracked = F.ftask.track.on != 0u;
    if (tracked && cfg->n_states > 0)
        return fail(MW_EINVAL, "a bank (n_states > 0) cannot be combined with mw_floatenv_tracking: the clips are the bank");
    if (!tracked && !groups && cfg->joint_vel == 0.f && cfg->n_states == 0 && !state_dev && !draws_dev) {
        I = mw::FloatInitF{};  // everything off: the env as it was made
        F.d_init_home.reset();
        return MW_OK;
    }
    MW_HIP(hipSetDevice(s->cfg.device));
    mw::dev_ptr<float[]> home;
    if (int rc = make_home_row(s, F.ftask, home)) return rc;
    F.d_init_home = std::move(home);
    I = mw::FloatInitF{};
    I.on = 1u;
    I.home = F.d_init_home.get();
    I.groups = groups;
    for (int k = 0; k < 3; ++k) {
        I.pos_lo[k] = cfg->pos_lo[k]; I.pos_hi[k] = cfg->pos_hi[k];
        I.rpy_lo[k] = cfg->rpy_lo[k]; I.rpy_hi[k] = cfg->rpy_hi[k];
        I.lin_lo[k] = cfg->lin_vel_lo[k]; I.lin_hi[k] = cfg->lin_vel_hi[k];
        I.ang_lo[k] = cfg->ang_vel_lo[k]; I.ang_hi[k] = cfg->ang_vel_hi[k];
    }
    I.joint_vel = cfg->joint_vel;
    I.state_prob = cfg->state_prob;
    I.n_states = cfg->n_states;
    I.states = states_dev;
    I.state_out = state_dev;
    I.draws_out = draws_dev;
    return MW_OK;
}

// Motion-clip tracking task of a floating-base env: one more block-uniform
// runtime branch of the post launch (float_env_kernel.hip, T.track.on) -- the
// frame clock, the blended reference rows staged through LDS, the five errors
// and terms, the clip-end truncation, the block of the observation -- and, in
// its reset block, the clip row as the base row of init_reset, which this call
// therefore turns on where mw_floatenv_init_state has not.  The clips and the
// four outputs are the caller's; the env's own are the clip table and the joint
// weights in device memory and every world's clip and start frame.
static_assert(mw::kMaxClips == MW_FLOAT_MAX_CLIPS && mw::kTrackTerms == MW_FLOAT_TRACK_TERMS,
              "the clip and term counts of float_task.hpp are the ABI's");
int mw_floatenv_tracking(mw_vecenv* e, const mw_float_track_config* cfg, const float* clips_dev, float* terms_dev,
                         float* errors_dev, int32_t* clip_dev, int32_t* frame_dev) {
    if (int rc = check_configurable(e, cfg, "mw_floatenv_tracking")) return rc;
    mw_sim* s = e->sim;
    mw::FloatEnv& F = *e->fenv;
    mw::FloatTaskF& T = F.ftask;
    // it changes the width of the rows, which the noise amplitudes were checked against
    if (T.noise.amp || T.noise.ring) return fail(MW_ESTATE, "mw_floatenv_tracking must be called before mw_floatenv_noise");
    if (!clips_dev) return fail(MW_EINVAL, "clips_dev is null");
    if (cfg->n_clips < 1 || cfg->n_clips > mw::kMaxClips)
        return fail(MW_EINVAL, "n_clips must be in [1, " + std::to_string(mw::kMaxClips) + "]");
    if (cfg->n_frames < 2) return fail(MW_EINVAL, "n_frames must be >= 2");
    for (int c = 0; c < cfg->n_clips; ++c) {
        if (cfg->clip_length[c] < 2)
            return fail(MW_EINVAL, "clip " + std::to_string(c) + ": the length of a clip must be >= 2");
        if (cfg->clip_first[c] < 0 || cfg->clip_length[c] > cfg->n_frames ||
            cfg->clip_first[c] > cfg->n_frames - cfg->clip_length[c])
            return fail(MW_EINVAL, "clip " + std::to_string(c) + " does not lie inside the n_frames rows of clips_dev");
    }
    if (cfg->frame_num < 1 || cfg->frame_den < 1) return fail(MW_EINVAL, "frame_num and frame_den must be >= 1");
    const int n = s->n;
    auto bad = [](float f) { return !std::isfinite(f) || f < 0.f; };
    for (int k = 0; k < mw::kTrackTerms; ++k)
        if (bad(cfg->weights[k]) || bad(cfg->scales[k]))
            return fail(MW_EINVAL, "the weights and scales of mw_float_track_config must be finite and >= 0");
    if (bad(cfg->ang_scale) || bad(cfg->max_pose) || bad(cfg->max_root_pos) || bad(cfg->max_root_rot))
        return fail(MW_EINVAL, "ang_scale, max_pose, max_root_pos and max_root_rot must be finite and >= 0");
    if (!(cfg->rsi_prob >= 0.f && cfg->rsi_prob <= 1.f)) return fail(MW_EINVAL, "rsi_prob must be in [0, 1]");
    std::vector<float> wj(static_cast<size_t>(n), 1.f);
    if (cfg->joint_weights)
        for (int d = 0; d < n; ++d) {
            if (bad(cfg->joint_weights[d])) return fail(MW_EINVAL, "every joint weight must be finite and >= 0");
            wj[d] = cfg->joint_weights[d];
        }
    if (T.init.n_states > 0)
        return fail(MW_EINVAL, "mw_floatenv_tracking cannot be combined with a bank of mw_floatenv_init_state (n_states > "
                               "0): the clips are the bank");
    // the block goes behind the rows as they are; a second call replaces the first
    const int32_t nb = T.track.on ? T.track.nb : T.n_obs;
    const int32_t n_obs = nb + 3 + (cfg->obs_reference ? n : 0);
    mw::FloatTaskF grown = T;
    grown.n_obs = n_obs;
    grown.track.on = 1u;
    MW_HIP(hipSetDevice(s->cfg.device));
    if (int rc = check_post_lds(s, grown, "mw_floatenv_tracking")) return rc;
    std::vector<int32_t> table(static_cast<size_t>(cfg->n_clips) * mw::kTrackTableWords, 0);
    for (int c = 0; c < cfg->n_clips; ++c) {
        table[c * mw::kTrackTableWords] = cfg->clip_first[c];
        table[c * mw::kTrackTableWords + 1] = cfg->clip_length[c];
        table[c * mw::kTrackTableWords + 2] = cfg->clip_loop[c] ? 1 : 0;
    }
    const size_t W = static_cast<size_t>(s->W);
    mw::dev_ptr<int32_t[]> d_table, d_state;
    mw::dev_ptr<float[]> d_wj, home;
    MW_HIP(mw::dev_alloc(d_table, table.size() * sizeof(int32_t)));
    MW_HIP(mw::dev_alloc(d_wj, wj.size() * sizeof(float)));
    MW_HIP(mw::dev_alloc_zeroed(d_state, 2 * W * sizeof(int32_t), s->stream));
    if (!T.init.on)
        if (int rc = make_home_row(s, T, home)) return rc;
    MW_HIP(hipMemcpy(d_table.get(), table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    MW_HIP(hipMemcpy(d_wj.get(), wj.data(), wj.size() * sizeof(float), hipMemcpyHostToDevice));  // complete on return
    F.d_track_table = std::move(d_table);
    F.d_track_wj = std::move(d_wj);
    F.d_track_state = std::move(d_state);
    if (!T.init.on) {
        // the reset goes through init_reset: no offsets, no outputs, the home row for its pointer
        F.d_init_home = std::move(home);
        T.init = mw::FloatInitF{};
        T.init.on = 1u;
        T.init.home = F.d_init_home.get();
        T.init.state_prob = 1.f;
    }
    mw::FloatTrackF& K = T.track;
    K = mw::FloatTrackF{};
    K.on = 1u;
    K.n_clips = cfg->n_clips;
    K.frame_num = cfg->frame_num;
    K.frame_den = cfg->frame_den;
    K.obs_reference = cfg->obs_reference ? 1 : 0;
    K.nb = nb;
    K.rsi_prob = cfg->rsi_prob;
    K.ang_scale = cfg->ang_scale;
    for (int k = 0; k < mw::kTrackTerms; ++k) {
        K.weight[k] = cfg->weights[k];
        K.scale[k] = cfg->scales[k];
    }
    K.max_pose = cfg->max_pose;
    K.max_root_pos = cfg->max_root_pos;
    K.max_root_rot = cfg->max_root_rot;
    K.clips = clips_dev;
    K.table = F.d_track_table.get();
    K.wj = F.d_track_wj.get();
    K.clip = F.d_track_state.get();
    K.f0 = F.d_track_state.get() + W;
    K.terms_out = terms_dev;
    K.errors_out = errors_dev;
    K.clip_out = clip_dev;
    K.frame_out = frame_dev;
    T.n_obs = n_obs;
    e->task.n_obs = T.n_obs;  // mw_vecenv_obs_dim
    return MW_OK;
}

}  // extern "C"

// The effort word the next run clamps with: the world's record where the
// simulator has per-world link parameters (the pointer and stride RunArgs::wpar
// gets), else the shared model's.
static void shaping_effort(mw_vecenv* e) {
    mw_sim* s = e->sim;
    mw::FloatShapeF& H = e->fenv->ftask.shape;
    if (s->d_wpar) {
        H.effort = s->d_wpar.get() + mw::kWparBody0 + mw::kBodyEffort;
        H.effort_stride = s->wpar_stride;
    } else {
        H.effort = reinterpret_cast<const float*>(s->d_params.get()) + mw::kWparHeadWords + mw::kBodyEffort;
        H.effort_stride = 0;
    }
}

int floatenv_reset(mw_vecenv* e, float* obs) {
    mw_sim* s = e->sim;
    mw::FloatEnv& F = *e->fenv;
    F.was_reset = true;
    MW_HIP(mw::launch_float_env_post(s->d_params.get(), F.ftask, s->dev, s->fdev, e->dev, F.d_asq.get(), obs, nullptr,
                                     nullptr, nullptr, s->n, s->W, 1, s->stream));
    // a paused run applies the pending resets: the state (and the host
    // getters) show the reset at once
    return run_impl(s, 1, false);
}

int floatenv_step(mw_vecenv* e, const void* a, float* o, float* r, uint8_t* d, float* to) {
    mw_sim* s = e->sim;
    mw::FloatEnv& F = *e->fenv;
    const bool pos = F.ftask.action_mode == MW_FLOAT_ACTION_POSITION;
    MW_HIP(mw::launch_float_env_action(F.ftask, static_cast<const float*>(a), pos ? s->dev.ptgt : s->dev.cmd,
                                       F.d_asq.get(), s->dev.div, s->dev.ndiv, s->n, s->W, s->stream));
    if (pos) s->ptgt_stale = true;  // the host mirror of the targets re-reads the device copy
    if (int rc = run_impl(s, 0, false)) return rc;
    if (F.ftask.shape.on) shaping_effort(e);
    MW_HIP(mw::launch_float_env_post(s->d_params.get(), F.ftask, s->dev, s->fdev, e->dev, F.d_asq.get(), o, r, d, to,
                                     s->n, s->W, 0, s->stream));
    return MW_OK;
}

void floatenv_release(mw_vecenv* e) {
    mw_sim* s = e->sim;
    if (!s) return;
    s->env_owned = false;
    s->env_wrench = false;
    if (s->env_friction) {
        // the simulator keeps the last episode's coefficients: its host mirror takes them over
        (void)hipSetDevice(s->cfg.device);
        (void)pull_ground_friction(s);
        s->env_friction = false;
    }
    if (s->env_wpar()) {
        // ... and the last episode's link parameters (inertial and joint
        // words of one record); wpar_friction / wpar_damping stay as the
        // env set them: the records keep the drawn words
        (void)hipSetDevice(s->cfg.device);
        (void)pull_link_params(s);
        s->env_inertia = false;
        s->env_joints = false;
    }
}
