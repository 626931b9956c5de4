// vecenv.cpp -- the batched envs of the C ABI (include/mwstep.h, mw_vecenv_*):
// task kernels around a simulator's device state (vecenv_kernel.hip,
// group_kernel.hip).  The fixed-base tasks live here; a floating-base env
// (floatenv.cpp) shares the handle and is reached through floatenv_reset,
// floatenv_step and floatenv_release alone.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "errors.hpp"
#include "vecenv_state.hpp"

using mw::fail;

extern "C" {

int mw_vecenv_create(mw_sim* s, const mw_task_config* cfg, mw_vecenv** out) {
    int rc = check_sim(s);
    if (rc) return rc;
    if (!cfg || !out) return fail(MW_EINVAL, "null argument");
    *out = nullptr;
    const int n = s->n;
    // the batched env kernels step fixed-base chains only: a floating model
    // with a matching dof count would have its base and contacts ignored
    if (s->floating) return fail(MW_EINVAL, "the batched env tasks need a fixed-base model");
    // ... and a compiled chain topology: a generic fixed tree (wave kernel) or
    // a branched 1-2 dof model would be stepped as a serial chain
    if (s->fixed_tree || s->topo < 0)
        return fail(MW_EINVAL, "the batched env tasks need a serial-chain model (or the shipped Panda tree)");
    const bool cart = cfg->kind >= MW_TASK_CARTPOLE_DISCRETE && cfg->kind <= MW_TASK_CARTPOLE_CONTINUOUS_SWINGUP;
    const bool pidtask = cfg->kind == MW_TASK_PANDA_POSITION_TRACKING;
    if (cart && n != 2) return fail(MW_EINVAL, "CartPole tasks need the 2-dof cartpole model");
    if (cfg->kind == MW_TASK_PENDULUM_SWINGUP && n != 1) return fail(MW_EINVAL, "PendulumSwingUp needs the 1-dof pendulum model");
    if (pidtask && (n != 9 || s->topo != 1))
        return fail(MW_EINVAL, "PandaPositionTracking needs the 9-dof Panda model");
    if (pidtask && s->cfg.steps_per_run > 64) return fail(MW_EINVAL, "steps_per_run must be <= 64");
    if (!cart && !pidtask && cfg->kind != MW_TASK_PENDULUM_SWINGUP) return fail(MW_EINVAL, "unknown task kind");
    auto e = std::make_unique<mw_vecenv>();
    e->sim = s;
    e->cfg = *cfg;
    mw::TaskF& T = e->task;
    T.kind = cfg->kind;
    T.max_steps = cfg->max_episode_steps;
    T.reward_cart_at_center = cfg->reward_cart_at_center;
    T.n_obs = (cfg->kind == MW_TASK_PENDULUM_SWINGUP) ? 3 : (pidtask ? 2 * n : 4);
    T.seed_lo = static_cast<uint32_t>(cfg->seed);
    T.seed_hi = static_cast<uint32_t>(cfg->seed >> 32);
    if (cfg->world_offset < 0) return fail(MW_EINVAL, "world_offset must be >= 0");
    T.world_offset = static_cast<uint32_t>(cfg->world_offset);
    T.force_mag = 20.0f;  // cartpole_discrete_balancing.py:32
    const double pi = 3.14159265358979323846;
    switch (cfg->kind) {
    case MW_TASK_CARTPOLE_DISCRETE:
    case MW_TASK_CARTPOLE_CONTINUOUS_BALANCING:
        T.x_factor = (cfg->kind == MW_TASK_CARTPOLE_DISCRETE) ? 0.9f : 1.0f;
        T.hi[0] = 2.4f; T.hi[1] = 20.0f;
        T.hi[2] = static_cast<float>(12.0 * pi / 180.0);
        T.hi[3] = static_cast<float>(3.0 * 360.0 * pi / 180.0);
        break;
    case MW_TASK_CARTPOLE_CONTINUOUS_SWINGUP:
        T.x_factor = 0.8f;
        T.hi[0] = 2.4f; T.hi[1] = 20.0f;
        T.hi[2] = static_cast<float>(5.0 * 360.0 * pi / 180.0);
        T.hi[3] = static_cast<float>(3.0 * 360.0 * pi / 180.0);
        break;
    case MW_TASK_PENDULUM_SWINGUP:
        T.x_factor = 0.f;
        T.hi[0] = 1.f; T.hi[1] = 1.f; T.hi[2] = 10.f; T.hi[3] = 0.f;
        break;
    case MW_TASK_PANDA_POSITION_TRACKING: {
        // the Panda wrapper's initial configuration (models/panda.py:41-44) with
        // joints 1 and 6 at mid-range as test_pid_controllers.py:49-59 sets them
        // (so the config-4 sinusoids stay inside the limits) and the fingers
        // half open: no joint starts on a position limit
        const double wrapper[7] = {0.0, -0.785, 0.0, -2.356, 0.0, 1.571, 0.785};
        for (int d = 0; d < n; ++d) {
            const mw::ChainBody& b = s->model.bodies[d];
            double h = (d < 7) ? wrapper[d] : 0.5 * (b.lower + b.upper);
            if (d == 0 || d == 5) h = 0.5 * (b.lower + b.upper);
            T.home[d] = static_cast<float>(h);
        }
        T.home_noise = 0.05f;
        break;
    }
    }
    if (cfg->randomize & ~(MW_RAND_MASS | MW_RAND_GRAVITY)) return fail(MW_EINVAL, "unknown randomisation bits");
    if (cfg->randomize && pidtask) return fail(MW_EINVAL, "randomisation is available for the CartPole / Pendulum tasks");
    if ((cfg->randomize & MW_RAND_MASS) && !(cfg->mass_high >= cfg->mass_low))
        return fail(MW_EINVAL, "mass_high must be >= mass_low");
    if ((cfg->randomize & MW_RAND_GRAVITY) && !(cfg->gravity_std >= 0.f))
        return fail(MW_EINVAL, "gravity_std must be >= 0");
    T.randomize = cfg->randomize;
    T.mass_lo = cfg->mass_low;
    T.mass_hi = cfg->mass_high;
    T.g_mean = cfg->gravity_mean;
    T.g_std = cfg->gravity_std;
    {
        // the world z axis in the base frame: R_base^T e_z
        const auto& R = s->model.base_R;
        for (int k = 0; k < 3; ++k) T.gdir[k] = static_cast<float>(R[6 + k]);
    }
    MW_HIP(hipSetDevice(s->cfg.device));
    if (cfg->randomize) {
        const size_t bytes = (static_cast<size_t>(n) + 1) * s->W * sizeof(float);
        MW_HIP(mw::dev_alloc_zeroed(e->d_physics, bytes, s->stream));
        e->dev.rmass = static_cast<float*>(e->d_physics.get());
        e->dev.rgz = e->dev.rmass + static_cast<size_t>(n) * s->W;
    }
    MW_HIP(mw::dev_alloc_zeroed(e->d_counters, 2 * static_cast<size_t>(s->W) * sizeof(uint32_t), s->stream));
    e->dev.episode = static_cast<uint32_t*>(e->d_counters.get());
    e->dev.steps = e->dev.episode + s->W;
    if (pidtask) {
        // the JointController runs every physics step (period = step size);
        // set last: a failed create leaves the simulator as it was
        s->period_ns = s->dt_ns;
        s->controller = true;
        s->pid_reset_dofs = 0;  // the controller state is still all zero
    }
    *out = e.release();
    return MW_OK;
}

void mw_vecenv_destroy(mw_vecenv* e) {
    if (!e) return;
    if (e->fenv) floatenv_release(e);
    delete e;
}

int mw_vecenv_obs_dim(const mw_vecenv* e, int32_t* n) {
    if (!e || !n) return fail(MW_EINVAL, "null argument");
    *n = e->task.n_obs;
    return MW_OK;
}

int mw_vecenv_reset(mw_vecenv* e, float* obs) {
    if (!e || !obs) return fail(MW_EINVAL, "null argument");
    if (e->fenv) return floatenv_reset(e, obs);
    mw_sim* s = e->sim;
    MW_HIP(mw::launch_vecenv_reset(s->d_params.get(), s->n, e->task, s->dev, e->dev, obs, s->W, s->stream));
    if (e->task.kind == MW_TASK_PANDA_POSITION_TRACKING) s->pid_reset_dofs = 0;  // the reset zeroed every PID
    s->host_stale = true;
    return MW_OK;
}

static int vec_common(mw_vecenv* e, int32_t T, const void* a, float* o, float* r, uint8_t* d, float* to) {
    if (!e || !a || !o || !r || !d || !to) return fail(MW_EINVAL, "null argument");
    if (e->fenv) {
        if (T > 0) return fail(MW_EINVAL, "the fused rollout is not available for floating-base envs");
        return floatenv_step(e, a, o, r, d, to);
    }
    if (e->task.n_obs == 4 &&
        ((reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(to)) & 15u))
        return fail(MW_EINVAL, "obs buffers must be 16-byte aligned");
    mw_sim* s = e->sim;
    if (e->task.kind == MW_TASK_PANDA_POSITION_TRACKING) {
        if (T > 0) return fail(MW_EINVAL, "the fused rollout is not available for position-target tasks");
        if (s->pid_reset_dofs) {
            // Joint::setPID stores a new ignition::math::PID (Joint.cpp:479-525):
            // the controller of a dof whose gains changed since the last step
            // starts from a reset state.  mw_run does this through the reset
            // flags, which the env kernels do not read.
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            MW_HIP(hipStreamIsCapturing(s->stream, &cap));
            if (cap != hipStreamCaptureStatusNone)
                return fail(MW_ESTATE, "a PID reset after mw_set_joint_pid cannot be captured into a graph: "
                                       "step once before capturing");
            const size_t row = static_cast<size_t>(s->W) * sizeof(float);
            for (int d = 0; d < s->n && d < 64; ++d) {
                if (!((s->pid_reset_dofs >> d) & 1u)) continue;
                MW_HIP(hipMemsetAsync(s->dev.pid_e + static_cast<size_t>(d) * s->W, 0, row, s->stream));
                MW_HIP(hipMemsetAsync(s->dev.pid_i + static_cast<size_t>(d) * s->W, 0, row, s->stream));
                MW_HIP(hipMemsetAsync(s->dev.pid_u + static_cast<size_t>(d) * s->W, 0, row, s->stream));
                for (int32_t w = 0; w < s->W; ++w) s->hrflag()[s->idx(d, w)] &= static_cast<uint8_t>(~4u);
            }
            s->pid_reset_dofs = 0;
        }
        // one world per 16-lane row (group_kernel.hip) unless
        // MWSTEP_PANDA_KERNEL=lane asks for the one-world-per-lane kernel
        const char* kk = std::getenv("MWSTEP_PANDA_KERNEL");
        if (kk && std::strcmp(kk, "lane") == 0) {
            MW_HIP(mw::launch_vecenv_pid_step(s->d_params.get(), s->n, s->topo, needs_cons(s), needs_dual(s),
                                              baked_id(s), e->task, s->dev, e->dev, pid_set(s),
                                              static_cast<const float*>(a), o, r, d, to, s->W,
                                              static_cast<float>(s->cfg.step_size), s->cfg.steps_per_run,
                                              s->cfg.pgs_iters, s->stream));
        } else {
            // per-dof gains and reset pose: uploaded when they change (a
            // pageable copy, complete when the call returns; never inside a
            // captured step, where the gains are fixed)
            const mw::PidSet ps = pid_set(s);
            mw::GLaneTask lt[mw::kMaxKernelDofs] = {};
            for (int k = 0; k < s->n; ++k) {
                lt[k].pid = ps.g[k];
                lt[k].home = e->task.home[k];
            }
            if (!e->d_lane) MW_HIP(mw::dev_alloc(e->d_lane, sizeof(lt)));
            if (!e->lane_uploaded || std::memcmp(lt, e->h_lane, sizeof(lt)) != 0) {
                std::memcpy(e->h_lane, lt, sizeof(lt));
                MW_HIP(hipMemcpyAsync(e->d_lane.get(), e->h_lane, sizeof(lt), hipMemcpyHostToDevice, s->stream));
                e->lane_uploaded = true;
            }
            MW_HIP(mw::launch_vecenv_pid_group(s->d_params.get(), s->n, needs_cons(s), needs_dual(s), e->task, s->dev,
                                               e->dev, e->d_lane.get(), static_cast<const float*>(a), o, r, d, to, s->W,
                                               static_cast<float>(s->cfg.step_size), s->cfg.steps_per_run,
                                               s->cfg.pgs_iters, s->stream));
        }
        s->host_stale = true;
        s->iterations += s->cfg.steps_per_run;
        s->stepped = true;
        return MW_OK;
    }
    MW_HIP(mw::launch_vecenv_step(s->d_params.get(), s->n, needs_cons(s), needs_dual(s), baked_id(s), e->task, s->dev,
                                  e->dev, a, o, r, d, to, s->W, static_cast<float>(s->cfg.step_size),
                                  s->cfg.steps_per_run, s->cfg.pgs_iters, T, s->stream));
    s->host_stale = true;
    s->iterations += static_cast<int64_t>(s->cfg.steps_per_run) * (T > 0 ? T : 1);
    s->stepped = true;
    return MW_OK;
}

int mw_vecenv_step(mw_vecenv* e, const void* a, float* o, float* r, uint8_t* d, float* to) {
    return vec_common(e, 0, a, o, r, d, to);
}

int mw_vecenv_rollout(mw_vecenv* e, int32_t T, const void* a, float* o, float* r, uint8_t* d, float* to) {
    if (T <= 0) return fail(MW_EINVAL, "T must be positive");
    return vec_common(e, T, a, o, r, d, to);
}

int mw_vecenv_physics(mw_vecenv* e, float* mass, float* gz) {
    if (!e || !mass || !gz) return fail(MW_EINVAL, "null argument");
    if (!e->d_physics) return fail(MW_ESTATE, "the env was created without physics randomisation");
    const size_t nw = static_cast<size_t>(e->sim->n) * e->sim->W;
    MW_HIP(hipMemcpyAsync(mass, e->dev.rmass, nw * sizeof(float), hipMemcpyDeviceToDevice, e->sim->stream));
    MW_HIP(hipMemcpyAsync(gz, e->dev.rgz, e->sim->W * sizeof(float), hipMemcpyDeviceToDevice, e->sim->stream));
    return MW_OK;
}

int mw_vecenv_counters(mw_vecenv* e, uint32_t* episode, uint32_t* steps) {
    if (!e || !episode || !steps) return fail(MW_EINVAL, "null argument");
    const size_t bytes = static_cast<size_t>(e->sim->W) * sizeof(uint32_t);
    MW_HIP(hipMemcpyAsync(episode, e->dev.episode, bytes, hipMemcpyDeviceToDevice, e->sim->stream));
    MW_HIP(hipMemcpyAsync(steps, e->dev.steps, bytes, hipMemcpyDeviceToDevice, e->sim->stream));
    return MW_OK;
}

}  // extern "C"
