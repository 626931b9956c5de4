// vecenv_state.hpp -- the env behind an mw_vecenv handle, shared by the
// fixed-base envs (vecenv.cpp) and the floating-base env (floatenv.cpp).
// Internal, host only.
#pragma once

#include <memory>

#include "float_task.hpp"
#include "sim_state.hpp"

namespace mw {

// What mw_floatenv_create and the configure calls add to an env.
struct FloatEnv {
    FloatTaskF ftask{};
    dev_ptr<float[]> d_asq;  // sum a^2 per world
    bool was_reset = false;  // mw_vecenv_reset ran: the configure calls come too late
    // joint randomisation (mw_floatenv_joints): the simulator's wpar_friction /
    // wpar_damping before the first call turned the feature on
    bool joints_saved[2] = {false, false};
    // locomotion task (mw_floatenv_locomotion): the kept action rows [W][n], the
    // air-time counters [n_links][W] and the action-rate sums [W]
    dev_ptr<float[]> d_prev_action;
    dev_ptr<uint32_t[]> d_air_steps;
    dev_ptr<float[]> d_action_rate;
    // observation noise and action latency (mw_floatenv_noise): the amplitudes
    // [n_obs], the ring of raw actions [W][delay_hi + 1][n] and the episodes'
    // delays [W]
    dev_ptr<float[]> d_noise_amp;
    dev_ptr<float[]> d_action_ring;
    dev_ptr<int32_t[]> d_action_delay;
    // shaping rewards and episode statistics (mw_floatenv_shaping): qd of the
    // last step [n][W], in torque mode the command the action launch stored
    // [n][W], and the running sums of the current episodes: return [W] then
    // terms [10][W] in one buffer, length [W]
    dev_ptr<float[]> d_shape_qd;
    dev_ptr<float[]> d_shape_cmd;
    dev_ptr<float[]> d_shape_sums;
    dev_ptr<int32_t[]> d_shape_length;
    // initial-state randomisation (mw_floatenv_init_state): the home row [13 + 2 n]
    dev_ptr<float[]> d_init_home;
    // motion-clip tracking (mw_floatenv_tracking): the clip table [n_clips][4],
    // the per-joint weights [n], and clip then start frame of every world's
    // current episode [2][W]
    dev_ptr<int32_t[]> d_track_table;
    dev_ptr<float[]> d_track_wj;
    dev_ptr<int32_t[]> d_track_state;
};

}  // namespace mw

struct mw_vecenv {
    mw_sim* sim = nullptr;
    mw_task_config cfg{};
    mw::TaskF task{};
    mw::VecDev dev{};
    mw::dev_ptr<void> d_counters;
    mw::dev_ptr<void> d_physics;  // per-world randomised masses + gravity
    // lane-group Panda kernel: per-dof PID gains + reset pose (device), and
    // the host copy last uploaded
    mw::dev_ptr<mw::GLaneTask[]> d_lane;
    mw::GLaneTask h_lane[mw::kMaxKernelDofs] = {};
    bool lane_uploaded = false;
    // set by mw_floatenv_create: the env is a floating-base one
    std::unique_ptr<mw::FloatEnv> fenv;

    // the env's work (on its simulator's stream) drains before the members release their buffers
    ~mw_vecenv() { if (sim && sim->stream) (void)hipStreamSynchronize(sim->stream); }
};

// floatenv.cpp: what the handle's shared calls (vecenv.cpp) do for an env with fenv
int floatenv_reset(mw_vecenv* e, float* obs);
int floatenv_step(mw_vecenv* e, const void* a, float* o, float* r, uint8_t* d, float* to);
// mw_vecenv_destroy: the simulator takes back what the env owned
void floatenv_release(mw_vecenv* e);
