// Test-only host build of the locomotion task's arithmetic
// (gym-ignition_amd/csrc/float_task.hpp: ft_projected_gravity, ft_loco_reward
// on top of ft_reward, ft_cmd_index / ft_cmd_block / ft_cmd_is_zero /
// ft_command, ft_air_step): what the env kernels run per world, on the CPU in
// float32, so tests/test_float_loco_host.py can compare it with numpy fp64
// without a GPU.  Not part of the product.
#define MW_HOST_TEST 1
#include "float_task.hpp"

using namespace mw;

// par = {cmd_lo[3], cmd_hi[3], cmd_zero_prob, cmd_min, w_track_lin, w_track_yaw, track_sigma, w_lin_z, w_ang_xy,
//        w_action_rate, w_air_time, air_time_target, contact_force_min, env_dt,
//        alive_bonus, w_forward, w_action, w_pose}  (22 values)
static void fill(FloatTaskF& T, const float* par) {
    FloatLocoF& L = T.loco;
    L.on = 1u;
    for (int k = 0; k < 3; ++k) {
        L.cmd_lo[k] = par[k];
        L.cmd_hi[k] = par[3 + k];
    }
    L.cmd_zero_prob = par[6];
    L.cmd_min = par[7];
    L.w_track_lin = par[8];
    L.w_track_yaw = par[9];
    L.track_sigma = par[10];
    L.w_lin_z = par[11];
    L.w_ang_xy = par[12];
    L.w_action_rate = par[13];
    L.w_air_time = par[14];
    L.air_time_target = par[15];
    L.contact_force_min = par[16];
    L.env_dt = par[17];
    T.alive_bonus = par[18];
    T.w_forward = par[19];
    T.w_action = par[20];
    T.w_pose = par[21];
}

extern "C" unsigned fl_cmd_block(unsigned k) { return dev::ft_cmd_block(k); }
extern "C" unsigned fl_cmd_index(unsigned t, unsigned interval) { return dev::ft_cmd_index(t, interval); }

// count draws of four Philox words: cmd [count][3] and zero [count]
extern "C" void fl_commands(int count, const float* par, const unsigned* words, float* cmd, unsigned char* zero) {
    FloatTaskF T{};
    fill(T, par);
    for (int i = 0; i < count; ++i) {
        const uint32_t r[4] = {words[4 * i], words[4 * i + 1], words[4 * i + 2], words[4 * i + 3]};
        float c[3];
        dev::ft_command(T.loco, r, c);
        for (int k = 0; k < 3; ++k) cmd[3 * i + k] = c[k];
        zero[i] = dev::ft_cmd_is_zero(r[3], T.loco.cmd_zero_prob) ? 1 : 0;
    }
}

// count states: base [count][13], q / a / a_prev [count][n], cmd [count][3], air_pay [count], terminated [count];
// out: gravity [count][3], reward [count] -- the action kernel's sums and the post kernel's reward
extern "C" int fl_eval(int count, int n, const float* par, const float* base, const float* q, const float* a,
                       const float* a_prev, const float* home, const float* cmd, const float* air_pay,
                       const unsigned char* terminated, float* gravity, float* reward) {
    if (n < 0 || n > kMaxBodies) return 1;
    FloatTaskF T{};
    fill(T, par);
    for (int d = 0; d < n; ++d) T.home_q[d] = home[d];
    float diff[kMaxBodies];
    for (int i = 0; i < count; ++i) {
        float b[13], lin[3], ang[3], g[3];
        for (int k = 0; k < 13; ++k) b[k] = base[13 * i + k];
        dev::ft_world_velocity(b, lin, ang);
        dev::ft_projected_gravity(b[3], b[4], b[5], b[6], g);
        for (int k = 0; k < 3; ++k) gravity[3 * i + k] = g[k];
        const size_t o = static_cast<size_t>(i) * n;
        for (int d = 0; d < n; ++d) diff[d] = a[o + d] - a_prev[o + d];
        const float plain = dev::ft_reward(T, terminated[i] != 0, lin[0], dev::ft_sum_sq(a + o, n, 1),
                                           dev::ft_sum_sq_diff(q + o, 1, T.home_q, n));
        const float c[3] = {cmd[3 * i], cmd[3 * i + 1], cmd[3 * i + 2]};
        const float v[3] = {b[10], b[11], b[12]}, w[3] = {b[7], b[8], b[9]};
        reward[i] = dev::ft_loco_reward(T.loco, plain, c, v, w, dev::ft_sum_sq(diff, n, 1), air_pay[i]);
    }
    return 0;
}

// one link over `steps` steps: fz [steps] -> the counter after every step, the steps flown where the step is a
// touchdown (0 elsewhere) and the payment of every step
extern "C" void fl_air(int steps, const float* par, const float* fz, unsigned* counter, unsigned* flown, float* pay) {
    FloatTaskF T{};
    fill(T, par);
    uint32_t air = 0u;
    for (int t = 0; t < steps; ++t) {
        const uint32_t before = air;
        pay[t] = dev::ft_air_step(T.loco, fz[t], air);
        counter[t] = air;
        flown[t] = (air == 0u) ? before : 0u;
    }
}
