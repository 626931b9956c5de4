// Test-only host build of the arithmetic of the shaping rewards, the contact
// termination and the episode statistics (gym-ignition_amd/csrc/float_task.hpp:
// ft_soft_limits, ft_shape_tau, ft_shape_dof, ft_shape_contact,
// ft_shape_collision, ft_shape_slot_hit, ft_shape_combine, ft_shape_x,
// ft_shape_terms, ft_shape_reward, ft_shape_stats): what the post kernel runs
// per world, on the CPU in float32 and in the kernel's order of summation, so
// tests/test_float_shape_host.py can compare it with numpy fp64 and
// tests/test_gpu_float_shape.py with the device's words.  Not part of the
// product.
#define MW_HOST_TEST 1
#include "float_task.hpp"

using namespace mw;

extern "C" int fs_terms() { return kShapeTerms; }
extern "C" int fs_lanes() { return kShapeLanes; }
extern "C" int fs_max_links() { return kMaxContactLinks; }

extern "C" void fs_soft_limits(int n, const float* lower, const float* upper, float soft, float* lo, float* hi) {
    for (int d = 0; d < n; ++d) dev::ft_soft_limits(lower[d], upper[d], soft, lo[d], hi[d]);
}

extern "C" void fs_tau(int count, const float* u, const float* effort, float* tau) {
    for (int i = 0; i < count; ++i) tau[i] = dev::ft_shape_tau(u[i], effort[i]);
}

// par: weights[10], base_height_target, collision_force_min, stumble_ratio,
// max_contact_force, termination_force, env_dt
static FloatShapeF shape_of(const float* par) {
    FloatShapeF H{};
    H.on = 1u;
    for (int k = 0; k < kShapeTerms; ++k) H.w[k] = par[k];
    H.base_height_target = par[10];
    H.collision_force_min = par[11];
    H.stumble_ratio = par[12];
    H.max_contact_force = par[13];
    H.termination_force = par[14];
    H.env_dt = par[15];
    return H;
}

// One world's ten terms and its ten x, in the post kernel's order: dof d,
// contact link j and penalised link j go to partial d % 4 / j % 4, the
// partials are added in order.  tau, q, qd, qd_prev, lo, hi, home: [n];
// contact_f [n_links][3] and pen_f [n_pen][3] the links' summed force vectors;
// pose: x y z qw qx qy qz.
extern "C" void fs_world(const float* par, int n, const float* tau, const float* q, const float* qd,
                         const float* qd_prev, const float* lo, const float* hi, const float* home, int n_links,
                         const float* contact_f, int n_pen, const float* pen_f, const float* pose, int standing,
                         int diverged, float* x, float* term) {
    const FloatShapeF H = shape_of(par);
    float part[kShapeLanes][kShapeSums] = {};
    for (int v = 0; v < kShapeLanes; ++v) {
        float ds[kShapeDofSums] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int d = v; d < n; d += kShapeLanes)
            dev::ft_shape_dof(tau[d], q[d], qd[d], qd_prev[d], H.env_dt, lo[d], hi[d], home[d], ds);
        for (int e = 0; e < kShapeDofSums; ++e) part[v][e] = ds[e];
        float col = 0.f, stu = 0.f, exc = 0.f;
        if (H.w[kShStumble] != 0.f || H.w[kShContactForce] != 0.f)
            for (int j = v; j < n_links; j += kShapeLanes)
                dev::ft_shape_contact(H, contact_f[3 * j], contact_f[3 * j + 1], contact_f[3 * j + 2], stu, exc);
        if (H.w[kShCollision] != 0.f)
            for (int j = v; j < n_pen; j += kShapeLanes)
                col = col + dev::ft_shape_collision(H, pen_f[3 * j], pen_f[3 * j + 1], pen_f[3 * j + 2]);
        part[v][5] = col;
        part[v][6] = stu;
        part[v][7] = exc;
    }
    float sum[kShapeSums];
    for (int e = 0; e < kShapeSums; ++e) {
        float p[kShapeLanes];
        for (int v = 0; v < kShapeLanes; ++v) p[v] = part[v][e];
        sum[e] = dev::ft_shape_combine(p);
    }
    const float b[7] = {pose[0], pose[1], pose[2], pose[3], pose[4], pose[5], pose[6]};
    float xs[kShapeTerms], ts[kShapeTerms];
    dev::ft_shape_x(H, sum, b, standing != 0, xs);
    dev::ft_shape_terms(H, xs, diverged != 0, ts);
    for (int k = 0; k < kShapeTerms; ++k) {
        x[k] = xs[k];
        term[k] = ts[k];
    }
}

extern "C" float fs_reward(float r_existing, const float* term) {
    float t[kShapeTerms];
    for (int k = 0; k < kShapeTerms; ++k) t[k] = term[k];
    return dev::ft_shape_reward(r_existing, t);
}

extern "C" float fs_force_norm(float fx, float fy, float fz) { return dev::ft_force_norm(fx, fy, fz); }

extern "C" int fs_standing(float cx, float cy, float cmd_min) { return dev::ft_shape_standing(cx, cy, cmd_min) ? 1 : 0; }

// the termination predicate over a world's active slots of the termination links: f [count][3]
extern "C" int fs_terminated(const float* par, int count, const float* f) {
    const FloatShapeF H = shape_of(par);
    bool hit = false;
    for (int i = 0; i < count; ++i) hit = hit || dev::ft_shape_slot_hit(H, f[3 * i], f[3 * i + 1], f[3 * i + 2]);
    return hit ? 1 : 0;
}

// One world over `steps` steps: reward [steps], term [steps][10], diverged and
// done [steps]; after every step the running sums (acc_*) and, where the step
// finished an episode (finished[t] = 1), the copied-out ep_* of that step.
extern "C" void fs_stats(int steps, const float* reward, const float* term, const unsigned char* diverged,
                         const unsigned char* done, float* acc_return, int* acc_length, float* acc_terms,
                         unsigned char* finished, float* ep_return, int* ep_length, float* ep_terms) {
    float ar = 0.f, at[kShapeTerms] = {};
    int32_t al = 0;
    for (int t = 0; t < steps; ++t) {
        float tk[kShapeTerms], et[kShapeTerms] = {}, er = 0.f;
        int32_t el = 0;
        for (int k = 0; k < kShapeTerms; ++k) tk[k] = term[t * kShapeTerms + k];
        finished[t] = dev::ft_shape_stats(reward[t], tk, diverged[t] != 0, done[t] != 0, ar, al, at, er, el, et) ? 1 : 0;
        acc_return[t] = ar;
        acc_length[t] = al;
        ep_return[t] = er;
        ep_length[t] = el;
        for (int k = 0; k < kShapeTerms; ++k) {
            acc_terms[t * kShapeTerms + k] = at[k];
            ep_terms[t * kShapeTerms + k] = et[k];
        }
    }
}
