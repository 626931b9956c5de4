// lifecycle_driver.cpp -- what the handles of the C ABI own, under ASan/UBSan.
//
// Links the host layer (sim.cpp, world_params.cpp, vecenv.cpp, floatenv.cpp, scene.cpp, model.cpp, mesh.cpp)
// against hip_standin.cpp instead of the HIP runtime.  Every scenario runs
// once cleanly, then once for each k = 0, 1, ... with the k-th creating call
// (buffer, stream, event) failing, until a run no longer reaches its k-th
// call.  A failing run must report MW_EHIP with a message, every later call on
// the handle up to its destroy must stay clean under the sanitizers, and after
// the destroy the count of live objects must be what it was before.
//
// usage: lifecycle_san <models dir>; one line per scenario
//   "<name> points <n> leaks <m>", exit status 1 on any violation.
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "mwscene.h"
#include "mwstep.h"

extern "C" long standin_live();
extern "C" void standin_fail_at(long k);
extern "C" int standin_fired();

namespace {

constexpr int W = 8;
constexpr long kMaxPoints = 1000;  // far above any scenario: the loops end by a clean run
const mw_config kCfg = {1e-3, 1.0, 1, W, 0, 0};
std::string g_models;
int g_violations = 0;

void violation(const std::string& scenario, const std::string& what) {
    std::fprintf(stderr, "VIOLATION %s: %s\n", scenario.c_str(), what.c_str());
    ++g_violations;
}

// the first failing call of a run
struct Trace {
    int rc = MW_OK;
    std::string msg, bad;
    int note(int r) {
        if (r != MW_OK && rc == MW_OK) {
            rc = r;
            msg = mw_last_error();
        }
        return r;
    }
};

// create -> load -> initialize -> run -> destroy; a failed initialize is repeated
mw_sim* start_sim(const char* model, Trace& t) {
    mw_sim* s = nullptr;
    t.note(mw_create(&kCfg, &s));
    t.note(mw_load_model(s, (g_models + "/" + model).c_str(), nullptr, ""));
    if (t.note(mw_initialize(s)) != MW_OK) (void)mw_initialize(s);
    return s;
}

void sim_case(const char* model, Trace& t) {
    mw_sim* s = start_sim(model, t);
    t.note(mw_run(s, 0));
    mw_destroy(s);
}

void env_case(const char* model, int kind, int randomize, Trace& t) {
    mw_sim* s = start_sim(model, t);
    int32_t n = 0;
    (void)mw_dofs(s, &n);
    mw_task_config tc{};
    tc.kind = kind;
    tc.max_episode_steps = 10;
    tc.seed = 1;
    tc.randomize = randomize;
    tc.mass_low = 0.5f;
    tc.mass_high = 2.0f;
    tc.gravity_mean = -9.8f;
    tc.gravity_std = 0.1f;
    mw_vecenv* e = nullptr;
    if (t.note(mw_vecenv_create(s, &tc, &e)) != MW_OK && e) t.bad = "a failed mw_vecenv_create returned a handle";
    const size_t no = (kind == MW_TASK_PANDA_POSITION_TRACKING) ? 2 * static_cast<size_t>(n) : 4;
    std::vector<float> act(static_cast<size_t>(W) * (n ? n : 1)), obs(W * no), tobs(W * no), rew(W);
    std::vector<uint8_t> done(W);
    t.note(mw_vecenv_reset(e, obs.data()));
    for (int k = 0; k < 2; ++k)  // the second step finds the buffers a failed first one left
        t.note(mw_vecenv_step(e, act.data(), obs.data(), rew.data(), done.data(), tobs.data()));
    mw_vecenv_destroy(e);
    mw_destroy(s);
}

// The floating-base env of the quadruped with every configuration call that
// allocates: pushes and friction (wrench and friction arrays), inertia and
// joints (the per-world link parameter records; damping also re-uploads the
// shared blocks), locomotion (the env's own buffers).  A call that fails leaves
// the env without its feature, and the calls after it go on.
void float_env_case(Trace& t) {
    mw_sim* s = start_sim("quadruped.urdf", t);
    int32_t n = 0;
    (void)mw_dofs(s, &n);
    t.note(mw_set_ground_plane(s, 1, 1.0));
    t.note(mw_enable_contacts(s, 1));
    const std::vector<float> home_q(n ? n : 1, 0.f);
    const int32_t feet[4] = {1, 3, 5, 7};
    mw_float_task_config tc{};
    tc.action_mode = MW_FLOAT_ACTION_POSITION;
    tc.max_episode_steps = 10;
    tc.n_contact_links = 4;
    tc.seed = 1;
    tc.cos_tilt_max = -1.f;
    tc.alive_bonus = 1.f;
    tc.joint_noise = 0.05f;
    tc.home_base[2] = 0.45f;
    tc.home_base[3] = 1.f;
    tc.home_q = home_q.data();
    tc.contact_links = feet;
    mw_vecenv* e = nullptr;
    if (t.note(mw_floatenv_create(s, &tc, &e)) != MW_OK && e) t.bad = "a failed mw_floatenv_create returned a handle";
    const size_t nd = static_cast<size_t>(n);
    std::vector<float> push(W * 6), mu(W), inertial(W * (nd + 1) * 10), idraw(W * (nd + 5)), joints(W * nd * 3),
        jdraw(W * nd * 3), command(W * 3);
    const mw_float_rand_config rc = {4, 2, 20.f, 5.f, 0.4f, 1.2f};
    t.note(mw_floatenv_randomize(e, &rc, push.data(), mu.data()));
    const mw_float_inertia_config ic = {0.8f, 1.2f, 0.f, 2.f, {0.1f, 0.05f, 0.02f}};
    t.note(mw_floatenv_inertia(e, &ic, inertial.data(), idraw.data()));
    const mw_float_joint_config jc = {0.f, 0.5f, 0.f, 2.f, 0.5f, 1.f, 0};
    t.note(mw_floatenv_joints(e, &jc, joints.data(), jdraw.data()));
    mw_float_loco_config lc{};
    lc.cmd_lo[0] = -1.f;
    lc.cmd_hi[0] = 1.f;
    lc.cmd_interval = 5;
    lc.action_scale = 0.25f;
    lc.w_track_lin = 1.f;
    lc.track_sigma = 0.25f;
    lc.w_air_time = 1.f;
    lc.air_time_target = 0.1f;
    lc.contact_force_min = 1.f;
    t.note(mw_floatenv_locomotion(e, &lc, command.data()));
    const size_t no = 25 + 3 * nd + 4;  // the locomotion row, the widest
    std::vector<float> act(W * (nd ? nd : 1)), obs(W * no), tobs(W * no), rew(W);
    std::vector<uint8_t> done(W);
    t.note(mw_vecenv_reset(e, obs.data()));
    for (int k = 0; k < 2; ++k) t.note(mw_vecenv_step(e, act.data(), obs.data(), rew.data(), done.data(), tobs.data()));
    mw_vecenv_destroy(e);
    mw_destroy(s);
}

// `cubes` cubes in a row on a ground plane; eight of them need the large-contact
// workspace and a larger contact output, which the first run reallocates
void scene_case(int cubes, Trace& t) {
    mw_scene* sc = nullptr;
    if (t.note(mw_scene_create(&kCfg, &sc)) != MW_OK && sc) t.bad = "a failed mw_scene_create returned a handle";
    const std::string cube = g_models + "/cube.urdf";
    for (int c = 0; c < cubes; ++c) {
        const double pose[7] = {1.0001 * c, 0, 0.4999, 1, 0, 0, 0};
        int32_t m = -1;
        t.note(mw_scene_insert_model(sc, cube.c_str(), pose, ("c" + std::to_string(c)).c_str(), 0, W, &m));
    }
    if (cubes) {
        t.note(mw_scene_set_ground_plane(sc, 1, 0.8));
        for (int k = 0; k < 2; ++k) t.note(mw_scene_run(sc, 0));  // the second run follows a failed first one
    }
    mw_scene_destroy(sc);
}

// Two cubes run, then a third one raises the scene's worst case past the
// contact output's capacity: the paused run that applies the insertion
// reallocates the contact block and must report the last step's contacts
// again -- read before the insertion (the host mirror was current) or not --
// with every identity a valid index.
void scene_regrow_case(bool read_before, Trace& t) {
    mw_scene* sc = nullptr;
    t.note(mw_scene_create(&kCfg, &sc));
    const std::string cube = g_models + "/cube.urdf";
    auto insert = [&](int c) {
        const double pose[7] = {1.0001 * c, 0, 0.4999, 1, 0, 0, 0};
        int32_t m = -1;
        t.note(mw_scene_insert_model(sc, cube.c_str(), pose, ("c" + std::to_string(c)).c_str(), 0, W, &m));
    };
    constexpr int kCap = 128, w = W - 1;
    std::vector<double> before(kCap * 14, -7.0), after(kCap * 14, -7.0);
    int32_t nb = -1, na = -1;
    insert(0);
    insert(1);
    t.note(mw_scene_set_ground_plane(sc, 1, 0.8));
    t.note(mw_scene_run(sc, 0));
    t.note(mw_scene_get_contacts(sc, w, before.data(), kCap, &nb));
    if (!read_before) {
        // a second step: the mirror is stale when the block is reallocated
        t.note(mw_scene_run(sc, 0));
    }
    insert(2);
    if (t.note(mw_scene_run(sc, 1)) != MW_OK) (void)mw_scene_run(sc, 1);   // a failed reallocation is repeated
    const int rc = t.note(mw_scene_get_contacts(sc, w, after.data(), kCap, &na));
    if (t.rc == MW_OK && rc == MW_OK) {
        if (nb != 16 || na != nb) t.bad = "contacts " + std::to_string(nb) + " before and " + std::to_string(na) +
                                          " after the capacity change (16 expected)";
        else if (before != after) t.bad = "the paused run after a capacity change reports other contacts";
        for (int c = 0; c < na && c < kCap; ++c)
            if (after[c * 14 + 10] < 0 || after[c * 14 + 10] > 2 || after[c * 14 + 12] != -1)
                t.bad = "a contact names a model that does not exist";
    }
    t.note(mw_scene_run(sc, 0));
    t.note(mw_scene_get_contacts(sc, w, after.data(), kCap, &na));
    if (t.rc == MW_OK && na != 24) t.bad = "contacts " + std::to_string(na) + " after the step with three cubes (24 expected)";
    mw_scene_destroy(sc);
}

void check(const std::string& name, const std::function<void(Trace&)>& run) {
    long leaks = 0;
    auto once = [&](long k, Trace& t) {
        const long base = standin_live();
        standin_fail_at(k);
        run(t);
        const bool fired = standin_fired() != 0;
        standin_fail_at(-1);
        if (!t.bad.empty()) violation(name, t.bad);
        if (standin_live() != base) {
            ++leaks;
            violation(name, "k = " + std::to_string(k) + ": " + std::to_string(standin_live() - base) +
                                " object(s) live after destroy");
        }
        return fired;
    };
    Trace clean;
    once(-1, clean);
    if (clean.rc != MW_OK) violation(name, "the clean run failed: " + clean.msg);
    long k = 0;
    for (;; ++k) {
        if (k >= kMaxPoints) {
            violation(name, "no clean run within " + std::to_string(kMaxPoints) + " injection points");
            break;
        }
        Trace t;
        const bool fired = once(k, t);
        if (!fired) {  // the run never reached its k-th creating call
            if (t.rc != MW_OK) violation(name, "a run without an injected failure failed: " + t.msg);
            break;
        }
        if (t.rc != MW_EHIP || t.msg.empty())
            violation(name, "k = " + std::to_string(k) + ": status " + std::to_string(t.rc) + ", message '" + t.msg +
                                "' (expected MW_EHIP and a message)");
    }
    std::printf("%s points %ld leaks %ld\n", name.c_str(), k, leaks);
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <models dir>\n", argv[0]);
        return 2;
    }
    g_models = argv[1];
    for (const char* m : {"cartpole", "cube", "icub"})
        check(std::string("sim_") + m, [m](Trace& t) { sim_case((std::string(m) + ".urdf").c_str(), t); });
    check("env_cartpole", [](Trace& t) {
        env_case("cartpole.urdf", MW_TASK_CARTPOLE_DISCRETE, MW_RAND_MASS | MW_RAND_GRAVITY, t);
    });
    check("env_panda", [](Trace& t) { env_case("panda.urdf", MW_TASK_PANDA_POSITION_TRACKING, 0, t); });
    check("env_float", [](Trace& t) { float_env_case(t); });
    check("scene_create", [](Trace& t) { scene_case(0, t); });
    check("scene_run", [](Trace& t) { scene_case(2, t); });
    check("scene_big", [](Trace& t) { scene_case(8, t); });
    check("scene_regrow_read", [](Trace& t) { scene_regrow_case(true, t); });
    check("scene_regrow_stale", [](Trace& t) { scene_regrow_case(false, t); });
    return g_violations ? 1 : 0;
}
