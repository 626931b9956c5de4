// sim_state.hpp -- the simulator behind an mw_sim handle and the helpers
// sim.cpp, world_params.cpp and the batched envs (vecenv.cpp, floatenv.cpp) share.
// Internal, host only.
#pragma once

#include "mwstep.h"

#include <array>
#include <limits>
#include <string>
#include <vector>

#include "chain_params.hpp"
#include "device_mem.hpp"
#include "float_tree.hpp"
#include "free_body.hpp"
#include "kernels.hpp"
#include "model.hpp"

struct mw_sim {
    mw_config cfg{};
    bool stream_set = false;  // mw_set_stream called (NULL = the legacy default stream)
    // declared before every buffer: members are destroyed in reverse order, so
    // a stream created here outlives the buffers and is destroyed last
    mw::stream_ptr own_stream;
    hipStream_t stream = nullptr;  // own_stream or the caller's (mw_set_stream)
    bool loaded = false;
    bool initialized = false;
    bool stepped = false;     // model parameters become read-only after the first run
    bool servo_used = false;  // a joint was put in VelocityFollowerDart
    bool host_stale = false;  // device state changed by the VecEnv path
    // a floating-base env (mw_floatenv_create) writes the commands and pending
    // resets on the device: the host setters of either fail with MW_ESTATE
    bool env_owned = false;
    bool cmd_dirty = true;
    bool ptgt_dirty = false;  // host position targets newer than the device copy
    bool ptgt_stale = false;  // device position targets newer than the host mirror
    bool ptgt_view = false;   // a device view of the targets was handed out (always re-read)
    int topo = 0;             // kernel topology id (kernels.hpp: kernel_topology)
    mw::ChainModel model;
    std::string model_name;
    double gravity[3] = {0.0, 0.0, -9.8};  // sdformat default world gravity
    int64_t iterations = 0;
    int64_t dt_ns = 0;
    // JointController (one per model): Model.cpp:181-185 initialises the period
    // to the maximum duration; the plugin is inserted by the first Position /
    // Velocity / VelocityFollowerDart joint (Joint.cpp:376-404)
    bool controller = false;
    int64_t period_ns = std::numeric_limits<int64_t>::max();
    int64_t prev_ns = 0;      // JointController prevUpdateTime (0 = first iteration)
    // JointPID per dof in scenario::core::PID order {p, i, d, cmdMin, cmdMax,
    // cmdOffset, iMin, iMax}; default = Joint.cpp:63 DefaultPID
    std::vector<std::array<double, 8>> pid;

    int n = 0, W = 0;
    size_t nw = 0;  // n * W
    // device block layout: [q qd qdd | cmd vtgt rq rqd | act rflag]; the host
    // mirror has the same layout so the command slab moves in one copy
    mw::dev_ptr<void> d_block;
    mw::pin_ptr<uint8_t[]> h_block;
    size_t block_bytes = 0, cmd_off = 0, cmd_bytes = 0, state_bytes = 0;
    mw::dev_ptr<mw::ChainF> d_params;
    mw::ChainF h_params{};
    // [ptgt | pid_e | pid_i | pid_u | qlo] on the device; h_ptgt mirrors ptgt
    mw::dev_ptr<float[]> d_aux;
    mw::pin_ptr<float[]> h_ptgt;
    // pinned staging copy of [command slab | position targets]: the H2D copies
    // of a run read it, so the host mirror can be cleared / rewritten right
    // after the launch; stage_ev marks when the last copy out of it finished
    mw::pin_ptr<uint8_t[]> h_stage;
    mw::event_ptr stage_ev;
    bool stage_pending = false;
    // floating single-body models (free_body.hpp)
    bool floating = false;
    bool ground = false;          // a ground plane z = 0 is in the world
    double ground_mu = 1.0;       // SDF <surface><friction><ode><mu> default
    bool contacts = false;        // Model::enableContacts
    mw::FreeF h_free{};
    mw::dev_ptr<mw::FreeF> d_free;
    mw::FreeDev fdev{};
    mw::dev_ptr<void> d_fblock;   // [base 13 | rpose 7 | rvel 6 | contacts 7*slots][W] f32 + rflag u8 + cmask u32
    mw::pin_ptr<float[]> h_base;  // [13][W] host mirror (pinned)
    mw::pin_ptr<float[]> h_cdata; // [slots][7][W]
    mw::pin_ptr<uint32_t[]> h_cmask;  // [W]
    std::vector<float> h_rpose, h_rvel;
    std::vector<uint8_t> h_rflag;
    bool free_dirty = false;
    bool contacts_stale = false;  // contacts written on the device by mw_run_device
    // articulated models on a floating base (float_tree.hpp): the joint state
    // of a fixed-base model plus the base block above
    bool float_tree = false;
    // a fixed-base tree outside the compiled chain topologies (more than 9
    // dofs, or branched other than the Panda): the world-per-wavefront kernel
    // with a welded base (FloatF::fixed); its joint and base state live where a
    // floating tree's do
    bool fixed_tree = false;
    bool fbase() const { return floating || fixed_tree; }
    mw::FloatF h_float{};
    mw::dev_ptr<mw::FloatF> d_float;
    mw::dev_ptr<float[]> d_ws;    // constraint-row workspace [words][W]
    int n_slots = mw::kMaxFreeSlots;
    std::vector<int32_t> slot_body;  // body of every contact slot (-1 = base)
    // large trees (or MWSTEP_WAVE_TREE=1): one world per wavefront (wave_tree.hpp)
    bool wave = false;
    bool wave_depth_ok = false;   // the tree fits the wave kernel's depth stack
    int wave_depth = 0;           // the tree's depth in joints (picks the wave kernel's instance)
    mw::dev_ptr<mw::PidF[]> d_pid;  // PID gains of every dof (device)
    mw::pin_ptr<mw::PidF[]> h_pid;  // pinned staging copy
    bool pid_dirty = true;        // gains changed since the last upload
    // dofs whose gains mw_set_joint_pid replaced since the last step (bit per
    // dof < 64): the position-target env starts their controller state from
    // zero, as mw_run does through the reset flags
    uint64_t pid_reset_dofs = 0;
    mw::dev_ptr<int[]> d_overflow;  // constraint rows dropped by the wave kernel
    mw::dev_ptr<float[]> d_warm;  // wave kernel: previous step's PGS impulses [kWaveWarmWordsHost][W]
    double pgs_tol = 0.0;         // mw_set_pgs_options
    bool pgs_warm = false;
    // world wrenches (mw_apply_link_wrench, wave kernel): host records
    // [slot][6][node][W] / [slot][node][W], device copies, the last iteration
    // any record covers
    std::vector<float> h_wr;
    std::vector<int32_t> h_wl;
    mw::dev_ptr<float[]> d_ext;    // [6][node][W]: the summed wrenches of one launch
    mw::pin_ptr<float[]> h_ext;    // pinned staging of d_ext
    int64_t wr_until = 0;
    // an env with pushes (mw_floatenv_randomize) writes d_ext on the device:
    // every run passes it to the kernel as it is (no staging, no
    // synchronisation), and mw_apply_link_wrench fails with MW_ESTATE
    bool env_wrench = false;
    // per-world ground friction (mw_set_ground_friction, wave kernel): [W] on
    // the device (RunArgs::mu) and its host mirror; allocated by the first call
    mw::dev_ptr<float[]> d_mu;
    std::vector<float> h_mu;
    // an env with friction randomisation writes d_mu on the device: the host
    // setters fail with MW_ESTATE, mw_ground_friction reads the device copy
    bool env_friction = false;
    // per-world link parameters (mw_set_link_params, wave kernel): W records of
    // wpar_stride words on the device (RunArgs::wpar, world_params.hpp) and their
    // host mirror; allocated by the first call, together with d_mu (the
    // kernel's per-world-parameter instances read the friction per world too)
    mw::dev_ptr<float[]> d_wpar;
    std::vector<float> h_wpar;
    int wpar_stride = 0;
    // an env with inertia randomisation (mw_floatenv_inertia) writes d_wpar on
    // the device: mw_set_link_params fails with MW_ESTATE, mw_link_params reads
    // the device copy
    bool env_inertia = false;
    // per-world joint dynamics (mw_set_joint_dynamics: BodyF::damping, friction
    // and effort of the same records).  The host chooses two things from the
    // nominal model that a world's own words can change, so both are sticky
    // from the first non-zero word (or an env's draw, mw_floatenv_joints) on:
    // friction rows need the wave kernel's CONS instance (needs_cons), damping
    // the second recursion of its ABA (FloatF::dual, build_float)
    bool wpar_friction = false;
    bool wpar_damping = false;
    // an env with joint randomisation (mw_floatenv_joints) writes those words on
    // the device; like env_inertia it owns the records while it lives
    bool env_joints = false;
    bool env_wpar() const { return env_inertia || env_joints; }
    mw::pin_ptr<int[]> h_overflow;  // pinned copy read back with each synchronous run
    int64_t overflow_seen = 0;    // drops already reported
    // divergence detection: [W] sticky per-world flags + the uint64 count of
    // worlds flagged (device), its pinned copy (read back with every
    // synchronous run) and the flags already reported
    mw::dev_ptr<uint8_t[]> d_health;
    mw::pin_ptr<uint64_t> h_ndiv;
    int64_t div_seen = 0;
    int32_t lcp_mode = MW_LCP_EXACT;  // mw_set_lcp_solver (wave kernel)
    int32_t lcp_solves = 48;          // linear-solve budget of the exact solve per step (r06: a random humanoid impact needed 25-32)
    mw::SimDev dev;
    // host-only component data
    std::vector<int32_t> mode;      // JointControlMode per [d][w]
    std::vector<double> ptgt;       // JointPositionTarget
    std::vector<double> cmd64;      // JointForceCmd exactly as set (double)

    float* hq() { return reinterpret_cast<float*>(h_block.get()); }
    float* hqd() { return hq() + nw; }
    float* hqdd() { return hq() + 2 * nw; }
    float* hcmd() { return hq() + 3 * nw; }
    float* hvt() { return hq() + 4 * nw; }
    float* hrq() { return hq() + 5 * nw; }
    float* hrqd() { return hq() + 6 * nw; }
    uint8_t* hact() { return h_block.get() + 7 * nw * sizeof(float); }
    uint8_t* hrflag() { return hact() + nw; }
    size_t idx(int d, int w) const { return static_cast<size_t>(d) * W + w; }

    // the stream drains before the members release their resources (nothing to do before mw_initialize)
    ~mw_sim() {
        if (!own_stream && !d_health) return;
        (void)hipSetDevice(cfg.device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

// sim.cpp, shared with the batched envs (vecenv.cpp, floatenv.cpp)
int check_sim(const mw_sim* s, bool need_init = true);
int run_impl(mw_sim* s, int paused, bool readback);
bool needs_cons(const mw_sim* s);
bool needs_dual(const mw_sim* s);
int baked_id(const mw_sim* s);
mw::PidSet pid_set(const mw_sim* s);
// the wrench array an env's pushes write (zeroed, [6][n + 1][W])
int alloc_env_wrench(mw_sim* s);
// rebuild and upload the shared parameter blocks; the per-world records follow
// (set_dof, set_word: the joint dynamics word a shared setter overwrites in all)
int upload_params(mw_sim* s, int set_dof = -1, int set_word = -1);
// world_params.cpp.  alloc_*: on the first call, every world at the current
// coefficient / nominal words; pull_*: device copy -> host mirror (synchronises)
int alloc_ground_friction(mw_sim* s);
int pull_ground_friction(mw_sim* s);
int fill_ground_friction(mw_sim* s, double mu);  // every world takes mu, if the array exists
int check_not_env_friction(const mw_sim* s, const char* what);
int alloc_link_params(mw_sim* s);
int pull_link_params(mw_sim* s);
int refresh_link_params(mw_sim* s, int set_dof, int set_word);
// wpar_friction / wpar_damping (re-uploads FloatF when its dual flag may follow)
int set_joint_dynamics_flags(mw_sim* s, bool friction, bool damping);
