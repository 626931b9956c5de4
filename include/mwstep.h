/*
 * mwstep.h -- C ABI of the MI355X many-worlds articulated-body stepper.
 *
 * This is the drop-in boundary that replaces the reference's ScenarI/O Gazebo
 * backend on the env-step hot path:
 *   GazeboRuntime.step()            python/gym_ignition/runtimes/gazebo_runtime.py:91-120
 *   -> scenario.GazeboSimulator.run cpp/scenario/gazebo/src/GazeboSimulator.cpp:202-251
 *   -> Physics system Update        cpp/scenario/plugins/Physics/Physics.cpp:646-685
 *   -> DART World::step             [EXT]
 * Every world of a simulator is one slot of structure-of-arrays device state;
 * one mw_run() steps all of them (the reference steps one ECM per world,
 * GazeboSimulator.cpp:435-488 / Physics.cpp:1832-1834).
 *
 * Conventions
 *   - every function returns MW_OK (0) or an MW_E* status; the message of the
 *     last failure on the calling thread is mw_last_error().  Bool-returning
 *     ScenarI/O calls map MW_OK -> true; getters that throw in the reference
 *     (exceptions::DOFMismatch etc., cpp/scenario/gazebo/include/scenario/
 *     gazebo/exceptions.h) map a failure to RuntimeError in the Python shim.
 *   - host buffers are double precision, row-major [n_worlds_in_range, n_dofs];
 *     device buffers are float32 and owned by the caller unless stated.
 *   - no torch or HIP types appear in these signatures; a HIP stream is passed
 *     as void*.
 */
#ifndef MWSTEP_H
#define MWSTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MW_OK 0
#define MW_EINVAL 1      /* bad argument (dof/world out of range, bad mode) */
#define MW_ESTATE 2      /* wrong lifecycle state (not initialized, ...)    */
#define MW_EPARSE 3      /* model file could not be parsed / unsupported    */
#define MW_EHIP 4        /* HIP runtime failure                            */
#define MW_ENOTFOUND 5   /* unknown joint / model / field name             */
#define MW_ECAPACITY 6   /* a per-step capacity was exceeded: contact points /
                            constraint rows were dropped (the step ran without
                            them; DART would have kept them); from
                            mw_floatenv_tracking / _shaping: the env's tiles
                            exceed a block's local memory, nothing changed  */
#define MW_EDIVERGED 7   /* a world's state became non-finite in this run (the
                            run advanced every world; mw_diverged lists the
                            flagged ones) -- failure detection, SURVEY.md §5 */

/* JointControlMode, same numbering as scenario::core::JointControlMode
 * (cpp/scenario/core/include/scenario/core/Joint.h:37-75). */
#define MW_MODE_INVALID 0
#define MW_MODE_IDLE 1
#define MW_MODE_FORCE 2
#define MW_MODE_VELOCITY 3
#define MW_MODE_VELOCITY_FOLLOWER_DART 4
#define MW_MODE_POSITION 5
#define MW_MODE_POSITION_INTERPOLATED 6

/* JointType, same numbering as scenario::core::JointType (Joint.h:25-31). */
#define MW_JOINT_INVALID 0
#define MW_JOINT_FIXED 1
#define MW_JOINT_REVOLUTE 2
#define MW_JOINT_PRISMATIC 3
#define MW_JOINT_BALL 4
/* An SDF ball joint (3 dofs) is compiled as three revolute dofs named
 * <joint>#x, <joint>#y, <joint>#z: rotations about the x, y, z axes of the
 * joint frame at one point (intrinsic X-Y-Z angles), the first two on
 * massless links <joint>#x, <joint>#y; mw_joint_type reports MW_JOINT_BALL
 * for all three.  The ScenarI/O mirror (scenario/gazebo.py BallJoint)
 * presents them in DART's BallJoint coordinates (rotation vector, child-frame
 * angular velocity and torque). */

/* per-joint parameters that the reference lets a just-created model change
 * (Joint::setCoulombFriction / setViscousFriction / setMaxGeneralizedForce,
 * cpp/scenario/gazebo/src/Joint.cpp:258-318,622-640) */
#define MW_PARAM_COULOMB_FRICTION 0
#define MW_PARAM_VISCOUS_FRICTION 1
#define MW_PARAM_MAX_GENERALIZED_FORCE 2
#define MW_PARAM_POSITION_LIMIT_MIN 3
#define MW_PARAM_POSITION_LIMIT_MAX 4

typedef struct mw_sim mw_sim;
typedef struct mw_vecenv mw_vecenv;

typedef struct {
    double step_size;        /* GazeboSimulator(step_size, rtf, steps_per_run) */
    double rtf;              /* validated (> 0) like helpers.cpp:391-400;       */
                             /* no wall-clock throttling is performed           */
    int32_t steps_per_run;   /* physics substeps per mw_run (> 0)              */
    int32_t n_worlds;        /* parallel worlds on this device (>= 1)          */
    int32_t device;          /* HIP device ordinal                             */
    int32_t pgs_iters;       /* boxed-LCP sweeps per substep (0 -> 20)          */
} mw_config;

/* ---- lifecycle (GazeboSimulator ctor / initialize / close) ---- */
const char* mw_last_error(void);
const char* mw_version(void);
int mw_create(const mw_config* cfg, mw_sim** out);
void mw_destroy(mw_sim* sim);
/* Load the articulated model replicated into every world.  `urdf` is a file
 * path or an inline string holding a URDF <robot> or an SDF <model>; pose =
 * {x, y, z, qw, qx, qy, qz} (World::insertModel,
 * cpp/scenario/gazebo/src/World.cpp:70-180; for SDF the identity pose keeps
 * the model's own <pose>, any other replaces it, World.cpp:169-177). */
int mw_load_model(mw_sim* sim, const char* urdf, const double pose[7], const char* name);
int mw_initialize(mw_sim* sim);
int mw_initialized(const mw_sim* sim);
/* Optional: launch on an external stream (e.g. torch's current stream);
 * NULL selects the default stream.  Without this call the simulator creates
 * its own non-blocking stream at mw_initialize. */
int mw_set_stream(mw_sim* sim, void* hip_stream);

/* ---- stepping (GazeboSimulator::run) ---- */
/* Applies pending resets and commands, executes steps_per_run substeps unless
 * paused, refreshes the host-side readback, and blocks until done. */
int mw_run(mw_sim* sim, int paused);
/* `runs` x mw_run(sim, 0) with the state kept on the device: no readback and
 * no host synchronisation (graph-capturable; the getters read back lazily). */
int mw_run_device(mw_sim* sim, int32_t runs);
/* Simulated time in seconds after the last run (World::time, World.cpp:326-332). */
int mw_time(const mw_sim* sim, double* seconds);
int mw_set_gravity(mw_sim* sim, const double g[3]);
int mw_gravity(const mw_sim* sim, double g[3]);

/* ---- model / joint introspection ---- */
int mw_n_worlds(const mw_sim* sim, int32_t* n);
int mw_dofs(const mw_sim* sim, int32_t* n);
int mw_joint_name(const mw_sim* sim, int32_t dof, char* buf, int32_t buflen);
/* the (lumped) link moved by joint dof (Model::linkNames, Model.cpp:479-520) */
int mw_link_name(const mw_sim* sim, int32_t dof, char* buf, int32_t buflen);
int mw_joint_index(const mw_sim* sim, const char* name, int32_t* dof);
int mw_joint_type(const mw_sim* sim, int32_t dof, int32_t* type);
int mw_model_name(const mw_sim* sim, char* buf, int32_t buflen);
int mw_base_frame(const mw_sim* sim, char* buf, int32_t buflen);
int mw_set_joint_param(mw_sim* sim, int32_t dof, int32_t which, double value);
int mw_joint_param(const mw_sim* sim, int32_t dof, int32_t which, double* value);
/* Export the compiled tree (fp64) for cross-checks: per dof, in depth-first
 * body order, {jtype, limited, E[9], r[3], axis[3], mass, com[3], Ic[6],
 * damping, friction, lower, upper, effort, vel_limit, parent} = 34 doubles,
 * then gravity_base[3]. */
int mw_model_export(const mw_sim* sim, double* out, int32_t len);
/* The base of the compiled tree: {floating, base_R[9], base_p[3] (the model
 * frame in the world), base_mass, base_com[3], base_Ic[6]} = 23 doubles (the
 * inertia is zero for a fixed base). */
int mw_model_export_base(const mw_sim* sim, double out[23]);
/* Collision shapes of body `body` (-1 = the base), in its frame: per shape
 * {type (0 box, 1 sphere), size[3] (half extents / radius), R[9], p[3]} = 16
 * doubles; *count receives the number of shapes, at most `max_shapes` are
 * written (Physics.cpp:687-1219 creates one collision per <collision>). */
int mw_model_export_shapes(const mw_sim* sim, int32_t body, double* out, int32_t max_shapes, int32_t* count);
/* Compile a model (URDF / SDF file path or string; no simulator, no GPU) and
 * export every collision it holds, base first then by body, as the scene
 * kernel sees them (Physics.cpp:687-1219 builds one shape per <collision>;
 * meshes :897-931): per shape MW_COLLISION_WORDS doubles {body (-1 = base),
 * type (0 box, 1 sphere, 2 cylinder, 3 mesh), size[3], R[9], p[3], npts,
 * points[16][3]} -- a mesh's size is its bounding box half extents, p the box
 * centre, points its ground-contact support points in the shape frame
 * (gym-ignition_amd/csrc/mesh.cpp).  mw_sim: a floating model's mesh
 * contacts the ground at its support points (articulated: zero-radius
 * spheres; joint-less: free-body shape entries of <= 8 points), fixed-base
 * models drop mesh shapes. */
#define MW_COLLISION_WORDS 66
int mw_compile_collisions(const char* model, const double pose[7], double* out, int32_t max_shapes,
                          int32_t* count);

/* Copy of the float32 parameter block the kernels read (struct ChainF of
 * gym-ignition_amd/csrc/chain_params.hpp), for tests and tools. */
int mw_device_params(const mw_sim* sim, void* out, int32_t bytes);
/* the FloatF block (base inertia, shapes, contact slots) of an articulated
 * floating-base model, for the same test harness */
int mw_device_float_params(const mw_sim* sim, void* out, int32_t bytes);
/* Id of the shipped model whose parameter block the loaded model matches bit
 * for bit (1 cartpole, 2 pendulum): the batched env then runs a kernel with the
 * model constant-folded.  0 = generic kernel.  MWSTEP_DISABLE_BAKED=1 forces 0. */
int mw_baked_model(const mw_sim* sim, int32_t* id);

/* ---- batched ScenarI/O accessors over worlds [w0, w0 + nw) ----
 * dofs == NULL selects all dofs in model order (ndofs ignored). */
int mw_get_joint_positions(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_get_joint_velocities(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_get_joint_accelerations(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_get_joint_forces(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_get_joint_force_targets(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_get_joint_velocity_targets(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_get_joint_position_targets(const mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, double* out);
int mw_set_joint_force_targets(mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, const double* v);
int mw_set_joint_velocity_targets(mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, const double* v);
int mw_set_joint_position_targets(mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, const double* v);
int mw_reset_joint_positions(mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, const double* v);
int mw_reset_joint_velocities(mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, const double* v);
int mw_set_joint_control_mode(mw_sim* sim, int32_t w0, int32_t nw, const int32_t* dofs, int32_t ndofs, int32_t mode);
int mw_joint_control_mode(const mw_sim* sim, int32_t w, int32_t dof, int32_t* mode);

/* JointController PID of one dof, shared by all worlds of the simulator.
 * gains = {p, i, d, cmd_min, cmd_max, cmd_offset, i_min, i_max}, the field
 * order of scenario::core::PID (cpp/scenario/core/include/scenario/core/
 * Joint.h:505-523).  Replaces Joint::setPID / Joint::pid (Joint.cpp:466-525):
 * output limits less limiting than +-max generalized force are replaced by
 * them; the new PID starts from a reset state.  Default: Joint.cpp:63. */
int mw_set_joint_pid(mw_sim* sim, int32_t dof, const double gains[8]);
int mw_joint_pid(const mw_sim* sim, int32_t dof, double gains[8]);
/* Model::setControllerPeriod / controllerPeriod (Model.cpp:589-602, default
 * the maximum duration, Model.cpp:181-185): the PID force of Position /
 * Velocity joints is recomputed when at least one period of simulated time
 * has elapsed (JointController.cpp:130-169), else the last force is reused. */
int mw_set_controller_period(mw_sim* sim, double period);
int mw_controller_period(const mw_sim* sim, double* period);

/* ---- floating bases (root link not attached to "world": a DART FreeJoint
 * root).  This build steps single floating bodies and articulated models on
 * a floating base (any tree of <= 48 bodies), with box / sphere / cylinder
 * collision shapes on any link against a ground plane z = 0 and a contact LCP
 * with friction.  Fixed-base trees outside the compiled chain topologies run
 * on the same world-per-wavefront kernel with a welded base; for every
 * fixed-base model the base getters return the model frame at rest ---- */
int mw_is_floating(const mw_sim* sim, int32_t* floating);
/* Model::basePosition / baseOrientation: out [nw][7] = x y z qw qx qy qz. */
int mw_get_base_pose(const mw_sim* sim, int32_t w0, int32_t nw, double* out);
/* Model::baseWorldLinearVelocity / baseWorldAngularVelocity: out [nw][6] =
 * linear xyz (base origin), angular xyz, world frame. */
int mw_get_base_velocity(const mw_sim* sim, int32_t w0, int32_t nw, double* out);
/* Model::resetBasePose / resetBaseWorldVelocity (Model.cpp:256-400): applied by
 * the next run (pose first, then the velocity). */
int mw_reset_base_pose(mw_sim* sim, int32_t w0, int32_t nw, const double* pose);
int mw_reset_base_velocity(mw_sim* sim, int32_t w0, int32_t nw, const double* lin_ang);
/* Contact / joint-row solver options of the world-per-wavefront kernel
 * (articulated floating bases, generic fixed trees).  DART's primary boxed-LCP
 * solver is Dantzig's exact pivoting method [EXT]; the kernel runs projected
 * Gauss-Seidel sweeps (mw_config.pgs_iters).  tol > 0 ends the sweeps once a
 * sweep changed no row's constraint velocity (J dqd, m/s or rad/s) by more
 * than tol -- velocity space, where the redundant contact corners' null
 * directions do not count; warm_start != 0 starts
 * every row from the previous step's impulse of the same contact slot / joint
 * row (cold after a reset of the world).  Defaults: 0, 0 (a fixed sweep
 * count from zero).  Other kernels ignore the tolerance; warm_start != 0
 * fails with MW_ESTATE once an initialized simulator runs on another kernel
 * (they have no warm-start record). */
int mw_set_pgs_options(mw_sim* sim, double tol, int32_t warm_start);
int mw_pgs_options(const mw_sim* sim, double* tol, int32_t* warm_start);
/* The boxed-LCP solver of floating models.  MW_LCP_EXACT (default,
 * max_solves 48) solves the LCP as DART does: DART's primary solver is ODE's
 * Dantzig pivoting LCP [EXT], reached from ForwardStep (Physics.cpp:1824-1835),
 * whose friction index boxes every friction row once, by mu x the normal
 * impulses of the frictionless problem -- two strictly convex box QPs
 * (wave_lcp.hpp), each from the previous step's solution, PGS sweeps on the
 * stage's box problem (at most min(mw_config.pgs_iters, 4), ending once a
 * sweep moves no constraint velocity by more than 1e-6), then the primal
 * active-set method from the previous step's working set, with at most
 * max_solves dense linear solves (elimination over the wave's lanes) per
 * world-step.  It runs on the world-per-wavefront
 * kernel, which then steps every floating model (joint-less bodies, small
 * trees at any world count).  MW_LCP_PGS: the coupled PGS sweeps alone (cold
 * unless mw_set_pgs_options asks for the warm start); chosen before
 * mw_load_model it lets a joint-less body / small compiled tree take the
 * PGS-only lane kernels.  Selecting MW_LCP_EXACT for a model already loaded
 * onto a lane kernel fails with MW_ESTATE; mw_lcp_solver reports the solver
 * the model's kernel runs. */
#define MW_LCP_PGS 0
#define MW_LCP_EXACT 1
int mw_set_lcp_solver(mw_sim* sim, int32_t mode, int32_t max_solves);

/* Link::applyWorldWrench / applyWorldForce / applyWorldTorque
 * (cpp/scenario/gazebo/src/Link.cpp:484-560) on the worlds [w0, w0 + nw):
 * wrench[6 * nw] = world force at the link origin (xyz) and world torque
 * (xyz) per world, applied from the next physics step for
 * max(1, ceil(duration / dt)) steps; wrenches on one link add up (at most 4
 * distinct expiries at once).  link -1 = the base.  Carried by the
 * world-per-wavefront kernel (articulated floating bases, generic fixed-base
 * trees); other models fail with MW_ESTATE (use a scene).  Not seen by graphs
 * captured before the call. */
int mw_apply_link_wrench(mw_sim* sim, int32_t link, int32_t w0, int32_t nw, const double* wrench, double duration);
int mw_lcp_solver(const mw_sim* sim, int32_t* mode, int32_t* max_solves);
/* World-steps whose exact LCP solve ran out of budget since mw_initialize
 * (they keep their last impulses projected onto the friction boxes of their
 * normals and the joint rows' bounds: feasible, not optimal; 0 = every solve
 * converged).  64-bit device counters. */
int mw_lcp_unconverged(const mw_sim* sim, int64_t* world_steps);
/* The world's ground plane (z = 0, normal +z) and its friction coefficient. */
int mw_set_ground_plane(mw_sim* sim, int32_t enabled, double mu);
/* Per-world friction coefficients of the ground plane, worlds [w0, w0 + nw):
 * mu[nw] >= 0, used from the next run on (as float32, like the single
 * coefficient).  Models stepped by the world-per-wavefront kernel only
 * (mw_float_kernel == 2, generic fixed-base trees); others fail with
 * MW_ESTATE.  mw_set_ground_plane keeps its meaning: it sets every world to
 * its mu.  mw_ground_friction returns the values the next run will use; while
 * a floating-base env randomises the friction (mw_floatenv_randomize) it
 * reads the env's device copy back, and both setters fail with MW_ESTATE.
 * Friction is a parameter, not state: mw_get_state / mw_set_state records do
 * not hold it. */
int mw_set_ground_friction(mw_sim* sim, int32_t w0, int32_t nw, const double* mu);
int mw_ground_friction(mw_sim* sim, int32_t w0, int32_t nw, double* mu);
/* Per-world inertial parameters of one link, worlds [w0, w0 + nw):
 * params[nw][10] are the kernel's own float32 words, set and read back bit for
 * bit -- mass (> 0), centre of mass xyz in the link frame, rotational inertia
 * about the link ORIGIN (not the centre of mass) as xx yy zz xy xz yz; all
 * finite, else MW_EINVAL.  link -1 = the base, i = the body of dof i (the
 * numbering of mw_get_contact_bodies and mw_apply_link_wrench); links welded
 * by fixed joints are part of their body.  Used from the next run on.  Models
 * stepped by the world-per-wavefront kernel only (mw_float_kernel == 2,
 * generic fixed-base trees); others fail with MW_ESTATE.  The storage (one
 * copy of the model's body block and the base's words per world) is allocated
 * by the first mw_set_link_params; until then, and for every world and link
 * never set, mw_link_params returns the model's nominal words.  While a
 * floating-base env randomises the inertias (mw_floatenv_inertia)
 * mw_set_link_params fails with MW_ESTATE and mw_link_params reads the env's
 * device copy back.  These are parameters, not state: mw_get_state /
 * mw_set_state records do not hold them.  Quantities the host derives from
 * the model (mw_device_params / mw_device_float_params, the choice of the
 * kernel's instance) keep the nominal model.  Setters of the shared model
 * (mw_set_joint_param, mw_set_gravity) reach every world's copy and leave its
 * inertial words as they are. */
int mw_set_link_params(mw_sim* sim, int32_t w0, int32_t nw, int32_t link, const float* params);
int mw_link_params(mw_sim* sim, int32_t w0, int32_t nw, int32_t link, float* params);
/* Per-world joint dynamics of one joint, worlds [w0, w0 + nw): params[nw][3]
 * are the kernel's own float32 words of joint `dof`, set and read back bit for
 * bit -- viscous damping (N m s/rad, >= 0), Coulomb friction (N m, >= 0) and
 * the effort limit (N m, > 0; FLT_MAX is "unbounded"); all finite, dof and the
 * world range in bounds, else MW_EINVAL and nothing changes.  They live in the
 * records of mw_set_link_params and follow its rules: world-per-wavefront
 * models only (MW_ESTATE otherwise), the first set allocates the storage,
 * without it -- and for every world never set -- mw_joint_dynamics returns the
 * nominal words, used from the next run on, parameters and not state.  While a
 * floating-base env randomises inertias or joints (mw_floatenv_inertia,
 * mw_floatenv_joints) it owns the records: mw_set_joint_dynamics and
 * mw_set_link_params fail with MW_ESTATE and the getters read the env's device
 * copy back.
 *   Instance choice  the host picks the kernel's instance from the nominal
 *       model, with two exceptions that are sticky from the first non-zero
 *       word on: a friction word selects the instance with joint constraint
 *       rows even where the nominal model has neither limits nor friction, and
 *       a damping word turns on the second (non-implicit) recursion the
 *       impulses of a damped model need, for every world of the simulator.
 *   Shared setters  mw_set_joint_param(dof, which, value) keeps meaning "every
 *       world": it overwrites that one word of that dof in every record and
 *       keeps every other per-world joint word and all inertial words.
 *   Host-derived quantities keep the nominal model: the output limits that
 *       mw_set_joint_pid derives from the effort limit stay nominal; the clamp
 *       the run applies to the joint force is the per-world word.
 *   Row budget  friction adds one constraint row per moving joint to a world's
 *       LCP, which holds 64 rows (8 foot points of the iCub already take 24);
 *       rows beyond 64 are dropped and counted by mw_constraint_overflow. */
int mw_set_joint_dynamics(mw_sim* sim, int32_t w0, int32_t nw, int32_t dof, const float* params);
int mw_joint_dynamics(mw_sim* sim, int32_t w0, int32_t nw, int32_t dof, float* params);
/* Model::enableContacts / contactsEnabled (Model.cpp:674-700). */
int mw_enable_contacts(mw_sim* sim, int32_t enable);
int mw_contacts_enabled(const mw_sim* sim, int32_t* enabled);
/* Contacts of world w after the last run (Physics.cpp:2351-2540): up to cap
 * rows of 10 doubles = point xyz, normal xyz (into the body), force on the
 * body xyz (N), penetration depth; *n = number of contact points. */
int mw_get_contacts(const mw_sim* sim, int32_t w, double* out, int32_t cap, int32_t* n);
/* The body of every contact point of mw_get_contacts, same order: -1 = the
 * base link, i >= 0 = the link moved by joint i (Link::contacts,
 * Link.cpp:365-440, collects the contacts of one link). */
int mw_get_contact_bodies(const mw_sim* sim, int32_t w, int32_t* bodies, int32_t cap, int32_t* n);
/* Articulated floating-base models: which kernel steps them -- 0 none (not
 * such a model), 1 one world per lane (small compiled trees), 2 one world per
 * wavefront (any tree of <= 48 bodies; MWSTEP_WAVE_TREE=1 forces it) -- and the
 * number of constraint rows the wave kernel dropped so far (its per-step
 * capacity is 64 active rows; 0 in every test and bench configuration).
 * mw_run returns MW_ECAPACITY when its run dropped rows (the state has
 * advanced without them); mw_run_device, which does not synchronise, leaves
 * the check to mw_constraint_overflow. */
int mw_float_kernel(const mw_sim* sim, int32_t* kind);
int mw_constraint_overflow(const mw_sim* sim, int64_t* rows);

/* Zero-copy device views, float32 [n_dofs][n_worlds] (world index fastest):
 * the SoA state "q", "qd", "qdd", and "position_target" (the Position-mode
 * targets; after the view is taken, writes through it drive the next runs
 * and the host getters/setters re-read the device copy). */
int mw_device_ptr(mw_sim* sim, const char* field, void** dptr, int64_t* world_stride);
/* Device-to-device copy of the SoA state ([n_dofs][n_worlds] float32 each) to
 * (to_sim = 0) or from (to_sim = 1) caller buffers, on the sim's stream. */
int mw_copy_state(mw_sim* sim, float* q_dev, float* qd_dev, int to_sim);

/* ---- failure detection and per-world snapshots ----
 * The run kernels flag a world (sticky) when the joint or base state they
 * store is not finite -- tested on the exponent bits, the kernels being
 * built finite-math-only -- and count the flagged worlds.  mw_run reads the
 * count back with its state and returns MW_EDIVERGED when new worlds were
 * flagged (the reference has no such check: GazeboSimulator::run,
 * GazeboSimulator.cpp:202-251, only reports a failed server step);
 * mw_run_device leaves the check to mw_diverged.  mw_diverged: flags[nw] of
 * worlds [w0, w0 + nw) (flags may be NULL) and the number of flag events
 * since mw_initialize (a world counts again each time it is flagged after
 * its flag was re-armed); mw_clear_diverged re-arms the flags of a range.
 * Any reset of a world's state re-arms its flag too: mw_reset_joint_positions
 * / _velocities, mw_reset_base_pose / _velocity and mw_set_state, so a world
 * that diverges, is reset and diverges again is reported again. */
int mw_diverged(mw_sim* sim, int32_t w0, int32_t nw, uint8_t* flags, int64_t* count);
int mw_clear_diverged(mw_sim* sim, int32_t w0, int32_t nw);
/* The full per-world record as float32 words, [nw][words] in host memory, in
 * this order: q, qd, qdd, then the JointController PID state pErrLast, iErr,
 * cmd, then qlo (the low word of the compensated joint positions) -- n_dofs
 * words each, absent for joint-less bodies -- then the base pose (x y z, qw qx
 * qy qz) and body-frame twist (w, v) (13 words, floating and welded-tree
 * models), then the previous step's constraint impulses that the wave
 * kernel's warm start / exact LCP starts from (its models only: the final
 * impulses, then the stage-1 impulses, per contact slot and joint row).
 * mw_set_state writes the record back (bit-exact: a restored world steps
 * exactly as it did from the saved state), drops the worlds' pending resets
 * and clears their divergence flags.  The simulator time, the controller
 * period gate and the commands / targets are not per-world state and are not
 * part of the record. */
int mw_state_words(const mw_sim* sim, int32_t* words);
int mw_get_state(mw_sim* sim, int32_t w0, int32_t nw, float* out);
int mw_set_state(mw_sim* sim, int32_t w0, int32_t nw, const float* in);

/* ---- batched environment (device-side Task logic) ----
 * Tasks mirror python/gym_ignition_environments/tasks/ (CartPole x3,
 * Pendulum); the TimeLimit of
 * the gym registration (max_episode_steps, __init__.py:14-52) and
 * auto-reset of done worlds (Philox4x32-10 keyed by seed) run in-kernel. */
#define MW_TASK_CARTPOLE_DISCRETE 0
#define MW_TASK_CARTPOLE_CONTINUOUS_BALANCING 1
#define MW_TASK_CARTPOLE_CONTINUOUS_SWINGUP 2
#define MW_TASK_PENDULUM_SWINGUP 3
/* Position-target control of the 9-dof Panda (BASELINE config 4): actions
 * float32 [n_worlds, 9] are the Position-mode targets of every joint, the
 * JointController PID (gains: mw_set_joint_pid; called between steps, the
 * next step starts that dof's controller from a reset state in every world)
 * runs every physics step; obs = [q, qd] (18), reward = -|q - target|^2, done = TimeLimit only; reset
 * to the Panda wrapper's pose (python/gym_ignition_environments/models/
 * panda.py:41-44) with joints 1 and 6 at mid-range (test_pid_controllers.py:
 * 49-59) and the fingers half open, + U(-0.05, 0.05) per joint. */
#define MW_TASK_PANDA_POSITION_TRACKING 4

typedef struct {
    int32_t kind;
    int32_t max_episode_steps;       /* 0 = no time limit                   */
    int32_t reward_cart_at_center;   /* CartPole balancing tasks            */
    int32_t world_offset;            /* global index of world 0 (sharding):  */
                                     /* reset streams do not depend on P     */
    uint64_t seed;
    /* Per-world physics randomisation, resampled at every (auto-)reset like
     * GazeboEnvRandomizer.reset (python/gym_ignition/randomizers/
     * gazebo_env_randomizer.py): MW_RAND_MASS adds max(U(mass_low, mass_high), 0)
     * to every moving body's mass (randomizers/cartpole.py:100-135 with
     * SDFRandomizer's force_positive, randomizers/model/sdf.py:294-295; COM and
     * rotational inertia unchanged), MW_RAND_GRAVITY sets the world gravity to
     * (0, 0, N(gravity_mean, gravity_std)) (randomizers/cartpole.py:51-56). */
    int32_t randomize;
    float mass_low, mass_high;
    float gravity_mean, gravity_std;
    int32_t pad_;
} mw_task_config;
#define MW_RAND_MASS 1
#define MW_RAND_GRAVITY 2

int mw_vecenv_create(mw_sim* sim, const mw_task_config* cfg, mw_vecenv** out);
void mw_vecenv_destroy(mw_vecenv* env);
int mw_vecenv_obs_dim(const mw_vecenv* env, int32_t* n);
/* Reset every world (episode 0); obs_dev float32 [n_worlds, obs_dim]. */
int mw_vecenv_reset(mw_vecenv* env, float* obs_dev);
/* One env step of every world, asynchronous on the sim's stream.
 *   actions_dev: int32 [n_worlds] (discrete), float32 [n_worlds], or
 *                float32 [n_worlds, dofs] (position-target tasks)
 *   obs_dev float32 [n_worlds, obs_dim]  (reset obs where done)
 *   reward_dev float32 [n_worlds], done_dev uint8 [n_worlds]
 *   terminal_obs_dev float32 [n_worlds, obs_dim] (written only where done) */
int mw_vecenv_step(mw_vecenv* env, const void* actions_dev, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, float* terminal_obs_dev);
/* T env steps fused in one launch (open loop: actions [T, n_worlds]); outputs
 * [T, ...]. */
int mw_vecenv_rollout(mw_vecenv* env, int32_t T, const void* actions_dev, float* obs_dev,
                      float* reward_dev, uint8_t* done_dev, float* terminal_obs_dev);
/* Copy the per-world episode / step counters (uint32 [n_worlds]) into caller
 * device buffers (async, on the sim's stream). */
int mw_vecenv_counters(mw_vecenv* env, uint32_t* episode_dev, uint32_t* steps_dev);
/* Copy the per-world randomised physics (body masses float32 [n_dofs][n_worlds],
 * gravity z float32 [n_worlds]) into caller device buffers; MW_ESTATE when the
 * env was created without randomisation. */
int mw_vecenv_physics(mw_vecenv* env, float* mass_dev, float* gravity_z_dev);

/* ---- batched environment of articulated floating-base models ----
 * Any model stepped by the world-per-wavefront kernel with a floating base
 * (mw_float_kernel == 2 and mw_is_floating: the quadruped, the iCub-class
 * humanoid, any tree of <= 48 bodies without ball joints).  One step is three
 * launches on the sim's stream -- actions -> device commands, the unchanged
 * run, observation / reward / done / auto-reset -- with no host copy and no
 * synchronisation, so a step can be captured into a graph.
 *   actions  float32 [n_worlds, n_dofs]: joint torques (MW_FLOAT_ACTION_TORQUE,
 *            every dof in Force mode, clipped to the effort limits by the run
 *            as mw_set_joint_force_targets' values are) or Position-mode
 *            targets (MW_FLOAT_ACTION_POSITION: JointController PID every
 *            physics step, gains from mw_set_joint_pid before creation)
 *   obs      float32 [n_worlds, 13 + 2 n_dofs + n_contact_links]: base position
 *            (3), orientation wxyz (4), world linear velocity of the base
 *            origin (3), world angular velocity (3) -- mw_get_base_velocity's
 *            quantities --, q, qd, then per contact link the world z force (N)
 *            summed over the link's contact points of the last physics step
 *   done     base z < z_min, or the world z component of the base's z axis
 *            < cos_tilt_max, or the world diverged (mw_diverged: its state is
 *            not finite, or its action was not -- the env flags and counts
 *            such a world itself, since the run's effort clamp would turn a
 *            NaN torque into -effort silently), or max_episode_steps (0 =
 *            none) reached
 *   reward   alive_bonus [not done by height / tilt / divergence] + w_forward
 *            v_x - w_action sum a^2 - w_pose sum (q - home_q)^2, on the state
 *            after the run and before any reset
 *   reset    q = clip(home_q + U(-joint_noise, joint_noise), limits) from
 *            Philox4x32-10 keyed by seed, counter (world_offset + world,
 *            episode, dof / 4, 0); qd = 0; base at home_base, at rest.  A done
 *            world's reset is left on the device as pending resets, applied by
 *            the next step's run exactly as the host reset setters' are (warm
 *            start cold, PID state zero, divergence flag re-armed); its obs
 *            row already shows the reset state (zero velocities and contact
 *            forces), terminal_obs the finished episode's last observation.
 * The handle is an mw_vecenv: mw_vecenv_destroy / _obs_dim / _reset / _step /
 * _counters work on it (mw_vecenv_reset also runs the simulator paused, so the
 * state getters show the reset at once); mw_vecenv_rollout fails with
 * MW_EINVAL, mw_vecenv_physics with MW_ESTATE.
 * While the env exists it owns the simulator's commands and pending resets:
 * the host setters that write them -- mw_set_joint_{force,velocity,position}
 * _targets, mw_reset_joint_positions / _velocities, mw_reset_base_pose /
 * _velocity, mw_set_joint_control_mode, mw_set_joint_pid and mw_set_state --
 * fail with MW_ESTATE instead of being overwritten by (or overwriting) the
 * device writes; they work again after mw_vecenv_destroy. */
#define MW_FLOAT_ACTION_TORQUE 0
#define MW_FLOAT_ACTION_POSITION 1
typedef struct {
    int32_t action_mode;
    int32_t max_episode_steps;      /* 0 = no time limit                    */
    int32_t world_offset;           /* global index of world 0 (sharding)   */
    int32_t n_contact_links;        /* <= 8                                 */
    uint64_t seed;
    float z_min, cos_tilt_max;
    float alive_bonus, w_forward, w_action, w_pose;
    float joint_noise;
    float pad_;
    float home_base[7];             /* x y z qw qx qy qz                    */
    const float* home_q;            /* [n_dofs] (the caller's length; FloatVecEnv checks it) */
    const int32_t* contact_links;   /* [n_contact_links] dof index of the link, -1 = base */
} mw_float_task_config;
int mw_floatenv_create(mw_sim* sim, const mw_float_task_config* cfg, mw_vecenv** out);

/* Domain randomisation of a floating-base env: pushes on the base and
 * per-world ground friction, sampled on the device.  Call it after
 * mw_floatenv_create and before the first mw_vecenv_reset (MW_ESTATE after
 * it, or on another kind of env).  The step stays three launches without host
 * copies or synchronisation; the observation layout does not change.
 * Every draw is Philox4x32-10 keyed by the env's seed with the counter (global
 * world, episode, block, 0), in blocks the reset draw never reaches:
 *   episode  block 0x40000000: phase = r[0] % push_interval,
 *            mu = U(friction_lo, friction_hi) from r[1]; drawn when the
 *            episode's reset is issued and applied by the run that applies
 *            the reset (friction randomisation is on when friction_hi > 0)
 *   pushes   with t the steps already taken in the episode, k = (t + phase) /
 *            push_interval and o = (t + phase) % push_interval: the step is
 *            pushed iff o < push_steps, with the world wrench (fx, fy, 0, 0,
 *            0, tz) on the base link in mw_apply_link_wrench's convention,
 *            constant over the run's substeps; fx, fy = U(-push_force,
 *            push_force) from r[0], r[1] and tz = U(-push_torque,
 *            push_torque) from r[2] of block 0x80000000 | k
 * U(lo, hi) of a word r is lo + (hi - lo) (r >> 8) 2^-24 in float32.
 * push_dev float32 [n_worlds, 6] and friction_dev float32 [n_worlds] are
 * caller-owned device buffers (either may be NULL) that must outlive the env:
 * every step writes the wrench it applied into push_dev, every reset the new
 * episode's coefficient into friction_dev.
 * While an env with pushes exists mw_apply_link_wrench fails with MW_ESTATE
 * (the wrench buffer is the env's), while one with friction randomisation
 * exists mw_set_ground_friction and mw_set_ground_plane do. */
typedef struct {
    int32_t push_interval;          /* steps between push starts; 0 = no pushes */
    int32_t push_steps;             /* steps a push lasts, 1..push_interval     */
    float push_force;               /* N, >= 0                                  */
    float push_torque;              /* N m, >= 0                                */
    float friction_lo, friction_hi; /* 0 <= lo <= hi; hi > 0 turns it on        */
} mw_float_rand_config;
int mw_floatenv_randomize(mw_vecenv* env, const mw_float_rand_config* cfg, float* push_dev, float* friction_dev);

/* Velocity-command locomotion task of a floating-base env, sampled and scored
 * on the device.  Call it after mw_floatenv_create and before the first
 * mw_vecenv_reset (MW_ESTATE after it, or on another kind of env); it combines
 * freely with mw_floatenv_randomize, in either order.  The step stays three
 * launches without host copies or synchronisation.  A refused call leaves the
 * env as it was.
 *   obs      the row grows to 25 + 3 n_dofs + n_contact_links words
 *            (mw_vecenv_obs_dim returns the new width): behind the words of
 *            the plain env come the projected gravity (world -z in the body
 *            frame, 3), the body-frame linear (3) and angular (3) velocity of
 *            the base, the command (v_x, v_y, yaw rate) in force for the next
 *            step (3) and the raw action just applied (n_dofs, zeros after a
 *            reset)
 *   command  a pure function of (seed, global world, episode, k), k = steps
 *            taken / cmd_interval (0 with cmd_interval 0, k < 2^30): Philox
 *            block 0xC0000000 | k of the counter mw_floatenv_randomize
 *            describes; r[0..2] give U(cmd_lo[i], cmd_hi[i]), and the command
 *            is zero where (r[3] >> 8) 2^-24 < cmd_zero_prob.  The reward of a
 *            step uses the command the previous observation showed; the
 *            observation after it shows the command of step count t + 1
 *            (terminal_obs: the one the finished episode would have had), a
 *            reset observation command 0 of the new episode.
 *   actions  kept raw for the observation and the action-rate term; with
 *            action_scale > 0 the run receives home_q[d] + action_scale a_d
 *            (position mode, one fused multiply-add) or action_scale a_d
 *            (torque mode).  sum a^2 and the non-finite test use the raw action.
 *   reward   the four terms of mw_floatenv_create, and with v, w the
 *            body-frame linear and angular velocity and c the command
 *              + w_track_lin exp(-((c_x - v_x)^2 + (c_y - v_y)^2) / track_sigma)
 *              + w_track_yaw exp(-(c_yaw - w_z)^2 / track_sigma)
 *              - w_lin_z v_z^2 - w_ang_xy (w_x^2 + w_y^2)
 *              - w_action_rate sum (a_t - a_{t-1})^2        (a_{t-1} = 0 on an
 *                episode's first step)
 *              + w_air_time sum_j [touchdown_j] (air_steps_j env_dt -
 *                air_time_target) where c_x^2 + c_y^2 > cmd_min^2
 *            Contact link j is in contact when its observed z force exceeds
 *            contact_force_min; air_steps_j counts the steps without contact,
 *            is paid and zeroed on the first step with contact after a flight
 *            and zeroed on reset; env_dt = steps_per_run step_size.
 * command_dev float32 [n_worlds, 3] is a caller-owned device buffer (may be
 * NULL) that must outlive the env: every step and reset writes the command
 * words of obs into it. */
typedef struct {
    float cmd_lo[3], cmd_hi[3];     /* v_x, v_y (m/s), yaw rate (rad/s); lo <= hi */
    int32_t cmd_interval;           /* steps between draws; 0 = once per episode  */
    float cmd_zero_prob;            /* in [0, 1]                                  */
    float cmd_min;                  /* m/s                                        */
    float action_scale;             /* >= 0; 0 = raw actions                      */
    float w_track_lin, w_track_yaw;
    float track_sigma;              /* > 0                                        */
    float w_lin_z, w_ang_xy, w_action_rate;
    float w_air_time;               /* != 0 needs contact links                   */
    float air_time_target;          /* s                                          */
    float contact_force_min;        /* N                                          */
} mw_float_loco_config;
int mw_floatenv_locomotion(mw_vecenv* env, const mw_float_loco_config* cfg, float* command_dev);

/* Inertia randomisation of a floating-base env: per-world link masses and a
 * payload on the base, drawn on the device wherever a reset is issued (every
 * world on mw_vecenv_reset).  Call it after mw_floatenv_create and before the
 * first mw_vecenv_reset (MW_ESTATE after it, or on another kind of env), in
 * any order with mw_floatenv_randomize and mw_floatenv_locomotion.  The step
 * stays three launches without host copies or synchronisation; a refused call
 * leaves the env as it was.  The draws are words of new blocks of the Philox
 * counter (global world, episode, block, 0) mw_floatenv_randomize describes,
 * so they are a pure function of (seed, global world, episode):
 *   scales   link k (0 = the base, 1 + i = the body of dof i) takes s_k =
 *            U(mass_scale_lo, mass_scale_hi) from word k % 4 of block
 *            0x40000100 | (k / 4): mass = s mass0, Io[j] = s Io0[j], the centre
 *            of mass kept (mass0, Io0: the model's nominal float32 words).  On
 *            when mass_scale_hi > 0; needs 0 < lo <= hi.
 *   payload  a point mass m_p = U(payload_lo, payload_hi) kg at p =
 *            (U(-box_x, box_x), U(-box_y, box_y), U(-box_z, box_z)) m in the
 *            base frame, words 0..3 of block 0x40000180, added to the (scaled)
 *            base:  m' = m + m_p,  com' = (m com + m_p p) / m',
 *            Io' = Io + m_p (|p|^2 1 - p p^T).  On when payload_hi > 0; needs
 *            0 <= lo <= hi and payload_box >= 0.
 * A feature that is off is skipped, not fed neutral values.  The words are
 * written into the simulator's per-world link parameters (mw_link_params
 * reads them back) and the run that applies the reset reads them with it.
 * inertial_dev float32 [n_worlds, n_dofs + 1, 10] is a caller-owned device
 * buffer (may be NULL) that must outlive the env: every reset writes the words
 * in force for the new episode, base first, in mw_set_link_params' layout.
 * draws_dev float32 [n_worlds, n_dofs + 5], likewise: the draws themselves,
 * s_0 .. s_n, m_p, p xyz (scales of 1 and a zero payload where a feature is
 * off) -- what a critic with privileged information would be given.
 * While such an env exists mw_set_link_params fails with MW_ESTATE. */
typedef struct {
    float mass_scale_lo, mass_scale_hi; /* 0 < lo <= hi; hi > 0 turns it on  */
    float payload_lo, payload_hi;       /* kg, 0 <= lo <= hi; hi > 0 turns it on */
    float payload_box[3];               /* m, half extents in the base frame */
} mw_float_inertia_config;
int mw_floatenv_inertia(mw_vecenv* env, const mw_float_inertia_config* cfg, float* inertial_dev, float* draws_dev);

/* Joint randomisation of a floating-base env: per-world viscous damping,
 * Coulomb friction and effort limit of the joints, drawn on the device
 * wherever a reset is issued (every world on mw_vecenv_reset).  Call order and
 * refusals are mw_floatenv_inertia's: after mw_floatenv_create and before the
 * first mw_vecenv_reset (MW_ESTATE after it, or on another kind of env), in any
 * order with the other three configuration calls; the step stays three
 * launches; a refused call leaves the env as it was, everything off returns
 * the env as made.  Joint d takes words 0, 1 and 2 of block 0x40000200 | d of
 * the Philox counter (global world, episode, block, 0), so the draws are a
 * pure function of (seed, global world, episode):
 *   damping   a_d = U(damping_lo, damping_hi) N m s/rad added to the nominal
 *             word.  On when damping_hi > 0; needs 0 <= lo <= hi.
 *   friction  f_d = U(friction_lo, friction_hi) N m added to the nominal word,
 *             likewise.
 *   effort    s_d = U(effort_scale_lo, effort_scale_hi), effort = s_d effort0;
 *             an unbounded nominal limit (FLT_MAX) is kept.  On when
 *             effort_scale_hi > 0; needs 0 < lo <= hi.
 * dof_mask bit d selects joint d (0 = every joint); a feature that is off and
 * a joint outside the mask are skipped, not fed neutral values.  Friction adds
 * one LCP row per moving joint: see the row budget of mw_set_joint_dynamics --
 * the mask is there so that, say, only the legs are randomised.  The words go
 * into the simulator's per-world records (mw_joint_dynamics reads them back;
 * the instance choices of mw_set_joint_dynamics follow what is drawn) and the
 * run that applies the reset reads them with it.  joints_dev float32
 * [n_worlds, n_dofs, 3] is a caller-owned device buffer (may be NULL) that must
 * outlive the env: every reset writes damping, friction and effort in force
 * for the new episode (the nominal words of a joint outside the mask).
 * draws_dev float32 [n_worlds, n_dofs, 3], likewise: a_d, f_d, s_d, and 0, 0, 1
 * where a feature is off or the joint is outside the mask.  While such an env exists mw_set_joint_dynamics and
 * mw_set_link_params fail with MW_ESTATE. */
typedef struct {
    float damping_lo, damping_hi;           /* N m s/rad added to the nominal; 0 <= lo <= hi; hi > 0 turns it on */
    float friction_lo, friction_hi;         /* N m added to the nominal; likewise */
    float effort_scale_lo, effort_scale_hi; /* factor on the nominal limit; 0 < lo <= hi; hi > 0 turns it on */
    uint64_t dof_mask;                      /* bit d: joint d is drawn; 0 = every joint */
} mw_float_joint_config;
int mw_floatenv_joints(mw_vecenv* env, const mw_float_joint_config* cfg, float* joints_dev, float* draws_dev);

/* Observation noise and action latency of a floating-base env, both drawn on
 * the device inside the step's three launches (no host copy, capturable), each
 * off unless configured; with both off every output is what it was.  Call it
 * after mw_floatenv_create and before the first mw_vecenv_reset (MW_ESTATE
 * after it, or on another kind of env), and after mw_floatenv_locomotion,
 * which changes the width of the rows: once a feature is on here
 * mw_floatenv_locomotion fails with MW_ESTATE.  A refused call leaves the env
 * as it was; a call with amplitude NULL and delay_hi 0 returns it as made.
 *   noise    on when amplitude is not NULL: mw_vecenv_obs_dim host floats, all
 *            finite and >= 0, and 0 on the command and last-action words of
 *            the locomotion rows (MW_EINVAL otherwise).  Word k of a row of obs
 *            or terminal_obs is clean[k] + amplitude[k] u in one fused
 *            multiply-add, u = -1 + (x >> 8) 2^-23 in [-1, 1), x word k % 4 of
 *            Philox4x32-10 keyed by the env's seed with the counter (global
 *            world, episode, k / 4, 1 + t) -- every other draw has 0 in the
 *            fourth word.  (episode, t) are the counters the row belongs to: a
 *            row after a step the updated ones, a reset row (episode + 1, 0),
 *            a terminal_obs row the finished episode and its final step count,
 *            mw_vecenv_reset (0, 0).  A word of amplitude 0 keeps the clean
 *            word's bits.  Reward, termination, the command schedule and the
 *            air-time counters use the clean rows.  clean_obs_dev and
 *            clean_terminal_obs_dev, float32 [n_worlds, obs_dim], are
 *            caller-owned device buffers (either may be NULL) that must outlive
 *            the env: the clean rows of obs, and of terminal_obs for the done
 *            worlds, of every step and reset; ignored with the noise off.
 *   latency  on when delay_hi > 0; needs 0 <= delay_lo <= delay_hi <=
 *            MW_FLOAT_MAX_ACTION_DELAY.  Every episode draws d = delay_lo +
 *            r[2] % (delay_hi - delay_lo + 1) from word 2 of its episode block
 *            (0x40000000, see mw_floatenv_randomize) when its reset is issued.
 *            The step with t steps taken in the episode keeps its action in
 *            slot t % (delay_hi + 1) of a per-world ring and hands the run the
 *            action of step t - d: scaled like an undelayed one (action_scale,
 *            home_q), and while t < d the neutral command instead, home_q in
 *            position mode and 0 in torque mode.  sum a^2, the action-rate
 *            term, the last-action words and the non-finite test stay on the
 *            action just submitted.  delay_dev int32 [n_worlds] is a
 *            caller-owned device buffer (may be NULL) that must outlive the
 *            env: every reset writes the new episode's d. */
#define MW_FLOAT_MAX_ACTION_DELAY 8
typedef struct {
    int32_t delay_lo, delay_hi;     /* control steps, 0 <= lo <= hi <= 8; hi > 0 turns it on */
} mw_float_noise_config;
int mw_floatenv_noise(mw_vecenv* env, const mw_float_noise_config* cfg, const float* amplitude /* host, obs_dim words or NULL */,
                      float* clean_obs_dev, float* clean_terminal_obs_dev, int32_t* delay_dev);

/* Shaping rewards, contact termination and per-episode statistics of a
 * floating-base env, computed inside the step's three launches (no host copy,
 * capturable); off unless configured, and with it off every output is what it
 * was.  Call it after mw_floatenv_create and before the first mw_vecenv_reset
 * (MW_ESTATE after it, or on another kind of env), and after
 * mw_floatenv_locomotion where weights[9] (stand_still) is set (MW_ESTATE
 * without the locomotion task).  A refused call leaves the env as it was; a
 * config of all zeros without links returns it as made.
 *   terms    ten columns in fixed order; column k of a world's row is the signed
 *            contribution -weights[k] x_k of the step, 0 where weights[k] is 0:
 *              0 torque         sum_d tau_d^2
 *              1 power          sum_d |tau_d qd_d|
 *              2 joint_acc      sum_d ((qd_d - qd_d of the last step) / env_dt)^2,
 *                               env_dt = steps_per_run step_size; from rest on
 *                               an episode's first step
 *              3 orientation    g_x^2 + g_y^2 of the projected gravity (world -z
 *                               in the body frame)
 *              4 base_height    (z - base_height_target)^2
 *              5 joint_limits   sum_d max(0, lo_d - q_d) + max(0, q_d - hi_d), lo
 *                               / hi = centre -/+ soft_limit half-range of the
 *                               position limits; a joint without finite limits
 *                               contributes nothing
 *              6 collision      number of penalised_links whose contact force
 *                               norm exceeds collision_force_min
 *              7 stumble        number of contact links (mw_float_task_config)
 *                               with hypot(f_x, f_y) > stumble_ratio |f_z| and
 *                               |f_z| > 0
 *              8 contact_force  sum over the contact links of max(0, |f| -
 *                               max_contact_force)
 *              9 stand_still    sum_d |q_d - home_q_d| where the command the step
 *                               ran under has v_x^2 + v_y^2 <= cmd_min^2, else 0
 *            A link's f is the sum of the force vectors of its active contact
 *            points, in world axes.  tau_d is the torque the run applied:
 *            clamp(u_d, +-effort_d) with u_d the JointController's last output
 *            (position mode) or the command the run received, after scaling
 *            and latency (torque mode, where it acts on the first physics step
 *            of the run); effort_d is the limit the run clamped with, the
 *            world's own under mw_set_joint_dynamics / mw_floatenv_joints.
 *            Every product and sum has a defined float32 rounding
 *            (csrc/float_task.hpp); sums over dofs or links are taken as four
 *            partial sums, item i in partial i % 4, added in order.
 *   reward   the reward of the env as configured so far, then + term 0 ... +
 *            term 9 in that order.
 *   done     additionally terminated -- not truncated: the alive bonus is lost,
 *            as for z_min -- when a contact point of a termination link is
 *            active with a force norm above termination_force.  Contacts here
 *            and in the terms are those of the LAST physics step of the run
 *            (what mw_get_contacts shows), not of every step of it: with
 *            steps_per_run > 1 a touch that ends before the run's last physics
 *            step is not seen.
 *   diverged a world flagged diverged reports ten zeros and adds nothing to its
 *            running sums: its state is not finite, and the episode ends.
 *   stats    per world the running return (the sum of reward as written), the
 *            length and the ten term sums of the current episode; where done is
 *            set they are copied to ep_return_dev / ep_length_dev / ep_terms_dev
 *            and zeroed.  mw_vecenv_reset zeroes the running sums and leaves the
 *            finished-episode buffers alone; a world's entries are valid once it
 *            has been done.
 * penalised_links (at most 8) and termination_links (any number) are dof
 * indices of links, -1 = the base, as contact_links.  A link of either list
 * that owns none of the 32 contact slots of the wave kernel's mask -- no
 * collision shape, or only slots >= 32 -- is refused with MW_EINVAL, since it
 * could never fire; so are weights[6] without penalised links and weights[7] /
 * weights[8] without contact links, a negative weight or threshold, a
 * non-finite field and soft_limit outside (0, 1].
 * terms_dev float32 [n_worlds, 10], torque_dev float32 [n_worlds, n_dofs] (the
 * tau the terms used, written every step whatever the weights),
 * ep_return_dev float32 [n_worlds], ep_length_dev int32 [n_worlds] and
 * ep_terms_dev float32 [n_worlds, 10] are caller-owned device buffers (each may
 * be NULL) that must outlive the env. */
#define MW_FLOAT_SHAPE_TERMS 10
typedef struct {
    float weights[MW_FLOAT_SHAPE_TERMS]; /* >= 0, in the order above             */
    float base_height_target;            /* m                                   */
    float soft_limit;                    /* in (0, 1]                           */
    float collision_force_min;           /* N, >= 0                             */
    float stumble_ratio;                 /* >= 0                                */
    float max_contact_force;             /* N, >= 0                             */
    float termination_force;             /* N, >= 0                             */
    int32_t n_penalised_links;           /* <= 8                                */
    int32_t n_termination_links;
    const int32_t* penalised_links;      /* [n_penalised_links] dof index, -1 = base */
    const int32_t* termination_links;    /* [n_termination_links] likewise      */
} mw_float_shape_config;
int mw_floatenv_shaping(mw_vecenv* env, const mw_float_shape_config* cfg, float* terms_dev, float* torque_dev,
                        float* ep_return_dev, int32_t* ep_length_dev, float* ep_terms_dev);

/* Initial-state randomisation and a reset-state bank of a floating-base env:
 * where an episode starts is drawn on the device by the launch that issues the
 * reset (the post launch, and mw_vecenv_reset's), inside the step's three
 * launches (no host copy, capturable).  Off unless configured, and with it off
 * every output is what it was.  Call it after mw_floatenv_create and before the
 * first mw_vecenv_reset (MW_ESTATE after it, or on another kind of env), in any
 * order with the other configure calls.  A refused call leaves the env as it
 * was; a config of all zeros without a bank and without output buffers returns
 * it as made.
 *   base row 13 + 2 n float32 words in the layout of a row of obs: base
 *            position (3), quaternion wxyz (4), world linear (3) and angular
 *            (3) velocity, q (n), qd (n) -- a recorded observation row is a
 *            valid row.  Without a bank it is the home row: home_base, zeros,
 *            home_q, zeros.  With n_states = K > 0, states_dev float32 [K, 13 +
 *            2 n] is a caller-owned device buffer that must outlive the env;
 *            with r word 0 and 1 of block 0x40000300 of the counter (global
 *            world, episode, block, 0) mw_floatenv_randomize describes, an
 *            episode starts from row r[0] % K where (r[1] >> 8) 2^-24 <
 *            state_prob, else from the home row.  The rows are read through
 *            the pointer at every reset: rows overwritten on the env's stream
 *            between two steps are what the next resets see.  Their content is
 *            the caller's: a zero quaternion or a non-finite word gives a
 *            non-finite state, which the run flags diverged, so that the next
 *            step ends the episode and resets the world.
 *   draws    on top of the row, each group off when all its bounds are zero;
 *            U(lo, hi) is lo + (hi - lo) (x >> 8) 2^-24 of one Philox word:
 *              block 0x40000301  words 0..2: offsets added to the base position
 *                                (pos_lo / pos_hi, m, world frame)
 *              block 0x40000302  words 0..2: roll, pitch, yaw (rpy_lo / rpy_hi,
 *                                rad); the orientation becomes qz(yaw) qy(pitch)
 *                                qx(roll) q_row -- world-frame rotations after
 *                                the row's own -- normalised in float32.  With
 *                                the group off the row's quaternion is written
 *                                as it is (the run normalises what it takes)
 *              block 0x40000303  words 0..2: added to the world linear velocity
 *                                (lin_vel_lo / lin_vel_hi, m/s)
 *              block 0x40000304  words 0..2: added to the world angular velocity
 *                                (ang_vel_lo / ang_vel_hi, rad/s)
 *              block 0x40000340 | d / 4, word d % 4: U(-joint_vel, joint_vel)
 *                                added to qd of joint d (rad/s)
 *            Joint positions are row_q + U(-joint_noise, joint_noise) clipped
 *            into the position limits: the draw of mw_floatenv_create (blocks 0
 *            .. (n + 3) / 4 - 1) with row_q in the place of home_q.  No other
 *            draw of the env changes.
 *   reset    the reset row of obs is the observation of the drawn state (in the
 *            locomotion task the projected gravity and the body-frame
 *            velocities too), and joint_acc of the shaping terms is taken from
 *            the drawn qd on an episode's first step.  Nothing checks a drawn
 *            state against z_min, cos_tilt_max or the ground: a start beyond
 *            them ends at the next step, a start below the ground is the
 *            caller's to avoid through the ranges.
 * state_dev float32 [n_worlds, 13 + 2 n] (the state the current episode started
 * from: the first 13 + 2 n words of the clean reset row) and draws_dev float32
 * [n_worlds, 13 + n] (the position offsets, roll pitch yaw, the linear and the
 * angular velocity offsets, the bank row as a float -- -1 the home row -- and
 * the n joint-velocity draws) are caller-owned device buffers (each may be NULL)
 * that must outlive the env; a world's rows are written by every reset of it.
 * MW_EINVAL: a non-finite bound or lo > hi, joint_vel < 0 or non-finite,
 * state_prob outside [0, 1], n_states < 0, n_states > 0 with states_dev NULL
 * or n_states == 0 with states_dev given, n_states > 0 on an env with
 * mw_floatenv_tracking (whose clips are the bank). */
typedef struct {
    float pos_lo[3], pos_hi[3];         /* m, world frame                       */
    float rpy_lo[3], rpy_hi[3];         /* rad: roll, pitch, yaw                */
    float lin_vel_lo[3], lin_vel_hi[3]; /* m/s, world frame                     */
    float ang_vel_lo[3], ang_vel_hi[3]; /* rad/s, world frame                   */
    float joint_vel;                    /* rad/s, >= 0                          */
    float state_prob;                   /* in [0, 1]                            */
    int32_t n_states;                   /* rows of states_dev, 0 = no bank      */
} mw_float_init_config;
int mw_floatenv_init_state(mw_vecenv* env, const mw_float_init_config* cfg, const float* states_dev, float* state_dev,
                           float* draws_dev);

/* Motion-clip tracking task of a floating-base env (DeepMimic-style imitation
 * with reference-state initialisation): every world follows a clip of recorded
 * states on an integer frame clock, its episodes start from a drawn frame of a
 * drawn clip, and the reward, the termination and the observation compare the
 * state with the clip -- inside the step's three launches (no host copy,
 * capturable).  Off unless configured, and with it off every output is what it
 * was.  It changes the width of the rows: call it after mw_floatenv_create,
 * after mw_floatenv_locomotion (if any), before mw_floatenv_noise and before
 * the first mw_vecenv_reset (MW_ESTATE otherwise, or on another kind of env).
 * A refused call leaves the env as it was.
 *   clips    clips_dev float32 [n_frames, 13 + 2 n] is a caller-owned device
 *            buffer that must outlive the env, rows in the layout of the first
 *            13 + 2 n words of a row of obs (and of the bank of
 *            mw_floatenv_init_state): recorded observation rows make a clip.
 *            It is read through the pointer at every step and reset.  Clip c is
 *            rows clip_first[c] .. clip_first[c] + clip_length[c] - 1, length >=
 *            2, inside the buffer; at most MW_FLOAT_MAX_CLIPS clips.
 *   clock    frame_num / frame_den frames per control step, both >= 1.  With f0
 *            the start frame and t the steps taken in the episode, x_num = f0
 *            frame_den + t frame_num; the reference of that instant x_t is row
 *            i = x_num / frame_den blended with row i + 1 by a = (x_num %
 *            frame_den) / frame_den (float32): integers, no drift.  Every word
 *            is p0 + a (p1 - p0); the quaternion is blended the same way after
 *            q1 is negated where q0 . q1 < 0, then normalised (nlerp).
 *   loop     clip_loop[c] != 0: the period is length - 1 frames, the last row
 *            being the first pose again; i wraps modulo the period and the
 *            reference base x and y gain wraps (pos[last] - pos[first]).  The
 *            heading is assumed periodic: a clip that turns over a period is
 *            not followed across the wrap.  clip_loop[c] == 0: the episode ends
 *            truncated -- done, not terminated, the alive bonus kept, as at the
 *            time limit -- at the first step whose reference would need a row
 *            beyond the last; that step is compared with the last row.
 *   reset    a reset takes its base row from the clip where the plain reset
 *            takes the home row, through the path of mw_floatenv_init_state: with
 *            r the words of block 0x40000400 of the counter (global world,
 *            episode, block, 0) mw_floatenv_randomize describes, the clip is c =
 *            r[0] % n_clips and the start frame f0 = r[1] % (length_c - 1) where
 *            (r[2] >> 8) 2^-24 < rsi_prob, else 0.  The offset groups of
 *            mw_floatenv_init_state and joint_noise apply on top of the clip row
 *            exactly as on a bank row; a bank (n_states > 0) together with
 *            tracking is refused, whichever call comes second.
 *   errors   the state after step t against the reference at x_t (wj the
 *            per-joint weights, 1 where joint_weights is NULL):
 *              0 pose      sum_d wj[d] (q_d - q^_d)^2
 *              1 velocity  sum_d wj[d] (qd_d - qd^_d)^2
 *              2 root_pos  |p - p^|^2
 *              3 root_rot  1 - (q . q^)^2
 *              4 root_vel  |v - v^|^2 + ang_scale |w - w^|^2   (world frame)
 *            The reward gains weights[k] expf(-scales[k] e_k) per error (with
 *            mw_floatenv_shaping the episode return includes them); a diverged
 *            world's terms are 0.  The episode ends terminated, without the
 *            alive bonus, where pose, root_pos or root_rot exceeds max_pose,
 *            max_root_pos or max_root_rot (0 = off).
 *   obs      the rows grow by a block behind everything else (after the
 *            locomotion block where there is one): sin(2 pi phi), cos(2 pi phi),
 *            the clip as a float, phi = x_t / (length - 1) (1 at a clip's end),
 *            and with obs_reference != 0 the n reference joint positions at
 *            x_{t+1}, the target of the next action.  terminal_obs carries the
 *            finished episode's values, the reset row those of x_0 and x_1.
 *            These words take no noise.
 * terms_dev and errors_dev float32 [n_worlds, 5] (the step's signed terms and
 * errors), clip_dev and frame_dev int32 [n_worlds] (the clip and the start frame
 * of the current episode) are caller-owned device buffers (each may be NULL)
 * that must outlive the env.
 * MW_EINVAL: n_clips outside [1, MW_FLOAT_MAX_CLIPS], a clip shorter than 2 rows
 * or outside [0, n_frames), frame_num or frame_den < 1, a weight, scale, bound,
 * joint weight or ang_scale that is negative or not finite, rsi_prob outside
 * [0, 1], clips_dev NULL, or a bank configured by mw_floatenv_init_state.
 * MW_ECAPACITY: the post launch's tiles in local memory -- the rows of obs,
 * the shaping tiles where on, and the 64 reference rows of this task -- exceed
 * what a block of the device may use; nothing is changed (mw_floatenv_shaping
 * called after this call makes the same check). */
#define MW_FLOAT_MAX_CLIPS 16
#define MW_FLOAT_TRACK_TERMS 5
typedef struct {
    int32_t n_frames;                          /* rows of clips_dev            */
    int32_t n_clips;
    int32_t clip_first[MW_FLOAT_MAX_CLIPS];
    int32_t clip_length[MW_FLOAT_MAX_CLIPS];
    int32_t clip_loop[MW_FLOAT_MAX_CLIPS];
    int32_t frame_num, frame_den;              /* frames per control step      */
    float weights[MW_FLOAT_TRACK_TERMS];       /* >= 0                         */
    float scales[MW_FLOAT_TRACK_TERMS];        /* >= 0                         */
    float ang_scale;                           /* >= 0                         */
    float max_pose, max_root_pos, max_root_rot; /* >= 0, 0 = off               */
    float rsi_prob;                            /* in [0, 1]                    */
    int32_t obs_reference;
    const float* joint_weights;                /* [n] >= 0, NULL = all 1 (host) */
} mw_float_track_config;
int mw_floatenv_tracking(mw_vecenv* env, const mw_float_track_config* cfg, const float* clips_dev, float* terms_dev,
                         float* errors_dev, int32_t* clip_dev, int32_t* frame_dev);

#ifdef __cplusplus
}
#endif
#endif /* MWSTEP_H */
