/*
 * pgx.h -- C-ABI of the MI355X-native batched Panda environment (libpgx.so).
 *
 * One handle owns the structure-of-arrays state of N lockstep environments on
 * one GPU.  Every call is asynchronous on the caller's HIP stream (passed as
 * void*, NULL = default stream) and takes plain device pointers into
 * caller-owned buffers (torch tensors on the Python side).  No call allocates,
 * frees or synchronises on the step path, so a step can be captured in a
 * hipGraph.
 *
 * Reference interfaces each entry point replaces (paths relative to
 * RaikoPipe/panda-gym):
 *   pgx_create          PandaReachEnv/PandaPushEnv/PandaPickAndPlaceEnv.__init__
 *                       panda_gym/envs/panda_tasks.py:37-88, RobotTaskEnv.__init__
 *                       panda_gym/envs/core.py:264-284, gym registration
 *                       panda_gym/__init__.py:23-91 (max_episode_steps)
 *   pgx_reset           RobotTaskEnv.reset core.py:298-308 -> Panda.reset
 *                       panda.py:290-298, Reach.reset reach.py:63-78,
 *                       Push.reset push.py:69-87, PickAndPlace.reset
 *                       pick_and_place.py:65-85
 *   pgx_step            RobotTaskEnv.step core.py:352-368 -> Panda.set_action
 *                       panda.py:120-172 (IK: pybullet.py:465-493), PyBullet.step
 *                       pybullet.py:68-71 (20 x stepSimulation), _get_obs
 *                       core.py:286-296, Task.is_success / compute_reward
 *                       reach.py:80-89, + gymnasium TimeLimit and SB3 VecEnv
 *                       auto-reset (terminal_observation)
 *   pgx_compute_reward  Task.compute_reward bound as env.compute_reward
 *                       (core.py:282; reach.py:84-89, push.py:93-98,
 *                       pick_and_place.py:91-96) over a batch (HER relabel)
 *   pgx_get_state       PyBullet.get_joint_angles / get_joint_velocities
 *                       pybullet.py:313-348 (device views of the SoA state)
 *   pgx_snapshot /      RobotTaskEnv.save_state / restore_state / remove_state
 *   pgx_restore /       core.py:310-336 -> PyBullet.save_state / restore_state /
 *   pgx_release         remove_state pybullet.py:79-102 (state ids)
 *   pgx_save_state /    the same snapshot into / out of a caller-owned device
 *   pgx_restore_state   buffer (no id)
 *
 * Error convention: every call returns PGX_OK (0) or a negative PGX_E_* code;
 * pgx_last_error() returns a thread-local message for the last failure.
 */
#ifndef PGX_H
#define PGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGX_MAX_LINKS 16
#define PGX_MAX_DOFS 9
#define PGX_MAX_ROWS 27
#define PGX_MAX_CAPSULES 16
/* Contact row budgets per env (Bullet keeps <= 4 points per colliding pair; the kernels keep
 * the deepest of those up to a fixed budget per group -- DESIGN.md section 4):
 * object vs table / plane, and robot vs table / plane / object / obstacles, the latter
 * PGX_ROBOT_POINTS_ONE_LANE by default and with pgx_config.contacts = PGX_CONTACTS_FULL
 * PGX_ROBOT_POINTS in Push / PickAndPlace and PGX_ROBOT_POINTS_ARM in Reach / ReachAO. */
#define PGX_OBJECT_POINTS 4
#define PGX_ROBOT_POINTS 12
#define PGX_ROBOT_POINTS_ARM 8
#define PGX_ROBOT_POINTS_ONE_LANE 4
#define PGX_CONTACT_SLOTS (PGX_OBJECT_POINTS + PGX_ROBOT_POINTS)
#define PGX_CONTACTS_FULL 2
/* Bullet's persistent contact manifolds of the robot's pairs with the cube and with the obstacles
 * (PGX_CONTACTS_FULL; btPersistentManifold): a pool of at most
 * PGX_MANIFOLD_POOL (Push / PickAndPlace) or PGX_MANIFOLD_POOL_AO (ReachAO) points per env, kept
 * across substeps and steps -- the point count, then per point in pool order PGX_MANIFOLD_POINT
 * values: kid = key + slot (key 32 + 16 c for capsule c against the cube, 32 + 24 c + 4 o against
 * obstacle o; slot = the point's index in its manifold, < 4), local A [3] (in the frame of the arm
 * joint that carries the capsule), local B [3] (cube frame; world for a static obstacle), normal on
 * B [3] (world, from B to the robot), distance, applied normal impulse.  The row id of a point is
 * its kid. */
#define PGX_MANIFOLD_POOL 16
#define PGX_MANIFOLD_POOL_AO 8
#define PGX_MANIFOLD_POINT 12

#define PGX_OK 0
#define PGX_E_INVALID -1
#define PGX_E_HIP -2
#define PGX_E_UNSUPPORTED -3
#define PGX_E_NOMEM -4

#define PGX_JOINT_REVOLUTE 0
#define PGX_JOINT_PRISMATIC 1
#define PGX_JOINT_FIXED 4

#define PGX_TASK_REACH 0
#define PGX_TASK_PUSH 1
#define PGX_TASK_PICK_AND_PLACE 2
#define PGX_TASK_REACH_AO 3        /* ReachAO, scenario "reachao_rand" (reach_ao.py:587-599) */

/* ReachAO "reachao_rand" scene (reach_ao.py:268-290, 573-599, 819-860): 3 spheres of
 * radius 0.05 and 3 cuboids of half extent 0.05, 4-5 of them active per episode. */
#define PGX_AO_OBSTACLES 6
#define PGX_AO_LINKS 9             /* collision links: panda_link1..8, panda_ee */

#define PGX_CONTROL_EE 0
#define PGX_CONTROL_JOINTS 1

#define PGX_REWARD_SPARSE 0
#define PGX_REWARD_DENSE 1
#define PGX_REWARD_SPARSE_AO 2   /* ReachAO relabel reward: -1 + (d < thr) (reach_ao.py:1320), collision term 0 */

/* solver row kinds (pgx_model.row_kind) */
#define PGX_ROW_MOTOR 0
#define PGX_ROW_LIMIT_LOWER 1
#define PGX_ROW_LIMIT_UPPER 2

/* Multibody description in Bullet link order (built from the URDF by
 * panda-gym_amd/model.py).  All frames are URDF frames except that link
 * state is reported at the inertial origin (COM), like getLinkState()[0]. */
typedef struct pgx_model {
    int32_t n_links;                       /* links excluding the fixed base */
    int32_t n_dofs;
    int32_t ee_link;                       /* Panda.ee_link = 11 (panda.py:68) */
    int32_t n_rows;                        /* solver rows in Bullet order */
    int32_t parent[PGX_MAX_LINKS];         /* -1 = base */
    int32_t jtype[PGX_MAX_LINKS];
    int32_t dof_of_link[PGX_MAX_LINKS];    /* -1 for fixed joints */
    int32_t link_of_dof[PGX_MAX_DOFS];
    int32_t has_limit[PGX_MAX_DOFS];
    int32_t row_kind[PGX_MAX_ROWS];
    int32_t row_dof[PGX_MAX_ROWS];
    int32_t pad0;
    double jpos[PGX_MAX_LINKS][3];         /* joint origin in parent URDF frame */
    double jrot[PGX_MAX_LINKS][9];         /* row-major */
    double axis[PGX_MAX_LINKS][3];         /* joint axis in joint frame */
    double com[PGX_MAX_LINKS][3];          /* inertial origin in URDF link frame */
    double mass[PGX_MAX_LINKS];
    double inertia[PGX_MAX_LINKS][3];      /* principal inertia (Bullet AABB rule) */
    double lower[PGX_MAX_DOFS];
    double upper[PGX_MAX_DOFS];
    /* Collision geometry for contacts: the URDF's <collision> cylinders with their
     * end spheres fused into capsules (segment a-b in the URDF frame of link
     * cap_link, radius), lone spheres as zero-length capsules. */
    int32_t n_capsules;
    int32_t pad1;
    int32_t cap_link[PGX_MAX_CAPSULES];
    int32_t cap_flags[PGX_MAX_CAPSULES];   /* PGX_CAP_* */
    double cap_a[PGX_MAX_CAPSULES][3];
    double cap_b[PGX_MAX_CAPSULES][3];
    double cap_radius[PGX_MAX_CAPSULES];
    /* Bullet's link compound AABB (btCompoundShape::getAabb with the identity) in the link's COM
     * frame, child and compound margins included: centre and half extents.  The link's angular
     * motion disc |half| + |centre| scales its contact breaking threshold
     * (pgx_sim_params.contact_distance, btCollisionShape::getContactBreakingThreshold). */
    double link_aabb_center[PGX_MAX_LINKS][3];
    double link_aabb_half[PGX_MAX_LINKS][3];
} pgx_model;

#define PGX_CAP_VS_TABLE 1                 /* capsule end spheres collide with table / plane */
#define PGX_CAP_VS_OBJECT 2                /* capsule collides with the object (cube) */

/* Physics / solver constants (pybullet defaults as used by the reference). */
typedef struct pgx_sim_params {
    double dt;                    /* 1/500 (pybullet.py:50) */
    double gravity[3];            /* (0,0,-9.81) (pybullet.py:54) */
    double lin_damping;           /* btMultiBody default 0.04 */
    double ang_damping;           /* btMultiBody default 0.04 */
    double max_coord_vel;         /* btMultiBody::m_maxCoordinateVelocity 100 */
    double residual_threshold;    /* solver least-squares residual 1e-7 */
    double erp;                   /* joint-limit violation ERP 0.2 */
    double limit_max_impulse;     /* btMultiBodyConstraint default 100 */
    double motor_kp;              /* POSITION_CONTROL default positionGain 0.1 */
    double motor_kd;              /* POSITION_CONTROL default velocityGain 1.0 */
    double ik_residual;           /* calculateInverseKinematics residual 1e-4 */
    double ik_damping;            /* per-joint DLS damping 0.5 */
    double ik_max_angle;          /* BussIK MaxAngleDLS = pi/4 */
    int32_t n_substeps;           /* 20 (pybullet.py:25) */
    int32_t num_iterations;       /* numSolverIterations 50 */
    int32_t ik_max_iters;         /* maxNumIterations 20 */
    int32_t flags;                /* PGX_FLAG_* hypotheses (oracle only) */
    double contact_distance;      /* gContactBreakingThreshold 0.02.  Bullet's dispatcher scales it per
                                     pair (btCollisionDispatcher::getNewManifold with its default flag
                                     CD_USE_RELATIVE_CONTACT_BREAKING_THRESHOLD): the pair's manifold
                                     breaking threshold is the smaller of the two shapes'
                                     getContactBreakingThreshold(0.02) = angular motion disc x 0.02 --
                                     the distance within which the narrow phase reports a point
                                     (btManifoldResult::addContactPoint), merges it into a cached one
                                     (getCacheEntry) and keeps it (refreshContactPoints).  DESIGN.md
                                     section 2 "Contact breaking threshold". */
    double contact_erp;           /* ERP of multibody contact rows (m_erp 0.2) */
    double friction;              /* combined lateral friction of the cube against the table / plane:
                                     0.5 * 0.5 (each body's pybullet default; btManifoldResult
                                     multiplies the two) */
    double warmstart;             /* m_warmstartingFactor 0.85 (normal impulses) */
    /* combined lateral friction of robot link i (Bullet link index) against the scene's bodies --
     * table, plane, cube, obstacles, each at the default 0.5: 0.5 x the link's own, 0.5 x 0.5
     * except panda_ee and panda_leftfinger (links 9, 10), which Panda.__init__ raises to 1.0
     * (panda.py:69-70: set_lateral_friction(fingers_indices), pybullet.py:880-892 changeDynamics).
     * Their spinning friction 0.001 (panda.py:71-72) combines with the others' 0 to 0: no row. */
    double link_friction[PGX_MAX_LINKS];
} pgx_sim_params;

/* oracle-only modelling switches (documented in DESIGN.md) */
#define PGX_FLAG_CONSTRAINT_PASS_BIAS 1   /* re-apply velocity bias in the constraint pass */
#define PGX_FLAG_IK_COM 2                 /* IK targets the link COM instead of the joint pivot */
#define PGX_FLAG_NO_RESIDUAL_EXIT 4       /* run all solver iterations */
#define PGX_FLAG_LINKSTATE_CURRENT 8      /* getLinkState reports the pose after the last substep
                                             instead of Bullet's cached pose (rejected hypothesis) */
#define PGX_FLAG_DYN_RECURSIVE 16         /* M and b by composite rigid bodies + Newton-Euler (the
                                             kernel's formulation; same dynamics) instead of the
                                             Jacobian form: for the operation count */
#define PGX_FLAG_PERSISTENT_MANIFOLD 32   /* study: with PGX_CONTACTS_FULL, the robot's table / plane
                                             pairs through persistent manifolds too (each end sphere's
                                             manifold holds its one re-reported point, so it equals
                                             the fresh table rule to rounding: a test pins that) */
#define PGX_FLAG_FRESH_MANIFOLD 64        /* study: with PGX_CONTACTS_FULL, round 4's rule for the cube /
                                             obstacle pairs -- each pair's 4 deepest candidates of the
                                             substep -- instead of Bullet's persistent manifolds */
#define PGX_FLAG_GLOBAL_BREAKING 128      /* study: every pair's breaking threshold the global
                                             contact_distance (rounds 2-5) instead of Bullet's relative
                                             per-pair threshold */

typedef struct pgx_config {
    int32_t task;                 /* PGX_TASK_* */
    int32_t control;              /* PGX_CONTROL_* */
    int32_t reward;               /* PGX_REWARD_* */
    int32_t n_envs;
    int32_t max_episode_steps;    /* TimeLimit; 0 = never truncate */
    int32_t block_gripper;        /* Reach/Push: 1 */
    int32_t no_auto_reset;        /* 0: a finished env (terminated or truncated) is reset inside
                                     pgx_step, SB3 VecEnv style (terminal_* outputs hold the
                                     finished episode); 1: it keeps its final state until
                                     pgx_reset, like one gymnasium env (RobotTaskEnv + TimeLimit,
                                     core.py:352-368) */
    int32_t nonfinite_guard;      /* 0: off.  1: the step checks every float it is about to store for an
                                     env (q, qd, the cached pose, the object, the EE state, the goal
                                     distance, ReachAO's link observation); an env with a NaN / inf among
                                     them sets PGX_ERR_NONFINITE and pgx_step_out.nonfinite, reports
                                     reward 0, success = terminated = task_truncated = 0, truncated = 1,
                                     and -- unless no_auto_reset -- is reset in the same step like a
                                     TimeLimit truncation (the cube's velocity, which that reset keeps,
                                     zeroed), its terminal_* rows equal to its reset obs / goals.  Envs
                                     without one are bit for bit what they are with 0 */
    uint64_t seed;                /* device Philox key for auto-reset draws */
    uint64_t env_id_offset;       /* global id of env 0 (multi-GPU sharding) */
    double base_pos[3];           /* robot base (-0.6,0,0) (panda_tasks.py:85) */
    double distance_threshold;    /* 0.05 (reach.py:15) */
    double goal_low[3];
    double goal_high[3];
    double joint_forces[PGX_MAX_DOFS]; /* panda.py:63 */
    double neutral_q[PGX_MAX_DOFS];    /* panda.py:67 */
    double ee_step;               /* 0.05 (panda.py:235) */
    double joint_step;            /* 0.05 (panda.py:74) */
    const pgx_model* model;       /* host pointers, copied at create */
    const pgx_sim_params* params;
    /* scene (Task._create_scene, push.py:31-47; pybullet.py:759-817) */
    int32_t contacts;             /* 1: robot/table/object contacts (the reference's scene), the robot
                                     group's rows budgeted at PGX_ROBOT_POINTS_ONE_LANE (4) points;
                                     PGX_CONTACTS_FULL: Bullet's per-pair manifolds kept up to
                                     PGX_ROBOT_POINTS (object tasks) / _ARM points (16-lane layout) */
    int32_t lanes_per_env;        /* step layout: 0 auto (16 with contacts -- every object task
                                     and ReachAO -- at any batch, and up to 8192 envs without),
                                     1 = one env per lane, 16 = one env per 16-lane DPP row */
    double goal_offset[3];        /* goal = offset + uniform(goal_low, goal_high): (0,0,0.02) Push/PnP */
    double goal_z_zero_prob;      /* PickAndPlace: noise z = 0 with probability 0.3 */
    double obj_low[3];            /* object = obj_offset + uniform(obj_low, obj_high) */
    double obj_high[3];
    double obj_offset[3];
    double object_half;           /* cube half extent 0.02 */
    double object_mass;           /* 1.0 */
    double object_inertia;        /* principal inertia (Bullet compound-AABB rule) */
    double table_center[3];       /* (-0.3, 0, -0.2) */
    double table_half[3];         /* (0.55, 0.35, 0.2) */
    double plane_z;               /* top of the plane box: -0.4 */
    /* ReachAO (TrainConfig defaults, classes/train_config.py:24-35) */
    int32_t terminate_on_success; /* RobotTaskEnv(terminate_on_success): 1 for ReachAO */
    int32_t pad3;
    double collision_reward;      /* -100: added to the sparse reward on collision */
    double ao_ee_neutral[3];      /* ReachAO: the EE (panda_ee COM) at the neutral pose, fp64 -- the
                                     reset sampler's obstacle centre (reach_ao.py:635-644, the
                                     get_ee_position it reads after Panda.reset) and its goal
                                     fallback, a model constant computed once on the host; all zero:
                                     the kernel's own fp32 FK of that pose */
    /* ReachAO: the robot's capsules at the neutral pose in world coordinates, fp64, per capsule of
     * the model (model.n_capsules, the base's included) end A [3], end B [3], radius -- the geometry
     * of the reset sampler's accept / reject tests (reach_ao.py:1101-1161, get_distances against the
     * robot; host restatement panda-gym_amd/reach_ao.py RobotGeometry), which the device evaluates in
     * fp64 on exactly these values so that a reset drawn on the device decides every test as the
     * host's does.  All zero: pgx_create computes them by an fp64 FK of neutral_q from the model
     * (the same values to rounding). */
    double ao_capsules_neutral[PGX_MAX_CAPSULES][7];
} pgx_config;

typedef struct pgx_env* pgx_handle;

/* Output buffers of one batched step (device pointers; any may be NULL to skip).
 * obs [N,obs_dim] f32, achieved/desired [N,3] f32, reward [N] f32,
 * success/terminated/truncated [N] u8, terminal_obs [N,obs_dim] f32 (obs of the
 * finished episode, written only for envs that were auto-reset),
 * terminal_ag / terminal_dg [N,3] f32 (achieved / desired goal of the finished
 * episode: SB3 stores next_obs = infos["terminal_observation"] for them). */
typedef struct pgx_step_out {
    float* obs;
    float* achieved_goal;
    float* desired_goal;
    float* reward;
    uint8_t* success;
    uint8_t* terminated;
    uint8_t* truncated;
    float* terminal_obs;
    float* terminal_achieved_goal;
    float* terminal_desired_goal;
    uint8_t* task_truncated;      /* [N] u8 Task.is_truncated of the step (ReachAO: is_collided,
                                     reach_ao.py:1263-1264; 0 for the other tasks, reach.py:53-54),
                                     i.e. info["is_truncated"], without the TimeLimit part */
    uint8_t* nonfinite;           /* [N] u8 written by pgx_step only: 1 for an env the non-finite guard
                                     (pgx_config.nonfinite_guard) caught in this step, else 0; all 0
                                     from a handle without the guard */
} pgx_step_out;

/* Device-resident state views (SoA, env-minor: x[k*N + env]). */
typedef struct pgx_state_view {
    float* q;           /* [n_dofs][N] */
    float* qd;          /* [n_dofs][N] */
    float* qc;          /* [n_dofs][N] pose of Bullet's cached link transforms, which getLinkState
                           reports (EE obs, IK target): the pose the last substep started from */
    double* goal;       /* [3][N] */
    float* object;      /* [13][N] pos3, quat4 (x,y,z,w), linvel3, angvel3 */
    float* contacts;    /* [2*PGX_CONTACT_SLOTS][N] warm-start cache: (id, normal impulse) per slot */
    float* obstacles;   /* [4*PGX_AO_OBSTACLES][N] ReachAO obstacle centres (x,y,z) then active flags */
    int32_t* elapsed;   /* [N] steps in the current episode */
    uint32_t* episode;  /* [N] episodes finished (RNG counter) */
    uint32_t* errors;   /* [1] sticky PGX_ERR_* bits set by the kernels; the host clears them */
    int32_t robot_points;  /* the robot contact budget of this handle's kernels (0: no contacts) */
    int32_t* env_order;    /* [N] the env order of the last step launch that sorted its envs heavy-first
                              (per-pair manifold kernels; position -> env id), the identity before
                              the first such launch, NULL for handles without the per-pair budget;
                              not state (the next sorted launch rewrites it).  From a handle's
                              second step on, the step kernel derives the order itself, from one
                              key byte per env that the previous step's epilogue wrote (segments
                              of <= 1024 envs; PGX_SORT_FUSED=0: the sort kernel at every launch).
                              pgx_reset, pgx_restore_state and pgx_restore make the next step sort
                              from the state as it stands; pgx_get_state does not, so a caller who
                              writes `contacts` through this view steps once in an order one step
                              stale -- any order gives every env the same bits */
    float* manifolds;      /* [1 + manifold_pool * PGX_MANIFOLD_POINT][N] the persistent manifold pool
                              (PGX_MANIFOLD_POOL above), NULL without one */
    int32_t manifold_pool; /* its capacity in points (0: none) */
} pgx_state_view;

/* errors word (pgx_state_view.errors): a device-side reset that cannot complete the way the
 * reference's would.  PGX_ERR_AO_OBSTACLE: ReachAO.set_coll_free_obs drew 10000 obstacle
 * positions without a collision-free one, where the reference raises StopIteration
 * ("Couldn't find collision free obstacle!", reach_ao.py:1143-1145); the env keeps the last
 * draw and the host raises PgxError when it reads the bit. */
#define PGX_ERR_AO_OBSTACLE 1u
/* PGX_ERR_NONFINITE: the non-finite guard (pgx_config.nonfinite_guard) caught an env in some step
 * since the host last cleared the word; pgx_step_out.nonfinite names the envs of each step. */
#define PGX_ERR_NONFINITE 2u

const char* pgx_version(void);
const char* pgx_last_error(void);
int pgx_obs_dim(const pgx_config* cfg);
int pgx_action_dim(const pgx_config* cfg);

/* libpgx.so compiles the device constant block in (the robot, pgx_sim_params, the scene's table
 * box and plane): a cfg that folds to another block fails with PGX_E_UNSUPPORTED, and
 * libpgx_rtmodel.so (the same kernels reading the handle's block) takes any. */
int pgx_create(const pgx_config* cfg, int device, pgx_handle* out);
/* Host only: the device constant block (PgxDevModel, nbytes = its size) pgx_create folds from cfg;
 * the build's generator of the kernels' compile-time defaults uses it. */
int pgx_dev_model_bytes(const pgx_config* cfg, void* out, int64_t nbytes);
void pgx_destroy(pgx_handle h);
int pgx_get_state(pgx_handle h, pgx_state_view* out);

/* Reset envs whose mask byte is non-zero (mask NULL = all).  inject_goal
 * [N,3] f64 (host-computed PCG64 draws for seeded resets) and inject_object
 * [N,3] f64 (Push/PickAndPlace object position) or [N,PGX_AO_OBSTACLES,3] f64 (ReachAO
 * obstacle centres, parked ones at (99.9, 99.9, -99.9)) override the device draws
 * where given.  Writes the reset obs. */
int pgx_reset(pgx_handle h, const uint8_t* env_mask, const double* inject_goal,
              const double* inject_object, pgx_step_out* out, void* stream);

/* One lockstep env step for all N envs: action [N,A] f32 (device). */
int pgx_step(pgx_handle h, const float* action, pgx_step_out* out, void* stream);
/* The step kernel the last pgx_step on h launched, as rocprof names it (e.g.
 * "step_kernel<0, 0, 1, 0, 2>"; NULL before the first step): the label a benchmark reports beside
 * its kernel time and profiles. */
const char* pgx_step_kernel(pgx_handle h);

/* Fill action [N,A] with U[-1,1) from the device Philox stream (benchmark
 * random policy; counter = (global env id, step)). */
int pgx_sample_actions(pgx_handle h, float* action, uint64_t step, void* stream);

/* Batched reward for relabelled goals: ag, dg [B,3] f32 device, out [B] f32.
 * Follows utils.distance (round to 1e-6) in float32 like the reference does
 * for float32 inputs. */
int pgx_compute_reward(const float* achieved_goal, const float* desired_goal, int64_t batch,
                       int32_t reward_type, double distance_threshold, float* out, void* stream);

/* Single-kernel copies of the whole SoA state into / out of a caller-owned device buffer. */
int pgx_state_bytes(pgx_handle h, int64_t* nbytes);
int pgx_save_state(pgx_handle h, void* dst_device, void* stream);
int pgx_restore_state(pgx_handle h, const void* src_device, void* stream);

/* State ids (PyBullet.save_state / restore_state / remove_state, pybullet.py:79-102; reached
 * through RobotTaskEnv.save_state / restore_state / remove_state, core.py:310-336).
 * pgx_snapshot copies the whole state into a buffer the handle owns and returns its id: the
 * first non-negative integer not in use (pybullet's saveState rule, so a released id is handed
 * out again).  pgx_restore copies it back; pgx_release frees it (it synchronises the device:
 * queued copies may still read the buffer).  Restoring or releasing an id that is not in use
 * returns PGX_E_INVALID ("no such saved state"), as restoreState after removeState raises
 * pybullet.error (test/save_and_restore_test.py:30-36).  pgx_destroy frees every snapshot. */
int pgx_snapshot(pgx_handle h, int32_t* state_id, void* stream);
int pgx_restore(pgx_handle h, int32_t state_id, void* stream);
int pgx_release(pgx_handle h, int32_t state_id);

/* Reset draws from numpy PCG64 streams instead of the device Philox counter (a
 * seeded reset drawn on the device, no host injection).  RobotTaskEnv.reset reseeds the task's
 * generator on EVERY reset, task.np_random = seeding.np_random(seed) (core.py:302): a reset with
 * seed s draws from PCG64(SeedSequence(s)), which is what a record set from s reproduces bit for bit
 * (goal / object in the task's order, reach.py:75-78, push.py:75-87, pick_and_place.py:71-85;
 * ReachAO's rejection sampler, reach_ao.py:965-1082, with Generator.uniform / random / integers /
 * shuffle as numpy draws them, and every accept / reject test decided in fp64 on the host's
 * capsules, pgx_config.ao_capsules_neutral -- the draws and the record bit for bit, ReachAO's goal
 * to a few ulp: the device's sin / cos / cbrt are not the host libm's).  A reset without a seed -- the step's auto-reset included -- gets a
 * fresh OS-entropy generator in the reference, so no reference value exists for it: here it
 * continues stream i, a reproducible stand-in with the same distribution, not the reference's
 * draws.  states: [N][PGX_PCG64_WORDS] uint64 per env {state_lo, state_hi, inc_lo, inc_hi,
 * has_uint32, uinteger} -- numpy's PCG64 bit_generator.state -- host or device memory, copied on
 * `stream`; NULL returns to Philox.  The mode is a device word switched on `stream` and the stream
 * buffer lives as long as the handle, so a step loop captured in a HIP graph draws in the mode of
 * replay time.  An injected reset leaves its env's stream untouched.  Streams are not part of the
 * saved state (restoreState keeps np_random as it is).  pgx_get_rng_streams copies the current
 * records out (same layout, host or device memory). */
#define PGX_PCG64_WORDS 6
int pgx_set_rng_streams(pgx_handle h, const uint64_t* states, void* stream);
int pgx_get_rng_streams(pgx_handle h, uint64_t* states, void* stream);

/* ------------------------------------------------------------------------
 * Device HER replay ring: the goal-relabelling replay buffer the reference's
 * training uses (SB3 HerReplayBuffer / the fork's VecHerReplayBuffer,
 * training/utils/setup_training.py:176-179; classes/train_config.py:15),
 * "future" strategy, relabelled rewards from Task.compute_reward
 * (reach.py:84-89 / pick_and_place.py:91-96) in float32.
 *
 * Storage is [capacity][n_envs] slot-major like SB3's (buffer_size, n_envs)
 * arrays, one padded record per transition so a sampled transition is one
 * contiguous gather; add() writes one transition per env at the shared ring
 * position, keeps SB3's episode bookkeeping (ep_start / ep_length,
 * invalidation of an overwritten episode) and refreshes the list of valid
 * transitions (ep_length > 0); sample() draws uniformly over that list,
 * relabels the first int(her_ratio*B) draws with the next_achieved_goal of a
 * transition t' of the same episode (strategy below) and recomputes their
 * rewards.  Draws come from the device Philox stream.
 *
 * Batch row layout (floats), row_dim = 2*obs_dim + action_dim + 14, rows
 * row_stride = round_up(row_dim, 4) apart:
 *   obs[obs_dim] | achieved_goal[3] | desired_goal[3] | action[action_dim] |
 *   reward | next_obs[obs_dim] | next_achieved_goal[3] | next_desired_goal[3] | done
 * SB3 order: the B - int(her_ratio*B) real rows first, then the relabelled rows.
 * ---------------------------------------------------------------------- */
typedef struct pgx_replay* pgx_replay_handle;

#define PGX_HER_FUTURE 0   /* t' uniform in [t, episode end) */
#define PGX_HER_FINAL 1    /* t' = last transition of the episode */
#define PGX_HER_EPISODE 2  /* t' uniform in [episode start, episode end) */

typedef struct pgx_replay_config {
    int32_t n_envs;
    int32_t capacity;             /* transitions per env (SB3 buffer_size) */
    int32_t obs_dim;
    int32_t action_dim;
    int32_t reward_type;          /* PGX_REWARD_* */
    int32_t strategy;             /* PGX_HER_* goal selection (SB3 GoalSelectionStrategy) */
    double distance_threshold;    /* 0.05 */
    double her_ratio;             /* 1 - 1/(n_sampled_goal+1) = 0.8 */
    uint64_t seed;
} pgx_replay_config;

/* One transition per env (device pointers): obs/next_obs [N,obs_dim], ag/dg/next_ag/next_dg
 * [N,3], action [N,A] f32, reward [N] f32, done [N] u8, timeout [N] u8 (TimeLimit.truncated). */
typedef struct pgx_transition {
    const float* obs;
    const float* achieved_goal;
    const float* desired_goal;
    const float* action;
    const float* reward;
    const float* next_obs;
    const float* next_achieved_goal;
    const float* next_desired_goal;
    const uint8_t* done;
    const uint8_t* timeout;
} pgx_transition;

/* Sampled, relabelled batch (device pointers).  rows [B, row_stride] f32 in the layout
 * above; done = done * (1 - timeout).  slot/env/goal_slot [B] i32 (optional, may be NULL):
 * the drawn indices, goal_slot -1 for real rows.  When no episode has completed yet (SB3
 * raises), every row is zero and slot = -1. */
typedef struct pgx_replay_batch {
    float* rows;
    int32_t* slot;
    int32_t* env;
    int32_t* goal_slot;
} pgx_replay_batch;

/* row_dim / row_stride of a batch row for this config (floats). */
int pgx_replay_row_dim(const pgx_replay_config* cfg);
int pgx_replay_row_stride(const pgx_replay_config* cfg);
int pgx_replay_create(const pgx_replay_config* cfg, int device, pgx_replay_handle* out);
void pgx_replay_destroy(pgx_replay_handle h);
int pgx_replay_add(pgx_replay_handle h, const pgx_transition* t, void* stream);
/* Number of transitions added per env so far: the host mirror of the device word `added` (below),
 * no sync.  The mirror counts the add / collect calls the host made, so it is exact while every
 * add ran as a direct call; it is stale once a captured add or collect has been replayed (a replay
 * advances the device word only) or a collect without a carry was refused on the device, until
 * pgx_replay_state refreshes it. */
int64_t pgx_replay_size(pgx_replay_handle h);
int pgx_replay_sample(pgx_replay_handle h, int64_t batch, uint64_t draw, pgx_replay_batch* out, void* stream);
/* Device views of the bookkeeping arrays [capacity][n_envs] i32 and of the number of valid
 * transitions after the last add() (i32 scalar), for tests / checkpoint / the host guard. */
int pgx_replay_episode_arrays(pgx_replay_handle h, int32_t** ep_start, int32_t** ep_length, int32_t** n_valid);

/* Collection on the device.  The ring position is a device word: `added`, the adds and collects
 * stored so far (int64), pos = added % capacity.  Every kernel reads it from there (pgx_replay_add
 * too), and the single-workgroup scan that runs behind every add and collect advances it, so a
 * captured add or collect lands in the next slot on every replay.  Beside it live a sticky errors
 * word (PGX_REPLAY_ERR_*), the flag "carry set", and the carry: SB3's _last_original_obs, per env
 * carry_stride = round_up(obs_dim + 6, 4) floats laid out as the head of a record,
 *   obs[obs_dim] | achieved_goal[3] | desired_goal[3] | zero padding.
 *
 * set_last / collect / truncate_last_trajectory enqueue kernels on `stream` and nothing else: no
 * memcpy or memset node, no allocation, no synchronisation, so they capture into a hipGraph behind
 * pgx_step.
 *
 * collect, per env (SB3 OffPolicyAlgorithm._store_transition over the auto-resetting VecEnv):
 *   done    = terminated | truncated
 *   timeout = handle_timeout ? truncated & ~terminated : 0
 *   next_*  = done ? terminal_* : the post-step obs / achieved_goal / desired_goal
 *   record  = carry obs | ag | dg | action | reward | next_obs | next_ag | next_dg |
 *             done * (1 - timeout) | ep_start | ep_length, stored at pos with pgx_replay_add's
 *             bookkeeping (the overwritten episode invalidated, ep_start, the episode length
 *             written over the episode of a done env, whose next episode starts at pos + 1)
 *   carry   = the post-step observation (of a done env: the first one of its new episode)
 * then the valid list is refreshed and added += 1.  Without a carry (no set_last yet) nothing is
 * stored, added stays, and PGX_REPLAY_ERR_NO_CARRY is set.
 *
 * truncate_last_trajectory closes every open episode where it stands, SB3's
 * HerReplayBuffer.truncate_last_trajectory (after a forced reset, an env switch or the end of
 * learn()); for every env with cur_ep_start != pos:
 *   the episode [cur_ep_start, pos) (unwrapped by + capacity) gets its length, in ep_length and in
 *   the records' copies; cur_ep_start = pos;
 *   SB3 sets dones[pos - 1] = True and, with handle_timeout_termination, timeouts[pos - 1] = True:
 *   the stored done * (1 - timeout) of the transition at pos - 1 (capacity - 1 for pos = 0) becomes
 *   1 when handle_timeout is 0 and stays 0 when it is 1;
 * then the valid list is refreshed.  An env at an episode start is left alone, so a second call
 * changes nothing.  The carry stays: set it for the observation the next collect starts from. */
#define PGX_REPLAY_ERR_NO_CARRY 1   /* pgx_replay_collect before pgx_replay_set_last: nothing stored */

/* Device pointers of one collect: the step's action, then the env's step outputs (pgx_step_out's
 * buffers).  Nothing is written. */
typedef struct pgx_replay_step {
    const float* action;                  /* [N,action_dim] */
    const float* reward;                  /* [N] */
    const uint8_t* terminated;            /* [N] */
    const uint8_t* truncated;             /* [N] */
    const float* obs;                     /* [N,obs_dim] post-step observation (the next carry) */
    const float* achieved_goal;           /* [N,3] */
    const float* desired_goal;            /* [N,3] */
    const float* terminal_obs;            /* [N,obs_dim] read where terminated | truncated */
    const float* terminal_achieved_goal;  /* [N,3] */
    const float* terminal_desired_goal;   /* [N,3] */
    int32_t handle_timeout;               /* SB3 handle_timeout_termination */
    int32_t pad0;
} pgx_replay_step;

/* Device views of everything stored, for tests and a checkpoint: records
 * [capacity][n_envs][record_stride], the carry [n_envs][carry_stride], ep_start / ep_length
 * [capacity][n_envs], cur_ep_start [n_envs], the words. */
typedef struct pgx_replay_views {
    float* records;
    float* carry;
    int32_t* ep_start;
    int32_t* ep_length;
    int32_t* cur_ep_start;
    int32_t* n_valid;
    int64_t* added;
    uint32_t* errors;
    int32_t* carry_set;
    int32_t record_stride;
    int32_t carry_stride;
} pgx_replay_views;

/* The carry: obs [N,obs_dim], achieved_goal / desired_goal [N,3] f32 (the observation of
 * env.reset()); sets the flag "carry set".  One launch. */
int pgx_replay_set_last(pgx_replay_handle h, const float* obs, const float* achieved_goal, const float* desired_goal,
                        void* stream);
/* One collect launch in front of pgx_replay_add's count / scan / scatter. */
int pgx_replay_collect(pgx_replay_handle h, const pgx_replay_step* io, void* stream);
/* One launch, then count / scan / scatter. */
int pgx_replay_truncate_last_trajectory(pgx_replay_handle h, int32_t handle_timeout, void* stream);
/* added, n_valid and errors after synchronising `stream` (each may be NULL); refreshes the host
 * mirror of pgx_replay_size; clear != 0 zeroes errors. */
int pgx_replay_state(pgx_replay_handle h, int64_t* added, int32_t* n_valid, uint32_t* errors, int32_t clear,
                     void* stream);
int pgx_replay_arrays(pgx_replay_handle h, pgx_replay_views* out);

/* ------------------------------------------------------------------------
 * VecNormalize: the observation / reward normalisation the reference's training
 * settings turn on (classes/hyperparameters.py:42 `normalize = True`, :116), i.e.
 * stable-baselines3's VecNormalize (stable_baselines3/common/vec_env/vec_normalize.py)
 * over RunningMeanStd (common/running_mean_std.py), device-resident.
 *
 * Columns: C = obs_dim + 3 + 3 observation columns grouped by key -- observation,
 * achieved_goal, desired_goal -- then one returns column (index C).  Per column fp64
 * mean / var / count, RunningMeanStd(epsilon = 1e-4): mean 0, var 1, count 1e-4 at create;
 * update(batch) with the batch's mean, population variance and count N:
 *   delta = batch_mean - mean; tot = count + N; new_mean = mean + delta * N / tot;
 *   M2 = var * count + batch_var * N + delta^2 * count * N / tot; new_var = M2 / tot; new_count = tot.
 * Batch moments are accumulated in fp64 from the f32 inputs over fixed env slabs (mean, then
 * squared deviations) and merged in slab order with Chan's (n, mean, M2) rule: the same bits
 * in every run.  Outputs are clip((x - mean) / sqrt(var + epsilon), -clip, clip) and
 * clip(reward / sqrt(ret_var + epsilon), -clip_reward, clip_reward), evaluated in fp64 without
 * contraction and rounded once to f32: given the statistics, the bits numpy computes.
 *
 * pgx_norm_step and pgx_norm_reset are two kernel launches on `stream` each: no allocation,
 * no synchronisation, no copy node, so they capture into a hipGraph behind pgx_step, and a
 * captured sequence of any length replays correctly (which half of the statistics pair is
 * current, and whether statistics move, are device words).
 * ---------------------------------------------------------------------- */
typedef struct pgx_norm* pgx_norm_handle;

#define PGX_NORM_KEY_OBSERVATION 1   /* pgx_norm_config.key_mask bits (VecNormalize norm_obs_keys) */
#define PGX_NORM_KEY_ACHIEVED_GOAL 2
#define PGX_NORM_KEY_DESIRED_GOAL 4
#define PGX_NORM_KEY_ALL 7
/* pgx_norm_apply keys: 0 observation, 1 achieved_goal, 2 desired_goal, and */
#define PGX_NORM_REWARD 3

typedef struct pgx_norm_config {
    int32_t n_envs;
    int32_t obs_dim;              /* <= 249 */
    int32_t key_mask;             /* PGX_NORM_KEY_* of the normalised keys; 0 = norm_obs False */
    int32_t norm_reward;
    double clip_obs;              /* VecNormalize defaults: 10 */
    double clip_reward;           /* 10 */
    double gamma;                 /* 0.99 */
    double epsilon;               /* 1e-8 */
} pgx_norm_config;

/* Device pointers of one step (or reset).  Inputs are the raw step outputs (pgx_step_out's
 * buffers) and are never written; outputs are separate buffers, any may be NULL to skip.
 * flags / out_flags (optional): [flag_rows][N] u8 copied unchanged, so a host path fetches a whole
 * normalised step with one copy. */
typedef struct pgx_norm_io {
    const float* obs;                     /* [N,obs_dim] */
    const float* achieved_goal;           /* [N,3] */
    const float* desired_goal;            /* [N,3] */
    const float* reward;                  /* [N] (step only) */
    const uint8_t* terminated;            /* [N] (step only) */
    const uint8_t* truncated;             /* [N] (step only) */
    const float* terminal_obs;            /* step only, may be NULL: rows of done envs are normalised */
    const float* terminal_achieved_goal;
    const float* terminal_desired_goal;
    const uint8_t* flags;
    float* out_obs;
    float* out_achieved_goal;
    float* out_desired_goal;
    float* out_reward;
    float* out_terminal_obs;              /* written only for envs with terminated | truncated */
    float* out_terminal_achieved_goal;
    float* out_terminal_desired_goal;
    uint8_t* out_flags;
    int32_t flag_rows;
    int32_t pad0;
} pgx_norm_io;

/* VecNormalize.__init__ (training on).  PGX_E_INVALID, before any device call, for n_envs <= 0,
 * obs_dim outside [1, 249], epsilon < 0, clips <= 0, gamma < 0 or unknown key bits. */
int pgx_norm_create(const pgx_norm_config* cfg, int device, pgx_norm_handle* out);
void pgx_norm_destroy(pgx_norm_handle h);
/* VecNormalize.step_wait, in its order: (training) update the enabled keys' statistics from the
 * step's observation rows -- the post-auto-reset ones; write the normalised observations (keys
 * not enabled: copied); returns = returns * gamma + reward (fp64 per env; here also while not
 * training), (training) update the returns statistics from them, write the normalised (or, without
 * norm_reward, raw) reward; normalise the terminal_* rows of done envs with the updated
 * statistics; returns[done] = 0. */
int pgx_norm_step(pgx_norm_handle h, const pgx_norm_io* io, void* stream);
/* VecNormalize.reset: returns = 0, (training) update from the reset observations, write them
 * normalised.  Reads obs / achieved_goal / desired_goal and the out_* of those only. */
int pgx_norm_reset(pgx_norm_handle h, const pgx_norm_io* io, void* stream);
/* HerReplayBuffer.sample(batch_size, env=vec_normalize) -> _normalize_obs / _normalize_reward
 * (stable_baselines3/her/her_replay_buffer.py): a sampled batch rows [batch, row_stride] in the
 * layout above (pgx_replay_batch), in place, one launch, current statistics, no update.  obs /
 * next_obs and the four goal fields by their keys' statistics (enabled keys only), reward by the
 * returns statistics (with norm_reward); action, done and the row padding untouched. */
int pgx_norm_rows(pgx_norm_handle h, float* rows, int64_t batch, int32_t action_dim, int32_t row_stride, void* stream);
/* VecNormalize.normalize_obs / unnormalize_obs (one key) and normalize_reward /
 * unnormalize_reward (key = PGX_NORM_REWARD, width 1) over in / out [m, width] f32 (may alias),
 * stateless and whatever the key mask says.  inverse: x * sqrt(var + epsilon) + mean (rewards:
 * without the mean), unclipped as in SB3. */
int pgx_norm_apply(pgx_norm_handle h, int32_t key, int32_t inverse, const float* in, float* out, int64_t m, void* stream);
/* VecNormalize.training: a device word switched on `stream`, so a captured step loop follows the
 * value of replay time.  0 freezes every statistic. */
int pgx_norm_set_training(pgx_norm_handle h, int32_t training, void* stream);
/* VecNormalize.norm_obs / norm_obs_keys / norm_reward after create (host side: a captured graph keeps
 * the values of capture time). */
int pgx_norm_set_keys(pgx_norm_handle h, int32_t key_mask, int32_t norm_reward);
/* VecNormalize.obs_rms / ret_rms / returns (and save / load): host arrays mean, var, count
 * [obs_dim + 7] (the returns column last; the columns of a key share its count) and returns
 * [n_envs] (may be NULL).  Both synchronise `stream`. */
int pgx_norm_get_stats(pgx_norm_handle h, double* mean, double* var, double* count, double* returns, void* stream);
int pgx_norm_set_stats(pgx_norm_handle h, const double* mean, const double* var, const double* count,
                       const double* returns, void* stream);

/* ------------------------------------------------------------------------
 * VecMonitor: the episode statistics every stable-baselines3 run has -- make_vec_env wraps
 * each env in Monitor (the reference: training/utils/setup_training.py:43-47), whose
 * infos[i]["episode"] = {"r", "l", "t"} feed rollout/ep_rew_mean, ep_len_mean and success_rate
 * -- and the per-episode outcomes the reference's evaluation scores policies by
 * (evaluation/evaluate.py:88-317 perform_benchmark; setup_training.py:310-318), device-resident.
 * The arithmetic is stable_baselines3/common/vec_env/vec_monitor.py's.
 *
 * Per env: ret f32 (ret = ret + reward, one f32 add per step, as VecMonitor's float32
 * episode_returns), len i32, speed f64 (the running sum of the step's end-effector speed
 * sqrt(x*x + y*y + z*z), the three f32 columns obs[speed_col .. speed_col + 2] widened to fp64,
 * products and sums left to right, no contraction; a done env's row is read from terminal_obs,
 * the step's own observation, any other from obs), ep_count i32 (episodes recorded for the env).
 *
 * A finished episode (terminated | truncated) of an env below its target is recorded.  Its
 * outcome, first match: PGX_EP_NONFINITE -- the step's nonfinite flag is set or ret is not finite;
 * PGX_EP_SUCCESS -- the success flag; PGX_EP_COLLISION -- the task_truncated flag; PGX_EP_TIMEOUT
 * (evaluate.py:250-267).  The records of one step are appended in ascending env id -- VecMonitor's
 * `for i in range(len(dones))` -- to a ring of `window` records that keeps the newest `window`,
 * as deque(maxlen = window) does (more than `window` in one step: the last `window` in env order).
 * A record's `step` is the value of totals.steps after the step that finished it (the first
 * pgx_monitor_step is step 1).  Done envs get ep_r[env] = ret and ep_l[env] = len (recorded or
 * not), and their ret / len / speed go back to zero.
 *
 * Totals, over the recorded episodes: episodes and outcomes[code] count every one of them; the
 * sums leave PGX_EP_NONFINITE episodes out (one poisoned env cannot turn them into NaN):
 * length_sum and return_sum over the others, length_sum_success and speed_sum_success over the
 * PGX_EP_SUCCESS ones (every step of a successful episode: mean EE speed = speed_sum_success /
 * length_sum_success).  return_sum and speed_sum_success are fp64 sums of (double)ret and of
 * speed in this order: envs are cut into fixed slabs (a multiple of 256 envs, at most 64 slabs);
 * a slab's sum starts at 0.0 and adds its episodes in ascending env id; the step adds the slab
 * sums to the running total in slab order, total = (..((total + slab_0) + slab_1) ..).  The same
 * inputs give the same bits in every run.  steps counts pgx_monitor_step calls; envs_open the
 * envs with ep_count < target (all of them without targets).
 *
 * pgx_monitor_step is two kernel launches on `stream`: no allocation, no synchronisation, no
 * copy node, so it captures into a hipGraph behind pgx_step (and pgx_norm_step), and a captured
 * sequence of any length replays correctly: the ring head, the step counter and which half of
 * the totals pair is current are device words.
 * ---------------------------------------------------------------------- */
typedef struct pgx_monitor* pgx_monitor_handle;

#define PGX_EP_TIMEOUT 0
#define PGX_EP_SUCCESS 1
#define PGX_EP_COLLISION 2
#define PGX_EP_NONFINITE 3

typedef struct pgx_monitor_config {
    int32_t n_envs;
    int32_t obs_dim;
    int32_t window;               /* records the ring retains (SB3 stats_window_size: 100) */
    int32_t speed_col;            /* first of the three EE-velocity columns of obs (3 in every task
                                     here); < 0: no speed sums, obs / terminal_obs are not read */
} pgx_monitor_config;

/* Device pointers of one step: pgx_step_out's buffers, never written, and two optional outputs. */
typedef struct pgx_monitor_io {
    const float* reward;                  /* [N] */
    const uint8_t* success;               /* [N] */
    const uint8_t* terminated;            /* [N] */
    const uint8_t* truncated;             /* [N] */
    const float* obs;                     /* [N,obs_dim] (required with speed_col >= 0) */
    const float* terminal_obs;            /* [N,obs_dim] (required with speed_col >= 0) */
    const uint8_t* task_truncated;        /* [N], may be NULL: all 0 */
    const uint8_t* nonfinite;             /* [N], may be NULL: all 0 */
    float* ep_r;                          /* [N], may be NULL: the return of the episode an env finished */
    int32_t* ep_l;                        /* [N], may be NULL: its length; both valid where done */
} pgx_monitor_io;

typedef struct pgx_monitor_totals {
    int64_t episodes;
    int64_t outcomes[4];                  /* by PGX_EP_* */
    int64_t length_sum;
    int64_t length_sum_success;
    int64_t steps;
    int64_t envs_open;
    double return_sum;
    double speed_sum_success;
} pgx_monitor_totals;

/* PGX_E_INVALID, before any device call, for n_envs <= 0, obs_dim <= 0, window outside
 * [1, 2^24] or speed_col + 3 > obs_dim. */
int pgx_monitor_create(const pgx_monitor_config* cfg, int device, pgx_monitor_handle* out);
void pgx_monitor_destroy(pgx_monitor_handle h);
/* VecMonitor.step_wait over one step's outputs, as described above. */
int pgx_monitor_step(pgx_monitor_handle h, const pgx_monitor_io* io, void* stream);
/* VecMonitor.reset for the envs with mask[env] != 0 (device [N] u8; NULL: all): ret, len and
 * speed go to zero, the running episode is abandoned, not recorded.  One launch. */
int pgx_monitor_reset(pgx_monitor_handle h, const uint8_t* mask, void* stream);
/* Back to the state after create (accumulators, ring, totals, ep_count); targets stay. */
int pgx_monitor_clear(pgx_monitor_handle h, void* stream);
/* stable_baselines3 evaluate_policy's episode_count_targets: host int32 [N], each >= 0, or NULL
 * for none.  An env with ep_count >= target keeps stepping (ep_r / ep_l are written, its
 * accumulators cleared) but is not recorded, in the ring or in the totals.  Synchronises. */
int pgx_monitor_set_targets(pgx_monitor_handle h, const int32_t* targets, void* stream);
/* The current totals, after synchronising `stream`. */
int pgx_monitor_get_totals(pgx_monitor_handle h, pgx_monitor_totals* out, void* stream);
/* The newest min(max, retained) records, oldest first, into host arrays (any may be NULL);
 * *count is their number.  Synchronises `stream`. */
int pgx_monitor_read(pgx_monitor_handle h, int32_t max, float* r, int32_t* l, int32_t* env, int32_t* outcome,
                     int64_t* step, double* speed_sum, int32_t* count, void* stream);
/* The per-env state into host arrays [N] (any may be NULL).  Synchronises `stream`. */
int pgx_monitor_get_env_state(pgx_monitor_handle h, float* ret, int32_t* len, double* speed, int32_t* ep_count,
                              void* stream);

/* ------------------------------------------------------------------------
 * RolloutBuffer: the on-policy buffer stable-baselines3's OnPolicyAlgorithm.collect_rollouts
 * fills and PPO.train reads (stable_baselines3/common/buffers.py DictRolloutBuffer; the
 * reference imports PPO beside its off-policy algorithms, training/utils/setup_training.py:14),
 * device-resident: n_steps x n_envs transitions, the GAE(lambda) pass, the time-limit bootstrap
 * of collect_rollouts and get(batch_size)'s shuffled minibatches.
 *
 * Storage, one allocation per handle.  A transition's vector fields are one record of
 * record_stride = round_up(obs_dim + 6 + action_dim, 32) floats,
 *   observation[obs_dim] | achieved_goal[3] | desired_goal[3] | action[action_dim] | zero padding,
 * records [n_steps][n_envs][record_stride]; its six scalars live in six dense f32 planes
 * [n_steps][n_envs] -- reward, episode_start (0 / 1), value, log_prob, advantage, return -- so the
 * GAE pass, one lane per env, reads consecutive envs from consecutive addresses.  The carry is
 * what SB3 keeps in _last_obs / _last_episode_starts: observation [N,obs_dim], achieved_goal
 * [N,3], desired_goal [N,3], episode_start [N] f32 (ones after create).  Device words: pos and a
 * sticky errors word (PGX_ROLLOUT_ERR_*).  pos is kept once per workgroup of pgx_rollout_add's
 * launch (each reads and advances its own copy, so no workgroup hands anything to another); the
 * copies are equal between launches and the first one is "pos".
 *
 * Every entry point below but create / destroy / state / arrays is ONE kernel launch on `stream`:
 * no memcpy or memset node, no allocation, no synchronisation, so it captures into a hipGraph
 * behind pgx_step, and a captured fill replays correctly after pgx_rollout_reset.
 *
 * All arithmetic is f32, every operation rounded separately (no contraction):
 *   add:  reward' = reward + (float)gamma * terminal_value   where truncated & ~terminated and
 *         terminal_value is given (SB3 collect_rollouts' TimeLimit.truncated bootstrap)
 *   compute_returns_and_advantage, per env, SB3's loop and operation order:
 *     g = (float)gamma; gl = (float)(gamma * gae_lambda)   (the double product rounded once)
 *     last = 0
 *     for t = T-1 .. 0:
 *       nnt = 1 - (t == T-1 ? dones : episode_start[t+1]);  nv = (t == T-1 ? last_values : value[t+1])
 *       delta = (reward[t] + (g * nv) * nnt) - value[t]
 *       last  = delta + (gl * nnt) * last
 *       advantage[t] = last;  return[t] = last + value[t]
 *
 * Flat transition index p = env * n_steps + step (SB3 swap_and_flatten), M = n_steps * n_envs.
 * pgx_rollout_permutation replaces np.random.permutation(M) (numpy's global stream: no reference
 * value exists) by a pure function of (seed, epoch, M), a balanced 6-round Feistel network over
 * [0, 4^k) with cycle walking; uint32 arithmetic throughout:
 *   fmix(h): h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16
 *   s = fmix(lo32(seed) ^ 0x9E3779B9); s = fmix(s ^ hi32(seed)); s = fmix(s ^ lo32(epoch));
 *   s = fmix(s ^ hi32(epoch))
 *   key[r]: s = fmix(s + 0x9E3779B9 * (r + 1)), key[r] = s,   r = 0..5
 *   k = max(1, (bitlength(max(M - 1, 1)) + 1) / 2);  mask = 2^k - 1
 *   perm(i): x = i; repeat { L = x >> k; R = x & mask;
 *                            6 times, r = 0..5: (L, R) = (R, L ^ (fmix(R * 0x9E3779B1 + key[r]) & mask));
 *                            x = L << k | R } until x < M
 * (x lies on a cycle of a bijection of [0, 4^k) that passes through i < M, so the walk ends.)
 *
 * Batch row layout (floats), row_dim = obs_dim + 6 + action_dim + 4, rows row_stride =
 * round_up(row_dim, 4) apart:
 *   observation[obs_dim] | achieved_goal[3] | desired_goal[3] | action[action_dim] |
 *   old_value | old_log_prob | advantage | return
 * ---------------------------------------------------------------------- */
typedef struct pgx_rollout* pgx_rollout_handle;

#define PGX_ROLLOUT_ERR_OVERFLOW 1   /* pgx_rollout_add on a full buffer: nothing stored */
#define PGX_ROLLOUT_ERR_NOT_FULL 2   /* compute_returns_and_advantage with pos != n_steps: nothing written */
#define PGX_ROLLOUT_ERR_INDEX 4      /* pgx_rollout_gather: an index outside [0, M), its row is zero */

typedef struct pgx_rollout_config {
    int32_t n_envs;
    int32_t n_steps;              /* transitions per env (SB3 buffer_size) */
    int32_t obs_dim;
    int32_t action_dim;
    double gamma;                 /* in [0, 1] */
    double gae_lambda;            /* in [0, 1] */
    uint64_t seed;                /* of the minibatch permutations */
} pgx_rollout_config;

/* Device pointers of one add: the step's action and the policy's outputs for it, then the step's
 * results.  Nothing is written. */
typedef struct pgx_rollout_io {
    const float* action;                  /* [N,action_dim] */
    const float* reward;                  /* [N] */
    const float* value;                   /* [N] */
    const float* log_prob;                /* [N] */
    const float* terminal_value;          /* [N], may be NULL: no time-limit bootstrap */
    const float* obs;                     /* [N,obs_dim] post-step observation (the next carry); NULL with */
    const float* achieved_goal;           /* [N,3]        the two goals: the carry is left as it is       */
    const float* desired_goal;            /* [N,3] */
    const uint8_t* terminated;            /* [N], may be NULL: all 0 */
    const uint8_t* truncated;             /* [N], may be NULL: all 0 */
} pgx_rollout_io;

/* A gathered minibatch: rows [B, row_stride] f32 in the layout above, 16-byte aligned. */
typedef struct pgx_rollout_batch {
    float* rows;
} pgx_rollout_batch;

/* Device views of everything stored, for tests and tools: records [T][N][record_stride], the
 * planes [T][N], the carry, the words (pos: the first of the equal per-workgroup copies). */
typedef struct pgx_rollout_views {
    float* records;
    float* reward;
    float* episode_start;
    float* value;
    float* log_prob;
    float* advantage;
    float* returns;
    float* last_obs;
    float* last_achieved_goal;
    float* last_desired_goal;
    float* last_episode_start;
    int32_t* pos;
    uint32_t* errors;
    int32_t record_stride;
    int32_t pad0;
} pgx_rollout_views;

/* row_dim / row_stride of a batch row for this config (floats). */
int pgx_rollout_row_dim(const pgx_rollout_config* cfg);
int pgx_rollout_row_stride(const pgx_rollout_config* cfg);
/* PGX_E_INVALID, before any device call, for n_envs, n_steps, obs_dim or action_dim <= 0,
 * n_steps * n_envs >= 2^31, or gamma / gae_lambda outside [0, 1] (NaN included). */
int pgx_rollout_create(const pgx_rollout_config* cfg, int device, pgx_rollout_handle* out);
void pgx_rollout_destroy(pgx_rollout_handle h);
/* At slot pos: the carry's observation dict and episode_start with io's action, reward (plus the
 * bootstrap), value and log_prob; then carry = (io's observation dict, terminated | truncated) and
 * pos += 1.  With pos == n_steps: nothing stored, the carry untouched, PGX_ROLLOUT_ERR_OVERFLOW. */
int pgx_rollout_add(pgx_rollout_handle h, const pgx_rollout_io* io, void* stream);
/* The GAE pass above.  last_values [N] f32; dones [N] f32 0 / 1, or NULL: the carry's
 * episode_start.  With pos != n_steps: nothing written, PGX_ROLLOUT_ERR_NOT_FULL. */
int pgx_rollout_compute_returns_and_advantage(pgx_rollout_handle h, const float* last_values, const float* dones,
                                              void* stream);
/* out[i] = perm(i), i in [0, M), int32, for this handle's seed and the given epoch. */
int pgx_rollout_permutation(pgx_rollout_handle h, uint64_t epoch, int32_t* out, void* stream);
/* rows[b] = the transition with flat index indices[b] (device int32 [batch]); an index outside
 * [0, M) gives a row of zeros and PGX_ROLLOUT_ERR_INDEX. */
int pgx_rollout_gather(pgx_rollout_handle h, const int32_t* indices, int64_t batch, const pgx_rollout_batch* out,
                       void* stream);
/* SB3 rollout_buffer.reset(): pos = 0; the carry stays. */
int pgx_rollout_reset(pgx_rollout_handle h, void* stream);
/* The carry (SB3 _last_obs / _last_episode_starts after env.reset()): episode_start [N] f32 0 / 1,
 * or NULL: ones. */
int pgx_rollout_set_last(pgx_rollout_handle h, const float* obs, const float* achieved_goal, const float* desired_goal,
                         const float* episode_start, void* stream);
/* pos and errors after synchronising `stream` (either may be NULL); clear != 0 zeroes errors. */
int pgx_rollout_state(pgx_rollout_handle h, int32_t* pos, uint32_t* errors, int32_t clear, void* stream);
int pgx_rollout_arrays(pgx_rollout_handle h, pgx_rollout_views* out);

/* ----------------------------------------------------------------------
 * Actor: stable-baselines3's off-policy actor forward on the device (pgx_actor.hip), one launch
 * that reads the observation buffers of an env (or of a VecNormalize) and writes the action
 * buffer the next pgx_step reads, so observe -> act -> step -> collect captures into one graph.
 *
 * Features (SB3 CombinedExtractor over the Dict space, sorted keys), in_dim = obs_dim + 6:
 *   x = achieved_goal[3] | desired_goal[3] | observation[obs_dim]
 * Trunk: n_layers x (Linear + ReLU), widths hidden[l] in 1..512; relu(v) = v > 0 ? v : +0.
 * Heads: PGX_ACTOR_GAUSSIAN (SAC / TQC): mu and log_std, [action_dim] each;
 *        PGX_ACTOR_DETERMINISTIC (TD3 / DDPG): mu.
 *
 * Arithmetic contract (f32; what pgx_actor_forward_host restates and the kernel's f32-input MFMA
 * gives bit for bit).  Every Linear output o over inputs x[0..K):
 *   acc = bias[o];  for k = 0, 1, ..., K16 - 1 in ascending order:  acc = fmaf(x[k], W[o][k], acc)
 * THE ACCUMULATOR STARTS AT THE BIAS; nothing is added afterwards.  K16 = K rounded up to a
 * multiple of 16: the terms k >= K are fmaf(+0, +0, acc), which leave every accumulator but -0 as
 * it is (a -0 accumulator needs a -0 bias and only -0 products, and becomes +0).  One accumulator
 * per output, no split of the k range, no reassociation.
 *   mean    = mu's output; with clip_mean > 0: mean < -clip_mean ? -clip_mean : mean > clip_mean ?
 *             clip_mean : mean   (SB3's gSDE actor, Hardtanh); the `mean` debug plane holds this
 *   log_std = log_std's output v: v < -20 ? -20 : v > 2 ? 2 : v   (SB3 LOG_STD_MIN / LOG_STD_MAX)
 * Epilogue (f32, device tanhf / expf):
 *   GAUSSIAN:       action = tanhf(deterministic ? mean : fmaf(expf(log_std), eps, mean))
 *   DETERMINISTIC:  a = tanhf(mean); with noise (deterministic == 0): a = a + fmaf(noise_sigma, eps,
 *                   noise_mu) (SB3 _sample_action with NormalActionNoise); action = clip(a, -1, 1)
 *
 * Noise eps [N, action_dim]: the caller's buffer (io.eps), or, with io.eps NULL and deterministic
 * == 0, the device Philox4x32-10 stream: for env e and dimension pair p = d / 2
 *   r = philox(counter = (step lo, step hi, e, 0x41435430 ^ p), key = (seed lo, seed hi))
 *   u1 = ((r[0] >> 8) + 1) * 2^-24 in (0, 1],  u2 = (r[1] >> 8) * 2^-24 in [0, 1)
 *   rad = sqrtf(-2 logf(u1)), ang = 6.2831855f * u2
 *   eps[e][2 p] = rad * cosf(ang),  eps[e][2 p + 1] = rad * sinf(ang)        (r[2], r[3] unused)
 * `step` is a 64-bit device word (pgx_actor_state): a forward that draws from the stream adds one
 * to it behind its last read, inside the same launch, so every replay of a captured graph draws
 * new noise.  A forward with io.eps or with deterministic != 0 leaves the word alone.
 *
 * Weights are packed at pgx_actor_set_weights into the handle's buffers, per Linear as
 *   P[kb][tile][lane][i] = W[16 tile + (lane & 15)][16 kb + 4 i + (lane >> 4)], zero where W ends
 * (one 16-byte load per lane feeds four 16x16x4 MFMA steps); both heads share one tile, mu in
 * rows 0..6 and log_std in rows 8..14.
 * ---------------------------------------------------------------------- */
typedef struct pgx_actor* pgx_actor_handle;

#define PGX_ACTOR_GAUSSIAN 0
#define PGX_ACTOR_DETERMINISTIC 1
#define PGX_ACTOR_MAX_LAYERS 3
#define PGX_ACTOR_MAX_WIDTH 512
#define PGX_ACTOR_MAX_ACTION 7
#define PGX_ACTOR_LOG_STD_MIN -20.0f
#define PGX_ACTOR_LOG_STD_MAX 2.0f

typedef struct pgx_actor_config {
    int32_t n_envs;
    int32_t obs_dim;
    int32_t action_dim;           /* 1..7 */
    int32_t n_layers;             /* 1..3 hidden layers */
    int32_t hidden[3];            /* widths of the first n_layers, 1..512 each */
    int32_t kind;                 /* PGX_ACTOR_GAUSSIAN / PGX_ACTOR_DETERMINISTIC */
    double clip_mean;             /* >= 0; 0: off */
    double noise_mu;              /* DETERMINISTIC: NormalActionNoise mean */
    double noise_sigma;           /* >= 0 */
    uint64_t seed;                /* Philox key of the noise stream */
} pgx_actor_config;

/* torch-layout f32 parameters, device or host pointers: weight[l] [out, in] row-major and bias[l]
 * [out] for the hidden layers l < n_layers, then mu at index n_layers and, GAUSSIAN only, log_std
 * at index n_layers + 1. */
typedef struct pgx_actor_weights {
    const float* weight[5];
    const float* bias[5];
} pgx_actor_weights;

/* Device pointers of one forward.  Only `action` and the non-NULL debug planes are written. */
typedef struct pgx_actor_io {
    const float* obs;             /* [N,obs_dim] */
    const float* achieved_goal;   /* [N,3] */
    const float* desired_goal;    /* [N,3] */
    float* action;                /* [N,action_dim] */
    const float* eps;             /* [N,action_dim] or NULL: the device stream */
    float* mean_out;              /* debug [N,action_dim] or NULL: mean (after clip_mean) */
    float* log_std_out;           /* debug [N,action_dim] or NULL: log_std after the clamp (GAUSSIAN) */
    float* eps_out;               /* debug [N,action_dim] or NULL: the noise used (0 when deterministic) */
    uint32_t* philox_out;         /* debug [N,4,4] or NULL: r[0..3] of every pair p < (action_dim + 1) / 2,
                                     written when the device stream is drawn from */
} pgx_actor_io;

/* PGX_E_INVALID, before any device call and naming the field, for n_envs <= 0, obs_dim <= 0 (or
 * above 4096), action_dim outside 1..7, n_layers outside 1..3, a hidden width outside 1..512, an
 * unknown kind, a negative or NaN clip_mean / noise_sigma, a non-finite noise_mu, NULL cfg / out. */
int pgx_actor_create(const pgx_actor_config* cfg, int device, pgx_actor_handle* out);
void pgx_actor_destroy(pgx_actor_handle h);
/* Copies the parameters into the handle and packs them there, on `stream`: a captured graph sees
 * them at its next replay.  The sources must stay valid until the stream has run the copies. */
int pgx_actor_set_weights(pgx_actor_handle h, const pgx_actor_weights* w, void* stream);
/* One launch (see above). */
int pgx_actor_forward(pgx_actor_handle h, const pgx_actor_io* io, int32_t deterministic, void* stream);
/* The noise step word after synchronising `stream`; set: synchronises, then writes it. */
int pgx_actor_state(pgx_actor_handle h, uint64_t* step, void* stream);
int pgx_actor_set_state(pgx_actor_handle h, uint64_t step, void* stream);
/* The arithmetic contract above in plain C++ on host arrays (std::fmaf), for n rows: mean [n,
 * action_dim] and, GAUSSIAN with log_std_out != NULL, log_std.  cfg->n_envs is not read.  Never
 * touches a device; not a stepping path. */
int pgx_actor_forward_host(const pgx_actor_config* cfg, const pgx_actor_weights* w, const float* obs,
                           const float* achieved_goal, const float* desired_goal, int32_t n, float* mean_out,
                           float* log_std_out);

/* Action log-probability of a batch (GAUSSIAN kind): SB3's actor.action_log_prob(observations), i.e.
 * SquashedDiagGaussianDistribution.log_prob_from_params, for B rows in one launch.  B is a launch argument,
 * independent of n_envs; every row-indexed input carries its row stride in floats (row b of `obs` starts at
 * obs + b * obs_stride), so the fields of a HER batch's rows (pgx_replay_batch.rows) are read where they
 * lie; nothing batch-sized is kept in the handle.  Kernel launches only (one): it captures as one node.
 *
 * Features, trunk, the mu / log_std head tile, the clip_mean clamp and the [-20, 2] clamp: the forward's,
 * word for word (above).  Epilogue per (row b, dimension d), f32, NO CONTRACTION: every operation is
 * rounded on its own but the one fmaf written here (device expf / tanhf / logf):
 *   std = expf(log_std);  g = fmaf(std, eps, mean);  a = tanhf(g)                -> action[b][d]
 *   z = g - mean
 *   lp_d = ((-(z * z)) / (2 * (std * std)) - log_std) - 0.9189385f      (torch Normal.log_prob's order)
 *   c_d  = logf((1 - a * a) + 1e-6f)                                    (SB3: log(1 - actions**2 + epsilon))
 *   log_prob[b] = (lp_0 + lp_1 + ...) - (c_0 + c_1 + ...)
 * both sums start at their first term and add in ascending d.
 *
 * eps [B, action_dim]: the caller's dense buffer (io.eps), or, with io.eps NULL, the device Philox stream
 * through the forward's Box-Muller lines (above) with
 *   r = philox(counter = (word lo, word hi, b, PGX_ACTOR_LP_PHILOX_TAG ^ p), key = (seed lo, seed hi))
 * where `word` is a 64-bit device word of its own (pgx_actor_lp_state), moved on by one behind the last
 * read of every launch that draws, inside that launch: every replay of a captured graph draws new noise.
 * The forward's step word is never touched, and the tag is disjoint from the forward's (0x41435430 ^ p),
 * the ActorCritic's and the SdeActor's two.
 * Only action [B, A], log_prob [B] and the non-NULL debug planes are written, rows b < B only. */
#define PGX_ACTOR_LP_PHILOX_TAG 0x414C5030u

typedef struct pgx_actor_lp_io {
    const float* obs;             /* [B,obs_dim] */
    const float* achieved_goal;   /* [B,3] */
    const float* desired_goal;    /* [B,3] */
    const float* eps;             /* [B,action_dim] dense, or NULL: the device stream */
    float* action;                /* [B,action_dim] dense */
    float* log_prob;              /* [B] */
    float* mean_out;              /* debug [B,action_dim] or NULL: mean (after clip_mean) */
    float* log_std_out;           /* debug [B,action_dim] or NULL: log_std after the clamp */
    float* eps_out;               /* debug [B,action_dim] or NULL: the noise used */
    float* gaussian_action_out;   /* debug [B,action_dim] or NULL: g */
    uint32_t* philox_out;         /* debug [B,4,4] or NULL: as pgx_actor_io's, when the stream is drawn from
                                     (the host model never writes it) */
    int32_t obs_stride;           /* >= obs_dim */
    int32_t achieved_goal_stride; /* >= 3 */
    int32_t desired_goal_stride;  /* >= 3 */
    int32_t pad0;
} pgx_actor_lp_io;

/* One launch (see above).  PGX_E_INVALID, before any device call and naming the field, for a
 * DETERMINISTIC handle (kind), a NULL io / obs / achieved_goal / desired_goal / action / log_prob, B <= 0,
 * a stride below its width. */
int pgx_actor_action_log_prob(pgx_actor_handle h, const pgx_actor_lp_io* io, int32_t B, void* stream);
/* The log-probability noise word after synchronising `stream`; set: synchronises, then writes it. */
int pgx_actor_lp_state(pgx_actor_handle h, uint64_t* word, void* stream);
int pgx_actor_lp_set_state(pgx_actor_handle h, uint64_t word, void* stream);
/* The contract above in plain C++ on host arrays (std::fmaf, host libm; every pointer of io a host pointer,
 * strides honoured) for n rows, with the device entry's refusals and: a NULL io->eps (the host model has no
 * stream).  The mean and log_std planes are what the kernel meets bit for bit; the epilogue goes through
 * another libm.  Never touches a device. */
int pgx_actor_log_prob_host(const pgx_actor_config* cfg, const pgx_actor_weights* w, const pgx_actor_lp_io* io,
                            int32_t n);

/* ----------------------------------------------------------------------
 * ActorCritic: stable-baselines3's on-policy ActorCriticPolicy forward on the device
 * (pgx_actor_critic.hip), as MultiInputPolicy instantiates it for these envs (PPO): one launch gives
 * the action, the action clipped to the Box, V(obs) and the log-probability a RolloutBuffer stores; a
 * second entry gives V(obs) alone (predict_values), optionally only for the env tiles a mask names.
 *
 * Features: as the Actor's, x = achieved_goal[3] | desired_goal[3] | observation[obs_dim].
 * MlpExtractor: two separate trunks over x (SB3 >= 2.0 shares no layer): policy_net, n_pi_layers x
 * (Linear + ReLU) of widths pi_hidden[l], and value_net, n_vf_layers x (Linear + ReLU) of widths
 * vf_hidden[l]; 1..3 layers of 1..512 each, independently.  relu(v) = v > 0 ? v : +0.
 * Heads: action_net Linear(last pi width -> action_dim) gives mean; value_net Linear(last vf width
 * -> 1) gives value; log_std [action_dim] is a state-independent parameter (DiagGaussianDistribution).
 *
 * Arithmetic contract of every Linear: the Actor's, word for word (above): acc = bias[o], then
 * acc = fmaf(x[k], W[o][k], acc) for k = 0 .. K16 - 1 ascending, K16 = K rounded up to 16 with +0
 * padding, one accumulator per output, no split of K.  pgx_ac_forward_host restates it; the kernel's
 * v_mfma_f32_16x16x4_f32 meets it bit for bit.
 * Epilogue per env e and dimension d (f32, device expf; every operation rounded on its own, no
 * contraction but the one fmaf written here):
 *   std_d = expf(log_std[d])
 *   a_d   = deterministic ? mean_d : fmaf(std_d, eps_d, mean_d)            -> action[e][d]
 *           (SB3 stores the unclipped action)
 *   c_d   = a_d < -1 ? -1 : a_d > 1 ? 1 : a_d                               -> clipped_action[e][d]
 *           (collect_rollouts' np.clip to the Box: what the step reads)
 *   z_d   = a_d - mean_d
 *   lp_d  = ((-(z_d * z_d)) / (2 * (std_d * std_d)) - log_std[d]) - 0.9189385f
 *           (torch Normal.log_prob's order; log_std itself stands for log(scale))
 *   log_prob[e] = lp_0 + lp_1 + ... in ascending d
 *   value[e]    = value_net's one output
 * With deterministic != 0 log_prob is still written: the log-density of the mode, as SB3's
 * forward(deterministic=True) returns.
 *
 * Noise eps [N, action_dim]: io.eps, or with io.eps NULL and deterministic == 0 the device
 * Philox4x32-10 stream, defined as the Actor's but with the counter tag PGX_AC_PHILOX_TAG in place
 * of 0x41435430 (an Actor and an ActorCritic of one seed draw different numbers) and a 64-bit step
 * word of its own (pgx_ac_state), moved on by the same mechanism: the last workgroup to take a
 * ticket, behind every workgroup's read, adds one.  A forward with io.eps or deterministic != 0
 * leaves the word alone.
 *
 * pgx_ac_values: the value trunk and head alone; a computed value is bit for bit the forward's for
 * the same observation.  `need` (device uint8 [N], or NULL: all): a workgroup's tile of 16 (or 32)
 * consecutive envs none of which has need[e] != 0 runs no trunk and writes +0 for its envs; in every
 * other tile all envs are written.  (The time-limit bootstrap: few tiles hold a truncated env.)
 *
 * Packed weights: the Actor's P[kb][tile][lane][i] per Linear; action_net in rows 0..6 of the policy
 * head tile, value_net in row 0 of the value head tile.  One workgroup keeps the features in an LDS
 * region of their own (row stride: the first layer's K16 + 4 floats) beside the two activation
 * regions (row stride: the widest hidden layer's K16 + 4) and runs the policy trunk, then the value
 * trunk; it owns 32 envs from 4096 envs on where the three regions fit 160 KB, else 16.
 * ---------------------------------------------------------------------- */
typedef struct pgx_ac* pgx_ac_handle;

#define PGX_AC_PHILOX_TAG 0x50504F30u   /* counter word 3 of the noise stream, xor the dimension pair */

typedef struct pgx_ac_config {
    int32_t n_envs;
    int32_t obs_dim;
    int32_t action_dim;           /* 1..7 */
    int32_t n_pi_layers;          /* 1..3 */
    int32_t pi_hidden[3];         /* 1..512 each */
    int32_t n_vf_layers;          /* 1..3 */
    int32_t vf_hidden[3];         /* 1..512 each */
    int32_t pad0;
    uint64_t seed;                /* Philox key of the noise stream */
} pgx_ac_config;

/* torch-layout f32 parameters, device or host pointers: weight [out, in] row-major, bias [out]. */
typedef struct pgx_ac_weights {
    const float* pi_weight[3];
    const float* pi_bias[3];
    const float* vf_weight[3];
    const float* vf_bias[3];
    const float* action_net_weight;   /* [action_dim, last pi width] */
    const float* action_net_bias;
    const float* value_net_weight;    /* [1, last vf width] */
    const float* value_net_bias;
    const float* log_std;             /* [action_dim] */
} pgx_ac_weights;

/* Device pointers of one forward.  Only the non-NULL outputs and debug planes are written. */
typedef struct pgx_ac_io {
    const float* obs;             /* [N,obs_dim] */
    const float* achieved_goal;   /* [N,3] */
    const float* desired_goal;    /* [N,3] */
    float* action;                /* [N,action_dim] or NULL */
    float* clipped_action;        /* [N,action_dim] or NULL */
    float* value;                 /* [N] or NULL */
    float* log_prob;              /* [N] or NULL */
    const float* eps;             /* [N,action_dim] or NULL: the device stream */
    float* mean_out;              /* debug [N,action_dim] or NULL */
    float* eps_out;               /* debug [N,action_dim] or NULL: the noise used (0 when deterministic) */
    uint32_t* philox_out;         /* debug [N,4,4] or NULL: as pgx_actor_io's */
} pgx_ac_io;

/* PGX_E_INVALID, before any device call and naming the field, for n_envs <= 0, obs_dim <= 0 (or
 * above 4096), action_dim outside 1..7, n_pi_layers / n_vf_layers outside 1..3, a pi_hidden /
 * vf_hidden width outside 1..512, NULL cfg / out. */
int pgx_ac_create(const pgx_ac_config* cfg, int device, pgx_ac_handle* out);
void pgx_ac_destroy(pgx_ac_handle h);
/* Packs the parameters into the handle's buffers on `stream`: a captured graph sees them at its next
 * replay.  Device pointers are read where they lie, by kernel launches only; host pointers are first
 * copied into the handle (copy operations on `stream`).  The sources must stay valid until the stream
 * has run these.  pgx_ac_forward and pgx_ac_values are kernel launches only, whatever the arguments:
 * no memcpy or memset node, no allocation, no sync. */
int pgx_ac_set_weights(pgx_ac_handle h, const pgx_ac_weights* w, void* stream);
/* One launch on `stream` (see above). */
int pgx_ac_forward(pgx_ac_handle h, const pgx_ac_io* io, int32_t deterministic, void* stream);
/* V(obs) into value_out [N], one launch on `stream`; need: device uint8 [N] or NULL (see above). */
int pgx_ac_values(pgx_ac_handle h, const float* obs, const float* achieved_goal, const float* desired_goal,
                  const uint8_t* need, float* value_out, void* stream);
/* The noise step word after synchronising `stream`; set: synchronises, then writes it. */
int pgx_ac_state(pgx_ac_handle h, uint64_t* step, void* stream);
int pgx_ac_set_state(pgx_ac_handle h, uint64_t step, void* stream);
/* The arithmetic contract in plain C++ on host arrays (std::fmaf), for n rows: mean [n, action_dim]
 * and value [n] (either may be NULL).  cfg->n_envs is not read; w->log_std is not read.  Never
 * touches a device; not a stepping path. */
int pgx_ac_forward_host(const pgx_ac_config* cfg, const pgx_ac_weights* w, const float* obs, const float* achieved_goal,
                        const float* desired_goal, int32_t n, float* mean_out, float* value_out);

/* ----------------------------------------------------------------------
 * SdeActor: stable-baselines3's off-policy actor built with use_sde=True (sac/policies.py Actor;
 * sb3_contrib's TQC actor is the same class body), full_std=True, use_expln=False, latent_sde =
 * latent_pi: generalised state-dependent exploration on the device (pgx_sde_actor.hip).  Each env
 * holds an exploration matrix E[e] [H, A], resampled by pgx_sde_actor_reset_noise; between two
 * resets the noise is a fixed function of the state.
 *
 * Features and trunk: the Actor's, word for word (above): x = achieved_goal[3] | desired_goal[3] |
 * observation[obs_dim]; n_layers x (Linear + ReLU), widths hidden[l] in 1..512, every Linear output
 *   acc = bias[o];  for k = 0 .. K16 - 1 ascending:  acc = fmaf(x[k], W[o][k], acc)
 * with K16 = K rounded up to 16 (+0 padding), one accumulator per output.  latent[e][0..H) is the
 * last hidden activation, H = hidden[n_layers - 1].
 *   mean    = the mu Linear on that same chain over latent; with clip_mean > 0: mean < -clip_mean ?
 *             -clip_mean : mean > clip_mean ? clip_mean : mean (Hardtanh; SB3's default 2.0).  There
 *             is no log_std head and no [-20, 2] clamp: SB3's gSDE path has neither.
 *   std[h][a] = expf(log_std[h][a]), log_std a parameter [H, A]; computed by a kernel at
 *             pgx_sde_actor_set_weights and kept in the handle (pgx_sde_actor_get_std).
 *   noise[e][a]: ONE chain and nothing else,
 *             acc = +0;  for h = 0 .. H - 1 ascending:  acc = fmaf(latent[e][h], E[e][h][a], acc)
 *             (exactly H terms: no padding, no split into sub-chains, no reassociation).
 *   action  = tanhf(deterministic ? mean : mean + noise): one f32 add, device tanhf.  A
 *             deterministic forward reads no matrix.
 *
 * pgx_sde_actor_reset_noise resamples every env's matrix in one launch (SB3 sample_weights(log_std,
 * batch_size = n_envs): Normal(0, std).rsample() = eps * std).  `generation` is a 64-bit device word
 * (pgx_sde_actor_state); for env e, flat index j = h * A + a and block q = j / 4 (q < 1024):
 *   r = philox4x32_10(counter = (gen lo, gen hi, e, PGX_SDE_PHILOX_TAG ^ q), key = (seed lo, seed hi))
 *   (r[0], r[1]) through the Actor's Box-Muller lines (above) give eps[4 q], eps[4 q + 1];
 *   (r[2], r[3]) through the same lines give eps[4 q + 2], eps[4 q + 3];
 *   E[e][h][a] = eps[j] * std[h][a], one f32 multiply.
 * The counters are disjoint from the Actor's (0x41435430 ^ p) and the ActorCritic's (0x50504F30 ^ p).
 * The last workgroup of the launch to take a ticket, behind every workgroup's read of the word, adds
 * one to `generation`: every replay of a captured graph draws new matrices.  A forward never touches
 * the word or a matrix.
 *
 * The handle stores the matrices in a layout of its own (one 16-byte load per lane gives four
 * consecutive h of one (env, a), and a wave's loads are contiguous):
 *   S[e / 16][h / 4][e % 16][a][h % 4], H rounded up to 4 and n_envs to 16, padding kept at +0;
 * pgx_sde_actor_get_matrices / _set_matrices translate from and to SB3's [N, H, A] with a kernel.
 * Every entry below but create / destroy / state / set_state (and batch_state / batch_set_state) enqueues kernel launches only on the
 * caller's stream (no memcpy or memset node, no allocation, no sync), so everything captures;
 * pgx_sde_actor_set_weights first copies the parameters into the handle (copy operations on `stream`).
 * ---------------------------------------------------------------------- */
typedef struct pgx_sde_actor* pgx_sde_actor_handle;

#define PGX_SDE_PHILOX_TAG 0x53444500u   /* counter word 3 of the matrix draw, xor the block q */

typedef struct pgx_sde_actor_config {
    int32_t n_envs;
    int32_t obs_dim;
    int32_t action_dim;           /* 1..7 */
    int32_t n_layers;             /* 1..3 hidden layers */
    int32_t hidden[3];            /* widths of the first n_layers, 1..512 each */
    int32_t pad0;
    double clip_mean;             /* >= 0; 0: off */
    uint64_t seed;                /* Philox key of the matrix draw */
} pgx_sde_actor_config;

/* torch-layout f32 parameters, device or host pointers: weight[l] [out, in] row-major and bias[l]
 * [out] for the hidden layers l < n_layers, then mu at index n_layers; log_std [H, action_dim]. */
typedef struct pgx_sde_actor_weights {
    const float* weight[4];
    const float* bias[4];
    const float* log_std;
} pgx_sde_actor_weights;

/* Device pointers of one forward.  Only `action` and the non-NULL debug planes are written. */
typedef struct pgx_sde_actor_io {
    const float* obs;             /* [N,obs_dim] */
    const float* achieved_goal;   /* [N,3] */
    const float* desired_goal;    /* [N,3] */
    float* action;                /* [N,action_dim] */
    float* mean_out;              /* debug [N,action_dim] or NULL: mean (after clip_mean) */
    float* latent_out;            /* debug [N,H] or NULL */
    float* noise_out;             /* debug [N,action_dim] or NULL: the noise chain (+0 when deterministic) */
} pgx_sde_actor_io;

/* PGX_E_INVALID, before any device call and naming the field, for n_envs <= 0, obs_dim <= 0 (or
 * above 4096), action_dim outside 1..7, n_layers outside 1..3, a hidden width outside 1..512, a
 * negative or non-finite clip_mean, NULL cfg / out.  The matrices (+0) and std (+0) are allocated here. */
int pgx_sde_actor_create(const pgx_sde_actor_config* cfg, int device, pgx_sde_actor_handle* out);
void pgx_sde_actor_destroy(pgx_sde_actor_handle h);
/* Copies the parameters into the handle, packs them and computes std there, on `stream`: a captured
 * graph sees them at its next replay.  The sources must stay valid until the stream has run the copies. */
int pgx_sde_actor_set_weights(pgx_sde_actor_handle h, const pgx_sde_actor_weights* w, void* stream);
/* One launch: every env's matrix from `generation`, which it moves on by one (see above).  Debug planes
 * (device, or NULL): eps_out [N, H, A] f32, philox_out [N, 4, 4] u32 (r[0..3] of the blocks q < 4). */
int pgx_sde_actor_reset_noise(pgx_sde_actor_handle h, float* eps_out, uint32_t* philox_out, void* stream);
/* One launch (see above). */
int pgx_sde_actor_forward(pgx_sde_actor_handle h, const pgx_sde_actor_io* io, int32_t deterministic, void* stream);
/* The generation word after synchronising `stream`; set: synchronises, then writes it. */
int pgx_sde_actor_state(pgx_sde_actor_handle h, uint64_t* generation, void* stream);
int pgx_sde_actor_set_state(pgx_sde_actor_handle h, uint64_t generation, void* stream);
/* The matrices as SB3 lays them out, device f32 [N, H, A]: one launch each on `stream`. */
int pgx_sde_actor_get_matrices(pgx_sde_actor_handle h, float* out, void* stream);
int pgx_sde_actor_set_matrices(pgx_sde_actor_handle h, const float* in, void* stream);
/* std into device f32 [H, A]: one launch on `stream`. */
int pgx_sde_actor_get_std(pgx_sde_actor_handle h, float* out, void* stream);
/* The arithmetic contract above in plain C++ on host arrays (std::fmaf), for n rows with their
 * matrices [n, H, A]: mean [n, action_dim], latent [n, H], noise [n, action_dim] (each may be NULL).
 * cfg->n_envs, cfg->seed and w->log_std are not read.  Never touches a device; not a stepping path. */
int pgx_sde_actor_forward_host(const pgx_sde_actor_config* cfg, const pgx_sde_actor_weights* w, const float* obs,
                               const float* achieved_goal, const float* desired_goal, const float* matrices, int32_t n,
                               float* mean_out, float* latent_out, float* noise_out);

/* Action log-probability of a batch: SB3's actor.action_log_prob(observations) on the gSDE distribution
 * (StateDependentNoiseDistribution.log_prob_from_params) as TQC.train reaches it, for B rows in one
 * launch.  The batch length differs from the number of per-env matrices, so SB3's get_noise takes the ONE
 * shared exploration_mat [H, A], not the per-env ones: the handle holds a shared matrix Eb [H, A] beside
 * them, and std2[h][a] = std[h][a] * std[h][a] (one f32 multiply, computed where std is, at
 * pgx_sde_actor_set_weights).  B, the row strides, what is written and the capture are as
 * pgx_actor_action_log_prob's (above).
 *
 * latent and mean: the forward's, word for word.  With K16 = H rounded up to 16, per (row b, dimension a):
 *   noise[b][a] = the Linear chain:  acc = +0;  for h = 0 .. K16 - 1 ascending:  acc = fmaf(latent[b][h],
 *                 Eb[h][a], acc), the terms h >= H being fmaf(+0, +0, acc)
 *   var[b][a]   = the same chain over sq[b][h] = latent[b][h] * latent[b][h] (one f32 multiply) against std2[h][a]
 *   (Both are the mu Linear's chain with bias +0, so the kernel's MFMA carries them: Eb is packed into rows
 *   8..14 of mu's tile, std2 into a tile of its own.  The per-env forward's noise chain has exactly H terms:
 *   with the same matrix the two agree bit for bit where H is a multiple of 16, and elsewhere but for a -0
 *   sum, which the +0 padding turns into +0.)
 * then in f32, no contraction, every operation rounded on its own (device sqrtf / tanhf / log1pf / logf):
 *   scale = sqrtf(var + 1e-6f)                                  (SB3: sqrt(variance + epsilon))
 *   a = tanhf(mean + noise)                                                       -> action[b][a]
 *   x = a < -(1 - EPS) ? -(1 - EPS) : a > (1 - EPS) ? (1 - EPS) : a,   EPS = 1.1920929e-7f
 *   g' = 0.5f * (log1pf(x) - log1pf(-x))        (TanhBijector.inverse: SB3's gSDE path recovers the Gaussian
 *                                                action from the squashed one)
 *   z = g' - mean
 *   lp_a = ((-(z * z)) / (2 * (scale * scale)) - logf(scale)) - 0.9189385f
 *   t = tanhf(g');  c_a = logf((1 - t * t) + 1e-6f)
 *   log_prob[b] = (lp_0 + lp_1 + ...) - (c_0 + c_1 + ...)   both sums from their first term, ascending a
 *
 * pgx_sde_actor_reset_batch_noise draws Eb = eps * std in one launch (SB3 actor.reset_noise() at the top of a
 * gradient step: sample_weights' exploration_mat): for flat index j = h * A + a and block q = j / 4,
 *   r = philox4x32_10(counter = (bgen lo, bgen hi, 0, PGX_SDE_BATCH_PHILOX_TAG ^ q), key = (seed lo, seed hi))
 * and the per-env draw's lines from there.  `bgen` is a 64-bit device word of its own
 * (pgx_sde_actor_batch_state) that the launch moves on by one.  PGX_SDE_BATCH_PHILOX_TAG ^ q, q < 1024, spans
 * 0x53444000 .. 0x534443FF; PGX_SDE_PHILOX_TAG ^ q spans 0x53444400 .. 0x534447FF.  The per-env matrices,
 * their generation word and pgx_sde_actor_reset_noise are untouched by all of this. */
#define PGX_SDE_BATCH_PHILOX_TAG 0x53444200u

typedef struct pgx_sde_actor_lp_io {
    const float* obs;             /* [B,obs_dim] */
    const float* achieved_goal;   /* [B,3] */
    const float* desired_goal;    /* [B,3] */
    float* action;                /* [B,action_dim] dense */
    float* log_prob;              /* [B] */
    float* mean_out;              /* debug [B,action_dim] or NULL: mean (after clip_mean) */
    float* latent_out;            /* debug [B,H] or NULL */
    float* noise_out;             /* debug [B,action_dim] or NULL */
    float* variance_out;          /* debug [B,action_dim] or NULL: var */
    float* gaussian_action_out;   /* debug [B,action_dim] or NULL: g' */
    int32_t obs_stride;           /* >= obs_dim */
    int32_t achieved_goal_stride; /* >= 3 */
    int32_t desired_goal_stride;  /* >= 3 */
    int32_t pad0;
} pgx_sde_actor_lp_io;

/* One launch (see above).  PGX_E_INVALID, before any device call and naming the field, for a NULL io / obs /
 * achieved_goal / desired_goal / action / log_prob, B <= 0, a stride below its width. */
int pgx_sde_actor_action_log_prob(pgx_sde_actor_handle h, const pgx_sde_actor_lp_io* io, int32_t B, void* stream);
/* One launch: Eb from `bgen`, which it moves on by one.  Debug (device, or NULL): eps_out [H, A] f32. */
int pgx_sde_actor_reset_batch_noise(pgx_sde_actor_handle h, float* eps_out, void* stream);
/* Eb as SB3 lays exploration_mat out, device f32 [H, A]: one launch each on `stream`. */
int pgx_sde_actor_get_batch_matrix(pgx_sde_actor_handle h, float* out, void* stream);
int pgx_sde_actor_set_batch_matrix(pgx_sde_actor_handle h, const float* in, void* stream);
/* The batch generation word after synchronising `stream`; set: synchronises, then writes it. */
int pgx_sde_actor_batch_state(pgx_sde_actor_handle h, uint64_t* generation, void* stream);
int pgx_sde_actor_batch_set_state(pgx_sde_actor_handle h, uint64_t generation, void* stream);
/* The contract above in plain C++ on host arrays (std::fmaf, host libm; every pointer a host pointer, strides
 * honoured) for n rows, with the device entry's refusals and: a NULL exploration_mat.  std [H, A]: what the
 * handle holds (pgx_sde_actor_get_std), or NULL: expf(w->log_std) by the host's libm.  The mean, latent,
 * noise and variance planes are what the kernel meets bit for bit; the epilogue goes through another libm.
 * Never touches a device. */
int pgx_sde_actor_log_prob_host(const pgx_sde_actor_config* cfg, const pgx_sde_actor_weights* w, const float* std,
                                const float* exploration_mat, const pgx_sde_actor_lp_io* io, int32_t n);

/* ----------------------------------------------------------------------
 * QuantileCritic: sb3_contrib TQC's quantile critics on the device (pgx_quantile_critic.hip): the
 * forward of `critic` or `critic_target` (tqc/policies.py, Critic.forward), the no_grad block of
 * TQC.train that builds the truncated TD target (tqc/tqc.py) as one launch, and the Polyak step.  The
 * critic loss, its gradient and Adam: "the critic update", further down.  This is a restatement: neither library is importable where this is built,
 * parity against them is not pinned by a test.
 *
 * Networks: n_critics independent nets qf0 .. qf{n-1}; each n_layers x (Linear + ReLU), widths
 * hidden[l], then a Linear to n_quantiles outputs.  Features, K = obs_dim + 6 + action_dim:
 *   x = achieved_goal[3] | desired_goal[3] | observation[obs_dim] | action[action_dim]
 * (CombinedExtractor's order, then th.cat([obs, action], dim=1)).  quantiles [B, n_critics,
 * n_quantiles] (th.stack(..., dim=1)).  The handle holds two parameter sets, PGX_QC_ONLINE (`critic`)
 * and PGX_QC_TARGET (`critic_target`).
 *
 * Arithmetic contract of every Linear: the Actor's, word for word (above): acc = bias[o], then
 * acc = fmaf(x[k], W[o][k], acc) for k = 0 .. K16 - 1 ascending, K16 = K rounded up to 16 with +0
 * padding, one accumulator per output, no split of K; relu(v) = v > 0 ? v : +0.  The head spans
 * ceil(n_quantiles / 16) output tiles.  pgx_qc_forward_host restates it; the kernel's
 * v_mfma_f32_16x16x4_f32 meets it bit for bit.
 *
 * Truncated target (pgx_qc_target), T = n_critics * n_quantiles, per row b < B:
 *   z[c * n_quantiles + q] = quantile q of critic c of the TARGET set on the row's features
 *   sort z ascending by the ORDER RULE: element i precedes element j when key(z[i]) < key(z[j]), or
 *     the keys are equal and i < j, where for the f32's bits u (uint32)
 *       key(u) = u & 0x80000000 ? ~u : u | 0x80000000
 *     compared as unsigned integers.  The order is total on all bit patterns: -inf < negative < -0 <
 *     +0 < positive < +inf, equal bits by flat index; a NaN with the sign bit set sorts below -inf,
 *     one without above +inf.  Every element gets exactly one of the ranks 0 .. T - 1.
 *   keep the n_target lowest: z_(0) .. z_(n_target - 1)
 *   then in f32, every operation rounded on its own (no contraction):
 *     t1 = ent_coef * next_log_prob[b]
 *     t2 = z_(k) - t1
 *     m  = (1.0f - done[b]) * (float)gamma
 *     out[b][k] = reward[b] + m * t2
 *   (tqc.py: next_quantiles - ent_coef * next_log_prob.reshape(-1, 1); rewards + (1 - dones) * gamma *
 *   target_quantiles, with (1 - dones) * gamma evaluated first as Python does).  Every out[b][k], k <
 *   n_target, b < B, is written whatever the input bits; what a row with a NaN holds is outside the
 *   contract; nothing else is written.  ent_coef is read from device memory (one float) at every
 *   launch.  n_quantiles = 1, n_target = 1 is SAC's / TD3's min over the critics.
 *
 * Polyak (pgx_qc_polyak; SB3 polyak_update(critic.parameters(), critic_target.parameters(), tau)), on
 * the handle's plain copies, per parameter element, in f32:
 *     t = fmaf((float)tau, p, t * (float)(1.0 - tau))
 * the product t * (float)(1.0 - tau) rounded first, 1.0 - tau taken in double; then the target set is
 * packed again from its plain copy.  torch's kernel for mul_ / add_(alpha=) may round differently:
 * parity of this rule with torch is not pinned.  pgx_qc_sync_target copies online -> target bit for
 * bit (plain and packed).
 *
 * Packed weights: the Actor's P[kb][tile][lane][i] per Linear, per critic, per set.  A workgroup of 4
 * waves owns 32 rows (16 for B <= 16, or where 32 do not fit the LDS) and runs the critics one after the other on
 * features staged once; the pooled quantiles stay in LDS for the sort (rank by counting).  LDS per
 * workgroup: 4 rows (max(K16 + 4 + 2 (H16 + 4), T4) + 16 n_critics ceil(n_quantiles / 16) + 4) bytes, H16
 * the widest hidden width rounded up to 16, T4 = T rounded up to 4 (pgx_qc_create states the limit).
 * Every entry below but create / destroy / get_weights enqueues kernel launches only on the caller's
 * stream (no memcpy or memset node, no allocation, no sync), so everything captures as a single chain;
 * pgx_qc_set_weights first copies the parameters into the handle (copy operations on `stream`).
 * ---------------------------------------------------------------------- */
typedef struct pgx_qc* pgx_qc_handle;

#define PGX_QC_ONLINE 0          /* `critic` */
#define PGX_QC_TARGET 1          /* `critic_target` */
#define PGX_QC_MAX_CRITICS 5
#define PGX_QC_MAX_QUANTILES 32
#define PGX_QC_MAX_POOL 128      /* n_critics * n_quantiles at the most */

typedef struct pgx_qc_config {
    int32_t obs_dim;
    int32_t action_dim;           /* 1..7 */
    int32_t n_layers;             /* 1..3 hidden layers */
    int32_t hidden[3];            /* widths of the first n_layers, 1..512 each */
    int32_t n_critics;            /* 1..5 */
    int32_t n_quantiles;          /* 1..32; n_critics * n_quantiles <= 128 */
    double gamma;                 /* finite */
} pgx_qc_config;

/* torch-layout f32 parameters of one set, device or host pointers: for critic c, weight[c][l] [out, in]
 * row-major and bias[c][l] [out] for the hidden layers l < n_layers, then the quantile head at index
 * n_layers (state-dict keys qf{c}.{2 l}.weight / .bias). */
typedef struct pgx_qc_weights {
    const float* weight[5][4];
    const float* bias[5][4];
} pgx_qc_weights;

/* Pointers of one launch (device for pgx_qc_forward / pgx_qc_target, host for the host models), each
 * row-indexed input with its row stride in floats: row b of `obs` starts at obs + b * obs_stride.  A
 * dense [B, width] tensor has stride = width; the fields of a HER batch's rows (pgx_replay_batch.rows)
 * are read in place with stride = pgx_replay_row_stride.  pgx_qc_forward reads obs .. action and writes
 * `out`; pgx_qc_target reads everything (obs .. action hold the NEXT observation and the next action). */
typedef struct pgx_qc_io {
    const float* obs;             /* [B,obs_dim] */
    const float* achieved_goal;   /* [B,3] */
    const float* desired_goal;    /* [B,3] */
    const float* action;          /* [B,action_dim] */
    const float* reward;          /* target: [B] */
    const float* done;            /* target: [B], 0.0f or 1.0f */
    const float* next_log_prob;   /* target: [B], dense */
    const float* ent_coef;        /* target: one float */
    float* out;                   /* forward: [B,n_critics,n_quantiles]; target: [B,n_target]; dense */
    float* quantiles_out;         /* target: debug [B,n_critics,n_quantiles] or NULL: z before the sort */
    int32_t obs_stride;           /* >= obs_dim */
    int32_t achieved_goal_stride; /* >= 3 */
    int32_t desired_goal_stride;  /* >= 3 */
    int32_t action_stride;        /* >= action_dim */
    int32_t reward_stride;        /* target: >= 1 */
    int32_t done_stride;          /* target: >= 1 */
} pgx_qc_io;

/* tqc/policies.py, Critic.__init__ (both sets, parameters +0).  PGX_E_INVALID, before any device call and
 * naming the field, for obs_dim outside 1..4096, action_dim outside 1..7, n_layers outside 1..3, a
 * hidden width outside 1..512, n_critics outside 1..5, n_quantiles outside 1..32, n_critics *
 * n_quantiles > 128, a non-finite gamma, NULL cfg / out.  PGX_E_UNSUPPORTED where a workgroup's LDS
 *   64 * (max(K16 + 4 + 2 (H16 + 4), T4) + 16 n_critics ceil(n_quantiles / 16) + 4) bytes (16 rows)
 * exceeds 160 KiB - 512: with one hidden layer of 16, one critic, one quantile and action_dim 3 the
 * widest accepted obs_dim is 2471 (K16 = 2480). */
int pgx_qc_create(const pgx_qc_config* cfg, int device, pgx_qc_handle* out);
void pgx_qc_destroy(pgx_qc_handle h);
/* critic.load_state_dict / critic_target.load_state_dict: copies set `which`'s parameters into the handle
 * and packs them there, on `stream`: a captured graph sees them at its next replay.  The sources must
 * stay valid until the stream has run the copies. */
int pgx_qc_set_weights(pgx_qc_handle h, int32_t which, const pgx_qc_weights* w, void* stream);
/* The handle's plain copy of set `which` (what pgx_qc_polyak updates) into w's pointers, device or host:
 * copy operations on `stream`, then a synchronise of it.  (critic_target.state_dict().) */
int pgx_qc_get_weights(pgx_qc_handle h, int32_t which, const pgx_qc_weights* w, void* stream);
/* tqc.py: current_quantiles = self.critic(observations, actions) (which = PGX_QC_ONLINE), or
 * self.critic_target(...): one launch.  PGX_E_INVALID, before any device call and naming the field, for a
 * NULL obs / achieved_goal / desired_goal / action / out, B <= 0, a stride below its width. */
int pgx_qc_forward(pgx_qc_handle h, int32_t which, const pgx_qc_io* io, int32_t B, void* stream);
/* tqc.py, the no_grad block of train(): next_quantiles = self.critic_target(next_observations,
 * next_actions); sorted_z, _ = th.sort(next_quantiles.reshape(batch_size, -1)); sorted_z_part =
 * sorted_z[:, :n_target_quantiles]; target_quantiles = sorted_z_part - ent_coef * next_log_prob;
 * target_quantiles = rewards + (1 - dones) * gamma * target_quantiles: one launch (see above).
 * pgx_qc_forward's refusals, and: a NULL reward / done / next_log_prob / ent_coef, n_target outside 1..T,
 * reward_stride / done_stride < 1. */
int pgx_qc_target(pgx_qc_handle h, const pgx_qc_io* io, int32_t B, int32_t n_target, void* stream);
/* tqc.py: polyak_update(self.critic.parameters(), self.critic_target.parameters(), self.tau): one launch
 * over the plain copies, then the packing launches (see above).  PGX_E_INVALID naming tau (checked first)
 * for tau outside [0, 1] or NaN. */
int pgx_qc_polyak(pgx_qc_handle h, double tau, void* stream);
/* tqc/policies.py: self.critic_target.load_state_dict(self.critic.state_dict()): one launch. */
int pgx_qc_sync_target(pgx_qc_handle h, void* stream);
/* The contracts above in plain C++ on host arrays (std::fmaf; every pointer of io a host pointer, strides
 * honoured, *io->ent_coef read), with the device entries' refusals.  w: the set to use.  forward: io->out
 * [B, n_critics, n_quantiles]; target: io->out [B, n_target] and, non-NULL, io->quantiles_out.  Never
 * touch a device; not a stepping path. */
int pgx_qc_forward_host(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_io* io, int32_t B);
int pgx_qc_target_host(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_io* io, int32_t B,
                       int32_t n_target);

/* ----------------------------------------------------------------------
 * QuantileCritic, the critic update: TQC.train's critic loss, its gradient with respect to every
 * parameter of the ONLINE set, and torch.optim.Adam's step on them (pgx_quantile_critic.hip).  A
 * restatement of sb3_contrib (tqc.py: critic_loss = quantile_huber_loss(current_quantiles,
 * target_quantiles, sum_over_quantiles=False); critic.optimizer.zero_grad(); critic_loss.backward();
 * critic.optimizer.step()) and of torch's Adam; parity with either is held to fp64 by the tests, not
 * pinned bit for bit.  The actor loss, the ent_coef loss, dQ/d(action) and gradient clipping are not here.
 *
 * Loss.  q[b][c][j]: the ONLINE set's quantiles of row b, bit for bit pgx_qc_forward's.  t[b][k], k <
 * n_target: target_quantiles.  n_q = n_quantiles.  In f32, every operation rounded on its own but the
 * named fmaf:
 *     tau_j = ((float)j + 0.5f) / (float)n_q
 *     d     = t[b][k] - q[b][c][j]
 *     w     = fabsf(tau_j - (d < 0 ? 1.0f : 0.0f))
 *     huber = fabsf(d) > 1.0f ? fabsf(d) - 0.5f : (d * d) * 0.5f
 *     clamp = d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d)
 *     lt[b][c][j] = chain over k = 0 .. n_target - 1 ascending from +0: acc = fmaf(w, huber, acc)
 *     gs[b][c][j] = chain over k = 0 .. n_target - 1 ascending from +0: acc = fmaf(w, clamp, acc)
 *     inv_count = 1.0f / (float)(B * n_critics * n_q * n_target)     (the product as a 64-bit integer)
 *     dq[b][c][j] = (-inv_count) * gs[b][c][j]
 *     rl[b] = sum from +0 of lt[b][c][j] in ascending flat index c * n_q + j, one addition per term
 *     seg[i] = sum from +0 of rl[b], b = 64 i .. min(64 i + 63, B - 1) ascending
 *     loss = (sum from +0 of seg[i], i ascending) * inv_count
 * The segment length 64 is a constant: the order depends on B alone, never on the row tile or the grid.
 *
 * Backward.  A_l [B, H_l]: the output of hidden layer l behind its ReLU; A_{-1} = x, the features.  dZ_l:
 * the gradient at layer l's pre-activation; the head's (l = n_layers) is dq.  O16 / B4: a count rounded
 * up to 16 / 4, the padding terms +0 * +0 (they turn an accumulator of -0 into +0, nothing else).
 *     dA_{l-1}[b][k] = chain over o = 0 .. O16_l - 1 ascending from +0: acc = fmaf(dZ_l[b][o], W_l[o][k], acc)
 *     dZ_{l-1}[b][k] = A_{l-1}[b][k] > 0 ? dA_{l-1}[b][k] : +0        (a unit at +-0 passes nothing)
 *     dW_l[o][k] = chain over b = 0 .. B4 - 1 ascending from +0: acc = fmaf(dZ_l[b][o], A_{l-1}[b][k], acc)
 *     db_l[o]    = chain over b = 0 .. B4 - 1 ascending from +0: acc = fmaf(dZ_l[b][o], b < B ? 1.0f : +0, acc)
 * One accumulator per output, no split of any sum, no atomics: v_mfma_f32_16x16x4_f32 meets each chain bit
 * for bit (four terms per instruction, in ascending order).  A NaN in a row of target_quantiles makes the
 * loss NaN and poisons every sum its dq reaches, as in torch; a NaN feature goes through the forward's
 * relu(v) = v > 0 ? v : +0 as in pgx_qc_forward.
 *
 * Adam (torch.optim.Adam as SB3 builds it: no weight decay, no amsgrad), per parameter element with its
 * gradient g, in f32, every operation rounded on its own:
 *     step = step + 1                                              (a 64-bit device word)
 *     p1 = beta1 ^ step, p2 = beta2 ^ step in double by squaring: p = 1, s = beta; for the bits of step
 *          from the lowest: if the bit is set p = p * s; then s = s * s
 *     bc1 = (float)(1.0 - p1); bc2 = (float)(1.0 - p2)
 *     step_size = lr / bc1; c2 = sqrtf(bc2)                       (lr: one device float, read at every launch)
 *     m = m + (g - m) * (float)(1.0 - beta1)
 *     v = v * (float)beta2 + (float)(1.0 - beta2) * (g * g)
 *     u = step_size * (m / (sqrtf(v) / c2 + (float)eps))
 *     p = u == 0 ? p : p - u                                       (lr = 0 leaves every bit of p alone)
 * then the online set is packed again, and so is the transposed packing the backward reads.
 *
 * Workspace.  The backward needs every row's activations and dZ; the handle keeps no batch-sized storage.
 * The caller passes pgx_qc_grad_workspace_floats(cfg, B) floats: per row, K16 features, per critic the A_l
 * and dZ_l planes (each width rounded up to 16), and 16 floats of loss terms.  Rows past B are never
 * written.  The gradient buffer (torch layout, as pgx_qc_weights addresses it), exp_avg, exp_avg_sq, the
 * step word and the transposed packing live in the handle, allocated by pgx_qc_init_training, never by a
 * launch entry.  pgx_qc_critic_grad and pgx_qc_adam_step enqueue kernel launches only (no memcpy or
 * memset node, no allocation, no sync).
 * ---------------------------------------------------------------------- */
typedef struct pgx_qc_grad_io {
    const float* obs;              /* [B,obs_dim] */
    const float* achieved_goal;    /* [B,3] */
    const float* desired_goal;     /* [B,3] */
    const float* action;           /* [B,action_dim] */
    const float* target_quantiles; /* [B,n_target], dense (pgx_qc_target's out) */
    float* workspace;              /* workspace_floats floats */
    float* loss;                   /* one float */
    float* quantiles_out;          /* debug [B,n_critics,n_quantiles] or NULL: q */
    float* dq_out;                 /* debug [B,n_critics,n_quantiles] or NULL */
    float* dz_out;                 /* debug [B, n_critics * (hidden[0] + .. )] or NULL: dZ_l of critic c at
                                      column c * sum(hidden) + hidden[0] + .. + hidden[l - 1] */
    int64_t workspace_floats;      /* >= pgx_qc_grad_workspace_floats(cfg, B) */
    int32_t obs_stride;            /* >= obs_dim */
    int32_t achieved_goal_stride;  /* >= 3 */
    int32_t desired_goal_stride;   /* >= 3 */
    int32_t action_stride;         /* >= action_dim */
} pgx_qc_grad_io;

/* Floats of workspace one pgx_qc_critic_grad of B rows needs; negative (PGX_E_INVALID) for a config
 * pgx_qc_create refuses or B <= 0. */
int64_t pgx_qc_grad_workspace_floats(const pgx_qc_config* cfg, int32_t B);
/* Allocates the training state (see above), zeroes exp_avg, exp_avg_sq and step, and packs the online
 * set's transposed copy.  Again: zeroes the state and takes the new constants, allocates nothing.
 * PGX_E_INVALID naming the field for beta1 / beta2 outside [0, 1), eps not finite or <= 0. */
int pgx_qc_init_training(pgx_qc_handle h, double beta1, double beta2, double eps);
/* The loss and the gradient buffer of one batch: two launches.  pgx_qc_forward's refusals on obs ..
 * action, and, naming the field: a NULL target_quantiles / workspace / loss, n_target outside 1..T,
 * workspace_floats below pgx_qc_grad_workspace_floats; "pgx_qc_init_training" where that was not called.
 * A refusal launches nothing. */
int pgx_qc_critic_grad(pgx_qc_handle h, const pgx_qc_grad_io* io, int32_t B, int32_t n_target, void* stream);
/* The gradient buffer into w's pointers (device or host), then a synchronise of `stream`. */
int pgx_qc_get_grads(pgx_qc_handle h, const pgx_qc_weights* w, void* stream);
/* One Adam step on the online set from the gradient buffer (see above).  lr: one device float. */
int pgx_qc_adam_step(pgx_qc_handle h, const float* lr, void* stream);
/* The optimiser state, for checkpoints: exp_avg / exp_avg_sq in torch layout, and the step word.  get
 * synchronises `stream` behind its copies; set synchronises, then writes all three. */
int pgx_qc_get_opt_state(pgx_qc_handle h, const pgx_qc_weights* exp_avg, const pgx_qc_weights* exp_avg_sq,
                         uint64_t* step, void* stream);
int pgx_qc_set_opt_state(pgx_qc_handle h, const pgx_qc_weights* exp_avg, const pgx_qc_weights* exp_avg_sq,
                         uint64_t step, void* stream);
/* The contracts above in plain C++ on host arrays (std::fmaf), with the device entries' refusals (one
 * launch check serves both).  critic_grad_host: w the online set, grads written through its pointers,
 * *io->loss, the debug planes where non-NULL, io->workspace used as the device entry uses it.
 * adam_step_host: params, exp_avg and exp_avg_sq updated in place, *step moved on.  Never touch a device. */
int pgx_qc_critic_grad_host(const pgx_qc_config* cfg, const pgx_qc_weights* w, const pgx_qc_grad_io* io, int32_t B,
                            int32_t n_target, const pgx_qc_weights* grads);
int pgx_qc_adam_step_host(const pgx_qc_config* cfg, const pgx_qc_weights* params, const pgx_qc_weights* grads,
                          const pgx_qc_weights* exp_avg, const pgx_qc_weights* exp_avg_sq, uint64_t* step, double lr,
                          double beta1, double beta2, double eps);

#ifdef __cplusplus
}
#endif

#endif /* PGX_H */
