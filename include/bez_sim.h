/* bez_sim.h -- C ABI of the MI355X-native Bez `bez_kick` simulator (libbez_sim.so).
 *
 * This is the drop-in boundary for the hot path VecTask.step():
 *   reference  bez_isaacgym/tasks/base/vec_task.py:303-349   (step orchestration)
 *              bez_isaacgym/tasks/kick_env.py:410-438,749-850 (pre/post physics, obs, reset)
 * The reference has no FFI of its own: everything below the Python `VecTask` goes into the
 * closed Isaac Gym binary through the `gymapi` tensor API.  Each entry point therefore cites
 * the gym call (and its call site in the reference) that it replaces.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*
 *     (NULL = the null stream).  All work is enqueued on that stream; nothing synchronises
 *     unless stated.
 *   - every pointer named *_dev is device memory on the sim's GPU, borrowed for the call.
 *   - every function returns 0 on success, <0 on error (message: bez_sim_last_error()).
 *   - the sim owns all state buffers for its lifetime; bez_sim_get_tensor() exposes them
 *     zero-copy (gymtorch.wrap_tensor equivalent, kick_env.py:155-157).
 *   - Isaac-layout tensors (row-major AoS, fp32, per env: A actors, B bodies, 18 DOFs):
 *       ROOT_STATE        (N*A, 13)  pos3 quat_xyzw4 linvel3 angvel3     kick_env.py:143
 *       DOF_STATE         (N*18, 2)  pos vel                             kick_env.py:144
 *       RIGID_BODY_STATE  (N*B, 13)                                      kick_env.py:145
 *       NET_CONTACT_FORCE (N*B, 3)                                       kick_env.py:146
 *     bez_kick: A = 2 (robot, ball), B = 22 (21 robot bodies + ball); with the cleats asset (BEZ_FLAG_CLEATS) B = 30;
 *     bez_walk / bez_orient have no ball actor: A = 1, B = 21 (29 with cleats); OBS is (N,54) for bez_kick, (N,52) otherwise.
 *     They are *materialised on demand* by bez_sim_refresh_tensor (gym.refresh_*_tensor);
 *     the simulator's own state is SoA ([field][env], one env per lane).
 */
#ifndef BEZ_SIM_H
#define BEZ_SIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEZ_SIM_ABI_VERSION 5

#define BEZ_NUM_OBS 54       /* bez_kick; bez_walk / bez_orient: 52 (no ball tail)  walk_env.py:104 */
#define BEZ_NUM_OBS_WALK 52
#define BEZ_NUM_ACTIONS 18
#define BEZ_NUM_DOFS 18
#define BEZ_NUM_BODIES 22 /* 21 robot + ball */
#define BEZ_NUM_ACTORS 2

/* flags */
#define BEZ_FLAG_IMU_PREV_ALIAS 1u /* quirk Q1 (kick_env.py:930,441): prev_lin_vel aliases the live \
                                      velocity, so the finite difference is identically 0 */

#define BEZ_FLAG_CF_LAST_SUBSTEP 4u   /* NET_CONTACT_FORCE = last substep only; default: mean over the substeps of the \
                                        control step (physx.contact_collection 2 = CC_ALL_SUBSTEPS, bez_kick.yaml:147) */
#define BEZ_FLAG_NO_SELF_COLLISION 8u /* disable leg<->leg contact (the reference enables self-collision) */
#define BEZ_FLAG_CF_WITH_FRICTION 2u /* NET_CONTACT_FORCE rows include friction; default off: Isaac Gym reports the \
                                        normal contact impulses only [ext] (checkpoint obs statistics) */

#define BEZ_FLAG_CLEATS 16u /* asset.cleats: True -> soccerbot_stl_sensor.urdf: 29 robot bodies, per-cleat contact rows \
                               13:17 / 25:29 and compute_feet_sensors_cleats (kick_env.py:187-191,267-276,1044-1069) */
#define BEZ_FLAG_BOX_ASSET 32u /* asset.stl: False -> soccerbot_box.urdf / soccerbot_box_sensor.urdf (kick_env.py:266-276): the stl \
                                  asset's dynamics with the URDF's own torso / head / forearm collision boxes (upper-body ground \
                                  points, ball <-> torso box); with BEZ_FLAG_CLEATS also that URDF's right ankle joint origin */

#define BEZ_FLAG_HARD_CONTACT 64u /* rigid contact: velocity-level impulses with Coulomb stiction and restitution 0 (projected Gauss-Seidel on \
                                     the articulated-body impulse responses) instead of the implicit spring-dampers; knobs in `tune`. \
                                     ORACLE ONLY (an experiment that did not earn a kernel): bez_sim_create / \
                                     bez_sim_set_flags of libbez_sim.so refuse it with rc -5 */
#define BEZ_FLAG_TGS_SOLVER 512u /* TGS-shaped unified substep: drives, joint friction, joint limits, joint speed limit and every contact \
                                    as clamped impulse rows relaxed together over posIters sub-steps of dt / posIters (+ velIters), the \
                                    solver shape PhysX is configured with (bez_kick.yaml:128-147); knobs in `tune[8..23]`.  ORACLE ONLY \
                                    (DESIGN.md 3.2 / 6.1): libbez_sim.so refuses it with rc -5 */

#define BEZ_FLAG_ANKLE_STOP 1024u /* same-leg calf <-> foot-plate contact.  `create_actor(..., collision_filter 0)` (kick_env.py:365-366) makes \
                                     PhysX collide every non-adjacent pair of the robot's shapes, and one such pair limits the robot's motion \
                                     all the time: the bottom corners of the calf box (soccerbot_stl.urdf:232-236) meet the top face of the \
                                     3 mm foot plate (:272-276) once the flexed ankle also rolls by 0.3-0.45 rad -- well inside the roll \
                                     joint's own +-0.785 rad.  The gap is a function of the two ankle angles alone, so the contact is a \
                                     coupled limit of those two joints: an implicit spring-damper along the gap's gradient.  A scenario-harness \
                                     variant (the reference policy's sim-to-sim does not move with it): stepped by the \
                                     one-env-per-lane kernel, stl asset without cleats only (any other asset: rc -5) */

#define BEZ_FLAG_ALL_GROUND_SHAPES 2048u /* ground contact at the corners of EVERY collision shape of soccerbot_stl.urdf (hip, thigh, calf, ankle, \
                                            forearm, neck, head boxes / mesh bounds), not only the foot corners and the upper-body guard points. \
                                            For the scenario harness (the get-up tables put knees, hips and forearms on the ground, \
                                            soccer_trajectories.py:56-91; nothing on the bez_kick path touches the ground with them before its \
                                            fall reset): stepped by the one-env-per-lane kernel, stl asset without cleats only (else rc -5) */

#define BEZ_FLAG_FIX_BASE 4096u /* urdfAsset.fixBaseLink: True (kick_env.py:287, bez_kick.yaml:83): the torso is welded to the world -- its spatial \
                                   acceleration is zero instead of the 6 x 6 root solve's, its twist stays zero, the pose stays where reset put it; \
                                   joints, contacts and the ball are unchanged.  (The reference's per-DOF sweep, test/test_kick_env.py:142-186, \
                                   notes "better when fixBaseLink = True".)  A test configuration: stepped by the one-env-per-lane kernel \
                                   (3.3 x 10^7 env-steps/s at 4096 envs), not by the 8-role-wave kernel of the default path. */

#define BEZ_FLAG_LEAN_STEP 128u /* bez_sim_step / bez_sim_step_many keep only what the rollout reads (state, obs, reward, reset / progress / \
                                   timeout, DOF targets): the stores of the NET_CONTACT_FORCE rows, FEET and PREV_LIN_VEL -- 308 B of the \
                                   912 B an env-step writes -- are skipped, and those three tensors then hold the values of the last call \
                                   without the flag.  The feet flags inside the observation are unaffected (computed from the in-kernel \
                                   forces).  Needs BEZ_FLAG_IMU_PREV_ALIAS (prev_lin_vel is then never read back). */

#define BEZ_FLAG_OBS_NOISE_IN_STEP 256u /* with a randomisation that has observation noise (bez_sim_set_randomization): the post-physics \
                                          part of bez_sim_step / bez_sim_post_physics writes the NOISY observations itself (the noise \
                                          rides on the kernel's copy-out, bit-identical to what bez_sim_add_dr_noise(OBS, OBS, 0) adds), \
                                          and that call on the observation tensor becomes a no-op: one launch less per control step */

#define BEZ_FLAG_NONFINITE_GUARD 8192u /* per-env non-finite guard (set by bez_sim_default_config; bez_sim_set_flags may clear it).  Every \
                                         launch that contains the post-physics bookkeeping (bez_sim_step, bez_sim_step_many, \
                                         bez_sim_post_physics; not bez_sim_observe_reward) TRIPS an env when, after its physics and any \
                                         pending reset, its root state, ball state, joint positions / velocities or reward hold a NaN or \
                                         an infinity.  A tripped env gets rew = 0, reset_buf = 1, nonfinite_count += 1 and \
                                         BEZ_HEALTH_NONFINITE in the health word; each non-finite stored value is replaced: positions by \
                                         the init pose (bez_init / ball_init), joint positions and targets by the default joint position, \
                                         velocities, prev_lin_vel and contact-force rows by 0.  Non-finite observation entries are written \
                                         as 0.  The next launch steps that finite replacement and then performs the ordinary reset (the \
                                         trip itself does not advance the episode counter).  Other envs, and every run without a \
                                         non-finite value, are bit-identical to a run without the flag.  Detection is class tests, plus \
                                         two sums (the pose error, a chain's joint velocities): a finite value so large \
                                         that one of them overflows trips too. */

#define BEZ_FLAG_REWARD_TERMS 16384u /* env.debug.rewards: every launch with post-physics bookkeeping adds each env's reward, split into its \
                                       terms, to BEZ_EPISODE_REWARD_TERMS (bez_sim_get_episode_tensor).  Not set by \
                                       bez_sim_default_config; bez_sim_set_flags may toggle it.  No other output changes. */

#define BEZ_FLAG_DOF_FORCE 32768u /* gym.enable_actor_dof_force_sensors (kick_env.py:368,375, walk_env.py:300, orient_env.py:302): every launch that \
                                     contains physics (bez_sim_simulate, bez_sim_step, bez_sim_step_many) records each joint's drive torque, net joint \
                                     force and actuator status ("Actuator tensors" below: bez_sim_get_actuator_tensor, \
                                     bez_sim_refresh_actuator_tensors).  Off by default; accepted by bez_sim_create and bez_sim_set_flags (the first \
                                     use allocates the tensors).  Without it the library launches the kernels it always did and allocates nothing; \
                                     with it the step kernels are other instantiations that compute the same state, observations, rewards and \
                                     contact rows bit for bit.  A captured graph keeps the kernels it was captured with: set the flag BEFORE \
                                     capturing.  Not served together with BEZ_FLAG_ANKLE_STOP / BEZ_FLAG_ALL_GROUND_SHAPES (rc -5: the joint forces \
                                     of these two scenario variants have no validation yet). */

/* Why an episode ended: cause code k has bit (1 << k) in BEZ_EPISODE_END_BITS.  A test "fires" exactly where the reward sets
 * reset_buf = 1.
 *   k  name                     bez_kick                          bez_walk                    bez_orient
 *   0  BEZ_END_CARRIED          reset_buf was already 1 when the reward was computed (bez_sim_observe_reward only: every
 *                               launch with bookkeeping performs that reset first)
 *   1  BEZ_END_FALL             torso z < 0.275                   up_proj < 0.7               up_proj < 0.7
 *   2  BEZ_END_OUT_OF_BOUNDS    torso > 0.5 m from its start      never                       torso > 0.3 m from its start
 *   3  BEZ_END_OFF_COURSE       goal-angle difference > 1.5708    heading error > 1.5708      never
 *   4  BEZ_END_GOAL             ball within 0.05 of the goal      state == 4                  state == 4
 *   5  BEZ_END_TIMEOUT          progress >= max_episode_length    same                        same
 *   6  BEZ_END_NONFINITE        the non-finite guard tripped the env (BEZ_FLAG_NONFINITE_GUARD): replaces every other bit
 *   7  (reserved)
 * The DECIDING cause of an ended episode is the last test that fired in the reference's order -- the one whose reward stands:
 *   bez_kick   fall, out of bounds, goal angle, goal, timeout
 *   bez_walk   fall, goal, heading, timeout
 *   bez_orient fall, goal, drift, timeout
 * CARRIED decides only when no test fired; NONFINITE always decides. */
#define BEZ_END_CARRIED 0
#define BEZ_END_FALL 1
#define BEZ_END_OUT_OF_BOUNDS 2
#define BEZ_END_OFF_COURSE 3
#define BEZ_END_GOAL 4
#define BEZ_END_TIMEOUT 5
#define BEZ_END_NONFINITE 6
#define BEZ_END_CAUSES 8

/* Slots of BEZ_EPISODE_REWARD_TERMS.  On a step where no test fired the slots sum to rew; on a step where one fired, slot 5 holds
 * the reward the deciding test assigned and every other slot is 0.  Over any run, the sum of all slots is the sum of rew.
 *   slot  bez_kick (kick_env.py:1224-1391)      bez_walk (walk_env.py:826-1031)        bez_orient (orient_env.py:843-1018)
 *   0     0.1 ball_fwd                          0                                      -0.5 |ang_goal|        (ang_goal >= 0.05)
 *   1     0.05 vel_fwd    (before the kick)     10 vel_fwd       (goal dist >= 0.05)   0
 *   2     -|0.325 - z|                          -|1 - up_proj|                         -|1 - up_proj|
 *   3     -0.05 |(v,w)|   (after the kick)      -0.05 |(v,w)|    (goal dist < 0.05)    -0.05 |(v,w)|          (ang_goal < 0.05)
 *   4     -0.05 |q - q0|  (after the kick)      -0.25 |q - q0| far, -0.05 |q - q0| near  -0.0025 |q - q0| far, -0.05 |q - q0| near
 *   5     terminal reward                       terminal reward                        terminal reward
 *   6, 7  0                                     0                                      0
 * ("after the kick": the ball is more than 0.3 m from its start; |q - q0|: the joints' distance from their default position) */

/* Bits of the health word (BEZ_TENSOR_HEALTH, bez_sim_health): set on the device, cleared only by the caller. */
#define BEZ_HEALTH_NONFINITE 1u    /* an env tripped the non-finite guard since the word was last cleared */
#define BEZ_HEALTH_SPIN_TIMEOUT 2u /* an LDS hand-over wait of the 8-role-wave kernel gave up after its bound (the step went on with \
                                      stale words: its results are suspect).  Set whether or not BEZ_FLAG_NONFINITE_GUARD is. */

/* Tasks sharing the robot, the physics and the tensor API; they differ in the post-physics logic (observation tail,
 * reward, reset conditions, goal sampling) and in the ball actor (bez_kick only). */
#define BEZ_TASK_KICK 0   /* tasks/kick_env.py    54 obs, ball + goal point                              */
#define BEZ_TASK_WALK 1   /* tasks/walk_env.py    52 obs, no ball, goal xy ~ U(-2,2)^2 redrawn at reset  */
#define BEZ_TASK_ORIENT 2 /* tasks/orient_env.py  52 obs, no ball, goal heading                          */

typedef struct BezSimConfig {
  int32_t abi_version; /* must be BEZ_SIM_ABI_VERSION */
  int32_t num_envs;    /* cfg["env"]["numEnvs"]                         vec_task.py:84 */
  int32_t substeps;    /* cfg["sim"]["substeps"]                        vec_task.py:430 */
  int32_t max_episode_length; /* int(episodeLength_s/dt+0.5)            kick_env.py:127 */
  float dt;            /* cfg["sim"]["dt"]                              vec_task.py:427 */
  float gravity[3];    /* cfg["sim"]["gravity"]                         vec_task.py:439 */
  float kp, kd;        /* control.stiffness / damping                   kick_env.py:324-325 */
  float armature;      /* urdfAsset.armature                            kick_env.py:326 */
  float effort;        /* 2.5 N*m all DOFs                              kick_env.py:329 */
  float vel_limit;     /* 2*pi rad/s                                    kick_env.py:327 */
  float joint_friction;/* 0.1                                           kick_env.py:328 */
  float plane_friction;/* plane.dynamicFriction                         kick_env.py:254 */
  float clip_actions;  /* env.clipActions                               vec_task.py:98,317 */
  float bez_init[7];   /* bezInitState pos + rot(xyzw)                  kick_env.py:60-64 */
  float ball_init[7];  /* ballInitState pos + rot                       kick_env.py:67-71 */
  float goal[2];       /* goalState.goal                                kick_env.py:74,159 */
  /* Contact / limit model of this build (PhysX's TGS contact solve has no source here; see
   * DESIGN.md "Physics model").  All forces are spring-dampers integrated implicitly. */
  float contact_kn;    /* normal stiffness per contact point  [N/m]   */
  float contact_cn;    /* normal damping                      [N*s/m] */
  float contact_ct;    /* max tangential (stick) viscosity    [N*s/m] */
  float contact_veps;  /* Coulomb regularisation speed        [m/s]   */
  float limit_k;       /* joint-limit spring                  [N*m/rad]   */
  float limit_d;       /* joint-limit damper                  [N*m*s/rad] */
  float jfric_veps;    /* joint-friction regularisation speed [rad/s] */
  float ball_ang_damping; /* Isaac asset default angular_damping 0.5 [ext] for the ball actor */
  float self_kn;       /* leg<->leg self-collision (kick_env.py:365-366, filter 0): spring [N/m]   */
  float self_cn;       /*                                                     damper [N*s/m] */
  float ball_kn;       /* ball <-> ground / ball <-> robot contact spring [N/m]; 0 = contact_kn */
  float ball_cn;       /* and damper [N*s/m]; 0 = contact_cn.  PhysX restitution is 0 (bez_kick.yaml:16): critical damping of the 0.3 kg
                          ball against contact_kn is 2 sqrt(kn m) = 155 N*s/m */
  float tune[24];      /* knobs of the oracle-only solver variants (BEZ_FLAG_HARD_CONTACT: [0..7], BEZ_FLAG_TGS_SOLVER: [8..23];
                          oracle/bez_oracle.c documents the slots); 0 = default.  libbez_sim.so refuses a non-zero entry (rc -5) */
  int32_t task;        /* BEZ_TASK_*: which env logic POST runs (tasks/__init__.py:10-16)                */
  float goal_angle;    /* bez_orient: env.goalState.goal_angle                       orient_env.py:61 */
  uint32_t flags;      /* BEZ_FLAG_* */
  uint64_t seed;       /* reset-noise stream key (config.yaml:11 seed: 42) */
  int64_t env_id_offset; /* global id of local env 0; reset noise is keyed by GLOBAL env id so
                            results do not depend on how envs are sharded over GPUs */
} BezSimConfig;

/* Fills `cfg` with the bez_kick.yaml / kick_env.py defaults for `num_envs` environments. */
int bez_sim_default_config(BezSimConfig* cfg, int32_t num_envs);

typedef struct BezSim BezSim;

enum BezTensor {
  BEZ_TENSOR_ROOT_STATE = 0,        /* f32 (N*2,13)   acquire_actor_root_state_tensor   kick_env.py:143 */
  BEZ_TENSOR_DOF_STATE = 1,         /* f32 (N*18,2)   acquire_dof_state_tensor          kick_env.py:144 */
  BEZ_TENSOR_RIGID_BODY_STATE = 2,  /* f32 (N*22,13)  acquire_rigid_body_state_tensor   kick_env.py:145 */
  BEZ_TENSOR_NET_CONTACT_FORCE = 3, /* f32 (N*22,3)   acquire_net_contact_force_tensor  kick_env.py:146 */
  BEZ_TENSOR_OBS = 4,               /* f32 (N,54)     obs_buf       vec_task.py:235 */
  BEZ_TENSOR_REW = 5,               /* f32 (N)        rew_buf       vec_task.py:239 */
  BEZ_TENSOR_RESET = 6,             /* i64 (N)        reset_buf     vec_task.py:241 (init 1) */
  BEZ_TENSOR_PROGRESS = 7,          /* i64 (N)        progress_buf  vec_task.py:245 */
  BEZ_TENSOR_TIMEOUT = 8,           /* i64 (N)        timeout_buf   vec_task.py:243 */
  BEZ_TENSOR_DOF_TARGET = 9,        /* f32 (N,18)     PD position targets */
  BEZ_TENSOR_PREV_LIN_VEL = 10,     /* f32 (N,3)      prev_lin_vel  kick_env.py:183 */
  BEZ_TENSOR_FEET = 11,             /* f32 (N,8)      self.feet     kick_env.py:185 */
  BEZ_TENSOR_GOAL = 12,             /* f32 (N,2)      self.goal     walk_env.py:143 (bez_walk / bez_orient: redrawn at reset) */
  BEZ_TENSOR_RANDOMIZE_BUF = 13,    /* i64 (N)        randomize_buf vec_task.py:247 (device-side domain randomisation) */
  BEZ_TENSOR_DR_NOISE = 14,         /* f32 (4)        mean / std of the observation noise, mean / std of the action noise as the schedule
                                                      currently has them (vec_task.py:544-618): the caller's noise lambdas read them on the device */
  BEZ_TENSOR_NONFINITE_COUNT = 15, /* i64 (N)       trips of the non-finite guard per env: 0 at create, never cleared by the library
                                                      (the view is writable: the caller may zero it) */
  BEZ_TENSOR_HEALTH = 16,           /* i64 (1)        health word: BEZ_HEALTH_* bits (read outside the hot loop: bez_sim_health) */
  BEZ_TENSOR_COUNT = 17
};
enum BezDtype { BEZ_DTYPE_F32 = 0, BEZ_DTYPE_I64 = 1, BEZ_DTYPE_I32 = 2 };

/* Episode statistics (bez_sim_get_episode_tensor): zeroed at create, always live (no bez_sim_refresh_tensor), writable views. */
enum BezEpisodeTensor {
  BEZ_EPISODE_END_BITS = 0,     /* i32 (N)    this launch's BEZ_END_* bits per env: nonzero exactly where reset_buf == 1.  Written by
                                                every launch with post-physics bookkeeping and by bez_sim_observe_reward */
  BEZ_EPISODE_END_COUNTS = 1,   /* i64 (8,N)  [cause][env]: ended episodes per deciding cause, one per ended episode in launches with
                                                bookkeeping (not bez_sim_observe_reward).  Never cleared by the library: take deltas */
  BEZ_EPISODE_REWARD_TERMS = 2, /* f32 (8,N)  [slot][env]: sums of the reward's terms (BEZ_FLAG_REWARD_TERMS; slot table above) since
                                                the caller last zeroed it, in launches with bookkeeping */
  BEZ_EPISODE_TENSORS = 3
};

/* Actuator tensors (BEZ_FLAG_DOF_FORCE; bez_sim_get_actuator_tensor), all in DOF_STATE order (env-major, 18 DOFs per env).
 * Per DOF d and substep, with h the substep, (q, qd) the joint state at its start, qdd the acceleration the substep solves,
 * qd+ = qd + h qdd and q+ = q + h qd+ (the state the substep leaves):
 *   drive torque  tau_drive = +-effort where the substep's saturation predictor clamped the drive, else the PD law at the end-of-substep
 *                 state, kp_d (target - q+) - kd_d qd+ (kp_d, kd_d include the env's BEZ_PARAM_KP_SCALE / BEZ_PARAM_KD_SCALE); on a joint locked
 *                 on its speed limit the same, with the prescribed qdd.
 *   net joint force  tau_net = everything the joint mechanism applies about its axis.  Unlocked joint: tau_drive - cf qd+ + tau_limit(q+, qd+),
 *                 cf = joint_friction / max(|qd|, jfric_veps) the regularised friction coefficient of the substep, tau_limit the joint-limit
 *                 spring-damper limit_k (bound - q+) - limit_d qd+ where q was beyond the bound at the start of the substep (with
 *                 BEZ_FLAG_ANKLE_STOP also the calf <-> foot-plate contact's share on the two ankle joints).  Locked joint: the reaction of the
 *                 constraint, the force that produces the prescribed qdd: S.pA + U.(a_parent + c) + (J + armature) qdd in the quantities of
 *                 the articulated-body recursion.  In both cases tau_net - armature qdd is what an inverse dynamics (RNEA) of the rigid links
 *                 finds at the joint; ground, ball, leg <-> leg contacts and external wrenches are link forces, not joint forces.
 *                 The head DOFs (never driven: their actions are zeroed) report what the same formulas give.
 *   status        bit 0 / 1: a substep saturated the drive at +effort / -effort; bit 2 / 3: a substep locked the joint on +vel_limit / -vel_limit.
 * A launch reports the MEAN over its substeps of tau_drive and tau_net (as NET_CONTACT_FORCE is the mean over the substeps) and the OR of
 * the status bits; bez_sim_step_many leaves its last step's values.  The values describe the physics that ran in the launch whether or not the
 * env was reset behind it: an env whose progress_buf is 0 after bez_sim_step was reset, and its row describes the discarded step.  A
 * non-finite entry is written as 0 (the state's own non-finite values are the non-finite guard's business). */
enum BezActuatorTensor {
  BEZ_ACTUATOR_DOF_FORCE = 0,    /* f32 (N*18)  tau_net: gym.acquire_dof_force_tensor */
  BEZ_ACTUATOR_DRIVE_TORQUE = 1, /* f32 (N*18)  tau_drive */
  BEZ_ACTUATOR_STATUS = 2,       /* i32 (N*18)  BEZ_ACTUATOR_* status bits */
  BEZ_ACTUATOR_TENSORS = 3
};
#define BEZ_ACTUATOR_SATURATED_POS 1
#define BEZ_ACTUATOR_SATURATED_NEG 2
#define BEZ_ACTUATOR_LOCKED_POS 4
#define BEZ_ACTUATOR_LOCKED_NEG 8

/* gym.create_sim + create_env/create_actor loop + prepare_sim + allocate_buffers
 * (vec_task.py:174-193, kick_env.py:240-408) followed by KickEnv.__init__'s reset_idx(all)
 * (kick_env.py:238): every env starts from its first reset draw with reset_buf = 0. */
int bez_sim_create(const BezSimConfig* cfg, int device_id, BezSim** out);
int bez_sim_destroy(BezSim* sim);
const char* bez_sim_last_error(const BezSim* sim); /* sim may be NULL: last create error */

/* gymtorch.wrap_tensor(gym.acquire_*_tensor(sim)): device pointer + shape of a sim-owned
 * buffer.  shape has `*ndim` valid entries. */
int bez_sim_get_tensor(BezSim* sim, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype);
/* The same for the episode statistics: `which` is a BezEpisodeTensor. */
int bez_sim_get_episode_tensor(BezSim* sim, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype);

/* The actuator tensors: `which` is a BezActuatorTensor.  Without BEZ_FLAG_DOF_FORCE: an error (rc -1) with a message, not zeros. */
int bez_sim_get_actuator_tensor(BezSim* sim, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype);
/* gym.refresh_dof_force_tensor: materialises the three actuator tensors from what the last physics launch recorded (one small kernel
 * on `stream`; captures into a HIP graph).  Without BEZ_FLAG_DOF_FORCE: rc -1 with a message. */
int bez_sim_refresh_actuator_tensors(BezSim* sim, void* stream);

/* Dynamics tensors: gym.acquire_jacobian_tensor / gym.refresh_jacobian_tensors and gym.acquire_mass_matrix_tensor /
 * gym.refresh_mass_matrix_tensors for the robot actor -- what operational-space and whole-body controllers read.
 *   Generalised velocity  u = [root_lin(3), root_ang(3), qd(18)]: columns 7:13 of the robot's ROOT_STATE row, then the DOF velocities in
 *     DOF_STATE order; world (env) axes.  24 = 6 + BEZ_NUM_DOFS entries.
 *   BEZ_DYNAMICS_JACOBIAN  f32 (N*NB, 6, 24), env-major; NB = 21 robot bodies (29 with cleats) in RIGID_BODY_STATE order.  There is no
 *     ball row: Isaac's Jacobian is per actor.  Rows 0:3 are the linear velocity of the body's ORIGIN, rows 3:6 its angular velocity,
 *     world axes, so that J[e,b] @ u[e] == RIGID_BODY_STATE[e,b,7:13].  Column 6+d is non-zero only where link d+1 is the body's link or
 *     an ancestor of it; there it is [a x (x_b - r_l); a] with a the joint axis in world axes, r_l the joint origin and x_b the body
 *     origin.  Base block: J[0:3,0:3] = I, J[3:6,3:6] = I, J[3:6,0:3] = 0, J[0:3,3:6] = -skew(x_b - root_pos).  Fixed bodies (imu_link,
 *     camera, the cleats) use their link's columns with their own origin; the joint origin that soccerbot_box_sensor.urdf moves
 *     (BEZ_FLAG_BOX_ASSET with BEZ_FLAG_CLEATS) is where the step kernels have it.  The ones and the structural zeros are exact.
 *   BEZ_DYNAMICS_MASS_MATRIX  f32 (N, 24, 24): the matrix of the kinetic energy in u,
 *       M = sum over links of J_com^T diag(m I3, I_c in world axes) J_com + armature * diag(0 x 6, 1 x 18),
 *     so that 1/2 u^T M u = KE + 1/2 armature |qd|^2 (the armature is included because the step's joint-space inertia includes it).
 *     Link masses and inertias carry the env's BEZ_PARAM_MASS_SCALE row (m and I_c alike, as in the step).  Both triangles are written
 *     from one computed value: M is bitwise symmetric; M[0:3,0:3] is the total mass times I with exact zeros off the diagonal.
 *   BEZ_FLAG_FIX_BASE changes no shape (bez_sim_set_flags may flip it while views exist): the fixed-base quantities are the sub-blocks
 *     J[..., 6:] and M[6:, 6:].  This is the one deliberate deviation from Isaac Gym, whose fixed-base tensors drop the six base columns.
 *   A non-finite state is written through as it is (the structural zeros and ones stay). */
enum BezDynamicsTensor { BEZ_DYNAMICS_JACOBIAN = 0, BEZ_DYNAMICS_MASS_MATRIX = 1, BEZ_DYNAMICS_COUNT = 2 };
/* gym.acquire_jacobian_tensor / gym.acquire_mass_matrix_tensor: `which` is a BezDynamicsTensor; *ndim is 3.  The FIRST call for a tensor
 * allocates it (12 KB per env for the Jacobian, 2.3 KB for the mass matrix: a sim that never asks allocates nothing), zero-filled;
 * bez_sim_destroy frees it.  Later calls return the same memory. */
int bez_sim_get_dynamics_tensor(BezSim* sim, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype);
/* gym.refresh_jacobian_tensors / gym.refresh_mass_matrix_tensors: ONE kernel launch on `stream` fills the tensors named in which_mask
 * (bit (1u << which)) from the state as it stands on the stream.  A tensor that was never acquired, a zero mask or an unknown bit:
 * rc -1 with a message.  The call allocates nothing, never synchronises, reads nothing on the host: it captures into a HIP graph. */
int bez_sim_refresh_dynamics_tensors(BezSim* sim, uint32_t which_mask, void* stream);

/* Inverse dynamics: the left side of the robot's equation of motion
 *       M(q) udot + h(q, u) = [0 x 6 ; tau_joint] + sum over bodies of J_b^T w_b
 * by a recursive Newton-Euler pass, without forming M -- what gravity compensation, computed torque and contact-wrench estimation need.
 *   Coordinates: u = [root_lin(3), root_ang(3), qd(18)] of the dynamics tensors above; udot_dev and out_dev are f32 (N, 24), env-major.
 *     udot is the time derivative of u: [d/dt root_lin, d/dt root_ang, qdd].  udot_dev == NULL means udot = 0.
 *   out = the sum of the terms selected in `terms`, evaluated on the state as it stands on `stream`:
 *     BEZ_ID_INERTIA   M(q) udot, the armature on the 18 joint diagonals as in BEZ_DYNAMICS_MASS_MATRIX;
 *     BEZ_ID_VELOCITY  the Coriolis and centrifugal forces of the state's u;
 *     BEZ_ID_GRAVITY   -sum over links of J_com^T m g: the generalised force that holds the robot still against gravity.
 *     All three: M udot + h.  A term is dropped by zeroing its input, and the terms are evaluated apart and meet only in the last two
 *     additions of each element: a term's value does not depend on which other terms were asked for, all terms together are the fp32
 *     sum (inertia + velocity) + gravity of the three single-term results, and the velocity term of a state at rest, the gravity term
 *     under zero gravity and the inertia term of udot = 0 are exact zeros.
 *   Rows of out: 0:3 the force in world axes, 3:6 the moment about the root origin in world axes (dual to u: u . out is a power),
 *     6:24 the joint torques in DOF_STATE order.
 *   Gravity is what the step would use: the env's BEZ_PARAM_GRAVITY row if set, else cfg.gravity.  Masses and inertias carry the env's
 *     BEZ_PARAM_MASS_SCALE row.  The asset (cleats, box, the joint origin box + cleats moves) is the step's.  The ball takes no part.
 *   BEZ_FLAG_FIX_BASE changes nothing: the stored state is evaluated as it is, and rows 0:6 are then the wrench the weld carries.
 *   A non-finite input is written through.
 *   One kernel launch.  The call allocates nothing, never synchronises, reads nothing on the host and writes only out_dev: it captures
 *   into a HIP graph.  terms == 0, an unknown bit or a null out_dev: rc -1 with a message. */
#define BEZ_ID_INERTIA  1u   /* M(q) udot, armature included as in BEZ_DYNAMICS_MASS_MATRIX */
#define BEZ_ID_VELOCITY 2u   /* Coriolis / centrifugal forces of the state's u */
#define BEZ_ID_GRAVITY  4u   /* -sum_l J_com,l^T m_l g: what holds the robot still against gravity */
#define BEZ_ID_ALL      7u
int bez_sim_inverse_dynamics(BezSim* sim, const float* udot_dev, uint32_t terms, float* out_dev, void* stream);

/* Forward dynamics: the accelerations that a generalised force produces,
 *       udot = M(q)^-1 (f - h(q, u)),
 * the inverse of the call above -- the free acceleration of a state, the response to a candidate joint torque, a push or a contact
 * wrench, M^-1 J^T for operational-space control, a model-based predictor.  (The Isaac Gym route: the mass-matrix tensor and
 * torch.linalg.solve.)  M is never formed: the tree is a torso and five chains, so M is a block arrow, and the solve is five Cholesky
 * factorisations of at most 6 x 6 and one of the 6 x 6 Schur complement on the base.
 *   Coordinates, rows and state are those of bez_sim_inverse_dynamics: u = [root_lin(3), root_ang(3), qd(18)]; force_dev is a generalised
 *     force, f32 (N, 24), env-major, rows [force, world axes; moment about the root origin, world axes; joint torques] -- what
 *     bez_sim_generalized_forces returns; out_dev is udot, f32 (N, 24).  The state is read as it stands on `stream`.
 *     force_dev == NULL means f = 0.
 *   bias: a subset of BEZ_ID_VELOCITY | BEZ_ID_GRAVITY, the terms of h that are taken off f.  bias == 0 with a force tensor is the plain
 *     mass solve M^-1 f.
 *   M is the matrix of BEZ_DYNAMICS_MASS_MATRIX: the armature on the 18 joint diagonals, the env's BEZ_PARAM_MASS_SCALE row, the asset's
 *     model (cleats, box, the joint origin box + cleats moves).  Gravity is the env's BEZ_PARAM_GRAVITY row if set, else cfg.gravity.
 *     The ball takes no part.
 *   bez_sim_inverse_dynamics(out, BEZ_ID_INERTIA | bias) gives f back.
 *   mode == 0: the floating base, all 24 rows are solved.  BEZ_FLAG_FIX_BASE changes nothing, as in every sibling call.
 *   mode == BEZ_FD_FIXED_BASE: the root is held.  Rows 0:6 of out are +0.0f to the bit, rows 6:24 solve M[6:,6:] qdd = (f - h)[6:], and
 *     rows 0:6 of force_dev take no part.  The five chains are then independent problems: with bias == 0 a chain whose 2 or 6 force rows
 *     are all zero returns +0.0f to the bit, and a chain's result does not depend on the other chains' rows.
 *   A non-finite input is written through for its own env and changes no bit of any other env.  An env's bits depend neither on N nor
 *     on where the env stands.
 *   One kernel launch.  The call allocates nothing, never synchronises, reads nothing on the host and writes only out_dev, which may
 *   alias force_dev: it captures into a HIP graph.  A pointer that is only 4-byte aligned gives the same bits.
 *   BEZ_ID_INERTIA or an unknown bit in bias, bias == 0 together with force_dev == NULL (nothing to solve for), an unknown mode bit or a
 *   null out_dev: rc -1 with a message, and nothing is written. */
#define BEZ_FD_FIXED_BASE 1u   /* hold the root: udot[0:6] = 0, solve the joint block alone */
int bez_sim_forward_dynamics(BezSim* sim, const float* force_dev, uint32_t bias, uint32_t mode, float* out_dev, void* stream);

/* Operational space: the quantities of operational-space control for the five frames that bez_sim_limb_ik controls (head, two hands, two
 * feet), in one launch on the factorisation of the call above:
 *       J_c,   J_c M^-1,   W = J_E M^-1 J_E^T (the Delassus matrix, J_E the five J_c stacked),   Lambda_c = W_cc^-1.
 * (The Isaac Gym route: both dynamics tensors, slicing and shifting rows by hand, torch.linalg.solve on N dense 24 x 24 systems, two bmm.)
 *   Chains, end bodies and params->offset[c] are those of bez_sim_limb_ik: the controlled frame of chain c is the chain's end body
 *     displaced by offset[c] in that body's axes.
 *   Coordinates are those of the dynamics tensors: u = [root_lin(3), root_ang(3), qd(18)]; rows 0:3 of a frame are the linear velocity of
 *     the controlled point, rows 3:6 its angular velocity, world axes.  M is the matrix of BEZ_DYNAMICS_MASS_MATRIX (armature, the env's
 *     BEZ_PARAM_MASS_SCALE row, the asset's model, the joint origin box + cleats moves).  The state is read as it stands on `stream`.  The
 *     ball takes no part.  BEZ_FLAG_FIX_BASE changes nothing, as in every sibling call.
 *   Outputs, f32, env-major, each may be NULL (not written); all four NULL is an error:
 *     jac_dev    (N, 5, 6, 24)  J_c of the controlled frame; with offset 0 the rows of the end body in BEZ_DYNAMICS_JACOBIAN.  The base block
 *                is exact as there (I, I, 0, -skew(x - root_pos)); the columns of the other four chains are +0.0f.  The mode does not
 *                change it.
 *     jminv_dev  (N, 5, 6, 24)  J_c M^-1: jminv[c] @ f is the frame's acceleration response to a generalised force f, and
 *                Lambda_c @ jminv[c] is the transpose of the dynamically consistent inverse.
 *     w_dev      (N, 30, 30)    W, block (a, b) 6 x 6 in chain order; both triangles are written from one computed value (bitwise symmetric).
 *                W is singular by structure (rank <= 24): the call never returns its full inverse.
 *     lambda_dev (N, 5, 6, 6)   W_cc^-1 by a 6 x 6 Cholesky factorisation, bitwise symmetric.
 *   mode == BEZ_FD_FIXED_BASE holds the root, M becomes M[6:,6:]: jminv[..., 0:6] and the other chains' columns are +0.0f, the off-diagonal
 *     blocks of w are +0.0f, W_cc = J_cc M_cc^-1 J_cc^T.  Those blocks are singular by structure (rank 2 for the head and the arms, a
 *     straight knee for a leg): a non-NULL lambda_dev in this mode is an error.
 *   To the bit: block (a, b) of w and chain c's jac, jminv and lambda do not depend on any other chain's offset; an env's bits depend
 *     neither on N, nor on its place, nor on the buffers' alignment (4-byte-aligned pointers give the same bits); which outputs are asked
 *     for does not change the others; a non-finite state is written through for its own env and changes no bit of any other env.
 *   One kernel launch with params in its arguments.  The call allocates nothing, never synchronises, reads nothing on the host and writes
 *   only the given outputs: it captures into a HIP graph.  rc -1 with a message, and nothing written: a null sim or params, all outputs
 *   NULL, an unknown mode bit, a non-finite offset, lambda_dev with BEZ_FD_FIXED_BASE. */
#ifndef BEZ_IK_CHAINS
#define BEZ_IK_CHAINS 5
#endif
typedef struct BezOpSpaceParams {
  float offset[BEZ_IK_CHAINS][3];   /* controlled frame = the chain's end body displaced by this, in that body's axes */
  uint32_t mode;                    /* 0, or BEZ_FD_FIXED_BASE */
} BezOpSpaceParams;
int bez_sim_operational_space(BezSim* sim, const BezOpSpaceParams* params,
                              float* jac_dev    /* (N,5,6,24) or NULL */,
                              float* jminv_dev  /* (N,5,6,24) or NULL */,
                              float* w_dev      /* (N,30,30)  or NULL */,
                              float* lambda_dev /* (N,5,6,6)  or NULL */, void* stream);

/* Centroidal dynamics: the robot's centre of mass, its momentum about it, the map from u to that momentum, and the mechanical energy --
 * what balance controllers, capture-point and angular-momentum rewards and energy diagnostics read.
 *   Coordinates: u = [root_lin(3), root_ang(3), qd(18)] of the dynamics tensors above; world (env) axes throughout.
 *   state_dev  f32 (N, BEZ_CM_WORDS), env-major, the words named below.  COM is in the coordinates of the ROOT_STATE positions; ANG_MOM is
 *     taken ABOUT THE CENTRE OF MASS; COM_VEL is LIN_MOM / MASS; KINETIC is 1/2 u^T M u with M of BEZ_DYNAMICS_MASS_MATRIX (the armature
 *     on the 18 joint diagonals included, as there); POTENTIAL is -MASS * g . COM (zero at the origin of the env's coordinates).
 *   matrix_dev f32 (N, 6, 24): the centroidal momentum matrix A_G, so that matrix[e] @ u[e] == [LIN_MOM; ANG_MOM]: rows 0:3 the linear
 *     momentum, rows 3:6 the angular momentum about the centre of mass.  matrix[0:3,0:3] = MASS * I with exact zeros off the diagonal;
 *     matrix[3:6,0:3] = 0 exactly (the momentum about the centre of mass does not see the root's translation); matrix[3:6,3:6] is the
 *     centroidal composite inertia, bitwise symmetric; matrix[0:3,3:6] = -MASS * skew(COM - root_pos); column 6+d is [F_lin;
 *     F_ang - (COM - root_pos) x F_lin] with F = I^c_(d+1) S_(d+1) the composite inertia below joint d times the joint's axis.
 *   Gravity is what the step would use: the env's BEZ_PARAM_GRAVITY row if set, else cfg.gravity.  Masses and inertias carry the env's
 *     BEZ_PARAM_MASS_SCALE row.  Fixed bodies (imu, camera, cleats) are in their links; the asset (cleats, box, the joint origin
 *     box + cleats moves) is the step's.  The ball takes no part.  BEZ_FLAG_FIX_BASE changes nothing: the stored state is evaluated as
 *     it is.  A non-finite state is written through (the structural zeros stay).
 *   Zeros are +0.0f to the bit: the structural zeros of the matrix, word 15, COM_VEL / LIN_MOM / ANG_MOM / KINETIC of a state with u = 0 and
 *     POTENTIAL under a zero gravity row.
 *   Either pointer may be NULL: that output is not written.  Both NULL, or a NULL sim: rc -1 with a message.
 *   One kernel launch.  The call allocates nothing, never synchronises, reads nothing on the host and writes only the two outputs: it
 *   captures into a HIP graph. */
#define BEZ_CM_WORDS     16  /* floats per env of state_dev */
#define BEZ_CM_COM        0  /* 0:3   centre of mass, env (world) coordinates, as ROOT_STATE positions */
#define BEZ_CM_COM_VEL    3  /* 3:6   its velocity = LIN_MOM / MASS */
#define BEZ_CM_LIN_MOM    6  /* 6:9   sum_l m_l v_com,l, world axes */
#define BEZ_CM_ANG_MOM    9  /* 9:12  angular momentum ABOUT THE CENTRE OF MASS, world axes */
#define BEZ_CM_MASS      12  /* total mass (the env's BEZ_PARAM_MASS_SCALE row applied) */
#define BEZ_CM_KINETIC   13  /* 1/2 u^T M u with M of BEZ_DYNAMICS_MASS_MATRIX (armature included, as there) */
#define BEZ_CM_POTENTIAL 14  /* -MASS * g . COM, g = the env's BEZ_PARAM_GRAVITY row if set, else cfg.gravity */
                             /* word 15: 0.0f */
int bez_sim_centroidal(BezSim* sim, float* state_dev /* (N,16) or NULL */,
                       float* matrix_dev /* (N,6,24) or NULL */, void* stream);

/* Body accelerations: J_b udot + Jdot_b u of every rigid body of the robot, without forming J or differencing it -- the term of
 *       xddot_b = J_b udot + Jdot_b u,     tau = J^T Lambda (xddot_des - Jdot u) + h
 * that the Jacobian, the mass matrix and inverse dynamics leave open, and, with gravity taken off in the body's frame, what an
 * accelerometer on a body reads.
 *   Coordinates: u = [root_lin(3), root_ang(3), qd(18)] of the dynamics tensors above; udot_dev is f32 (N, 24), env-major, the time
 *     derivative of u as in inverse dynamics; udot_dev == NULL means udot = 0.
 *   out_dev  f32 (N, NB, 6), env-major; NB = 21 robot bodies (29 with cleats) in RIGID_BODY_STATE order, no ball row (as the Jacobian).
 *     With BEZ_SPACE_ENV rows 0:3 are the time derivative of RIGID_BODY_STATE[e,b,7:10] -- the classical acceleration of the body's
 *     ORIGIN in world axes, not the linear part of a spatial acceleration -- and rows 3:6 the derivative of [e,b,10:13].  With the link's
 *     velocity [w; v_O] and spatial acceleration [alpha; a_O] about the root origin (the torso's: [wdot; vdot - w x v]) and x the body's
 *     origin relative to the root origin, rows 0:3 are a_O + alpha x x + w x (v_O + w x x) and rows 3:6 are alpha.  Fixed bodies
 *     (imu_link, camera, the cleats) use their link's motion with their own origin; the asset (cleats, box, the joint origin box + cleats
 *     moves) is the step's.  Masses play no part, and neither do root_pos and root_lin: a uniform translation changes no acceleration.
 *   out = the sum of the terms selected in `terms`, evaluated on the state as it stands on `stream`:
 *     BEZ_ACC_UDOT      J[e,b] @ udot[e];
 *     BEZ_ACC_VELOCITY  Jdot[e,b] @ u[e], the bias acceleration of the state's u; with UDOT (BEZ_ACC_MOTION) it is d/dt (J[e,b] @ u[e]);
 *     BEZ_ACC_GRAVITY   -g on rows 0:3, zero on rows 3:6: all three (BEZ_ACC_ALL) are the specific force at the body's origin.
 *     A term is dropped by zeroing its input, and the terms are evaluated apart and meet only in the last additions of each element:
 *     in BEZ_SPACE_ENV, MOTION is the fp32 sum of the two single-term results and ALL is (udot + velocity) + gravity, bit for bit.
 *     +0.0f to the bit: the UDOT term of udot_dev == NULL, the VELOCITY term of a state with u = 0, rows 3:6 of the GRAVITY term, the
 *     GRAVITY term under a zero gravity row; its rows 0:3 are 0 - g exactly.  Body 0 (the torso, whose origin is the root's) in
 *     BEZ_SPACE_ENV: the UDOT term is udot[0:6] to the bit, the VELOCITY term zeros.
 *   Gravity is what the step would use: the env's BEZ_PARAM_GRAVITY row if set, else cfg.gravity.
 *   space: BEZ_SPACE_ENV -- world axes; BEZ_SPACE_LOCAL -- both row triples in the body's own frame: the transpose of the orientation
 *     RIGID_BODY_STATE reports for the body is applied after the terms are summed.
 *   BEZ_FLAG_FIX_BASE changes nothing: the stored state is evaluated as it is.  A non-finite input is written through.
 *   One kernel launch.  The call allocates nothing, never synchronises, reads nothing on the host and writes only out_dev: it captures
 *   into a HIP graph.  terms == 0, an unknown bit, an unknown space, a null out_dev or a null sim: rc -1 with a message. */
#define BEZ_ACC_UDOT     1u  /* J_b udot */
#define BEZ_ACC_VELOCITY 2u  /* Jdot_b u: the bias acceleration of the state's u */
#define BEZ_ACC_GRAVITY  4u  /* -g on rows 0:3: with the other two, the specific force an accelerometer at the body's origin reads */
#define BEZ_ACC_MOTION   3u
#define BEZ_ACC_ALL      7u
int bez_sim_body_accelerations(BezSim* sim, const float* udot_dev /* (N,24) or NULL */, uint32_t terms,
                               int32_t space /* BEZ_SPACE_ENV | BEZ_SPACE_LOCAL */, float* out_dev /* (N, NB, 6) */, void* stream);

/* Generalised forces: sum over bodies of J_b^T w_b -- the last term of the equation of motion above, the map from wrenches on rigid
 * bodies to generalised forces -- without forming J: operational-space control (tau = J^T F + h), virtual-model control on a foot or
 * hand, contact-wrench estimation, and the generalised force a bez_sim_apply_body_forces call exerts.
 *   forces_dev, torques_dev, positions_dev: exactly the tensors bez_sim_apply_body_forces takes -- f32 (N*B, 3) in RIGID_BODY_STATE order,
 *     B with the ball's row where the task has a ball (22 / 21, with cleats 30 / 29) -- so the same buffers can be handed to both calls.
 *     Any of the three may be NULL (zero forces / zero torques / the default point of application).  The ball is not part of u: its row
 *     is never read, and a NaN there changes nothing.
 *   space: BEZ_SPACE_ENV / BEZ_SPACE_LOCAL as for bez_sim_apply_body_forces -- a LOCAL vector is in the body's own frame (its link's), a
 *     LOCAL point in the body's frame, an ENV point in env coordinates.  With positions_dev == NULL the point of application is the
 *     body's own centre of mass (BEZ_BODY_COM), as in the apply call; with BEZ_GF_AT_ORIGIN OR-ed into `space` (this call only) it is
 *     the body's ORIGIN, and the call is out = sum_b J_b^T [f_b; t_b] with J of BEZ_DYNAMICS_JACOBIAN, rows and columns as defined there.
 *     BEZ_GF_AT_ORIGIN with a non-NULL positions_dev: rc -1.
 *   out_dev  f32 (N, 24), env-major, in u = [root_lin, root_ang, qd]: rows 0:3 the total force in world axes, rows 3:6 the total moment
 *     about the root origin in world axes, rows 6:24 the joint torques in DOF_STATE order -- the row convention of
 *     bez_sim_inverse_dynamics, dual to u: u . out is the power of the wrenches.  Fixed bodies (imu_link, camera, the cleats) act on
 *     their link at their own origin or centre of mass; the asset (cleats, box, the joint origin box + cleats moves) is the step's.
 *   Masses, gravity rows, velocities and BEZ_FLAG_FIX_BASE play no part: the stored q and root pose are evaluated as they stand on `stream`.
 *   A body whose force row and torque row are all zero contributes exactly nothing, whatever its position row holds; a NaN is not zero
 *     and goes in (the rule of the apply call).  A non-finite input is written through and stays in its own env.
 *   To the bit: all-zero inputs give 24 times +0.0f; a joint row is +0.0f when no loaded body lies on the joint's link or below it; a
 *     wrench on body 0 alone in BEZ_SPACE_ENV whose position row equals the root position gives out[0:6] = [f; t] and +0.0f on rows
 *     6:24.  (Every output is canonicalised with x + 0.0f: -0.0 becomes +0.0.)
 *   One kernel launch.  The call allocates nothing, never synchronises, reads nothing on the host, writes only out_dev and leaves the
 *   sim's state and any pending external wrenches untouched: it captures into a HIP graph.  Results do not depend on N or on an env's
 *   place in its tile.  forces_dev and torques_dev both NULL (nothing to map), a null out_dev, a null sim or an unknown `space`: rc -1
 *   with a message. */
#define BEZ_GF_AT_ORIGIN 2   /* OR-ed into `space`, for this call only */
int bez_sim_generalized_forces(BezSim* sim, const float* forces_dev, const float* torques_dev, const float* positions_dev,
                               int32_t space, float* out_dev /* (N, 24) */, void* stream);

/* Limb inverse kinematics: damped least squares per chain -- which joint angles put a foot, a hand or the camera at a pose.  The tree is
 * five serial chains off the torso with disjoint joints, in the order of their first DOF:
 *     0 head (DOF 0:2, end body /head), 1 left arm (2:4, /left_forearm), 2 left leg (4:10, /left_foot), 3 right arm (10:12,
 *     /right_forearm), 4 right leg (12:18, /right_foot);   the end body of a chain is the body of its last link,
 * so a torso-relative problem for all five end bodies is five independent problems of size 2, 2, 6, 2, 6, each solved in registers; no
 * Jacobian tensor is formed.
 *   targets_dev  f32 (N, 5, 7), env-major: per chain the wanted position (3) and orientation (quaternion xyzw, normalised by the call) of
 *     the controlled frame.  BEZ_IK_SPACE_ENV: as RIGID_BODY_STATE rows carry them (env position, world quaternion) -- they are taken into
 *     the root's frame once, by the state's root pose (its quaternion used as it stands, as every other query uses it).
 *     BEZ_IK_SPACE_ROOT: relative to the root origin in the root's axes (what a gait generator emits); the root pose is then not read.
 *   params (by value into the launch): weight[c] = {w_pos, w_rot} >= 0 on the squared position / rotation error; both 0: chain c is not
 *     asked for.  offset[c]: the controlled frame is the chain's end body displaced by this vector, in that body's frame (same axes).
 *     damping lambda > 0; max_step > 0: the largest |dq_i| of one iteration (the chain's step is scaled as a whole), <= 0: no limit;
 *     iters 0 .. BEZ_IK_MAX_ITERS; space.
 *   The iteration of chain c with k joints, on a private copy of its k angles that starts from the state's q, `iters` times:
 *     1. forward kinematics of the chain in the root's axes relative to the root origin (the asset's, the joint origin box + cleats moves
 *        included): the controlled frame's origin p and rotation R, the joints' axes a_j and origins r_j;
 *     2. e = [p_des - p ; 2 sign(w) (x, y, z)] with (x, y, z, w) the quaternion of R_des R^T, sign(0) = +1 (the rotation part is
 *        2 sin(theta / 2) axis);
 *     3. J_j = [a_j x (p - r_j) ; a_j];
 *     4. (J^T W J + lambda^2 I) dq = J^T W e with W = diag(w_pos x3, w_rot x3), by a k x k Cholesky factorisation;
 *     5. dq is scaled so that max |dq_i| <= max_step;
 *     6. q <- clamp(q + dq, lower, upper), the limits the env's BEZ_PARAM_DOF_LOWER / BEZ_PARAM_DOF_UPPER rows where set, else the model's.
 *   q_out_dev    f32 (N, 18) in DOF_STATE order, or NULL: the angles after the last iteration.
 *   err_out_dev  f32 (N, 5, 6), or NULL: e of step 2 at the final q (one more pass of steps 1 and 2), unweighted: iters = 0 is a pure
 *     pose-error query of the current state.
 *   To the bit: a chain with both weights 0 returns the state's q for its joints (unclamped) and +0.0f error rows, and nothing of its
 *     target row enters any output (a NaN there is harmless); a chain's outputs do not depend on any other chain's target, weights or
 *     offset; iters = 0 returns the state's q; results do not depend on N, on an env's place in its tile or on the buffers' alignment.
 *     A non-finite target on an active chain makes that chain's q_out (iters >= 1) and every error row it enters non-finite, and no
 *     other chain's.  lambda^2 must stay above the fp32 rounding of J^T W J (about 1e-6 of its largest entry).
 *   One kernel launch with params in its arguments.  The call allocates nothing, copies nothing, never synchronises and writes only the
 *   two outputs: the sim's state and every tensor are untouched, and it captures into a HIP graph.  rc -1 with a message: a null sim,
 *   targets_dev or params, both outputs NULL, iters out of range, damping not a positive finite number, a negative or non-finite weight,
 *   a non-finite offset, a NaN max_step, an unknown space. */
#define BEZ_IK_CHAINS 5
#define BEZ_IK_SPACE_ENV  0
#define BEZ_IK_SPACE_ROOT 1
#define BEZ_IK_MAX_ITERS 64
typedef struct BezIkParams {
  float weight[BEZ_IK_CHAINS][2];
  float offset[BEZ_IK_CHAINS][3];
  float damping;
  float max_step;
  int32_t iters;
  int32_t space;
} BezIkParams;
int bez_sim_limb_ik(BezSim* sim, const float* targets_dev /* (N,5,7) */, const BezIkParams* params,
                    float* q_out_dev /* (N,18) or NULL */, float* err_out_dev /* (N,5,6) or NULL */, void* stream);

/* Proximity: the contact geometry the step kernels decide on every substep -- 22 ground points against the plane z = 0, the ball against
 * eleven boxes, 28 left-leg x right-leg capsule pairs -- as distances, normals and points of the state as it stands on `stream`: foot
 * clearance, a self-collision penalty, the distance of the ball to the kicking foot, and a known answer for tests of the narrow phase.
 * All outputs are f32, env-major; any of them may be NULL.  Geometry is evaluated relative to the root origin, as the step does, and
 * root_pos enters only the last addition of an env-coordinate output: a root far from the env origin costs nothing in the gaps.
 *   ground_dev  (N, 23, 3): rows 0:22 the positions, in env coordinates, of the asset's ground points in table order (bez_model.json
 *     "ground_points": four per foot, the torso's guard points, the head's, one per forearm) -- the cleats table with BEZ_FLAG_CLEATS, the
 *     upper-body guard points BEZ_FLAG_BOX_ASSET moves, the joint origin box + cleats moves.  The z word is root_pos.z + x.z with x the
 *     point relative to the root origin -- the step's d = -z > 0 decision -- and does not depend on root_pos.x / root_pos.y, to the bit.
 *     Row 22 (BEZ_PROX_BALL_ROW) is ball_pos - (0, 0, R), the ball's lowest point.
 *   ball_dev    (N, 11, 8): one row per box in the model's box order (left leg hip -> foot 0:5, right leg 5:10, torso 10; with
 *     BEZ_FLAG_BOX_ASSET the box asset's own torso box).  gap: the signed distance from the ball's surface to the box, minus the step's
 *     depth and defined when positive too -- centre outside the box: |centre - clamped point| - R; centre inside: -(R + smallest face
 *     distance).  normal: from the box to the ball, world axes.  point: the closest point of the box surface, env coordinates; with the
 *     centre inside, its projection onto the nearest face (first of x, y, z on ties), as the step's.
 *   pairs_dev   (N, 28, 8): one row per capsule pair in the model's "capsule_pairs" order (a on the left leg, b on the right).  gap: the
 *     distance between the two axis segments minus (ra + rb).  normal: from capsule b's closest point to capsule a's -- the step's n: the
 *     contact force on link a is along +n.  point: the step's contact point cb + n (rb - depth / 2), depth = -gap, env coordinates, by
 *     the same formula for positive gaps.  Where the axes meet (squared distance <= 1e-12, where the step applies no force): gap =
 *     -(ra + rb), normal three +0.0f, point = cb.
 *   A row of 8 words is [gap, normal(3), point(3), +0.0f].
 *   Velocities, masses, gravity, BEZ_FLAG_FIX_BASE and BEZ_FLAG_NO_SELF_COLLISION play no part: the call reports geometry whether or not
 *   the step would act on it.  A task without a ball has it parked, and the ball rows are computed from the stored ball state like any
 *   other.  A non-finite state is written through and stays in its own env; the pad words stay +0.0f.  Results do not depend on N, on an
 *   env's place in its tile or on the buffers' alignment.
 *   Not reported: the calf <-> foot-plate pair of BEZ_FLAG_ANKLE_STOP and the 118 extra points of BEZ_FLAG_ALL_GROUND_SHAPES, which live
 *   on the one-env-per-lane step kernel only.
 *   One kernel launch.  The call allocates nothing, never synchronises, reads nothing on the host and writes only the outputs: it
 *   captures into a HIP graph.  All outputs NULL or a null sim: rc -1 with a message. */
#define BEZ_PROX_GROUND_ROWS 23   /* 22 ground points + the ball's lowest point */
#define BEZ_PROX_BALL_ROW    22
#define BEZ_PROX_BOXES       11
#define BEZ_PROX_PAIRS       28
#define BEZ_PROX_WORDS        8   /* gap, normal(3), point(3), 0.0f */
#define BEZ_PROX_GAP 0
#define BEZ_PROX_NORMAL 1
#define BEZ_PROX_POINT 4
int bez_sim_proximity(BezSim* sim, float* ground_dev /* (N,23,3) or NULL */,
                      float* ball_dev /* (N,11,8) or NULL */, float* pairs_dev /* (N,28,8) or NULL */, void* stream);

/* Query states.  Every query above is "of the current state".  A query state is a second state, of M rows with M >= 1 independent of
 * N, that the same kernels read instead: candidate poses of a planner (M = N x K), logged (q, u) samples, what limb_ik returned.  The
 * live state is never written.  A BezQueryState is owned by the sim that created it and holds
 *   - the fields the query kernels read -- root 13, q 18, qd 18, ball 13 -- as M-row SoA columns (no targets, contact forces, goal: no
 *     query reads them);
 *   - M-row copies of the four parameter rows those kernels use: BEZ_PARAM_MASS_SCALE, BEZ_PARAM_GRAVITY, BEZ_PARAM_DOF_LOWER,
 *     BEZ_PARAM_DOF_UPPER;
 *   - tensors of its own, each allocated when bez_query_state_tensor first hands it out: RIGID_BODY_STATE rows (M*NBE, 13), the Jacobian
 *     (M*NB, 6, 24) and the mass matrix (M, 24, 24), defined as the sim's.
 * bez_query_state_create allocates the state and the parameter copies (zeroed: fill it before asking) through the sim's buffer owner;
 * bez_query_state_destroy frees them, and bez_sim_destroy frees the query states still alive.  A sim that creates none allocates and
 * launches what it did without them.
 *
 * bez_query_state_set fills all M rows from Isaac-layout rows: root_dev (M, 13) as ROOT_STATE rows, dof_dev (M, 18, 2) as DOF_STATE
 * rows, ball_dev (M, 13) or NULL.  Values are copied as given (no normalisation, no finiteness filter), as the indexed setters do.
 * ball_dev must be NULL on a task without a ball; NULL on bez_kick is the config's ball_init pose at rest.  env_ids_dev NULL: every row
 * has the asset's nominal parameters -- the kernels are handed null parameter rows: mass scale 1, the config's gravity, the model's
 * limits.  env_ids_dev (M) int32: row i has a copy of env env_ids[i]'s four rows as they are when the call runs on `stream`; a parameter
 * the sim never allocated stays a null row here too; ids may repeat; an id outside 0 .. N-1 gives that row the default row's values
 * (the kernel checks the range and reads nothing outside the sim's arrays).
 * bez_query_state_capture sets row i to the live state of env env_ids[i] -- root, joints, ball -- with its parameter rows.  NULL is
 * the identity and needs M == N.  A row whose id is outside 0 .. N-1 is left as it was, parameters included.
 * Which parameter rows the kernels are handed is decided by the last set or capture, for the whole query state.
 *
 * bez_query_state_bind(sim, qs) redirects the query entry points and nothing else: until bez_query_state_bind(sim, NULL),
 * bez_sim_inverse_dynamics, _forward_dynamics, _operational_space, _centroidal, _body_accelerations, _generalized_forces, _limb_ik and
 * _proximity read the bound state, tile over its M rows and take and write M-row tensors where their comments say N.  Stepping, the
 * setters, the refreshes of the sim's own tensors, resets and randomisation never look at the binding.  The binding is host state: a
 * launch already enqueued keeps the state it was launched on.
 * bez_query_state_refresh(sim, qs, which_mask) fills the acquired tensors of the mask ((1u << BezQueryTensor) bits) with the kernels of
 * bez_sim_refresh_tensor(RIGID_BODY_STATE) and bez_sim_refresh_dynamics_tensors run on the query state; it needs no binding.
 *
 * rc -1 with a bez_sim_last_error message: a null sim or query state, a query state of another sim (also when binding it), rows <= 0,
 * ball_dev on a task without a ball, capture with NULL ids and M != N, destroying the bound query state, refreshing a tensor that was
 * never acquired.  create, destroy and the first bez_query_state_tensor of a tensor allocate or free (and may wait for the device);
 * set, capture, refresh and the bound queries are plain kernel launches on `stream` -- one per call, two for a refresh of rigid-body rows
 * together with a dynamics tensor -- that allocate nothing, never synchronise and capture into a HIP graph. */
typedef struct BezQueryState BezQueryState;
typedef enum BezQueryTensor {
  BEZ_QUERY_RIGID_BODY_STATE = 0, /* f32 (M*NBE, 13): the rows of BEZ_TENSOR_RIGID_BODY_STATE */
  BEZ_QUERY_JACOBIAN = 1,         /* f32 (M*NB, 6, 24): BEZ_DYNAMICS_JACOBIAN */
  BEZ_QUERY_MASS_MATRIX = 2,      /* f32 (M, 24, 24): BEZ_DYNAMICS_MASS_MATRIX */
  BEZ_QUERY_TENSOR_COUNT = 3
} BezQueryTensor;
int bez_query_state_create(BezSim* sim, int32_t rows, BezQueryState** out);
int bez_query_state_destroy(BezSim* sim, BezQueryState* qs);
int bez_query_state_set(BezSim* sim, BezQueryState* qs, const float* root_dev /* (M,13) */, const float* dof_dev /* (M,18,2) */,
                        const float* ball_dev /* (M,13) or NULL */, const int32_t* env_ids_dev /* (M) or NULL */, void* stream);
int bez_query_state_capture(BezSim* sim, BezQueryState* qs, const int32_t* env_ids_dev /* (M) or NULL */, void* stream);
int bez_query_state_bind(BezSim* sim, BezQueryState* qs /* or NULL */);
int bez_query_state_tensor(BezSim* sim, BezQueryState* qs, int which, void** dev_ptr, int64_t shape[3], int* ndim, int* dtype);
int bez_query_state_refresh(BezSim* sim, BezQueryState* qs, uint32_t which_mask, void* stream);

/* Env snapshots.  A snapshot holds whole envs -- everything that decides how an env continues -- in M rows, M >= 1 independent of N:
 * save copies envs into rows, restore copies rows back into envs of the owning sim or of another sim on the same device (a planner's
 * second sim), a row into as many envs as wanted.  A BezSnapshot is owned by the sim that created it, allocated through the sim's buffer
 * owner (one device buffer); bez_snapshot_destroy frees it, and bez_sim_destroy frees the snapshots still alive.  A sim that creates none
 * allocates and launches what it did without them.
 *
 * A row holds, as they are when the save runs on `stream` (DESIGN.md 4.3p has the inventory, buffer by buffer):
 *   - every field of the SoA state: root, joints, ball, position targets, previous velocity, contact-force rows, feet words, goal;
 *   - obs, rew, reset, progress, timeout, the episode counter, randomize, the non-finite count;
 *   - the three episode statistics (end counts, reward terms, end bits);
 *   - every BEZ_PARAM_* row the sim had allocated at the save (the snapshot remembers which: "present"); a save whose sim lacks a
 *     parameter leaves the snapshot's rows of it alone and clears its presence for the whole snapshot;
 *   - the actuator record, when the sim had BEZ_FLAG_DOF_FORCE on at bez_snapshot_create (a snapshot created before has no room for it).
 * The global block holds the host counters of observation passes, post-physics calls and explicit resets, whether the gravity rows are
 * uniform and whether the last step added the observation noise itself, and the device words: the goal-draw call counter and its last
 * draw, the randomisation clock with the noise parameters, and the action-noise record.  Every save records it.
 * Not in a snapshot: the Isaac-layout tensors, actuator tensors, Jacobian and mass matrix (derived: after a restore they are stale exactly
 * as after a set_*_indexed call, and their refresh calls bring them to the restored state); external wrenches pending for the next physics
 * launch (a restore does not touch the destination's either); the health word and the diagnostic records; the configuration (gains, time
 * step, flags, the randomisation's ranges).
 *
 * bez_snapshot_save: row i <- env env_ids_dev[i]; NULL: row i <- env i.  Ids may repeat; a row whose id is outside 0 .. N-1 keeps what it
 *   held (the kernel maps such an id to -1 before anything is indexed with it).
 * bez_snapshot_restore: env env_ids_dev[i] of `dst` <- row row_ids_dev[i], i < count; NULL env ids: env i, NULL row ids: row i.  An entry
 *   with either id out of range is skipped.  Valid env ids must be distinct: with duplicates which row wins is undefined, but nothing
 *   outside the buffers is touched.  `what`: BEZ_SNAPSHOT_ENVS leaves dst's global block alone (a partial restore; dst's "gravity rows are
 *   uniform" is cleared when gravity rows were written); BEZ_SNAPSHOT_ENVS | BEZ_SNAPSHOT_GLOBALS also gives dst the snapshot's global
 *   block (a rewind of the whole sim).  A parameter the snapshot has and dst never allocated is allocated as bez_sim_set_env_params does,
 *   default rows for the envs not restored -- with the same consequence: a HIP graph captured before has to be recaptured.  A parameter
 *   dst has and the snapshot lacks: the restored envs get dst's default row.  The packed copy of the gains and limits is rebuilt.  The
 *   actuator record is copied when both sides have it, with the same number of substeps.
 *   dst may differ from the owner in num_envs, seed, env_id_offset, gains and time step ("what if this env ran with other gains"); it
 *   must have the same device, task, asset bits (BEZ_FLAG_CLEATS, BEZ_FLAG_BOX_ASSET), ball and observation width.
 * The random identity of a restored env is the DESTINATION's: the Philox key of its draws stays (dst seed, dst global env id, episode),
 *   with `episode` the copied counter.  So copies of one row in several envs diverge at their next reset draw, and an env restored into
 *   its own slot of its own sim replays the draws it would have had.
 * bez_snapshot_export / bez_snapshot_import move a snapshot as one self-describing blob, in host or device memory: BEZ_SNAPSHOT_HEADER_WORDS
 *   uint32 words -- magic, layout version, rows, number of sections, presence bits, columns, then the width of every section, the host
 *   counters and what a compatible sim has in common --, then the sections as (width, rows) uint32 columns, a 64-bit item as (low, high),
 *   then the global device words.  export with blob NULL only reports the size in *bytes; otherwise *bytes is the room on entry and the
 *   size on return.  import refuses a blob that is too short or whose magic, layout version, rows, widths or task / asset do not fit, and
 *   leaves the snapshot as it was.  Both wait for `stream` before they return.
 * The host counters are read (save) and written (restore with GLOBALS) when the call is made, as a query-state binding is: a launch
 *   already enqueued and a captured graph keep what they were given.  Snapshot calls are not for use inside a graph capture.
 *
 * rc -1 with a bez_sim_last_error message: rows < 1; a null sim; a null or destroyed snapshot; a snapshot of another sim (save, destroy,
 * export, import); count < 0; count > the snapshot's rows with NULL row ids; a bit in `what` outside the two above, or without
 * BEZ_SNAPSHOT_ENVS; restoring a snapshot nothing was saved into; an incompatible dst.  create, destroy and a restore that has to allocate
 * a parameter allocate or free (and may wait for the device); every other save and restore is ONE kernel launch on `stream` (the global
 * device words move inside it) -- plus the rebuild of the packed gains and limits where dst has any of the four -- that allocates nothing. */
typedef struct BezSnapshot BezSnapshot;
#define BEZ_SNAPSHOT_ENVS 1u
#define BEZ_SNAPSHOT_GLOBALS 2u
#define BEZ_SNAPSHOT_MAGIC 0x4e535a42u /* "BZSN" */
#define BEZ_SNAPSHOT_LAYOUT 1
#define BEZ_SNAPSHOT_HEADER_WORDS 40
#define BEZ_SNAPSHOT_SECTIONS 20   /* state, obs, rew, reset, progress, timeout, episode, randomize, nonfinite, end_counts, reward_terms, \
                                      end_bits, the seven BEZ_PARAM_* rows in enum order, the actuator record */
#define BEZ_SNAPSHOT_GLOBAL_WORDS 16 /* call counter 2, randomisation clock and noise 8, action-noise record 4, goal draw 2 */
int bez_snapshot_create(BezSim* sim, int32_t rows, BezSnapshot** out);
int bez_snapshot_destroy(BezSim* sim, BezSnapshot* snap);
int bez_snapshot_save(BezSim* sim, BezSnapshot* snap, const int32_t* env_ids_dev /* (rows) or NULL */, void* stream);
int bez_snapshot_restore(BezSim* dst, const BezSnapshot* snap, const int32_t* env_ids_dev /* (count) or NULL */,
                         const int32_t* row_ids_dev /* (count) or NULL */, int32_t count, uint32_t what, void* stream);
int bez_snapshot_export(BezSim* sim, const BezSnapshot* snap, void* blob /* host or device, or NULL */, int64_t* bytes, void* stream);
int bez_snapshot_import(BezSim* sim, BezSnapshot* snap, const void* blob, int64_t bytes, void* stream);

/* gym.refresh_{actor_root_state,dof_state,rigid_body_state,net_contact_force}_tensor
 * (kick_env.py:750-753): materialise the Isaac-layout tensor from the SoA state.  ROOT_STATE, DOF_STATE, RIGID_BODY_STATE,
 * NET_CONTACT_FORCE, DOF_TARGET, PREV_LIN_VEL, FEET and GOAL need it; every other BezTensor is always live (the kernels
 * write it in place) and its refresh is a successful no-op.  An id outside the enum: rc -1. */
int bez_sim_refresh_tensor(BezSim* sim, int which, void* stream);

/* gym.set_actor_root_state_tensor_indexed (kick_env.py:831-837): teleport the actors listed in
 * actor_ids_dev (sim-domain actor index = env*2 + {0 robot, 1 ball}) to the rows of the full
 * (N*2,13) tensor root_states_dev. */
int bez_sim_set_actor_root_state_tensor_indexed(BezSim* sim, const float* root_states_dev,
                                                const int32_t* actor_ids_dev, int32_t n, void* stream);
/* gym.set_dof_state_tensor_indexed (kick_env.py:844-847); actor ids as above (robot actors). */
int bez_sim_set_dof_state_tensor_indexed(BezSim* sim, const float* dof_state_dev,
                                         const int32_t* actor_ids_dev, int32_t n, void* stream);
/* gym.set_dof_position_target_tensor (kick_env.py:419): (N,18) targets, used as given. */
int bez_sim_set_dof_position_target_tensor(BezSim* sim, const float* targets_dev, void* stream);
/* gym.set_dof_position_target_tensor_indexed (kick_env.py:839-842). */
int bez_sim_set_dof_position_target_tensor_indexed(BezSim* sim, const float* targets_dev,
                                                   const int32_t* actor_ids_dev, int32_t n, void* stream);
/* Writes the (N*22,3) net-contact-force tensor into the sim (test hook: the reference's feet
 * logic reads AND mutates this tensor, kick_env.py:987-990). */
int bez_sim_set_net_contact_force_tensor(BezSim* sim, const float* forces_dev, void* stream);

/* VecTask.step's clamp + KickEnv.pre_physics_step (vec_task.py:317, kick_env.py:410-419):
 * a = clamp(actions, +-clip); a[:,0:2] = 0; target = clamp(a + default_dof_pos, lower, upper). */
int bez_sim_pre_physics(BezSim* sim, const float* actions_dev, void* stream);
/* gym.simulate (vec_task.py:322-324): one control step dt = `substeps` substeps of articulated
 * dynamics (ABA, implicit PD drives, contact) for every env. */
int bez_sim_simulate(BezSim* sim, void* stream);
/* timeout fill + KickEnv.post_physics_step (vec_task.py:331-335, kick_env.py:426-438):
 * timeout = progress >= max_len-1; progress += 1; reset_idx(envs with reset_buf != 0);
 * observations; reward + reset flags. */
int bez_sim_post_physics(BezSim* sim, void* stream);
/* The three calls above fused into ONE kernel launch: the whole of VecTask.step
 * (vec_task.py:303-349) for all envs.  This is the hot path. */
int bez_sim_step(BezSim* sim, const float* actions_dev, void* stream);
/* bez_sim_step for n_steps consecutive control steps, actions_dev = (n_steps, N, 18); the
 * rollout inner loop without a host round trip per step (random-action benchmark). */
int bez_sim_step_many(BezSim* sim, const float* actions_dev, int32_t n_steps, void* stream);

/* KickEnv.reset_idx (kick_env.py:779-850) for the env ids in env_ids_dev. */
int bez_sim_reset_indexed(BezSim* sim, const int32_t* env_ids_dev, int32_t n, void* stream);

/* gym.apply_rigid_body_force_tensors / gym.apply_rigid_body_force_at_pos_tensors: external forces and torques on the rigid bodies,
 * for the NEXT physics launch (bez_sim_simulate, bez_sim_step, the first step of bez_sim_step_many) only -- they act through all of
 * its substeps and are then cleared on the device.  Several calls before one launch add up.
 *   forces_dev / torques_dev / positions_dev: fp32 (N*B, 3) in RIGID_BODY_STATE order (B = 22 for bez_kick, 21 for bez_walk /
 *   bez_orient; 30 / 29 with cleats); any of them may be NULL (no force / no torque / forces at each body's centre of mass).
 *   space: BEZ_SPACE_ENV -- vectors in world axes (each env is its own world), points in world coordinates;
 *          BEZ_SPACE_LOCAL -- vectors and points in the body's own frame.
 * Resolution: a force or torque given in world axes stays fixed in world axes across the substeps.  A BEZ_SPACE_LOCAL force or torque
 * and every point of application are resolved ONCE, in this call, against the body poses then on `stream` (the state the launches
 * enqueued before it leave); from there the world-axis vector stays fixed and the point moves with its body.  A force at a point acts
 * on the body as that force at the body's centre of mass plus its moment.  Fixed bodies (imu_link, camera, the cleats) add their wrench
 * to the dynamic link they are merged into.  Centres of mass: each rigid body's own URDF inertial origin (BEZ_BODY_COM).
 * The NET_CONTACT_FORCE rows, the feet flags and the reward terms stay contact-only; a non-finite input makes the env's state
 * non-finite, which the non-finite guard handles as any other (BEZ_FLAG_NONFINITE_GUARD).
 * The first call switches the sim, for the rest of its life, to step-kernel instantiations that read the pending wrenches (a captured
 * graph keeps the kernels it was captured with; a sim that never calls this launches the kernels it always did).  The call allocates
 * its buffer on first use; after that it allocates nothing, never synchronises and reads no device data on the host: it can be
 * captured into a HIP graph. */
#define BEZ_SPACE_ENV 0
#define BEZ_SPACE_LOCAL 1
int bez_sim_apply_body_forces(BezSim* sim, const float* forces_dev, const float* torques_dev, const float* positions_dev, int32_t space,
                              void* stream);

/* Domain randomisation parameters (vec_task.py:505-725 -> per-env arrays read by the kernel).
 * values_dev: (N, count) fp32 where count is fixed per param; NULL restores the default. */
enum BezEnvParam {
  BEZ_PARAM_FRICTION = 0,   /* (N,1)  ground/ball friction coefficient      bez_kick.yaml:179-186 */
  BEZ_PARAM_KP_SCALE = 1,   /* (N,18) stiffness scaling                     bez_kick.yaml:200-205 */
  BEZ_PARAM_KD_SCALE = 2,   /* (N,18) damping scaling                       bez_kick.yaml:194-199 */
  BEZ_PARAM_MASS_SCALE = 3, /* (N,19) link mass scaling (setup only)        bez_kick.yaml:170-177 */
  BEZ_PARAM_GRAVITY = 4,    /* (N,3)  gravity vector                        bez_kick.yaml:162-167 */
  BEZ_PARAM_DOF_LOWER = 5,  /* (N,18) physical lower joint limits           bez_kick.yaml:206-212 */
  BEZ_PARAM_DOF_UPPER = 6,  /* (N,18) physical upper joint limits           bez_kick.yaml:213-219 */
  BEZ_PARAM_COUNT = 7
};
int bez_sim_set_env_params(BezSim* sim, int param, const float* values_dev, void* stream);
/* copies the current (N, count) array of `param` into out_dev (defaults if the parameter was never set) */
int bez_sim_get_env_params(BezSim* sim, int param, float* out_dev, void* stream);

/* Device-side domain randomisation: VecTask.apply_randomizations (vec_task.py:505-725, called from reset_idx, kick_env.py:781-782)
 * without the host.  One entry of cfg/task/bez_kick.yaml:151-219 per BezDrRange: a, b = `range`; distribution and operation are
 * fixed per parameter as that file has them (uniform scaling: friction, stiffness, damping; gaussian additive, b = the number
 * numpy uses as the std: lower, upper, gravity, observations, actions); schedule_steps > 0 = `schedule: linear` (the range is
 * interpolated from "no randomisation" by min(frame, schedule_steps) / schedule_steps, vec_task.py:560-566 and gymutil [ext]).
 * Once set, every call that contains the post-physics first runs one small kernel that does what reset_idx's call does:
 * randomize_buf += 1; an env with reset_buf != 0 and randomize_buf >= frequency draws new friction / Kp / Kd / joint limits from
 * the Philox stream keyed by (seed, GLOBAL env id, episode, parameter) and clears its randomize_buf; if any env resets and
 * `frequency` frames have passed since the last time, gravity (one draw for the whole sim) and the noise parameters are
 * refreshed.  Nothing syncs with the host: the step stays HIP-graph capturable.  The first call randomises every env at
 * frame 0 (first_randomization, vec_task.py:521-523).  NULL switches it off (arrays keep their values). */
typedef struct BezDrRange {
  float a, b;
  int32_t enabled;
  int32_t schedule_steps;
} BezDrRange;
typedef struct BezDrConfig {
  int32_t frequency;        /* randomization_params.frequency                     bez_kick.yaml:153 */
  int32_t friction_buckets; /* rigid_shape_properties.friction.num_buckets        bez_kick.yaml:180 */
  BezDrRange friction;      /* bez_kick.yaml:179-186 */
  BezDrRange stiffness;     /* bez_kick.yaml:200-205 */
  BezDrRange damping;       /* bez_kick.yaml:194-199 */
  BezDrRange lower, upper;  /* bez_kick.yaml:206-219 */
  BezDrRange gravity;       /* bez_kick.yaml:162-167 */
  BezDrRange observations;  /* bez_kick.yaml:154-157 */
  BezDrRange actions;       /* bez_kick.yaml:158-161 */
} BezDrConfig;
int bez_sim_set_randomization(BezSim* sim, const BezDrConfig* dr, void* stream);
/* The randomisation kernel of the COMING control step (what the next call containing the post-physics would launch first), now, on
 * `stream`; that call then skips its own.  Lets a caller overlap it with whatever else precedes the step (a policy forward pass) on
 * another stream -- which must be joined before the step.  The previous step must be complete on a stream `stream` is ordered behind.
 * The action noise (bez_sim_add_dr_noise(which = 1), BezActionNoiseSource) reads a SNAPSHOT the previous step left, not the state this
 * kernel updates, so it may run concurrently with it. */
int bez_sim_dr_prelaunch(BezSim* sim, void* stream);
/* The same work as an opaque argument block for a launch of the caller's that executes it ITSELF, as one extra workgroup beside its own
 * (bez_ppo_policy_rollout_step's dr_step argument): fills blob[BEZ_DR_STEP_BYTES] for the COMING control step, which then skips its own
 * randomisation kernel -- the caller must run that launch before the step, on the step's stream.  Nothing in the block changes from step
 * to step (all clocks live in device memory), so a captured graph replays it.  Returns the bytes used, 0 without a randomisation. */
#define BEZ_DR_STEP_BYTES 512
int bez_sim_dr_step_args(BezSim* sim, void* blob, int32_t blob_bytes);
/* Takes back a hand-out of bez_sim_dr_prelaunch / bez_sim_dr_step_args whose consumer did NOT run (its launch failed or was skipped): the
 * coming control step launches its own randomisation kernel again.  Also implied by bez_sim_set_randomization and bez_sim_seed.  Only for
 * the not-run case: after a consumer that did run, the step would randomise twice. */
int bez_sim_dr_cancel(BezSim* sim);
/* For a consumer that adds the action noise of vec_task.py:586-592 itself (e.g. bez_ppo_policy_rollout_step): *snap_dev -> device struct
 * {float mean, std; uint32_t frame_lo, frame_hi} kept current by the step kernels; noise of element i of the flat (N, 18) action tensor =
 * mean + std * z, z = word (i & 3) of the Philox4x32-10 block with counter (key lo, key hi, frame lo, 0x4e4f4953 + 1 + (frame hi << 8)),
 * key = env_id_offset * 64 + (i >> 2), Philox key = seed, Box-Muller pairs (words 0,1 -> z0 = r cos, z1 = r sin; words 2,3 -> z2, z3) --
 * bit for bit what bez_sim_add_dr_noise(which = 1) adds.  Returns 1 if an action noise is configured, 0 if not, < 0 on error. */
int bez_sim_action_noise_source(BezSim* sim, const void** snap_dev, uint64_t* seed, int64_t* env_id_offset);
/* The noise lambdas of vec_task.py:544-618 in one launch: y[i] = x[i] + mean + std * N(0,1) for n floats (y_dev may be x_dev: in
 * place), mean / std = the current entries of BEZ_TENSOR_DR_NOISE for `which` (0 = observations, 1 = actions), normals from
 * Philox keyed by (seed, frame, which, i / 4) -- one call per control step and kind. */
int bez_sim_add_dr_noise(BezSim* sim, const float* x_dev, float* y_dev, int64_t n, int32_t which, void* stream);

/* Test hooks (state injection for the parity tests; no reference counterpart). */
int bez_sim_set_prev_lin_vel_tensor(BezSim* sim, const float* prev_dev, void* stream); /* (N,3) */
int bez_sim_set_flags(BezSim* sim, uint32_t flags);  /* the asset bits (BEZ_FLAG_CLEATS, BEZ_FLAG_BOX_ASSET) keep their creation value */
/* compute_observations + compute_reward on the current state, without timeout/progress/reset bookkeeping */
int bez_sim_observe_reward(BezSim* sim, void* stream);
/* writes the per-env goal (N,2) of bez_walk / bez_orient */
int bez_sim_set_goal_tensor(BezSim* sim, const float* goal_dev, void* stream);
/* number of compute_observations passes already done: only pass 0 differences against prev = zeros (Q1) */
int bez_sim_set_obs_calls(BezSim* sim, int64_t calls);

/* Reads the health word (BEZ_HEALTH_* bits) into *bits, synchronously on `stream` (work enqueued before on that stream is
 * included), and clears it when `clear` != 0.  For callers outside the hot loop: the word is also a zero-copy tensor
 * (BEZ_TENSOR_HEALTH) that a caller can fold into a device-side report of its own. */
int bez_sim_health(BezSim* sim, uint64_t* bits, int32_t clear, void* stream);

/* Re-keys the reset-noise stream (utils/utils.py:45-70 set_seed). */
int bez_sim_seed(BezSim* sim, uint64_t seed);

/* Measurement utility: launches a known-size dword-per-lane read (write=0) or write (write=1) of n_floats floats of
 * buf_dev, to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE for this library's access shape. */
int bez_sim_calibrate(void* buf_dev, uint64_t n_floats, int32_t write, void* stream);

/* Average device time [ms] of the fused step kernel over `n_steps` launches on `stream`,
 * measured with HIP events recorded on that same stream (bench.py roofline leg). */
int bez_sim_time_steps(BezSim* sim, const float* actions_dev, int32_t n_steps, void* stream, float* avg_ms);

/* ------------------------------------------------------------------------------------------------------------------
 * PPO glue kernels (bez_ppo.hip).  The reference trains through rl_games' a2c_continuous (call sites train.py:89-113,
 * hyper-parameters cfg/train/bez_kickPPO.yaml); its MLP stays in PyTorch-ROCm, these entry points replace the ~250 tiny
 * elementwise / reduction launches per minibatch step around it.  All pointers are device memory, fp32 unless noted. */

/* The signatures below change between rounds (round 3: scratch buffers of the fixed-order reductions, plan / run split of the weight
 * gradients, the optimiser tail's bookkeeping): a binding checks this number once after dlopen. */
#define BEZ_PPO_ABI_VERSION 9
int32_t bez_ppo_abi_version(void);

/* RunningMeanStd (normalize_input / normalize_value, bez_kickPPO.yaml:51-52): moments[0:D] = column sums, [D:2D] = sums of
 * squares, [2D] = rows, in fp64 (the caller may all-reduce them across ranks before applying).  scratch_dev: NULL = fp64 atomics (the
 * last bits vary from run to run); otherwise 1 + 1024 * 2 * cols doubles: per-workgroup partials, added in workgroup order by a second
 * small launch -- bit-reproducible. */
int bez_ppo_rms_moments(const float* x_dev, int64_t rows, int32_t cols, double* moments_dev, double* scratch_dev, void* stream);
int bez_ppo_rms_apply(const double* moments_dev, int32_t cols, double* mean_dev, double* var_dev, double* count_dev, void* stream);
/* y = clamp((x - mean) / sqrt(var + eps), -5, 5); y_dev is fp32 or (out_f16 != 0) fp16 */
int bez_ppo_rms_normalize(const float* x_dev, int64_t rows, int32_t cols, const double* mean_dev, const double* var_dev, float eps,
                          void* y_dev, int32_t out_f16, void* stream);
/* rollout: actions = mu + exp(logstd) * noise, neglogp(actions), env_actions = clamp(actions, -1, 1), sigma broadcast */
int bez_ppo_sample(const float* mu_dev, const float* logstd_dev, const float* noise_dev, int64_t n, int32_t num_actions,
                   float* actions_dev, float* env_actions_dev, float* neglogp_dev, float* sigma_dev, void* stream);
/* One rollout step between the policy forward and the env step (rl_games a2c_common.play_steps [ext] via train.py:89-113):
 * network outputs mu (n, num_actions) / value (n) as fp16 (inputs_f16 != 0) or fp32; the value is de-normalised with the running
 * value statistics (NULL = none); rows of the rollout buffers obs / dones / mu / value are written; actions are sampled as
 * bez_ppo_sample does. */
int bez_ppo_rollout_pre(const void* mu_dev, const void* value_dev, int32_t inputs_f16, const float* logstd_dev, const float* noise_dev, const float* obs_dev,
                        const float* dones_dev, const double* value_mean_dev, const double* value_var_dev, float value_eps, int64_t n, int32_t num_actions,
                        int32_t num_obs, float* mb_obs_dev, float* mb_dones_dev, float* mb_mu_dev, float* mb_val_dev, float* actions_dev,
                        float* env_actions_dev, float* neglogp_dev, float* sigma_dev, void* stream);

/* rollout bookkeeping of one env step: shaped = rew * reward_scale (+ gamma * value * time_out, value_bootstrap),
 * dones as float, running episode return / length, ep_stats[3] += (finished, sum of returns, sum of lengths) in fp64 */
int bez_ppo_rollout_post(const float* rew_dev, const int64_t* dones_dev, const int64_t* timeouts_dev, const float* values_dev, int64_t n,
                         float reward_scale, float gamma, int32_t value_bootstrap, float* shaped_dev, float* dones_f_dev,
                         float* cur_rew_dev, float* cur_len_dev, double* ep_stats_dev, void* stream);
/* ABI 8: the same launch with ONE EXTRA workgroup that adds the nslots per-workgroup slots of BezPpoRolloutPost.ep_parts (4 doubles each) to
 * ep_stats and clears them -- the last bookkeeping launch of a rollout whose policy launches filled the slots. */
int bez_ppo_rollout_post_fold(const float* rew_dev, const int64_t* dones_dev, const int64_t* timeouts_dev, const float* values_dev, int64_t n,
                              float reward_scale, float gamma, int32_t value_bootstrap, float* shaped_dev, float* dones_f_dev, float* cur_rew_dev,
                              float* cur_len_dev, double* ep_stats_dev, double* ep_parts_dev, int32_t nslots, void* stream);
/* PPO minibatch loss (clipped surrogate, clipped value loss, entropy, bounds loss) AND its gradient w.r.t. the network
 * outputs mu (B,A), value (B) and the log-std parameter (A), multiplied by *loss_scale_dev (GradScaler; NULL = 1).
 * stats_dev[5] = sums of a_loss, c_loss, b_loss, KL(current || old), entropy over the minibatch.
 * clip_value: bit 0 = clipped value loss; bit 1 = ACCUMULATE into grad_logstd_dev instead of clearing it first; bit 2 = stats_dev was
 * zeroed by the caller (e.g. as part of the flat gradient buffer's one clear per step); bit 3 = after the KL is taken, WRITE the
 * current mu and sigma = exp(logstd) over old_mu_dev / old_sigma_dev (rl_games' PPODataset.update_mu_sigma [ext]: from the second
 * mini-epoch on the KL is measured against the previous pass over the minibatch).
 * scratch_dev: NULL = the A + 5 sums are float atomics (last bits differ from run to run); otherwise 2 + ceil(batch / 64) * (A + 5)
 * floats: every workgroup stores its partials there and a second one-wave launch adds them in a fixed order -- bit-reproducible. */
int bez_ppo_loss(const float* mu_dev, const float* logstd_dev, const float* value_dev, const float* actions_dev, const float* old_logp_dev,
                 const float* adv_dev, const float* old_value_dev, const float* returns_dev, const float* old_mu_dev,
                 const float* old_sigma_dev, int64_t batch, int32_t num_actions, float e_clip, float critic_coef, float entropy_coef,
                 float bounds_coef, int32_t clip_value, const float* loss_scale_dev, float* grad_mu_dev, float* grad_value_dev,
                 float* grad_logstd_dev, float* stats_dev, float* scratch_dev, void* stream);

/* The rollout's policy forward pass (rl_games get_action_values [ext] via train.py:89-113) in one launch: observation normaliser
 * (NULL mean = none), num_hidden Linear + ELU layers, the mu head (num_actions <= 31) and the value head, on fp16 weights /
 * biases in torch layout ((out, in) row-major; hidden_* are HOST arrays of num_hidden device pointers / widths <= 416), fp32
 * accumulation, fp16 rounding after every Linear and ELU as torch's fp16 path does.  Outputs fp32: mu (n, num_actions), value (n). */
int bez_ppo_policy_forward(const float* obs_dev, int64_t n, int32_t num_obs, const double* obs_mean_dev, const double* obs_var_dev, float obs_eps,
                           int32_t num_hidden, const void* const* hidden_w_f16_dev, const void* const* hidden_b_f16_dev, const int32_t* hidden_width,
                           const void* mu_w_f16_dev, const void* mu_b_f16_dev, int32_t num_actions, const void* value_w_f16_dev,
                           const void* value_b_f16_dev, float* mu_dev, float* value_dev, int32_t weights_packed, void* stream);

/* The fused rollout step: bez_ppo_policy_forward followed, inside the same launch, by bez_ppo_rollout_pre's work (rollout-buffer
 * rows of obs / dones / mu / de-normalised value, a = mu + exp(logstd) * noise, neglogp, the clamped env action).  mu / value
 * never visit HBM in fp16; replaces a2c_common.py:1105-1135's per-step get_action_values + buffer updates.
 * prev_post (NULL = none; ABI 4): the bookkeeping of the env step BEFORE this one rides in the same launch -- exactly
 * bez_ppo_rollout_post(rew, reset, timeouts, prev_values, ...) on the env's still-unchanged reward / reset / time-out buffers, with
 * dones_f also written to this step's mb_dones row (dones_dev is then not read): a rollout step is two launches (policy, env). */
typedef struct BezPpoRolloutPost {
  const float* rew; const int64_t* reset; const int64_t* timeouts; const float* prev_values;
  float reward_scale, gamma; int32_t bootstrap;
  float* shaped; float* dones_f; float* cur_rew; float* cur_len; double* ep_stats;
  /* ABI 8 (NULL = the launch adds to ep_stats with atomics, as before): 4 doubles per workgroup of the launch (ceil(n / 32) of them at most), each
   * workgroup ADDS its finished episodes' (count, return sum, length sum) to its own slot -- no atomics: 128-256 workgroups adding to one cache line
   * cost the launch 1.7-3.2 us.  The caller adds the slots to ep_stats and clears them once per rollout. */
  double* ep_parts;
} BezPpoRolloutPost;
/* action_noise (NULL = none; ABI 4): the env's action-noise lambda of the domain randomisation inside this launch -- env_actions_dev receives
 * clamp(a, -1, 1) + noise, bit for bit what bez_sim_add_dr_noise(which = 1) would add to the clamped actions (the three fields are what
 * bez_sim_action_noise_source returns; the env must then not add it again). */
typedef struct BezPpoActionNoise { const void* snap_dev; uint64_t seed; int64_t env_id_offset; } BezPpoActionNoise;
/* layout (NULL = contiguous rows; ABI 4): row strides, in floats, of the rollout rows this launch writes -- mb_obs (>= num_obs); mb_mu / actions /
 * sigma (>= num_actions); neglogp (>= 1).  Lets the caller point them INTO its env-major dataset tensors (row of env e at step n = e * H + n:
 * strides H * width), so that the dataset needs no transposing copies after the rollout. */
typedef struct BezPpoRolloutLayout { int64_t obs_row_stride, act_row_stride, scalar_stride; } BezPpoRolloutLayout;
/* dr_step (NULL = none; ABI 4): the block bez_sim_dr_step_args filled -- the coming env step's randomisation runs as ONE EXTRA workgroup of this
 * launch (it touches nothing the forward pass reads: the action noise comes from the snapshot), instead of a launch of its own in front of
 * the step. */
int bez_ppo_policy_rollout_step(const float* obs_dev, int64_t n, int32_t num_obs, const double* obs_mean_dev, const double* obs_var_dev, float obs_eps,
                                int32_t num_hidden, const void* const* hidden_w_f16_dev, const void* const* hidden_b_f16_dev, const int32_t* hidden_width,
                                const void* mu_w_f16_dev, const void* mu_b_f16_dev, int32_t num_actions, const void* value_w_f16_dev,
                                const void* value_b_f16_dev, const float* logstd_dev, const float* noise_dev, const float* dones_dev,
                                const double* value_mean_dev, const double* value_var_dev, float value_eps, float* mb_obs_dev, float* mb_dones_dev,
                                float* mb_mu_dev, float* mb_val_dev, float* actions_dev, float* env_actions_dev, float* neglogp_dev, float* sigma_dev,
                                int32_t weights_packed, const BezPpoRolloutPost* prev_post, const BezPpoActionNoise* action_noise,
                                const void* dr_step, const BezPpoRolloutLayout* layout, void* stream);

/* The forward half of a PPO minibatch step (a2c_common.py calc_gradients: model(batch) under autocast): bez_ppo_policy_forward
 * that also keeps what the backward pass needs -- x0 (n, num_obs) fp16 = the normalised, clamped input of the first Linear, and
 * act[i] (n, hidden_width[i]) fp16 = the output of ELU i.  num_obs and the widths must be even. */
int bez_ppo_policy_forward_train(const float* obs_dev, int64_t n, int32_t num_obs, const double* obs_mean_dev, const double* obs_var_dev, float obs_eps,
                                 int32_t num_hidden, const void* const* hidden_w_f16_dev, const void* const* hidden_b_f16_dev, const int32_t* hidden_width,
                                 const void* mu_w_f16_dev, const void* mu_b_f16_dev, int32_t num_actions, const void* value_w_f16_dev,
                                 const void* value_b_f16_dev, void* x0_f16_dev, void* const* act_f16_dev, float* mu_dev, float* value_dev, int32_t weights_packed, void* stream);

/* Gradient reductions of explicit-fp16 linear layers into the fp32 master gradient: the sum over `splits` split-K partial
 * products ([splits][n] fp16) and the bias gradient = column sums of dY ((rows, cols) fp16).  accumulate != 0 adds to out_dev. */
int bez_ppo_wgrad_sum(const void* partials_f16_dev, int32_t splits, int64_t n, float* out_dev, int32_t accumulate, void* stream);
int bez_ppo_colsum_f16(const void* y_f16_dev, int64_t rows, int32_t cols, float* out_dev, int32_t accumulate, void* stream);
/* The weight gradients of `nlayers` (<= 8) Linear layers in one launch pair (csrc/bez_wgrad.hip): dW_L (+)= dY_L^T X_L with dY_L
 * (rows, out_L) and X_L (rows, in_L) fp16 row-major, dW_L (out_L, in_L) fp32.  A split-K MFMA kernel over the output blocks of
 * all layers -- each split along the rows in proportion to the bytes it streams, ~250 workgroups in all -- writes fp32 partial
 * blocks into partial_dev (room for nsplit * sum(out_L * in_L) floats; it uses what the balance needs), a second kernel adds a
 * block's splits in fixed order (deterministic).  Replaces torch.bmm + bez_ppo_wgrad_sum of a2c_common.py's backward [ext].
 * bez_ppo_wgrad_plan lays the work out ONCE for a set of tensors into plan_host (BEZ_PPO_WGRAD_PLAN_BYTES bytes of host memory;
 * rows % 64 must be 0; -3 = shapes the kernel does not take, the caller keeps its GEMM path); the caller copies the plan to
 * device memory and calls bez_ppo_wgrad_run(plan_host, plan_dev, accumulate, stream) per step. */
#define BEZ_PPO_WGRAD_PLAN_BYTES 3072
int bez_ppo_wgrad_plan(const void* const* dy_f16_dev, const void* const* x_f16_dev, const int32_t* out_features, const int32_t* in_features,
                       float* const* dw_dev, int32_t nlayers, int64_t rows, int32_t nsplit, float* partial_dev, void* plan_host);
int bez_ppo_wgrad_run(const void* plan_host, const void* plan_dev, int32_t accumulate, void* stream);
/* Every second-stage reduction of a minibatch step's gradient in ONE launch (ABI 4): the split-K images of bez_ppo_wgrad_run called
 * with accumulate = 2 ("partial images only"), the per-workgroup bias column sums of bez_ppo_policy_backward called with bit 1 of
 * weights_packed set ("column sums only"; same partial_dev, rows, widths and gradient pointers as there) and the per-workgroup sums of
 * bez_ppo_loss called with bit 4 of clip_value set ("partials only"; same scratch_dev, batch = loss_rows, grad_logstd_dev, stats_dev).
 * Fixed-order sums, one writer per output element: with accumulate = 0 the launch WRITES all weight / bias / log-sigma gradients and
 * the five statistics, so nothing has to be cleared in front of a step. */
int bez_ppo_grad_reduce_all(const void* plan_host, const void* plan_dev, const float* bias_partial_dev, int64_t rows, int32_t num_hidden,
                            const int32_t* hidden_width, int32_t num_actions, float* const* bias_grad_dev, float* mu_bias_grad_dev,
                            float* value_bias_grad_dev, const float* loss_scratch_dev, int64_t loss_rows, float* grad_logstd_dev, float* stats_dev,
                            int32_t accumulate, float* norm_parts_dev, void* stream);
/* norm_parts_dev (NULL = none; used with accumulate = 0 only): receives per workgroup (sum of squares, count of non-finite values) of the
 * gradient elements that workgroup wrote -- bez_ppo_grad_reduce_blocks(...) pairs of floats -- for bez_ppo_adam_step (BezPpoAdamExtra). */
int bez_ppo_grad_reduce_blocks(const void* plan_host, int32_t num_hidden, const int32_t* hidden_width, int32_t num_actions);
/* ELU (alpha 1) backward fused with the bias gradient: gz = gy * elu'(y) from the layer's ELU OUTPUT y, all (rows, cols) fp16;
 * the column sums of gz go to bias_grad_dev (fp32, cols). */
int bez_ppo_elu_bwd_colsum_f16(const void* gy_f16_dev, const void* y_f16_dev, void* gz_f16_dev, int64_t rows, int32_t cols, float* bias_grad_dev,
                               int32_t accumulate, void* stream);

/* The input-gradient half of a PPO minibatch's backward pass in one launch (torch autograd through the actor-critic MLP of
 * a2c_common.py calc_gradients): from d loss / d mu (n, A) and d loss / d value (n, 1) to gz[i] (n, hidden_width[i]) fp16 = d loss / d
 * (pre-activation of hidden layer i), using the ELU outputs act[i] kept by bez_ppo_policy_forward_train.  Also written: the fp16 casts of
 * the two loss gradients (operands of the head weight-gradient GEMMs); ADDED by atomics: the bias gradients of every hidden layer and of the
 * two heads.  Weight operands are transposed fp16 copies: wt[i] = W_i^T (hidden_width[i-1], hidden_width[i]) for i >= 1 (wt[0] unused) and
 * heads_t (hidden_width[last], 32) = [Wmu^T | Wvalue^T | 0]; bez_ppo_scatter_f16 refreshes them from a flat fp16 copy through an index map.
 * partial_dev: scratch of ceil(n / 64) * (sum(hidden_width) + 32) floats (per-workgroup column sums of the hidden layers and of the
 * two heads, added in fixed order by a second small launch: every bias gradient is bit-reproducible).
 * Widths even, 32 <= width <= 416. */
int bez_ppo_policy_backward(const float* grad_mu_dev, const float* grad_value_dev, int64_t n, int32_t num_hidden, const int32_t* hidden_width,
                            int32_t num_actions, const void* const* act_f16_dev, const void* const* wt_f16_dev, const void* heads_t_f16_dev,
                            void* const* gz_f16_dev, void* grad_mu_f16_dev, void* grad_value_f16_dev, float* const* bias_grad_dev,
                            float* mu_bias_grad_dev, float* value_bias_grad_dev, float* partial_dev, int32_t weights_packed, void* stream);
int bez_ppo_scatter_f16(const void* src_f16_dev, const int32_t* map_dev, int64_t n, void* dst_f16_dev, void* stream); /* dst[map[i]] = src[i], map[i] >= 0 */
int bez_ppo_scatter2_f16(const void* src_f16_dev, const int32_t* map_a_dev, const int32_t* map_b_dev, int64_t n, void* dst_f16_dev, void* stream);

/* weights_packed (last int argument of the four bez_ppo_policy_* functions above): 0 = the weight pointers are the row-major (out, in) fp16
 * matrices of nn.Linear (transposed ones for the backward function, as described there); 1 = they are FRAGMENT-MAJOR copies: for a Linear
 * (out, in), block nb = n / 32 and k-step ks = k / 16 form one 1 KB chunk at halfs ((nb * ceil(in / 16) + ks) * 512), in which element
 * (n, k) sits at ((k / 8 % 2) * 32 + n % 32) * 8 + k % 8, zero-padded beyond out / in -- a wave's MFMA B fragment as one coalesced load.
 * Forward: hidden_w[i] packs W_i, mu_w packs the (num_actions + 1, width_last) matrix [W_mu; W_value] (value_w unused).  Backward: wt[i]
 * packs W_i^T as a Linear (out = hidden_width[i-1], in = hidden_width[i]), heads_t packs [W_mu; W_value]^T as (out = width_last, in = 32).
 * bez_ppo_scatter2_f16 refreshes both sets from one flat fp16 copy of the parameters (two index maps) in one launch. */

/* rl_games AdaptiveScheduler.update (the `lr_schedule: adaptive` rule of bez_kickPPO.yaml) on device scalars: *lr /= 1.5 when *kl > 2 *
 * kl_threshold (floor min_lr), then *lr *= 1.5 when *kl < kl_threshold / 2 (cap max_lr).  No host round trip. */
int bez_ppo_adaptive_lr(float* lr_dev, const float* kl_dev, float kl_threshold, float min_lr, float max_lr, void* stream);

/* GAE (rl_games a2c_common.py discount_values, called from play_steps): advantages (H,N) from rewards / values (H,N), the done
 * flags recorded BEFORE each step (H,N), the current done flags (N) and the bootstrap values (N); returns_dev (optional) = advantages +
 * values.  One thread per env, the reference's operation order.  value_mean_dev != NULL: last_values_dev holds the network's NORMALISED
 * value outputs and the kernel de-normalises them first (RunningMeanStd(unnorm=True): clamp +-5, * sqrt(var + eps), + mean). */
int bez_ppo_gae(const float* rewards_dev, const float* values_dev, const float* mb_dones_dev, const float* dones_dev, const float* last_values_dev,
                int32_t horizon, int64_t num_envs, float gamma, float tau, float* advantages_dev, float* returns_dev, const double* value_mean_dev,
                const double* value_var_dev, float value_eps, void* stream);

/* bez_ppo_loss + bez_ppo_policy_backward of one minibatch as ONE launch: every 64-row tile forms its loss terms and d loss / d mu,
 * d loss / d value in front of the backward chain (the same code, the same bits), which reads them from on-chip memory.  The loss's per-
 * workgroup partial sums go to loss->scratch_dev (bez_ppo_loss's scratch, bit 4 semantics: bez_ppo_grad_reduce_all writes d loss / d
 * log-sigma and the statistics); weights_packed_flags must carry bits 0 and 1 (fragment-major weights, column sums only).  clip_value: bits 0
 * and 3 of bez_ppo_loss.  -3: a shape the fused kernel is not instantiated for (it exists for num_actions == 18 and hidden layers that fit
 * the two-workgroups-per-CU tiles) -- the caller keeps the two separate calls. */
typedef struct BezPpoLossOperands {
  const float* mu_dev; const float* logstd_dev; const float* value_dev; const float* actions_dev; const float* old_logp_dev; const float* adv_dev;
  const float* old_value_dev; const float* returns_dev; const float* old_mu_dev; const float* old_sigma_dev;
  float e_clip, critic_coef, entropy_coef, bounds_coef;
  int32_t clip_value;
  const float* loss_scale_dev;
  float* scratch_dev;
} BezPpoLossOperands;
int bez_ppo_policy_backward_with_loss(const BezPpoLossOperands* loss, int64_t n, int32_t num_hidden, const int32_t* hidden_width, int32_t num_actions,
                                      const void* const* act_f16_dev, const void* const* wt_f16_dev, const void* heads_t_f16_dev, void* const* gz_f16_dev,
                                      void* grad_mu_f16_dev, void* grad_value_f16_dev, float* const* bias_grad_dev, float* mu_bias_grad_dev,
                                      float* value_bias_grad_dev, float* partial_dev, int32_t weights_packed_flags, void* stream);

/* The epoch's dataset preparation between GAE and the first minibatch (rl_games a2c_continuous.py prepare_dataset [ext], called from
 * train_epoch via train.py:89-113, + the per-minibatch moments RunningMeanStd absorbs at every training forward) in four launches:
 *   - obs_moments_dev[i] (2 num_obs + 1 doubles: column sums, sums of squares, rows) of minibatch i's rows of obs_dev
 *     ((num_minibatches * minibatch_rows, num_obs) fp32), and value_moments_dev / return_moments_dev (3 doubles) of values_dev / returns_dev
 *     ((horizon, num_envs) fp32, the rollout's layout);
 *   - with value_mean_dev != NULL, RunningMeanStd.forward in train mode on the values, then on the returns: update with the values' moments,
 *     normalise the values (clamp +-5), update with the returns' moments, normalise the returns; the statistics (mean / var / count
 *     doubles) are updated in place;
 *   - old_values_dev, ds_returns_dev, advantages_dev (horizon * num_envs fp32, ENV-major: row e * horizon + t, swap_and_flatten01's order):
 *     the normalised values / returns and advantage = return - value, normalised as (adv - mean) / (std + 1e-8) (torch's unbiased std)
 *     when normalize_advantage != 0.
 * Every sum is a fixed-order two-stage fp64 sum (bit-reproducible).  scratch_dev: (num_minibatches + 2) * 256 * 128 + 2 * ceil(horizon *
 * num_envs / 256) doubles at most.  -3: horizon * num_envs is not a multiple of 64 (the caller keeps its separate launches). */
int bez_ppo_dataset_prep(const float* obs_dev, int64_t minibatch_rows, int32_t num_minibatches, int32_t num_obs, double* obs_moments_dev,
                         const float* values_dev, const float* returns_dev, int32_t horizon, int64_t num_envs, double* value_mean_dev, double* value_var_dev,
                         double* value_count_dev, float value_eps, double* value_moments_dev, double* return_moments_dev, float* old_values_dev,
                         float* ds_returns_dev, float* advantages_dev, int32_t normalize_advantage, double* scratch_dev, int64_t scratch_doubles, void* stream);

/* The same work in STAGES, for the data-parallel loop, whose two per-epoch collectives sit between them -- every moment above is
 * a plain sum (sum x, sum x^2, count), so an all-reduce of the local moments yields the global batch's:
 *   stage 1  the observation / value / return moments of THIS rank's rows                 (2 launches)   -> all-reduce of the moment buffers
 *   stage 2  value-normaliser statistics from the (now global) moments, normalised values / returns, advantages, and adv_sums_dev[0..2] =
 *            (sum adv, sum adv^2, count) of this rank's rows                              (2 launches)   -> all-reduce of adv_sums_dev
 *   stage 4  advantage normalisation with the (now global) adv_sums_dev; commits the value normaliser's statistics       (1 launch)
 * `stages` is a bit mask; 1 | 2 | 4 with adv_sums_dev == NULL is bez_ppo_dataset_prep.  The paths differ by the collectives only. */
int bez_ppo_dataset_prep_staged(int32_t stages, const float* obs_dev, int64_t minibatch_rows, int32_t num_minibatches, int32_t num_obs,
                                double* obs_moments_dev, const float* values_dev, const float* returns_dev, int32_t horizon, int64_t num_envs,
                                double* value_mean_dev, double* value_var_dev, double* value_count_dev, float value_eps, double* value_moments_dev,
                                double* return_moments_dev, float* old_values_dev, float* ds_returns_dev, float* advantages_dev,
                                int32_t normalize_advantage, double* adv_sums_dev, double* scratch_dev, int64_t scratch_doubles, void* stream);

/* The backward inputs of the two heads in one pass over the loss gradients (torch.autocast's cast nodes + the bias-gradient sums of
 * nn.Linear's backward): fp16 copies of d loss / d mu (rows, num_actions) and d loss / d value (rows, 1), and the column sums of those
 * fp16 values ADDED to the fp32 bias gradients of the mu and value heads. */
int bez_ppo_head_grads_f16(const float* grad_mu_dev, const float* grad_value_dev, int64_t rows, int32_t num_actions, void* grad_mu_f16_dev,
                           void* grad_value_f16_dev, float* mu_bias_grad_dev, float* value_bias_grad_dev, void* stream);

/* The optimiser tail of one minibatch step on flat fp32 buffers of n elements (replaces rl_games' scaler.unscale_ +
 * clip_grad_norm_ + scaler.step(Adam) + scaler.update, a2c_common.py [ext] via train.py:89-113): the gradient is divided by
 * *scale_dev (NULL = no loss scaling), clipped to max_norm (<= 0: no clipping), applied with torch's Adam formula; a non-finite
 * gradient skips the step and backs the scale off, growth_interval clean steps grow it.  steps_dev[nsteps] are the per-tensor
 * step counters of the optimiser state (all equal).  ONE launch (ABI 4; three before): every workgroup forms the squared norm of
 * the whole gradient itself, in the same fixed order (no float atomics: the clip coefficient, and with it every weight, is
 * bit-identical run to run and rank to rank), updates its slice, and the workgroup that draws the last ticket commits the step
 * counters / loss scale / learning rate after every other workgroup has read the old ones.  work_dev[BEZ_PPO_ADAM_WORK_FLOATS]:
 * [0] is that ticket counter -- ZERO on entry (allocate it zeroed), zero again on return (no memset per step).  grads_dev must be
 * 16-byte aligned.
 * params_f16_dev (NULL or n fp16): receives the updated parameters as fp16 in the same pass (the AMP working copy).
 * ntail (0..4) bookkeeping sums ride in the last launch: *tail_dst_dev[i] += *tail_src_dev[i] * tail_scale[i] (host arrays of
 * device pointers / host floats) -- the epoch's KL and loss accumulators of a2c_common.py's train_epoch [ext].
 * adapt_kl_dev (NULL = off): after the step, *lr_dev moves by rl_games' AdaptiveScheduler rule on *adapt_kl_dev (lr /= 1.5 above
 * 2 x adapt_kl_threshold, floor min_lr; lr *= 1.5 below half of it, cap max_lr) -- the 'legacy' schedule, once per minibatch step.
 * extra (NULL = none): work of neighbouring launches folded into this one -- (a) the fragment-major fp16 weight copies the MFMA
 * policy kernels read: packed_f16_dev[map_a_dev[i]] = packed_f16_dev[map_b_dev[i]] = fp16(param i) (negative map entry: no copy), what
 * bez_ppo_scatter2_f16 does from params_f16_dev; (b) the input normaliser's update for the NEXT minibatch, what bez_ppo_rms_apply
 * does from rms_moments_dev (rms_cols <= 1024); (c) the squared norm and non-finite count taken from the per-workgroup shares the
 * gradient's producer left instead of reading the gradient once more in every workgroup. */
typedef struct BezPpoAdamExtra {
  const float* norm_parts_dev; int32_t norm_parts; /* (c) the norm_parts pairs bez_ppo_grad_reduce_all (or bez_ppo_grad_norm_parts) left for THIS gradient */
  float grad_div;                                  /* data parallel: the gradient buffer holds the SUM over this many ranks (an all-reduce); 0 = 1.
                                                      Folded into the unscale factor: no separate division pass over the buffer */
  float* grid_norm_dev;                            /* data parallel, instead of norm_parts_dev: BEZ_PPO_ADAM_GRIDNORM_FLOATS zero-initialised floats; the launch
                                                      forms the norm itself -- every workgroup sums its own slice, the workgroups meet at a counter in this
                                                      buffer (all of them are co-resident: <= 256 workgroups), each adds the shares in the same fixed order --
                                                      and leaves the counter at zero.  No extra launch, no workgroup reads the whole gradient */
  const int32_t* map_a_dev; const int32_t* map_b_dev; void* packed_f16_dev;
  const double* rms_moments_dev; int32_t rms_cols; double* rms_mean_dev; double* rms_var_dev; double* rms_count_dev;
} BezPpoAdamExtra;
/* Data parallel: an all-reduce has replaced the gradient bez_ppo_grad_reduce_all left its norm shares for.  One small launch re-forms them
 * (workgroup b: sum g^2 and non-finite count of its slice of the n-element buffer, fixed order) so that the optimiser launch reads `parts`
 * pairs instead of the whole gradient in every workgroup.  parts_dev: 2 * parts floats; returns the number of pairs written (<= parts). */
int bez_ppo_grad_norm_parts(const float* grads_dev, int64_t n, float* parts_dev, int32_t parts, void* stream);
#define BEZ_PPO_ADAM_WORK_FLOATS 258
#define BEZ_PPO_ADAM_GRIDNORM_FLOATS 516
/* How many workgroups of bez_ppo_adam_step's launch can be resident on the current device at once (occupancy x compute units), and how
 * many the launch uses for n parameters.  With BezPpoAdamExtra.grid_norm_dev the launch's workgroups meet at a counter: that is only safe
 * when all of them are co-resident (a CU-masked or partitioned device, a smaller part, two ranks on one GPU can break the assumption) --
 * bez_ppo_adam_step then returns -6 instead of launching, and the caller falls back to bez_ppo_grad_norm_parts (PPO ABI 9). */
int bez_ppo_adam_grid_capacity(int64_t n, int32_t* resident_workgroups, int32_t* launch_workgroups);
int bez_ppo_adam_step(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n, float* steps_dev,
                      int32_t nsteps, float* lr_dev, float beta1, float beta2, float eps, float weight_decay, float max_norm, float* scale_dev,
                      int32_t* growth_tracker_dev, float growth_factor, float backoff_factor, int32_t growth_interval, float* work_dev,
                      void* params_f16_dev, int32_t ntail, float* const* tail_dst_dev, const float* const* tail_src_dev, const float* tail_scale,
                      const float* adapt_kl_dev, float adapt_kl_threshold, float min_lr, float max_lr, const BezPpoAdamExtra* extra, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEZ_SIM_H */
