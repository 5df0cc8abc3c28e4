"""ctypes mirror of include/bez_sim.h (the C ABI of libbez_sim.so).

Only declarations live here: struct layout, enums, and the default `BezSimConfig` for
`bez_kick` (values: bez_isaacgym/cfg/task/bez_kick.yaml:11-147, kick_env.py:322-329 of the
reference).  Loading / calling the library is in `bez_isaacgym_amd.sim`.
"""
import ctypes as C
import math

ABI_VERSION = 5
NUM_OBS = 54
NUM_ACTIONS = 18
NUM_DOFS = 18
NUM_BODIES = 22
NUM_ACTORS = 2
NUM_LINKS = 19

FLAG_IMU_PREV_ALIAS = 1
FLAG_CF_WITH_FRICTION = 2
FLAG_CF_LAST_SUBSTEP = 4
FLAG_NO_SELF_COLLISION = 8
FLAG_CLEATS = 16
FLAG_BOX_ASSET = 32
FLAG_HARD_CONTACT = 64
FLAG_LEAN_STEP = 128
FLAG_OBS_NOISE_IN_STEP = 256
FLAG_TGS_SOLVER = 512
FLAG_ANKLE_STOP = 1024          # scenario harness: calf <-> foot-plate contact (one-env-per-lane kernel, stl asset without cleats)
FLAG_ALL_GROUND_SHAPES = 2048   # scenario harness: ground contact at every collision shape's corners (same)
FLAG_FIX_BASE = 4096            # urdfAsset.fixBaseLink: the torso welded to the world
FLAG_NONFINITE_GUARD = 8192     # per-env non-finite guard of the post-physics (on by default; include/bez_sim.h)
FLAG_REWARD_TERMS = 16384       # env.debug.rewards: per-env sums of the reward's terms (EPISODE_REWARD_TERMS; off by default)
FLAG_DOF_FORCE = 32768          # env.enableDofForceSensors: the step kernels record joint forces / drive torques / actuator status (off by default)
# actuator tensors (include/bez_sim.h BezActuatorTensor, BezSim.actuator_tensor), DOF_STATE order, present with FLAG_DOF_FORCE only
ACTUATOR_DOF_FORCE, ACTUATOR_DRIVE_TORQUE, ACTUATOR_STATUS, ACTUATOR_TENSORS = range(4)
ACTUATOR_SATURATED_POS, ACTUATOR_SATURATED_NEG, ACTUATOR_LOCKED_POS, ACTUATOR_LOCKED_NEG = 1, 2, 4, 8
ACTUATOR_SATURATED = ACTUATOR_SATURATED_POS | ACTUATOR_SATURATED_NEG
ACTUATOR_LOCKED = ACTUATOR_LOCKED_POS | ACTUATOR_LOCKED_NEG
# dynamics tensors (include/bez_sim.h BezDynamicsTensor, BezSim.dynamics_tensor): the robot's Jacobian (N*NB, 6, NUM_GEN) and mass matrix
# (N, NUM_GEN, NUM_GEN) in the generalised velocity [root_lin 3, root_ang 3, qd 18]; allocated on first acquisition
DYNAMICS_JACOBIAN, DYNAMICS_MASS_MATRIX, DYNAMICS_COUNT = range(3)
NUM_GEN = 24
# bez_sim_inverse_dynamics (include/bez_sim.h "Inverse dynamics", BezSim.inverse_dynamics): the terms of M(q) udot + h(q, u) to add up
ID_INERTIA, ID_VELOCITY, ID_GRAVITY = 1, 2, 4
ID_ALL = 7
# bez_sim_forward_dynamics (include/bez_sim.h "Forward dynamics", BezSim.forward_dynamics): udot = M^-1 (f - h); `bias` is a subset of
# ID_VELOCITY | ID_GRAVITY, the mode bit holds the root and solves the joint block alone
FD_FIXED_BASE = 1
# bez_sim_centroidal (include/bez_sim.h "Centroidal dynamics", BezSim.centroidal): the words of a (N, CM_WORDS) state row; the momentum
# matrix is (N, 6, NUM_GEN) with rows [linear momentum 3; angular momentum about the centre of mass 3]
CM_WORDS = 16
CM_COM, CM_COM_VEL, CM_LIN_MOM, CM_ANG_MOM, CM_MASS, CM_KINETIC, CM_POTENTIAL = 0, 3, 6, 9, 12, 13, 14
# bez_sim_body_accelerations (include/bez_sim.h "Body accelerations", BezSim.body_accelerations): the terms of J udot + Jdot u - g to add up
ACC_UDOT, ACC_VELOCITY, ACC_GRAVITY = 1, 2, 4
ACC_MOTION, ACC_ALL = 3, 7
DOF_FORCE_KEY = "env.enableDofForceSensors"   # this build's task key for FLAG_DOF_FORCE (default False)
SPACE_ENV = 0                   # bez_sim_apply_body_forces: world axes / world points (gymapi.ENV_SPACE)
SPACE_LOCAL = 1                 # the body's own frame (gymapi.LOCAL_SPACE)
GF_AT_ORIGIN = 2                # bez_sim_generalized_forces only, OR-ed into the space: without positions, wrenches act at the bodies' origins
# bez_sim_limb_ik (include/bez_sim.h "Limb inverse kinematics", BezSim.limb_ik): the five chains off the torso in the order of their first
# DOF, their DOF ranges and end bodies; targets are (N, IK_CHAINS, 7) [position, quaternion xyzw], errors (N, IK_CHAINS, 6)
IK_CHAINS = 5
IK_SPACE_ENV, IK_SPACE_ROOT = 0, 1
IK_MAX_ITERS = 64
IK_CHAIN_NAMES = ("head", "left_arm", "left_leg", "right_arm", "right_leg")
IK_CHAIN_DOFS = ((0, 2), (2, 4), (4, 10), (10, 12), (12, 18))
IK_END_BODIES = ("/head", "/left_forearm", "/left_foot", "/right_forearm", "/right_foot")
# bez_sim_proximity (include/bez_sim.h "Proximity", BezSim.proximity): ground (N, PROX_GROUND_ROWS, 3), ball (N, PROX_BOXES, PROX_WORDS),
# pairs (N, PROX_PAIRS, PROX_WORDS); a row of PROX_WORDS is [gap, normal 3, point 3, 0].  The names follow bez_model.json: a ground point
# is "<kind><link>_<its index among the link's points>" (the cleats asset's foot points are its cleats, in the same rows)
PROX_GROUND_ROWS, PROX_BALL_ROW, PROX_BOXES, PROX_PAIRS, PROX_WORDS = 23, 22, 11, 28, 8
PROX_GAP, PROX_NORMAL, PROX_POINT = 0, 1, 4
PROX_GROUND_NAMES = (tuple("foot/%s_foot_%d" % (s, i) for s in ("left", "right") for i in range(4)) + tuple("guard/torso_%d" % i for i in range(8))
                     + tuple("guard/head_%d" % i for i in range(4)) + ("guard/left_forearm_0", "guard/right_forearm_0"))
_PROX_LEG = ("hip_front", "thigh", "calve", "ankle", "foot")
PROX_BOX_BODIES = tuple("/%s_%s" % (s, p) for s in ("left", "right") for p in _PROX_LEG) + ("/torso",)
_PROX_CAPSULES = tuple("/%s_%s" % (s, p) for s in ("left", "right") for p in _PROX_LEG + ("foot",))   # two capsules per foot
PROX_PAIRS_CAPSULES = ((0, 6), (0, 7)) + tuple((1, b) for b in range(6, 12)) + tuple((a, b) for a in range(2, 6) for b in range(7, 12))
PROX_PAIR_BODIES = tuple((_PROX_CAPSULES[a], _PROX_CAPSULES[b]) for a, b in PROX_PAIRS_CAPSULES)
# query states (include/bez_sim.h "Query states", BezSim.query_state): the tensors a query state owns, (1 << id) in a refresh mask, and the
# four parameter rows (PARAM_* below) it copies row by row
QUERY_RIGID_BODY_STATE, QUERY_JACOBIAN, QUERY_MASS_MATRIX, QUERY_TENSOR_COUNT = range(4)
QUERY_PARAMS = (3, 4, 5, 6)     # PARAM_MASS_SCALE, PARAM_GRAVITY, PARAM_DOF_LOWER, PARAM_DOF_UPPER
# env snapshots (include/bez_sim.h "Env snapshots", BezSim.snapshot): the `what` bits of a restore, the blob's header, and the sections of
# a row in the blob's order -- each a run of uint32 columns (width, rows), a 64-bit item as (low, high)
SNAPSHOT_ENVS, SNAPSHOT_GLOBALS = 1, 2
SNAPSHOT_MAGIC, SNAPSHOT_LAYOUT, SNAPSHOT_HEADER_WORDS, SNAPSHOT_GLOBAL_WORDS = 0x4e535a42, 1, 40, 16
SNAPSHOT_SECTIONS = ("state", "obs", "rew", "reset", "progress", "timeout", "episode", "randomize", "nonfinite", "end_counts", "reward_terms", "end_bits",
                     "param_friction", "param_kp_scale", "param_kd_scale", "param_mass_scale", "param_gravity", "param_dof_lower", "param_dof_upper",
                     "dof_force_record")
HEALTH_NONFINITE = 1            # health word bits (TENSOR_HEALTH, BezSim.health)
HEALTH_SPIN_TIMEOUT = 2
TASK_KICK, TASK_WALK, TASK_ORIENT = 0, 1, 2
TASK_IDS = {"bez_kick": TASK_KICK, "bez_walk": TASK_WALK, "bez_orient": TASK_ORIENT}

(TENSOR_ROOT_STATE, TENSOR_DOF_STATE, TENSOR_RIGID_BODY_STATE, TENSOR_NET_CONTACT_FORCE, TENSOR_OBS,
 TENSOR_REW, TENSOR_RESET, TENSOR_PROGRESS, TENSOR_TIMEOUT, TENSOR_DOF_TARGET, TENSOR_PREV_LIN_VEL,
 TENSOR_FEET, TENSOR_GOAL, TENSOR_RANDOMIZE_BUF, TENSOR_DR_NOISE, TENSOR_NONFINITE_COUNT, TENSOR_HEALTH, TENSOR_COUNT) = range(18)
DTYPE_F32, DTYPE_I64, DTYPE_I32 = 0, 1, 2
# episode statistics (include/bez_sim.h BezEpisodeTensor, BezSim.episode_tensor): why episodes end, and the reward's terms
EPISODE_END_BITS, EPISODE_END_COUNTS, EPISODE_REWARD_TERMS, EPISODE_TENSORS = range(4)
# cause codes: code k has bit 1 << k in EPISODE_END_BITS and row k in EPISODE_END_COUNTS
(END_CARRIED, END_FALL, END_OUT_OF_BOUNDS, END_OFF_COURSE, END_GOAL, END_TIMEOUT, END_NONFINITE) = range(7)
END_CAUSES = 8
END_NAMES = ("carried", "fall", "out_of_bounds", "off_course", "goal", "timeout", "nonfinite", "reserved")
# the deciding cause: the last test that fired in the reference's order, per task (CARRIED only when none did; NONFINITE always)
END_ORDER = {TASK_KICK: (END_FALL, END_OUT_OF_BOUNDS, END_OFF_COURSE, END_GOAL, END_TIMEOUT),
             TASK_WALK: (END_FALL, END_GOAL, END_OFF_COURSE, END_TIMEOUT),
             TASK_ORIENT: (END_FALL, END_GOAL, END_OUT_OF_BOUNDS, END_TIMEOUT)}
REWARD_TERM_SLOTS = 8
REWARD_TERM_TERMINAL = 5   # the slot that holds a terminating step's reward


def end_cause(task, bits):
    """The deciding cause code of a nonzero EPISODE_END_BITS word (include/bez_sim.h)."""
    if bits & (1 << END_NONFINITE):
        return END_NONFINITE
    for k in reversed(END_ORDER[int(task)]):
        if bits & (1 << k):
            return k
    return END_CARRIED
(PARAM_FRICTION, PARAM_KP_SCALE, PARAM_KD_SCALE, PARAM_MASS_SCALE, PARAM_GRAVITY, PARAM_DOF_LOWER, PARAM_DOF_UPPER,
 PARAM_COUNT) = range(8)
PARAM_WIDTH = {PARAM_FRICTION: 1, PARAM_KP_SCALE: 18, PARAM_KD_SCALE: 18, PARAM_MASS_SCALE: 19, PARAM_GRAVITY: 3,
               PARAM_DOF_LOWER: 18, PARAM_DOF_UPPER: 18}


class BezSimConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("num_envs", C.c_int32),
        ("substeps", C.c_int32),
        ("max_episode_length", C.c_int32),
        ("dt", C.c_float),
        ("gravity", C.c_float * 3),
        ("kp", C.c_float),
        ("kd", C.c_float),
        ("armature", C.c_float),
        ("effort", C.c_float),
        ("vel_limit", C.c_float),
        ("joint_friction", C.c_float),
        ("plane_friction", C.c_float),
        ("clip_actions", C.c_float),
        ("bez_init", C.c_float * 7),
        ("ball_init", C.c_float * 7),
        ("goal", C.c_float * 2),
        ("contact_kn", C.c_float),
        ("contact_cn", C.c_float),
        ("contact_ct", C.c_float),
        ("contact_veps", C.c_float),
        ("limit_k", C.c_float),
        ("limit_d", C.c_float),
        ("jfric_veps", C.c_float),
        ("ball_ang_damping", C.c_float),
        ("self_kn", C.c_float),
        ("self_cn", C.c_float),
        ("ball_kn", C.c_float),
        ("ball_cn", C.c_float),
        ("tune", C.c_float * 24),
        ("task", C.c_int32),
        ("goal_angle", C.c_float),
        ("flags", C.c_uint32),
        ("seed", C.c_uint64),
        ("env_id_offset", C.c_int64),
    ]

    def as_dict(self):
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            out[name] = list(v) if hasattr(v, "__len__") else v
        return out


class BezDrRange(C.Structure):
    _fields_ = [("a", C.c_float), ("b", C.c_float), ("enabled", C.c_int32), ("schedule_steps", C.c_int32)]


class BezDrConfig(C.Structure):
    """device-side domain randomisation (include/bez_sim.h); one BezDrRange per entry of bez_kick.yaml:151-219"""
    _fields_ = [("frequency", C.c_int32), ("friction_buckets", C.c_int32), ("friction", BezDrRange), ("stiffness", BezDrRange),
                ("damping", BezDrRange), ("lower", BezDrRange), ("upper", BezDrRange), ("gravity", BezDrRange),
                ("observations", BezDrRange), ("actions", BezDrRange)]


def dr_config_from_params(dr_params):
    """randomization_params of cfg/task/bez_kick.yaml:151-219 -> BezDrConfig.  Distribution / operation per parameter are the ones
    that file uses; anything else is refused rather than silently reinterpreted."""
    d = BezDrConfig()
    d.frequency = int(dr_params.get("frequency", 1))

    def put(dst, attr, dist, op):
        if attr is None:
            return
        if attr.get("distribution") != dist or attr.get("operation") != op:
            raise ValueError("domain randomisation: %s must be %s / %s as in bez_kick.yaml (got %s / %s)" % (dst, dist, op, attr.get("distribution"), attr.get("operation")))
        r = getattr(d, dst)
        r.a, r.b = float(attr["range"][0]), float(attr["range"][1])
        r.enabled = 1
        sch = attr.get("schedule")
        if sch not in (None, "linear"):
            raise ValueError("domain randomisation: only `schedule: linear` is supported (%s)" % dst)
        r.schedule_steps = int(attr["schedule_steps"]) if sch == "linear" else 0
    put("observations", dr_params.get("observations"), "gaussian", "additive")
    put("actions", dr_params.get("actions"), "gaussian", "additive")
    put("gravity", (dr_params.get("sim_params") or {}).get("gravity"), "gaussian", "additive")
    ap = ((dr_params.get("actor_params") or {}).get("bez") or {})
    fr = (ap.get("rigid_shape_properties") or {}).get("friction")
    put("friction", fr, "uniform", "scaling")
    d.friction_buckets = int((fr or {}).get("num_buckets", 0) or 0)
    dp = ap.get("dof_properties") or {}
    put("stiffness", dp.get("stiffness"), "uniform", "scaling")
    put("damping", dp.get("damping"), "uniform", "scaling")
    put("lower", dp.get("lower"), "gaussian", "additive")
    put("upper", dp.get("upper"), "gaussian", "additive")
    return d


# Contact / limit model constants of this build (no reference counterpart; DESIGN.md "Physics model")
CONTACT_DEFAULTS = dict(contact_kn=2.0e4, contact_cn=20.0, contact_ct=1.0e3, contact_veps=0.01,
                        limit_k=200.0, limit_d=2.0, jfric_veps=0.1, ball_ang_damping=0.5,
                        self_kn=2.0e4, self_cn=5.0, ball_kn=0.0, ball_cn=0.0)


def default_config(num_envs=4096, seed=42, env_id_offset=0):
    """bez_kick defaults; must agree field-for-field with bez_sim_default_config() in the library."""
    c = BezSimConfig()
    c.abi_version = ABI_VERSION
    c.num_envs = int(num_envs)
    c.substeps = 2
    c.dt = 0.01667
    c.max_episode_length = int(15.0 / 0.01667 + 0.5)  # kick_env.py:127 -> 900
    c.gravity[:] = [0.0, 0.0, -9.81]
    c.kp, c.kd = 100.0, 7.5
    c.armature = 0.001
    c.effort = 2.5
    c.vel_limit = 2.0 * math.pi
    c.joint_friction = 0.1
    c.plane_friction = 1.0
    c.clip_actions = 3.9
    c.bez_init[:] = [0.0, 0.0, 0.34, 0.0, 0.0, 0.0, 1.0]
    c.ball_init[:] = [0.175, 0.0, 0.1, 0.0, 0.0, 0.0, 1.0]
    c.goal[:] = [1.5, 0.0]
    for k, v in CONTACT_DEFAULTS.items():
        setattr(c, k, v)
    c.flags = FLAG_IMU_PREV_ALIAS | FLAG_NONFINITE_GUARD
    c.seed = int(seed)
    c.env_id_offset = int(env_id_offset)
    return c


def refuse_unmodelled(cfg):
    """Config keys the reference forwards to Isaac Gym that this build's rigid-body step does not model: a non-default value raises
    instead of being read and ignored (the defaults of bez_kick.yaml are what the kernels implement; fixBaseLink IS modelled: BEZ_FLAG_FIX_BASE).
    kick_env.py:250-256 (plane), :283-294 (asset options)."""
    env = cfg["env"]
    ua, plane = env.get("urdfAsset", {}), env.get("plane", {})

    def no(cond, key, value, why):
        if cond:
            raise ValueError("task config: %s = %r is not modelled by the HIP simulator (%s); only the value of the reference's "
                             "yaml is implemented" % (key, value, why))
    no(bool(ua.get("disable_gravity", False)), "env.urdfAsset.disable_gravity", ua.get("disable_gravity"),
       "gravity acts on every body; set sim.gravity to zero instead")
    for k in ("angular_damping", "linear_damping"):
        no(float(ua.get(k, 0.0)) != 0.0, "env.urdfAsset." + k, ua.get(k), "per-body velocity damping is not part of the step")
    no(float(plane.get("restitution", 0.0)) != 0.0, "env.plane.restitution", plane.get("restitution"), "contacts are inelastic")
    if "staticFriction" in plane and "dynamicFriction" in plane:
        no(float(plane["staticFriction"]) != float(plane["dynamicFriction"]), "env.plane.staticFriction", plane["staticFriction"],
           "one Coulomb coefficient (dynamicFriction) serves for both")
    # vec_task.py:90 reads env.controlFrequencyInv (the yaml's env.control.controlFrequencyInv is never read by the reference):
    # k simulate calls per env step, taken by KickEnv._fused_step through the split entry points
    cfi = int(env.get("controlFrequencyInv", 1))
    no(cfi < 1, "env.controlFrequencyInv", cfi, "must be >= 1")
    # this build's key for gym.enable_actor_dof_force_sensors: a switch, nothing else
    dfs = env.get("enableDofForceSensors", False)
    if not isinstance(dfs, bool):
        raise ValueError("task config: %s = %r must be True or False" % (DOF_FORCE_KEY, dfs))


def config_from_task_cfg(cfg, seed=42, env_id_offset=0, strict_reference_quirks=True, task="bez_kick"):
    """Build a BezSimConfig from the task config dict (the structure of cfg/task/bez_{kick,walk,orient}.yaml)."""
    env, sim = cfg["env"], cfg["sim"]
    refuse_unmodelled(cfg)
    c = default_config(int(env["numEnvs"]), seed=seed, env_id_offset=env_id_offset)
    c.task = TASK_IDS[task]
    c.goal_angle = float(env["goalState"].get("goal_angle", 0.0))
    c.substeps = int(sim.get("substeps", 2))
    c.dt = float(sim["dt"])
    c.max_episode_length = int(float(env["learn"]["episodeLength_s"]) / float(sim["dt"]) + 0.5)
    c.gravity[:] = [float(x) for x in sim["gravity"]]
    c.kp = float(env["control"]["stiffness"])
    c.kd = float(env["control"]["damping"])
    c.armature = float(env["urdfAsset"]["armature"])
    c.plane_friction = float(env["plane"]["dynamicFriction"])
    c.clip_actions = float(env.get("clipActions", float("inf")))
    c.bez_init[:] = [float(x) for x in env["bezInitState"]["pos"] + env["bezInitState"]["rot"]]
    if "ballInitState" in env:  # bez_walk / bez_orient have no ball actor
        c.ball_init[:] = [float(x) for x in env["ballInitState"]["pos"] + env["ballInitState"]["rot"]]
    c.goal[:] = [float(x) for x in env["goalState"]["goal"]]
    for k in CONTACT_DEFAULTS:
        if k in sim.get("bez", {}):
            setattr(c, k, float(sim["bez"][k]))
    for k in ("effort", "vel_limit", "joint_friction"):   # kick_env.py:322-329 hard-codes these; sim.bez.<k> overrides them for experiments
        if k in sim.get("bez", {}):
            setattr(c, k, float(sim["bez"][k]))
    c.flags = FLAG_IMU_PREV_ALIAS if strict_reference_quirks else 0
    if env.get("nonfiniteGuard", True):  # not a key of the reference's yaml: this build's per-env non-finite guard, on unless False
        c.flags |= FLAG_NONFINITE_GUARD
    if (env.get("debug") or {}).get("rewards", False):  # bez_kick.yaml:125-126 env.debug.rewards: the reward's terms per env (kick_env.py:584-600)
        c.flags |= FLAG_REWARD_TERMS
    if env.get("enableDofForceSensors", False):  # not a key of the reference's yaml (it enables the sensors in code, kick_env.py:368,375)
        c.flags |= FLAG_DOF_FORCE
    if env.get("asset", {}).get("cleats", False):
        c.flags |= FLAG_CLEATS
    if not env.get("asset", {}).get("stl", True):  # kick_env.py:266-276: soccerbot_box*.urdf
        c.flags |= FLAG_BOX_ASSET
    if env.get("urdfAsset", {}).get("fixBaseLink", False):  # kick_env.py:287
        c.flags |= FLAG_FIX_BASE
    return c


def _enum(value, names, ids, bad_name, bad_id):
    """The id of an enum value from the int or from its name (any case, blanks around it stripped; a bool is no int).  `names`: name -> id,
    `ids`: the ints taken as they are.  Anything else raises ValueError: `bad_name` % the value for a string, `bad_id` % it otherwise."""
    if isinstance(value, str):
        key = value.strip().lower()
        if key not in names:
            raise ValueError(bad_name % (value,))
        return names[key]
    if isinstance(value, bool) or not isinstance(value, int) or value not in ids:
        raise ValueError(bad_id % (value,))
    return int(value)


def _tensor_id(kind, names, which):
    """The id of a `kind` tensor from the int or from its name (any case); `names`: the names in id order."""
    return _enum(which, {k: i for i, k in enumerate(names)}, range(len(names)), "%s tensor must be one of %s, got %%r" % (kind, sorted(names)),
                 "%s tensor id must be in [0, %d), got %%r" % (kind, len(names)))


def actuator_tensor_id(which):
    """ACTUATOR_DOF_FORCE / ACTUATOR_DRIVE_TORQUE / ACTUATOR_STATUS from the int or from "dof_force" / "drive_torque" / "status"."""
    return _tensor_id("actuator", ("dof_force", "drive_torque", "status"), which)


def dynamics_tensor_id(which):
    """DYNAMICS_JACOBIAN / DYNAMICS_MASS_MATRIX from the int or from "jacobian" / "mass_matrix"."""
    return _tensor_id("dynamics", ("jacobian", "mass_matrix"), which)


_SPACE_NAMES = {"env": SPACE_ENV, "env_space": SPACE_ENV, "local": SPACE_LOCAL, "local_space": SPACE_LOCAL}
_AT_NAMES = {"com": 0, "origin": GF_AT_ORIGIN}
_IK_SPACE_NAMES = {"env": IK_SPACE_ENV, "root": IK_SPACE_ROOT}


def body_force_space(space):
    """SPACE_ENV / SPACE_LOCAL from the int or from "env" / "local" (any case); anything else raises ValueError."""
    return _enum(space, _SPACE_NAMES, (SPACE_ENV, SPACE_LOCAL), "space must be 'env' or 'local', got %r",
                 "space must be SPACE_ENV (0) or SPACE_LOCAL (1), got %r")


def generalized_force_space(space, at="com"):
    """the `space` word of bez_sim_generalized_forces: body_force_space(space), with GF_AT_ORIGIN OR-ed in for at="origin" (at="com",
    the default point of application of apply_body_forces, adds nothing); any other `at` raises ValueError."""
    at = _enum(at, _AT_NAMES, (), "at must be 'com' or 'origin', got %r", "at must be 'com' or 'origin', got %r")   # a name only
    return body_force_space(space) | at


class BezIkParams(C.Structure):
    """include/bez_sim.h BezIkParams, passed to bez_sim_limb_ik by pointer and to its kernel by value"""
    _fields_ = [
        ("weight", (C.c_float * 2) * IK_CHAINS),
        ("offset", (C.c_float * 3) * IK_CHAINS),
        ("damping", C.c_float),
        ("max_step", C.c_float),
        ("iters", C.c_int32),
        ("space", C.c_int32),
    ]


def ik_space(space):
    """IK_SPACE_ENV / IK_SPACE_ROOT from the int or from "env" / "root" (any case); anything else raises ValueError."""
    return _enum(space, _IK_SPACE_NAMES, (IK_SPACE_ENV, IK_SPACE_ROOT), "space must be 'env' or 'root', got %r",
                 "space must be IK_SPACE_ENV (0) or IK_SPACE_ROOT (1), got %r")


def _read_offsets(offsets, dst):
    """`offsets`, (IK_CHAINS, 3) and finite, into the `offset` field `dst` of a parameter struct; None leaves it zero"""
    if offsets is None:
        return
    try:
        rows = [list(r) for r in offsets]
    except TypeError:
        rows = None
    if rows is None or len(rows) != IK_CHAINS or any(len(r) != 3 for r in rows):
        raise ValueError("offsets must be (%d, 3) or None" % IK_CHAINS)
    for c, r in enumerate(rows):
        for k, o in enumerate(r):
            o = float(o)
            if not math.isfinite(o):
                raise ValueError("offsets[%d][%d] must be finite, got %r" % (c, k, o))
            dst[c][k] = o


def ik_params(weights, offsets=None, damping=0.05, max_step=0.0, iters=1, space=IK_SPACE_ENV):
    """The BezIkParams of a bez_sim_limb_ik call, every argument checked here (ValueError) before the library sees it.  weights:
    (IK_CHAINS, 2) [w_pos, w_rot] >= 0, finite; a chain with both 0 is not asked for.  offsets: (IK_CHAINS, 3), finite, or None for zero.
    damping: a positive finite number.  max_step: > 0 the largest |dq_i| of one iteration, <= 0 no limit; not NaN.  iters: an int in
    0 .. IK_MAX_ITERS.  space: ik_space()."""
    import operator
    p = BezIkParams()
    rows = [list(r) for r in weights] if weights is not None else None
    if rows is None or len(rows) != IK_CHAINS or any(len(r) != 2 for r in rows):
        raise ValueError("weights must be (%d, 2): [w_pos, w_rot] per chain (%s)" % (IK_CHAINS, ", ".join(IK_CHAIN_NAMES)))
    for c, r in enumerate(rows):
        for k, w in enumerate(r):
            w = float(w)
            if not math.isfinite(w) or w < 0.0:
                raise ValueError("weights[%d][%d] must be finite and >= 0, got %r" % (c, k, w))
            p.weight[c][k] = w
    _read_offsets(offsets, p.offset)
    damping, max_step = float(damping), float(max_step)
    if not math.isfinite(damping) or damping <= 0.0:
        raise ValueError("damping must be a positive finite number, got %r" % damping)
    if math.isnan(max_step):
        raise ValueError("max_step is NaN (<= 0 means no step limit)")
    try:   # any integer type (numpy and torch scalars included), never a bool or a float
        iters = None if isinstance(iters, bool) else operator.index(iters)
    except TypeError:
        iters = None
    if iters is None or not 0 <= iters <= IK_MAX_ITERS:
        raise ValueError("iters must be an integer in 0 .. %d" % IK_MAX_ITERS)
    p.damping, p.max_step, p.iters, p.space = damping, max_step, iters, ik_space(space)
    return p


class BezOpSpaceParams(C.Structure):
    """include/bez_sim.h BezOpSpaceParams, passed to bez_sim_operational_space by pointer and to its kernel by value"""
    _fields_ = [
        ("offset", (C.c_float * 3) * IK_CHAINS),
        ("mode", C.c_uint32),
    ]


def op_space_params(offsets=None, fixed_base=False):
    """The BezOpSpaceParams of a bez_sim_operational_space call, checked here (ValueError) before the library sees it.  offsets:
    (IK_CHAINS, 3), finite, or None for zero: the controlled frame of chain c is its end body (IK_END_BODIES) displaced by offsets[c] in that
    body's axes.  fixed_base: hold the root (FD_FIXED_BASE)."""
    p = BezOpSpaceParams()
    _read_offsets(offsets, p.offset)
    if not isinstance(fixed_base, (bool, int)):
        raise ValueError("fixed_base must be True or False, got %r" % (fixed_base,))
    p.mode = FD_FIXED_BASE if fixed_base else 0
    return p
