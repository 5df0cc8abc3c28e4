"""Env / VecTask base classes with the reference's public surface (bez_isaacgym/tasks/base/vec_task.py),
re-implemented over the HIP simulator: there is no gymapi, `gym.simulate` is libbez_sim.so.

Kept from the reference: constructor signature (vec_task.py:51,150), device parsing (:61-73), spaces
(:92-95), buffer names/dtypes/initial values (:226-249), step()/reset() return contract (:303-377),
zero_actions (:351-359), get_state (:287-289), properties (:122-145), domain-randomisation entry point
apply_randomizations (:505-725, here: per-env parameter arrays pushed to the kernel).
"""
import abc
from typing import Any, Dict, Tuple

import numpy as np
import torch


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is not a dependency): low/high/shape/dtype."""

    def __init__(self, low, high, dtype=np.float32):
        self.low = np.asarray(low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype)
        self.shape = self.low.shape
        self.dtype = np.dtype(dtype)

    def __repr__(self):
        return "Box(%s, %s, %s, %s)" % (self.low.min(), self.high.max(), self.shape, self.dtype)


class Env(abc.ABC):
    def __init__(self, config: Dict[str, Any], sim_device: str, graphics_device_id: int, headless: bool):
        split_device = sim_device.split(":")
        self.device_type = split_device[0]
        self.device_id = int(split_device[1]) if len(split_device) > 1 else 0

        # vec_task.py:65-71.  This build has no CPU pipeline: the simulator is HIP-only.
        self.device = "cpu"
        if config["sim"]["use_gpu_pipeline"]:
            if self.device_type.lower() in ("cuda", "gpu"):
                self.device = "cuda" + ":" + str(self.device_id)
            else:
                print("GPU Pipeline can only be used with GPU simulation. Forcing CPU Pipeline.")
                config["sim"]["use_gpu_pipeline"] = False

        self.rl_device = config.get("rl_device", "cuda:0")
        self.headless = headless
        self.graphics_device_id = graphics_device_id
        if not config.get("enableCameraSensors", False) and self.headless:
            self.graphics_device_id = -1

        self.num_environments = config["env"]["numEnvs"]
        self.num_agents = config["env"].get("numAgents", 1)
        self.num_observations = config["env"]["numObservations"]
        self.num_states = config["env"].get("numStates", 0)
        self.num_actions = config["env"]["numActions"]
        self.control_freq_inv = config["env"].get("controlFrequencyInv", 1)

        self.obs_space = Box(np.ones(self.num_obs) * -np.inf, np.ones(self.num_obs) * np.inf)
        self.state_space = Box(np.ones(self.num_states) * -np.inf, np.ones(self.num_states) * np.inf)
        self.act_space = Box(np.ones(self.num_actions) * -1., np.ones(self.num_actions) * 1.)

        self.clip_obs = config["env"].get("clipObservations", np.inf)
        self.clip_actions = config["env"].get("clipActions", np.inf)

    @abc.abstractmethod
    def allocate_buffers(self): ...

    @abc.abstractmethod
    def step(self, actions: torch.Tensor) -> Tuple[Dict[str, torch.Tensor], torch.Tensor, torch.Tensor, Dict[str, Any]]: ...

    @abc.abstractmethod
    def reset(self) -> Dict[str, torch.Tensor]: ...

    @property
    def observation_space(self):
        return self.obs_space

    @property
    def action_space(self):
        return self.act_space

    @property
    def num_envs(self) -> int:
        return self.num_environments

    @property
    def num_acts(self) -> int:
        return self.num_actions

    @property
    def num_obs(self) -> int:
        return self.num_observations


MASS_DRAW_TAG = 0x4D415353  # "MASS": Philox counter word of the setup-only mass scale draw


class VecTask(Env):
    """Subclasses create `self.sim` (a bez_isaacgym_amd.sim.BezSim) in create_sim()."""

    def __init__(self, config, sim_device, graphics_device_id, headless):
        super().__init__(config, sim_device, graphics_device_id, headless)
        if self.cfg["physics_engine"] not in ("physx", "flex"):  # vec_task.py:162-168
            raise ValueError(f"Invalid physics engine backend: {self.cfg['physics_engine']}")
        if self.cfg["sim"]["up_axis"] not in ["z", "y"]:        # vec_task.py:421-424
            msg = f"Invalid physics up-axis: {self.cfg['sim']['up_axis']}"
            print(msg)
            raise ValueError(msg)
        if self.device == "cpu":
            raise RuntimeError("bez_isaacgym_amd is HIP-only: run with sim_device=cuda:<k> pipeline=gpu "
                               "(the CPU restatement lives in oracle/ and is test infrastructure)")
        self.first_randomization = True
        self.dr_randomizations = {}
        self.last_step = -1
        self.last_rand_step = -1
        self.viewer = None
        self.enable_viewer_sync = True
        self.sim_initialized = False
        self.create_sim()
        self.sim_initialized = True
        self.allocate_buffers()
        self.obs_dict = {}

    def allocate_buffers(self):
        """Same names / dtypes as vec_task.py:226-249; obs/rew/reset/progress/timeout are zero-copy views of
        the simulator's own buffers (the fused kernel writes them in place)."""
        from ... import abi
        s = self.sim
        self.obs_buf = s.tensor(abi.TENSOR_OBS)
        self.states_buf = torch.zeros((self.num_envs, self.num_states), device=self.device, dtype=torch.float)
        self.rew_buf = s.tensor(abi.TENSOR_REW)
        self.reset_buf = s.tensor(abi.TENSOR_RESET)
        self.timeout_buf = s.tensor(abi.TENSOR_TIMEOUT)
        self.progress_buf = s.tensor(abi.TENSOR_PROGRESS)
        self.randomize_buf = s.tensor(abi.TENSOR_RANDOMIZE_BUF)
        self.nonfinite_buf = s.tensor(abi.TENSOR_NONFINITE_COUNT)  # trips of the non-finite guard per env (abi.FLAG_NONFINITE_GUARD)
        self.health_buf = s.tensor(abi.TENSOR_HEALTH)              # the sim's health word (abi.HEALTH_* bits)
        # why episodes end (abi.END_*): this step's cause bits per env, ended episodes per deciding cause [cause][env] (never cleared),
        # and with env.debug.rewards (abi.FLAG_REWARD_TERMS) the sums of the reward's terms [slot][env] (zeroed by their consumer)
        self.episode_end_bits = s.episode_tensor(abi.EPISODE_END_BITS)
        self.episode_end_counts = s.episode_tensor(abi.EPISODE_END_COUNTS)
        self.reward_terms_buf = s.episode_tensor(abi.EPISODE_REWARD_TERMS)
        self.reward_terms_on = bool(int(s.cfg.flags) & abi.FLAG_REWARD_TERMS)
        # gym.acquire_dof_force_tensor (env.enableDofForceSensors / abi.FLAG_DOF_FORCE): (N, 18) views of the sim's actuator tensors,
        # filled by refresh_dof_force_tensor(); without the key the three properties below raise and say why
        self.dof_force_on = bool(int(s.cfg.flags) & abi.FLAG_DOF_FORCE)
        self._dof_force_views = None
        if self.dof_force_on:
            self._dof_force_views = tuple(s.actuator_tensor(k).view(self.num_envs, abi.NUM_DOFS)
                                          for k in (abi.ACTUATOR_DOF_FORCE, abi.ACTUATOR_DRIVE_TORQUE, abi.ACTUATOR_STATUS))
        self.extras = {}

    def _dof_force_view(self, k, name):
        views = self.__dict__.get("_dof_force_views")
        if views is None:
            from ... import abi
            raise AttributeError("%s exists only with the task key %s: True (abi.FLAG_DOF_FORCE): without it the step kernels "
                                 "record no joint forces" % (name, abi.DOF_FORCE_KEY))
        return views[k]

    dof_force_tensor = property(lambda self: self._dof_force_view(0, "dof_force_tensor"), doc="(N, 18) f32 net joint force (Isaac's DOF force)")
    dof_drive_torque = property(lambda self: self._dof_force_view(1, "dof_drive_torque"), doc="(N, 18) f32 drive torque")
    dof_status = property(lambda self: self._dof_force_view(2, "dof_status"), doc="(N, 18) i32 abi.ACTUATOR_* status bits")

    def refresh_dof_force_tensor(self):
        """gym.refresh_dof_force_tensor: fills dof_force_tensor / dof_drive_torque / dof_status from the last physics launch."""
        self._dof_force_view(0, "refresh_dof_force_tensor()")
        self.sim.refresh_actuator_tensors()
        return True

    # ---- gym.acquire_jacobian_tensor / acquire_mass_matrix_tensor (include/bez_sim.h "Dynamics tensors"): allocated by the acquisition
    def _dynamics_view(self, name):
        view = self.__dict__.get("_" + name + "_view")
        if view is None:
            raise AttributeError("%s exists only after acquire_%s_tensor(): the sim allocates the tensor on its first acquisition" % (name, name))
        return view

    jacobian = property(lambda self: self._dynamics_view("jacobian"), doc="(N, NB, 6, 24) f32 Jacobian of the robot's bodies")
    mass_matrix = property(lambda self: self._dynamics_view("mass_matrix"), doc="(N, 24, 24) f32 mass matrix")

    def acquire_jacobian_tensor(self):
        """gym.acquire_jacobian_tensor (wrapped): the (N, NB, 6, 24) view of the sim's Jacobian, NB = the robot's rigid bodies."""
        from ... import abi
        self._jacobian_view = self.sim.dynamics_tensor(abi.DYNAMICS_JACOBIAN).view(self.num_envs, -1, 6, abi.NUM_GEN)
        return self._jacobian_view

    def acquire_mass_matrix_tensor(self):
        """gym.acquire_mass_matrix_tensor (wrapped): the (N, 24, 24) view of the sim's mass matrix."""
        from ... import abi
        self._mass_matrix_view = self.sim.dynamics_tensor(abi.DYNAMICS_MASS_MATRIX)
        return self._mass_matrix_view

    def refresh_jacobian_tensors(self):
        self._dynamics_view("jacobian")
        self.sim.refresh_dynamics_tensors("jacobian")
        return True

    def refresh_mass_matrix_tensors(self):
        self._dynamics_view("mass_matrix")
        self.sim.refresh_dynamics_tensors("mass_matrix")
        return True

    # ---- inverse dynamics of the current state (include/bez_sim.h "Inverse dynamics"); usable between steps like the refreshes above
    def inverse_dynamics(self, udot=None, terms=7):
        """(N, 24): the terms (abi.ID_INERTIA | ID_VELOCITY | ID_GRAVITY; default all) of M(q) udot + h(q, u) in u = [root_lin, root_ang,
        qd]; udot (N, 24) or None for zero.  The tensor is the sim's one result buffer: the next call overwrites it."""
        return self.sim.inverse_dynamics(udot, terms)

    def bias_forces(self):
        """(N, 24): h(q, u), the Coriolis, centrifugal and gravity forces of the current state"""
        from ... import abi
        return self.sim.inverse_dynamics(None, abi.ID_VELOCITY | abi.ID_GRAVITY)

    def gravity_forces(self):
        """(N, 24): the generalised force that holds the robot still against gravity in its current configuration"""
        from ... import abi
        return self.sim.inverse_dynamics(None, abi.ID_GRAVITY)

    # ---- forward dynamics of the current state (include/bez_sim.h "Forward dynamics"); each method is one launch, and what it returns
    # is the sim's one result buffer of that kind: the next call overwrites it
    def forward_dynamics(self, force=None, bias=6, fixed_base=None):
        """(N, 24): udot = M(q)^-1 (force - h(q, u)) in u = [root_lin, root_ang, qd]; force (N, 24) or None for zero; bias: the terms of
        h taken off it (abi.ID_VELOCITY | ID_GRAVITY; default both); fixed_base: hold the root (rows 0:6 zero), None: as the task's
        urdfAsset.fixBaseLink says"""
        from ... import abi
        if fixed_base is None:
            fixed_base = bool(int(self.sim.cfg.flags) & abi.FLAG_FIX_BASE)
        return self.sim.forward_dynamics(force, bias, fixed_base)

    def free_acceleration(self):
        """(N, 24): the acceleration of the current state with nothing acting on it but gravity and its own motion"""
        return self.forward_dynamics(None)

    def mass_solve(self, b):
        """(N, 24): M(q)^-1 b for a generalised force b (N, 24)"""
        return self.forward_dynamics(b, 0)

    # ---- operational space of the current state (include/bez_sim.h "Operational space"), for the five frames limb_ik controls; each
    # method is one launch, and what it returns is the sim's one result buffer of that kind: the next call overwrites it
    def operational_space(self, offsets=None, fixed_base=None, want=("jac", "jminv", "w", "lambda")):
        """(jac (N, 5, 6, 24), jminv (N, 5, 6, 24), w (N, 30, 30), lam (N, 5, 6, 6)): J_c, J_c M^-1, J_E M^-1 J_E^T and W_cc^-1 of the frames
        of abi.IK_CHAIN_NAMES, each the chain's end body displaced by offsets[c] (5, 3) in its own axes (None: zero); None for what `want`
        leaves out.  fixed_base: hold the root, None: as the task's urdfAsset.fixBaseLink says; "lambda" cannot be wanted with it"""
        from ... import abi
        if fixed_base is None:
            fixed_base = bool(int(self.sim.cfg.flags) & abi.FLAG_FIX_BASE)
        return self.sim.operational_space(offsets, fixed_base, want=want)

    def end_effector_jacobian(self, offsets=None):
        """(N, 5, 6, 24): the Jacobians of the five controlled frames, rows [linear; angular] in world axes"""
        return self.operational_space(offsets, want=("jac",))[0]

    def delassus_matrix(self, offsets=None):
        """(N, 30, 30): W = J_E M^-1 J_E^T, what a wrench on one controlled frame does to every other; bitwise symmetric"""
        return self.operational_space(offsets, want=("w",))[2]

    def operational_space_inertia(self, offsets=None):
        """(N, 5, 6, 6): Lambda_c = (J_c M^-1 J_c^T)^-1 of each controlled frame (floating base alone)"""
        return self.operational_space(offsets, want=("lambda",))[3]

    def dynamically_consistent_inverse(self, offsets=None):
        """(N, 5, 24, 6): Jbar_c = M^-1 J_c^T Lambda_c of each controlled frame, J_c @ Jbar_c = I (floating base alone): the launch and one
        matmul on its outputs"""
        _, jminv, _, lam = self.operational_space(offsets, want=("jminv", "lambda"))
        return torch.matmul(lam, jminv).transpose(-1, -2)

    # ---- centroidal dynamics of the current state (include/bez_sim.h "Centroidal dynamics"); each method is one launch, and what it
    # returns is (a view of) the sim's one result buffer of that kind: the next call overwrites it
    def centroidal_state(self):
        """(N, 16): the abi.CM_* words -- COM, COM_VEL, LIN_MOM, ANG_MOM about the centre of mass, MASS, KINETIC, POTENTIAL"""
        return self.sim.centroidal()[0]

    def center_of_mass(self):
        """((N, 3) position in env coordinates, (N, 3) velocity) of the robot's centre of mass"""
        from ... import abi
        s = self.centroidal_state()
        return s[:, abi.CM_COM:abi.CM_COM + 3], s[:, abi.CM_COM_VEL:abi.CM_COM_VEL + 3]

    def centroidal_momentum(self):
        """(N, 6): [linear momentum; angular momentum about the centre of mass], world axes"""
        from ... import abi
        return self.centroidal_state()[:, abi.CM_LIN_MOM:abi.CM_LIN_MOM + 6]

    def centroidal_momentum_matrix(self):
        """(N, 6, 24): A_G with A_G @ u == centroidal_momentum(), u = [root_lin, root_ang, qd]"""
        return self.sim.centroidal(want_matrix=True)[1]

    def mechanical_energy(self):
        """((N,) kinetic energy 1/2 u^T M u, (N,) potential energy -m g . com)"""
        from ... import abi
        s = self.centroidal_state()
        return s[:, abi.CM_KINETIC], s[:, abi.CM_POTENTIAL]

    # ---- body accelerations of the current state (include/bez_sim.h "Body accelerations"); each method is one launch, and what it
    # returns is (a view of) the sim's one result buffer of that kind: the next call overwrites it
    def body_accelerations(self, udot=None, terms=3, space="env"):
        """(N, NB, 6): the terms (abi.ACC_UDOT | ACC_VELOCITY | ACC_GRAVITY; default ACC_MOTION = d/dt of the bodies' velocity rows) of
        J_b udot + Jdot_b u - g for the robot's NB bodies in RIGID_BODY_STATE order; udot (N, 24) or None for zero; space "env" / "local"."""
        return self.sim.body_accelerations(udot, terms, space)

    def jacobian_dot_u(self):
        """(N, NB, 6): Jdot_b u, the bias acceleration of every body in the current state, world axes"""
        from ... import abi
        return self.sim.body_accelerations(None, abi.ACC_VELOCITY, abi.SPACE_ENV)

    def body_index(self, name):
        """the RIGID_BODY_STATE row of the robot body `name` (the model's body_names for the asset in use)"""
        from ... import abi
        names = self.__dict__.get("_body_names")
        if names is None:
            import json
            import os
            model = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "model", "bez_model.json")))
            names = self._body_names = list((model["cleats"] if int(self.sim.cfg.flags) & abi.FLAG_CLEATS else model)["body_names"])
        if name not in names:
            raise ValueError("no rigid body %r: the asset's bodies are %s" % (name, ", ".join(names)))
        return names.index(name)

    def accelerometer(self, udot, body="/imu_link"):
        """(N, 3): the specific force at the origin of `body` in the body's own frame for the acceleration udot (N, 24) of the current
        state -- J udot + Jdot u - g, what an accelerometer mounted there reads"""
        from ... import abi
        return self.sim.body_accelerations(udot, abi.ACC_ALL, abi.SPACE_LOCAL)[:, self.body_index(body), 0:3]

    # ---- generalised forces of wrenches on the rigid bodies (include/bez_sim.h "Generalised forces"); one launch, and what is returned is
    # the sim's one result buffer of that kind: the next call overwrites it
    def generalized_forces(self, forces=None, torques=None, positions=None, space="env", at="com"):
        """(N, 24): sum over bodies of J_b^T [f; t] in u = [root_lin, root_ang, qd], rows [force; moment about the root origin; joint
        torques]; forces / torques / positions / space as for apply_rigid_body_force_tensors, (N*B, 3) or (N, B, 3); at "com" / "origin":
        where a wrench acts when positions is None"""
        return self.sim.generalized_forces(forces, torques, positions, space, at)

    def body_wrench_forces(self, body, force=None, torque=None, space="env", at="origin"):
        """(N, 24): J_body^T [f; t] for (N, 3) vectors on the one rigid body `body` (a name of body_index), the generalised force of
        operational-space control on a foot or hand; at "origin" J is the Jacobian tensor's row block of that body"""
        if force is None and torque is None:
            raise ValueError("body_wrench_forces: force and torque are both None")
        b = self.body_index(body)
        bufs = self.__dict__.get("_wrench_rows")
        if bufs is None:   # two zero (N, B, 3) tensors per env object; each call rewrites row b of them and zeroes it again
            bufs = self._wrench_rows = [torch.zeros(self.num_envs, self.sim.num_bodies, 3, device=self.sim.device) for _ in range(2)]
        for buf, v in zip(bufs, (force, torque)):
            if v is not None:
                buf[:, b].copy_(v)
        out = self.sim.generalized_forces(bufs[0], bufs[1], None, space, at)
        for buf in bufs:
            buf[:, b].zero_()
        return out

    # ---- limb inverse kinematics (include/bez_sim.h "Limb inverse kinematics"); one launch, and what is returned are the sim's two result
    # buffers of that kind: the next call overwrites them.  Chains: abi.IK_CHAIN_NAMES, end bodies abi.IK_END_BODIES
    def limb_ik(self, targets, weights, offsets=None, damping=0.05, max_step=0.0, iters=1, space="env", out=None, err_out=None):
        """((N, 18) joint angles, (N, 5, 6) pose errors at them) after `iters` damped-least-squares iterations per chain towards `targets`
        (N, 5, 7) [position, quaternion xyzw]; weights (5, 2) [w_pos, w_rot], both 0 leaves a chain alone; offsets (5, 3) or None; space
        "env" (as RIGID_BODY_STATE rows) or "root" (relative to the root, in its axes).  The state is not written: hand the angles to
        set_dof_position_target_tensor or a setter."""
        return self.sim.limb_ik(targets, weights, offsets, damping, max_step, iters, space, out, err_out)

    def limb_pose_error(self, targets, weights=None, offsets=None, space="env"):
        """(N, 5, 6): [p_des - p ; 2 sin(theta/2) axis] of the current state's controlled frames against `targets`, in the root's axes;
        weights only select the chains (default: all five)"""
        from ... import abi
        if weights is None:
            weights = [[1.0, 1.0]] * abi.IK_CHAINS
        return self.sim.limb_ik(targets, weights, offsets, iters=0, space=space)[1]

    def limb_targets(self):
        """(N, 5, 7): the current poses of the five end bodies as RIGID_BODY_STATE reports them (one refresh) -- the "env" targets that
        hold every limb where it is"""
        from ... import abi
        rb = self.sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(self.num_envs, -1, 13)
        return rb[:, [self.body_index(b) for b in abi.IK_END_BODIES], 0:7].contiguous()

    def ik_offset(self, body):
        """(chain index, (3,) offset) with which limb_ik controls the frame of `body`, a rigid body fixed to a chain's end link (/camera,
        a cleat, the end body itself): its origin relative to the end body's, in that body's frame -- offsets[chain] = the offset"""
        from ... import abi
        b = self.body_index(body)
        model = self.__dict__.get("_ik_model")
        if model is None:
            import json
            import os
            model = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "model", "bez_model.json")))
            model = self._ik_model = model["cleats"] if int(self.sim.cfg.flags) & abi.FLAG_CLEATS else model
        for c, end in enumerate(abi.IK_END_BODIES):
            e = self.body_index(end)
            if model["body_link"][b] == model["body_link"][e]:
                return c, tuple(float(x) - float(y) for x, y in zip(model["body_offset"][b], model["body_offset"][e]))
        raise ValueError("rigid body %r is not fixed to the end link of a chain (%s)" % (body, ", ".join(abi.IK_END_BODIES)))

    # ---- proximity (include/bez_sim.h "Proximity"): the contact geometry the step decides on; one launch, and what is returned are the
    # sim's result buffers of that kind: the next call overwrites them
    def proximity(self, ground=None, ball=None, pairs=None, want=("ground", "ball", "pairs")):
        """(ground (N, 23, 3), ball (N, 11, 8), pairs (N, 28, 8)) of the current state: the ground points' positions (abi.PROX_GROUND_NAMES,
        then the ball's lowest point), and [gap, normal, point, 0] of the ball against every box (abi.PROX_BOX_BODIES) and of every
        left-leg x right-leg capsule pair (abi.PROX_PAIR_BODIES); an output not named in `want` is None"""
        return self.sim.proximity(ground, ball, pairs, want)

    def foot_clearance(self):
        """(N, 2): the height above the ground of the lowest of each foot's four ground points (left, right); negative: in contact"""
        g = self.sim.proximity(want=("ground",))[0]
        return g[:, 0:8, 2].reshape(self.num_envs, 2, 4).min(dim=2).values

    def self_collision_gap(self):
        """(N,): the smallest gap of the 28 leg-to-leg capsule pairs; negative: the legs overlap by that much"""
        from ... import abi
        return self.sim.proximity(want=("pairs",))[2][:, :, abi.PROX_GAP].min(dim=1).values

    def ball_gap(self):
        """((N,) gap, (N,) box index): the smallest gap of the ball to the eleven boxes and the box (abi.PROX_BOX_BODIES) it belongs to;
        on ties the first box in the step's order: the legs first, the torso last (an env with a non-finite gap: NaN and abi.PROX_BOXES)"""
        import torch
        from ... import abi
        gap = self.sim.proximity(want=("ball",))[1][:, :, abi.PROX_GAP]
        least = gap.min(dim=1).values
        order = torch.arange(abi.PROX_BOXES, device=gap.device).expand_as(gap)
        return least, torch.where(gap == least[:, None], order, abi.PROX_BOXES).min(dim=1).values

    def actuator_snapshot(self):
        """(drive torque, status, joint velocity), each (N, 18), of the last physics launch: one refresh of the actuator tensors and one of
        DOF_STATE (the PPO loop's per-epoch actuator statistics)."""
        from ... import abi
        self.refresh_dof_force_tensor()
        qd = self.sim.refresh(abi.TENSOR_DOF_STATE).view(self.num_envs, abi.NUM_DOFS, 2)[:, :, 1]
        return self.dof_drive_torque, self.dof_status, qd

    def get_state(self):
        return torch.clamp(self.states_buf, -self.clip_obs, self.clip_obs).to(self.rl_device)

    @abc.abstractmethod
    def pre_physics_step(self, actions: torch.Tensor): ...

    @abc.abstractmethod
    def post_physics_step(self): ...

    def step(self, actions: torch.Tensor):
        """vec_task.py:303-349.  With no Python-side hooks active this is ONE kernel launch
        (bez_sim_step: clamp, PD targets, physics, bookkeeping, reset, obs, reward)."""
        if self.dr_randomizations.get('actions', None) and not self.external_action_noise:
            actions = self.dr_randomizations['actions']['noise_lambda'](actions)
        actions = actions.to(self.device, torch.float32).contiguous()
        self._fused_step(actions)
        if self.dr_randomizations.get('observations', None):
            out = self.dr_randomizations['observations']['noise_lambda'](self.obs_buf)
            if out.data_ptr() != self.obs_buf.data_ptr():
                self.obs_buf.copy_(out)
        self.extras["time_outs"] = self.timeout_buf.to(self.rl_device)
        self.obs_dict["obs"] = self._clipped_obs()
        if self.num_states > 0:
            self.obs_dict["states"] = self.get_state()
        return self.obs_dict, self.rew_buf.to(self.rl_device), self.reset_buf.to(self.rl_device), self.extras

    def _clipped_obs(self):
        """vec_task.py:347: clamp(obs_buf, +-clipObservations).to(rl_device).  With the default clipObservations = inf the clamp
        is the identity: the simulator's own buffer is returned (zero-copy, valid until the next step()) instead of a
        full-tensor copy per control step.  A consumer that keeps obs_dict["obs"] across step() calls sets
        env.copyObservations: True in the task config to get the reference's fresh tensor per step."""
        if np.isinf(self.clip_obs) and not self.cfg["env"].get("copyObservations", False):
            return self.obs_buf.to(self.rl_device)
        return torch.clamp(self.obs_buf, -self.clip_obs, self.clip_obs).to(self.rl_device)

    def _fused_step(self, actions):
        """Default: the split path through the subclass hooks (vec_task.py:317-335)."""
        action_tensor = torch.clamp(actions, -self.clip_actions, self.clip_actions)
        self.pre_physics_step(action_tensor)
        for _ in range(self.control_freq_inv):
            self.render()
            self.sim.simulate()
        self.post_physics_step()

    def zero_actions(self) -> torch.Tensor:
        return torch.zeros([self.num_envs, self.num_actions], dtype=torch.float32, device=self.rl_device)

    def reset(self):
        """vec_task.py:361-377: one step with zero actions."""
        self.step(self.zero_actions())
        self.obs_dict["obs"] = self._clipped_obs()
        if self.num_states > 0:
            self.obs_dict["states"] = self.get_state()
        return self.obs_dict

    def render(self):
        """Headless only (viewer is out of scope): no-op."""
        return None

    def get_number_of_agents(self):
        return self.num_agents

    # ---- external forces: gym.apply_rigid_body_force_tensors / gym.apply_rigid_body_force_at_pos_tensors.  Tensors (N*B, 3) or (N, B, 3)
    # float32 on the sim's device in RIGID_BODY_STATE order; space "env" / "local" (or abi.SPACE_ENV / abi.SPACE_LOCAL).  They act during
    # the next physics launch only (with controlFrequencyInv = k: the first of the k simulate calls) and several calls add up
    # (include/bez_sim.h: bez_sim_apply_body_forces).
    def apply_rigid_body_force_tensors(self, forces=None, torques=None, space="env"):
        """Forces at each body's centre of mass and torques on the bodies."""
        self.sim.apply_body_forces(forces=forces, torques=torques, positions=None, space=space)
        return True

    def apply_rigid_body_force_at_pos_tensors(self, forces, positions=None, space="env"):
        """Forces at the given points (world coordinates in "env" space, body frame in "local" space; None = the centres of mass)."""
        self.sim.apply_body_forces(forces=forces, torques=None, positions=positions, space=space)
        return True

    # ---- domain randomisation (vec_task.py:505-725), device-side: bez_sim_set_randomization
    # ---- hooks for a trainer that drives the randomised env at full speed (ppo/a2c_continuous.py): both default to "the env does it"
    external_action_noise = False   # True: the caller adds the action noise itself (action_noise_source), step() must not add it again

    def action_noise_source(self):
        """(snapshot pointer, seed, env id offset) of the action-noise lambda for a consumer that adds it in its own launch, or None"""
        return self.sim.action_noise_source() if self.dr_randomizations.get('actions', None) else None

    def dr_prelaunch(self):
        """The coming step's randomisation kernel now, on the current stream (overlappable with the policy's forward pass); no-op
        without a device-side randomisation."""
        if not self.first_randomization and self.randomize:
            self.sim.dr_prelaunch()

    def dr_step_args(self):
        """The coming step's randomisation as an argument block for a launch that carries it (sim.dr_step_args); None without one."""
        return self.sim.dr_step_args() if (not self.first_randomization and self.randomize) else None

    def apply_randomizations(self, dr_params):
        """The reference calls this from reset_idx on every step in which some env resets (kick_env.py:781-782); what it does
        there -- per-env redraws at reset time once `frequency` steps have passed, gravity and the noise parameters on the same
        clock, all scaled by the linear schedule -- now happens inside the simulator, in a small kernel in front of the step
        kernel (include/bez_sim.h: bez_sim_set_randomization), keyed by (seed, global env id, episode).  The first call hands
        the parameters over (and randomises every env at frame 0, first_randomization); later calls have nothing left to do,
        so the step never syncs with the host and stays HIP-graph capturable with randomize: True."""
        from ... import abi
        if not self.first_randomization:
            return
        self.sim.set_randomization(abi.dr_config_from_params(dr_params))
        self.randomize_buf = self.sim.tensor(abi.TENSOR_RANDOMIZE_BUF)     # the kernel counts it (kick_env.py:430)
        # vec_task.py:544-618 noise lambdas (gaussian additive, range_correlated absent in bez_kick.yaml): one launch each, the mean /
        # std (BEZ_TENSOR_DR_NOISE, moved by the schedule) are read on the device.  The caller's action tensor is not modified.
        sim = self.sim
        if "observations" in dr_params:
            # BEZ_FLAG_OBS_NOISE_IN_STEP: the step kernel adds this noise on its way out (one launch less per step); on the simulator's
            # own observation buffer the call below is then a no-op inside the library, any other tensor still gets a launch
            sim.set_flags(int(sim.cfg.flags) | abi.FLAG_OBS_NOISE_IN_STEP)
            sim.cfg.flags = int(sim.cfg.flags) | abi.FLAG_OBS_NOISE_IN_STEP
            self.dr_randomizations["observations"] = {"noise_lambda": lambda t: sim.add_dr_noise(t if t.is_contiguous() else t.contiguous(), 0)}
        if "actions" in dr_params:
            self._noisy_actions = torch.empty(self.num_envs, self.num_actions, device=self.device, dtype=torch.float32)  # persistent: graph-safe

            def act_noise(t):
                t = t.to(self.device, torch.float32)
                return sim.add_dr_noise(t if t.is_contiguous() else t.contiguous(), 1, out=self._noisy_actions.view(t.shape))
            self.dr_randomizations["actions"] = {"noise_lambda": act_noise}
        # rigid_shape_properties.restitution (bez_kick.yaml:187-192) SCALES the asset's restitution, which is 0 (plane
        # restitution 0, bez_kick.yaml:16; asset default 0 [ext]): 0 * U(0, 0.7) = 0 -- nothing to randomise.
        # rigid_body_properties.mass is setup_only (bez_kick.yaml:175): drawn once, here, at frame 0 -- where its linear schedule
        # still interpolates to "no randomisation" (scale 1); without a schedule it is a real one-time draw.
        rbp = (((dr_params.get("actor_params") or {}).get("bez") or {}).get("rigid_body_properties") or {})
        if "mass" in rbp and rbp["mass"].get("schedule") != "linear":
            # one draw per (GLOBAL env id, link) from the simulator's own counter-based generator: the same env gets the same
            # masses whatever the number of ranks (every other per-env draw is keyed that way, include/bez_sim.h)
            from ...utils.utils import per_env_uniform
            lo, hi = (float(v) for v in rbp["mass"]["range"])
            off = int(self.cfg.get("env_id_offset", 0))
            u = per_env_uniform(int(self.cfg.get("seed", 42)), range(off, off + self.num_envs), MASS_DRAW_TAG, 19)
            self.sim.set_env_params(abi.PARAM_MASS_SCALE, torch.from_numpy(u * (hi - lo) + lo).to(self.device).contiguous())
        self.first_randomization = False
