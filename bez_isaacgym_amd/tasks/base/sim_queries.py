"""This project's own conveniences on a task: the actuator and dynamics tensors, the query calls of the simulator (BezSim, include/bez_sim.h)
with the task's defaults, what is read off their results, and external forces on the rigid bodies.  The reference's vec_task.py has none
of this; VecTask (vec_task.py) inherits the mixin, so every method is an attribute of every task class.

The mixin has no __init__ and keeps its caches lazily in the instance's dict: it needs nothing but `self.sim` (and `self.num_envs`
where a result is reshaped per env), so an object made with __new__ serves.
"""
import json
import os

import torch

from ... import abi


class SimQueries:
    """Mixin of VecTask over `self.sim` (a bez_isaacgym_amd.sim.BezSim)."""

    def _fixed_base(self, fixed_base):
        """`fixed_base` as a query takes it: None means what the task's urdfAsset.fixBaseLink says (abi.FLAG_FIX_BASE)"""
        return bool(int(self.sim.cfg.flags) & abi.FLAG_FIX_BASE) if fixed_base is None else fixed_base

    def _model(self):
        """the model dict of the asset in use: bez_model.json, its "cleats" sub-dict with abi.FLAG_CLEATS (read once per env object)"""
        model = self.__dict__.get("_asset_model")
        if model is None:
            model = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "model", "bez_model.json")))
            model = self._asset_model = model["cleats"] if int(self.sim.cfg.flags) & abi.FLAG_CLEATS else model
        return model

    # ---- gym.acquire_dof_force_tensor (env.enableDofForceSensors / abi.FLAG_DOF_FORCE): VecTask.allocate_buffers makes the views
    def _dof_force_view(self, k, name):
        views = self.__dict__.get("_dof_force_views")
        if views is None:
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
        self._jacobian_view = self.sim.dynamics_tensor(abi.DYNAMICS_JACOBIAN).view(self.num_envs, -1, 6, abi.NUM_GEN)
        return self._jacobian_view

    def acquire_mass_matrix_tensor(self):
        """gym.acquire_mass_matrix_tensor (wrapped): the (N, 24, 24) view of the sim's mass matrix."""
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
        return self.sim.inverse_dynamics(None, abi.ID_VELOCITY | abi.ID_GRAVITY)

    def gravity_forces(self):
        """(N, 24): the generalised force that holds the robot still against gravity in its current configuration"""
        return self.sim.inverse_dynamics(None, abi.ID_GRAVITY)

    # ---- forward dynamics of the current state (include/bez_sim.h "Forward dynamics"); each method is one launch, and what it returns
    # is the sim's one result buffer of that kind: the next call overwrites it
    def forward_dynamics(self, force=None, bias=6, fixed_base=None):
        """(N, 24): udot = M(q)^-1 (force - h(q, u)) in u = [root_lin, root_ang, qd]; force (N, 24) or None for zero; bias: the terms of
        h taken off it (abi.ID_VELOCITY | ID_GRAVITY; default both); fixed_base: hold the root (rows 0:6 zero), None: as the task's
        urdfAsset.fixBaseLink says"""
        return self.sim.forward_dynamics(force, bias, self._fixed_base(fixed_base))

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
        return self.sim.operational_space(offsets, self._fixed_base(fixed_base), want=want)

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
        s = self.centroidal_state()
        return s[:, abi.CM_COM:abi.CM_COM + 3], s[:, abi.CM_COM_VEL:abi.CM_COM_VEL + 3]

    def centroidal_momentum(self):
        """(N, 6): [linear momentum; angular momentum about the centre of mass], world axes"""
        return self.centroidal_state()[:, abi.CM_LIN_MOM:abi.CM_LIN_MOM + 6]

    def centroidal_momentum_matrix(self):
        """(N, 6, 24): A_G with A_G @ u == centroidal_momentum(), u = [root_lin, root_ang, qd]"""
        return self.sim.centroidal(want_matrix=True)[1]

    def mechanical_energy(self):
        """((N,) kinetic energy 1/2 u^T M u, (N,) potential energy -m g . com)"""
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
        return self.sim.body_accelerations(None, abi.ACC_VELOCITY, abi.SPACE_ENV)

    def body_index(self, name):
        """the RIGID_BODY_STATE row of the robot body `name` (the model's body_names for the asset in use)"""
        names = self._model()["body_names"]
        if name not in names:
            raise ValueError("no rigid body %r: the asset's bodies are %s" % (name, ", ".join(names)))
        return names.index(name)

    def accelerometer(self, udot, body="/imu_link"):
        """(N, 3): the specific force at the origin of `body` in the body's own frame for the acceleration udot (N, 24) of the current
        state -- J udot + Jdot u - g, what an accelerometer mounted there reads"""
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
        if weights is None:
            weights = [[1.0, 1.0]] * abi.IK_CHAINS
        return self.sim.limb_ik(targets, weights, offsets, iters=0, space=space)[1]

    def limb_targets(self):
        """(N, 5, 7): the current poses of the five end bodies as RIGID_BODY_STATE reports them (one refresh) -- the "env" targets that
        hold every limb where it is"""
        rb = self.sim.refresh(abi.TENSOR_RIGID_BODY_STATE).view(self.num_envs, -1, 13)
        return rb[:, [self.body_index(b) for b in abi.IK_END_BODIES], 0:7].contiguous()

    def ik_offset(self, body):
        """(chain index, (3,) offset) with which limb_ik controls the frame of `body`, a rigid body fixed to a chain's end link (/camera,
        a cleat, the end body itself): its origin relative to the end body's, in that body's frame -- offsets[chain] = the offset"""
        b, model = self.body_index(body), self._model()
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
        return self.sim.proximity(want=("pairs",))[2][:, :, abi.PROX_GAP].min(dim=1).values

    def ball_gap(self):
        """((N,) gap, (N,) box index): the smallest gap of the ball to the eleven boxes and the box (abi.PROX_BOX_BODIES) it belongs to;
        on ties the first box in the step's order: the legs first, the torso last (an env with a non-finite gap: NaN and abi.PROX_BOXES)"""
        gap = self.sim.proximity(want=("ball",))[1][:, :, abi.PROX_GAP]
        least = gap.min(dim=1).values
        order = torch.arange(abi.PROX_BOXES, device=gap.device).expand_as(gap)
        return least, torch.where(gap == least[:, None], order, abi.PROX_BOXES).min(dim=1).values

    def actuator_snapshot(self):
        """(drive torque, status, joint velocity), each (N, 18), of the last physics launch: one refresh of the actuator tensors and one of
        DOF_STATE (the PPO loop's per-epoch actuator statistics)."""
        self.refresh_dof_force_tensor()
        qd = self.sim.refresh(abi.TENSOR_DOF_STATE).view(self.num_envs, abi.NUM_DOFS, 2)[:, :, 1]
        return self.dof_drive_torque, self.dof_status, qd

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

    # ---- query states (include/bez_sim.h "Query states"): everything above on states the caller supplies, the episode left alone
    def query_state(self, rows=None):
        """A StateQueries of `rows` rows (None: num_envs): fill it with set(root, dof, ball=None, env_ids=None) or capture(env_ids=None),
        then ask it what the task is asked -- bias_forces(), center_of_mass(), foot_clearance(), limb_ik(), acquire_jacobian_tensor() ... --
        about those rows; env_ids gives row i the randomised masses, gravity and joint limits of env env_ids[i].  close() frees it."""
        return StateQueries(self.sim.query_state(self.num_envs if rows is None else rows))

    # ---- env snapshots (include/bez_sim.h "Env snapshots"): whole envs saved and put back, for planning through the real step and rewinds
    def save_state(self, env_ids=None):
        """A sim.Snapshot holding env env_ids[i] in row i ((M,) int32 on the sim's device; None: every env, row i = env i), with the
        sim-global counters and randomisation clock and what this object itself holds per step (last_step, last_rand_step, the last
        actions).  close() frees it; load_state() puts it back."""
        snap = self.sim.snapshot(self.num_envs if env_ids is None else int(env_ids.numel()))
        snap.save(env_ids)
        actions = getattr(self, "actions", None)   # (materialises the borrowed action tensor of the last step: KickEnv.actions)
        snap.host = {"last_step": getattr(self, "last_step", -1), "last_rand_step": getattr(self, "last_rand_step", -1),
                     "actions": actions.clone() if isinstance(actions, torch.Tensor) else None}
        return snap

    def load_state(self, snap, env_ids=None, row_ids=None, globals_=None):
        """Env env_ids[i] becomes row row_ids[i] of `snap` (None: env i / row i), a snapshot of this task's sim or of another sim of the
        same task and asset.  `globals_`: also take the snapshot's sim-global block and this object's own per-step state -- None: True
        exactly when every env is restored by the identity (no ids, as many rows as envs), a rewind of the whole sim; a partial restore
        leaves them alone.  Afterwards every accessor (obs_buf, root_states, net_contact_forces, dof_force_tensor after its refresh ...)
        shows the restored envs: the lazily refreshed tensors are marked stale, the copies handed out by the last step() are renewed."""
        whole = env_ids is None and row_ids is None and snap.rows == self.num_envs
        if globals_ is None:
            globals_ = whole
        snap.restore(self.sim, env_ids=env_ids, row_ids=row_ids, globals_=bool(globals_))
        self._stale = True   # root_states, dof_state, rigid_body, net_contact_forces: refreshed by their next read (kick_env.py)
        host = getattr(snap, "host", None)
        if whole and globals_ and host is not None:   # what only a whole-sim restore can put back
            self.last_step, self.last_rand_step = host["last_step"], host["last_rand_step"]
            if host["actions"] is not None:
                self.actions = host["actions"].clone()
        extras, obs_dict = self.__dict__.get("extras"), self.__dict__.get("obs_dict")
        if extras is not None and "time_outs" in extras:
            extras["time_outs"] = self.timeout_buf.to(self.rl_device)
        if obs_dict is not None and "obs" in obs_dict:
            obs_dict["obs"] = self._clipped_obs()


class StateQueries(SimQueries):
    """SimQueries over a query state (bez_isaacgym_amd.sim.QueryState) in the place of the sim: `num_envs` is its row count.  What asks
    about the last physics launch, or acts on the next one, has no meaning on a supplied state and says so."""

    def __init__(self, state):
        self.sim, self.num_envs = state, state.rows
        self.set, self.capture, self.close = state.set, state.capture, state.close

    def _not_here(name):
        def refuse(self, *args, **kwargs):
            raise AttributeError("%s is about the physics launches of the live simulation; a query state has none "
                                 "(ask the task, not its query_state())" % name)
        return refuse

    dof_force_tensor = property(_not_here("dof_force_tensor"))
    dof_drive_torque = property(_not_here("dof_drive_torque"))
    dof_status = property(_not_here("dof_status"))
    refresh_dof_force_tensor = _not_here("refresh_dof_force_tensor()")
    actuator_snapshot = _not_here("actuator_snapshot()")
    apply_rigid_body_force_tensors = _not_here("apply_rigid_body_force_tensors()")
    apply_rigid_body_force_at_pos_tensors = _not_here("apply_rigid_body_force_at_pos_tensors()")
    query_state = _not_here("query_state()")
    save_state = _not_here("save_state()")
    load_state = _not_here("load_state()")
    del _not_here
