"""Python binding of the C ABI (include/bez_sim.h) -- thin ctypes calls, torch only for device memory
and the current HIP stream.  There is NO CPU fallback: if libbez_sim.so is missing or no GPU is
visible, construction raises."""
import ctypes as C
import os

import torch

from . import abi
from .build import lib_path

_LIB = None


class BezSimError(RuntimeError):
    pass


vp, i32, i64, u32, u64, fp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_void_p
# a getter of a sim-owned buffer: sim, which -> pointer, shape, rank, dtype (the episode getter's line stays spelled out: a test reads it)
_GETTER = [vp, C.c_int, C.POINTER(vp), C.POINTER(i64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
# (restype, argtypes) of every bez_sim_* entry point of include/bez_sim.h (the bez_ppo_* ones of the same library: ppo/fused.py)
SIGS = {
    "bez_sim_default_config": (C.c_int, [C.POINTER(abi.BezSimConfig), i32]),
    "bez_sim_create": (C.c_int, [C.POINTER(abi.BezSimConfig), C.c_int, C.POINTER(vp)]),
    "bez_sim_destroy": (C.c_int, [vp]),
    "bez_sim_last_error": (C.c_char_p, [vp]),
    "bez_sim_get_tensor": (C.c_int, _GETTER),
    "bez_sim_refresh_tensor": (C.c_int, [vp, C.c_int, vp]),
    "bez_sim_get_episode_tensor": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(i64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "bez_sim_set_actor_root_state_tensor_indexed": (C.c_int, [vp, fp, vp, i32, vp]),
    "bez_sim_set_dof_state_tensor_indexed": (C.c_int, [vp, fp, vp, i32, vp]),
    "bez_sim_set_dof_position_target_tensor": (C.c_int, [vp, fp, vp]),
    "bez_sim_set_dof_position_target_tensor_indexed": (C.c_int, [vp, fp, vp, i32, vp]),
    "bez_sim_set_net_contact_force_tensor": (C.c_int, [vp, fp, vp]),
    "bez_sim_set_prev_lin_vel_tensor": (C.c_int, [vp, fp, vp]),
    "bez_sim_set_goal_tensor": (C.c_int, [vp, fp, vp]),
    "bez_sim_set_flags": (C.c_int, [vp, u32]),
    "bez_sim_set_obs_calls": (C.c_int, [vp, i64]),
    "bez_sim_pre_physics": (C.c_int, [vp, fp, vp]),
    "bez_sim_simulate": (C.c_int, [vp, vp]),
    "bez_sim_post_physics": (C.c_int, [vp, vp]),
    "bez_sim_observe_reward": (C.c_int, [vp, vp]),
    "bez_sim_step": (C.c_int, [vp, fp, vp]),
    "bez_sim_step_many": (C.c_int, [vp, fp, i32, vp]),
    "bez_sim_reset_indexed": (C.c_int, [vp, vp, i32, vp]),
    "bez_sim_set_env_params": (C.c_int, [vp, C.c_int, fp, vp]),
    "bez_sim_get_env_params": (C.c_int, [vp, C.c_int, fp, vp]),
    "bez_sim_set_randomization": (C.c_int, [vp, C.POINTER(abi.BezDrConfig), vp]),
    "bez_sim_dr_prelaunch": (C.c_int, [vp, vp]),
    "bez_sim_dr_step_args": (C.c_int, [vp, vp, i32]),
    "bez_sim_dr_cancel": (C.c_int, [vp]),
    "bez_sim_action_noise_source": (C.c_int, [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(i64)]),
    "bez_sim_add_dr_noise": (C.c_int, [vp, fp, fp, i64, i32, vp]),
    "bez_sim_seed": (C.c_int, [vp, u64]),
    "bez_sim_health": (C.c_int, [vp, C.POINTER(u64), i32, vp]),
    "bez_sim_calibrate": (C.c_int, [vp, u64, i32, vp]),
    "bez_sim_time_steps": (C.c_int, [vp, fp, i32, vp, C.POINTER(C.c_float)]),
    "bez_sim_apply_body_forces": (C.c_int, [vp, fp, fp, fp, i32, vp]),
    "bez_sim_get_actuator_tensor": (C.c_int, _GETTER),
    "bez_sim_refresh_actuator_tensors": (C.c_int, [vp, vp]),
    "bez_sim_get_dynamics_tensor": (C.c_int, _GETTER),
    "bez_sim_refresh_dynamics_tensors": (C.c_int, [vp, u32, vp]),
    "bez_sim_inverse_dynamics": (C.c_int, [vp, fp, u32, fp, vp]),
    "bez_sim_forward_dynamics": (C.c_int, [vp, fp, u32, u32, fp, vp]),
    "bez_sim_operational_space": (C.c_int, [vp, C.POINTER(abi.BezOpSpaceParams), fp, fp, fp, fp, vp]),
    "bez_sim_centroidal": (C.c_int, [vp, fp, fp, vp]),
    "bez_sim_body_accelerations": (C.c_int, [vp, fp, u32, i32, fp, vp]),
    "bez_sim_generalized_forces": (C.c_int, [vp, fp, fp, fp, i32, fp, vp]),
    "bez_sim_limb_ik": (C.c_int, [vp, fp, C.POINTER(abi.BezIkParams), fp, fp, vp]),
    "bez_sim_proximity": (C.c_int, [vp, fp, fp, fp, vp]),
}
EXPORTS = list(SIGS)
# the bez_query_state_* entry points of the same header ("Query states"): sim, query state, ...
QUERY_STATE_SIGS = {
    "bez_query_state_create": (C.c_int, [vp, i32, C.POINTER(vp)]),
    "bez_query_state_destroy": (C.c_int, [vp, vp]),
    "bez_query_state_set": (C.c_int, [vp, vp, fp, fp, fp, vp, vp]),
    "bez_query_state_capture": (C.c_int, [vp, vp, vp, vp]),
    "bez_query_state_bind": (C.c_int, [vp, vp]),
    "bez_query_state_tensor": (C.c_int, [vp, vp] + _GETTER[1:]),
    "bez_query_state_refresh": (C.c_int, [vp, vp, u32, vp]),
}
# the bez_snapshot_* entry points of the same header ("Env snapshots"): sim, snapshot, ...
SNAPSHOT_SIGS = {
    "bez_snapshot_create": (C.c_int, [vp, i32, C.POINTER(vp)]),
    "bez_snapshot_destroy": (C.c_int, [vp, vp]),
    "bez_snapshot_save": (C.c_int, [vp, vp, vp, vp]),
    "bez_snapshot_restore": (C.c_int, [vp, vp, vp, vp, i32, u32, vp]),
    "bez_snapshot_export": (C.c_int, [vp, vp, vp, C.POINTER(i64), vp]),
    "bez_snapshot_import": (C.c_int, [vp, vp, vp, i64, vp]),
}
# the entry points a binding redirects (include/bez_sim.h): what a QueryState brackets with bind / unbind
BOUND_QUERIES = ("bez_sim_inverse_dynamics", "bez_sim_forward_dynamics", "bez_sim_operational_space", "bez_sim_centroidal",
                 "bez_sim_body_accelerations", "bez_sim_generalized_forces", "bez_sim_limb_ik", "bez_sim_proximity")


def load_library():
    """dlopen libbez_sim.so and declare every entry point of include/bez_sim.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise BezSimError("libbez_sim.so not built (%s): run `python -m bez_isaacgym_amd.build` -- "
                          "the HIP extension is required, there is no fallback path" % path)
    lib = C.CDLL(path)
    for name, (res, args) in list(SIGS.items()) + list(QUERY_STATE_SIGS.items()) + list(SNAPSHOT_SIGS.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _LIB = lib
    return lib


class _DevView:
    """__cuda_array_interface__ holder: lets torch wrap a sim-owned device buffer zero-copy
    (the gymtorch.wrap_tensor equivalent, kick_env.py:155-157)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner  # keeps the sim alive as long as the view lives


class BezSim:
    """One simulator instance on one GPU (one per process / rank)."""

    _flags_set = None   # the flags the library holds after the last set_flags(); None: cfg.flags as created

    def __init__(self, cfg: abi.BezSimConfig, device_id: int = 0):
        if not torch.cuda.is_available():
            raise BezSimError("no GPU visible: the bez_kick simulator is HIP-only (sim_device must be a GPU)")
        self.lib = load_library()
        self.cfg = cfg
        self.device_id = int(device_id)
        self.device = torch.device("cuda", self.device_id)
        self.num_envs = int(cfg.num_envs)
        self.has_ball = int(cfg.task) == abi.TASK_KICK
        h = C.c_void_p()
        rc = self.lib.bez_sim_create(C.byref(cfg), self.device_id, C.byref(h))
        if rc != 0:
            raise BezSimError("bez_sim_create failed (%d): %s" % (rc, self.lib.bez_sim_last_error(None).decode()))
        self.h = h
        self._views = {}
        # the layout is the library's: shapes as bez_sim_get_tensor reports them for this task and asset
        self._shape = {w: self._describe(self.lib.bez_sim_get_tensor, w)[1] for w in range(abi.TENSOR_COUNT)}
        self.num_actors = self._shape[abi.TENSOR_ROOT_STATE][0] // self.num_envs
        self.num_bodies = self._shape[abi.TENSOR_RIGID_BODY_STATE][0] // self.num_envs
        self.num_obs = self._shape[abi.TENSOR_OBS][1]

    def close(self):
        if getattr(self, "h", None):
            self._views = {}
            for qs in self.__dict__.pop("_query_states", []):   # bez_sim_destroy frees them: their objects only forget the handles
                qs._forget()
            for snap in self.__dict__.pop("_snapshots", []):
                snap._forget()
            self.lib.bez_sim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _check(self, rc):
        if rc != 0:
            raise BezSimError("libbez_sim call failed (%d): %s" % (rc, self.lib.bez_sim_last_error(self.h).decode()))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _ptr(self, t, dtype, numel=None):
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous():
            raise BezSimError("expected a contiguous %s tensor on %s, got %s on %s" % (dtype, self.device, t.dtype, t.device))
        if numel is not None and t.numel() != numel:
            raise BezSimError("expected %d elements, got %d" % (numel, t.numel()))
        return C.c_void_p(t.data_ptr())

    def _checked(self, name, t, shapes):
        """t, once it is known to be a torch tensor of one of `shapes`"""
        if not isinstance(t, torch.Tensor):
            raise BezSimError("%s: expected a torch tensor, got %s" % (name, type(t).__name__))
        if tuple(t.shape) not in shapes:
            raise BezSimError("%s: expected shape %s, got %s" % (name, " or ".join(str(s) for s in shapes), tuple(t.shape)))
        return t

    # the query calls resolve their tensors in two steps, every method in the same order: first _in / _out / _wanted for each argument
    # (is it a tensor, has it an accepted shape -- the shape fixes the element count --, which buffer takes a result), then, when
    # every other argument is checked too, _f32 for each pointer (dtype, layout, device)
    def _in(self, name, t, *shapes):
        """an optional input: None, or t once it is _checked against the shapes it may have"""
        return None if t is None else self._checked(name, t, shapes)

    def _out(self, name, t, key, shape):
        """an output: the caller's tensor once it is _checked against `shape`; None: the sim's own float32 result buffer `key` of that
        shape, allocated by the first call that needs it, overwritten by every later one"""
        if t is not None:
            return self._checked(name, t, (shape,))
        bufs = self.__dict__.setdefault("_buffers", {})
        if key not in bufs:
            bufs[key] = torch.zeros(shape, device=self.device, dtype=torch.float32)
        return bufs[key]

    def _f32(self, t):
        """what the library is handed for a resolved tensor: NULL for None, else the pointer of a contiguous float32 tensor on the device"""
        return None if t is None else self._ptr(t, torch.float32)

    def _wanted(self, method, shapes, given, want, prefix, refused=None):
        """The outputs of a call that computes a chosen subset of them.  `shapes`: output name -> shape, in the library's order;
        `given`: (keyword, tensor or None) per output in that order, a given tensor is wanted and written; `want`: the names (or one
        name) to compute into the scratch buffers `prefix` + name; `refused`: None or (name, why) of an output this call must not want.
        Returns ({name: tensor or None}, [pointer or NULL per output])."""
        if isinstance(want, str):
            want = (want,)
        for k in want:
            if k not in shapes:
                raise BezSimError("%s: want holds %r, expected a subset of %s" % (method, k, tuple(shapes)))
        out = {name: (name in want or None) if t is None else self._checked(keyword, t, (shapes[name],)) for name, (keyword, t) in zip(shapes, given)}
        if all(t is None for t in out.values()):
            raise BezSimError("%s: nothing is wanted (want is empty and no output tensor is given)" % method)
        if refused is not None and out[refused[0]] is not None:
            raise BezSimError("%s: %s" % (method, refused[1]))
        ptrs = []
        for name, t in out.items():
            if t is True:
                t = out[name] = self._out(name, None, prefix + name, shapes[name])
            ptrs.append(self._f32(t))
        return out, ptrs

    def _body_vectors(self, forces, torques, positions):
        """the pointers (NULL for None) of the three per-body vector tensors of apply_body_forces and generalized_forces, each float32 on
        the sim's device, contiguous, (N*B, 3) or (N, B, 3)"""
        n, nb = self.num_envs, self.num_bodies
        shapes = ((n * nb, 3), (n, nb, 3))
        return [None if t is None else self._ptr(self._checked(name, t, shapes), torch.float32)
                for name, t in (("forces", forces), ("torques", torques), ("positions", positions))]

    def _describe(self, getter, which):
        """(device pointer, shape, typestr) of a sim-owned buffer"""
        p, shape, nd, dt = C.c_void_p(), (C.c_int64 * 3)(), C.c_int(), C.c_int()
        self._check(getter(self.h, which, C.byref(p), shape, C.byref(nd), C.byref(dt)))
        return p.value, tuple(int(shape[i]) for i in range(nd.value)), {abi.DTYPE_F32: "<f4", abi.DTYPE_I64: "<i8", abi.DTYPE_I32: "<i4"}[dt.value]

    def _wrap(self, key, getter, which):
        if key not in self._views:
            p, shp, typestr = self._describe(getter, which)
            view = _DevView(p, shp, typestr, self)
            with torch.cuda.device(self.device):
                self._views[key] = torch.as_tensor(view, device=self.device)
        return self._views[key]

    def tensor(self, which):
        """Zero-copy torch view of a sim-owned buffer (gymtorch.wrap_tensor)."""
        return self._wrap(which, self.lib.bez_sim_get_tensor, which)

    def episode_tensor(self, which):
        """Zero-copy, always-live torch view of an episode statistic (abi.EPISODE_*): END_BITS (N,) int32, END_COUNTS (8, N) int64
        [cause][env] (never cleared by the library: take deltas), REWARD_TERMS (8, N) float32 [slot][env] (the caller zeroes it)."""
        return self._wrap(("episode", int(which)), self.lib.bez_sim_get_episode_tensor, which)

    # ---- gym.acquire_dof_force_tensor / refresh_dof_force_tensor (abi.FLAG_DOF_FORCE)
    @property
    def dof_force_enabled(self):
        flags = int(self.cfg.flags) if self._flags_set is None else self._flags_set
        return bool(flags & abi.FLAG_DOF_FORCE)

    def _need_dof_force(self, what):
        if not self.dof_force_enabled:
            raise BezSimError("%s needs abi.FLAG_DOF_FORCE (task key %s: True): without it the step kernels record no joint forces"
                              % (what, abi.DOF_FORCE_KEY))

    def actuator_tensor(self, which):
        """Zero-copy torch view of an actuator tensor (abi.ACTUATOR_* or "dof_force" / "drive_torque" / "status"), shape (N*18,) in
        DOF_STATE order: DOF_FORCE and DRIVE_TORQUE float32, STATUS int32.  Filled by refresh_actuator_tensors()."""
        which = abi.actuator_tensor_id(which)
        self._need_dof_force("actuator_tensor()")
        return self._wrap(("actuator", which), self.lib.bez_sim_get_actuator_tensor, which)

    def refresh_actuator_tensors(self):
        """gym.refresh_dof_force_tensor: materialises the three actuator tensors from what the last physics launch recorded."""
        self._need_dof_force("refresh_actuator_tensors()")
        self._check(self.lib.bez_sim_refresh_actuator_tensors(self.h, self._stream()))

    # ---- gym.acquire_jacobian_tensor / acquire_mass_matrix_tensor and their refreshes
    def dynamics_tensor(self, which):
        """Zero-copy torch view of a dynamics tensor (abi.DYNAMICS_* or "jacobian" / "mass_matrix"): the Jacobian (N*NB, 6, 24) of the
        robot's NB bodies, the mass matrix (N, 24, 24), both float32 (definitions: include/bez_sim.h).  The first call for a tensor
        allocates it; refresh_dynamics_tensors() fills it."""
        which = abi.dynamics_tensor_id(which)
        return self._wrap(("dynamics", which), self.lib.bez_sim_get_dynamics_tensor, which)

    def refresh_dynamics_tensors(self, which=None):
        """gym.refresh_jacobian_tensors / refresh_mass_matrix_tensors in one launch on the current stream.  `which`: one tensor or a
        sequence of them (ids or names); None: every tensor acquired so far.  A tensor that was never acquired is an error."""
        if which is None:
            ids = [k[1] for k in self._views if isinstance(k, tuple) and k[0] == "dynamics"]
        elif isinstance(which, (str, int)):
            ids = [abi.dynamics_tensor_id(which)]
        else:
            ids = [abi.dynamics_tensor_id(w) for w in which]
        mask = 0
        for k in ids:
            mask |= 1 << k
        self._check(self.lib.bez_sim_refresh_dynamics_tensors(self.h, mask, self._stream()))

    # ---- inverse dynamics: M(q) udot + h(q, u) of the current state without forming M
    def inverse_dynamics(self, udot=None, terms=abi.ID_ALL, out=None):
        """(N, 24) float32: the sum of the terms of M udot + h selected by `terms` (abi.ID_INERTIA | ID_VELOCITY | ID_GRAVITY), in the
        dynamics tensors' coordinates u = [root_lin, root_ang, qd]: rows 0:3 force, 3:6 moment about the root origin (world axes), 6:24
        joint torques (include/bez_sim.h "Inverse dynamics").  `udot`: (N, 24) float32 on the sim's device, contiguous, or None for zero.
        `out`: the same kind of tensor to write into; None: one buffer per sim, allocated by the first such call and overwritten by
        every later one.  One launch on the current stream."""
        shape = (self.num_envs, abi.NUM_GEN)
        udot, out = self._in("udot", udot, shape), self._out("out", out, "inverse_dynamics", shape)
        self._check(self.lib.bez_sim_inverse_dynamics(self.h, self._f32(udot), int(terms), self._f32(out), self._stream()))
        return out

    # ---- forward dynamics: udot = M(q)^-1 (f - h(q, u)) of the current state without forming M
    def forward_dynamics(self, force=None, bias=abi.ID_VELOCITY | abi.ID_GRAVITY, fixed_base=False, out=None):
        """(N, 24) float32: udot = M^-1 (f - h), the accelerations that the generalised force `force` produces on the current state, in
        the coordinates and rows of inverse_dynamics (include/bez_sim.h "Forward dynamics").  `force`: (N, 24) float32 on the sim's
        device, contiguous, or None for zero.  `bias`: the terms of h taken off the force, a subset of abi.ID_VELOCITY | ID_GRAVITY; 0
        with a force is the plain mass solve M^-1 f.  `fixed_base`: hold the root -- rows 0:6 are zero and rows 6:24 solve the joint
        block alone.  `out`: the same kind of tensor to write into (it may be `force`); None: one buffer per sim, allocated by the first
        such call and overwritten by every later one.  One launch on the current stream; everything is checked before the library is
        called."""
        shape = (self.num_envs, abi.NUM_GEN)
        force, out = self._in("force", force, shape), self._out("out", out, "forward_dynamics", shape)
        bias = int(bias)
        if bias & ~(abi.ID_VELOCITY | abi.ID_GRAVITY):
            raise BezSimError("forward_dynamics: bias must be a subset of abi.ID_VELOCITY | abi.ID_GRAVITY, got %d" % bias)
        if bias == 0 and force is None:
            raise BezSimError("forward_dynamics: bias is 0 and force is None (nothing to solve for)")
        self._check(self.lib.bez_sim_forward_dynamics(self.h, self._f32(force), bias, abi.FD_FIXED_BASE if fixed_base else 0, self._f32(out),
                                                      self._stream()))
        return out

    # ---- operational space: end-frame Jacobians, J M^-1, the Delassus matrix J M^-1 J^T and the operational-space inertias
    def operational_space(self, offsets=None, fixed_base=False, jac=None, jminv=None, w=None, lam=None, want=("jac", "jminv", "w", "lambda")):
        """(jac, jminv, w, lam) of the current state in one launch on the current stream (include/bez_sim.h "Operational space"), for the
        five frames limb_ik controls (abi.IK_CHAIN_NAMES, end bodies abi.IK_END_BODIES, each displaced by `offsets[c]` in the body's axes;
        (5, 3) or None for zero).  jac (N, 5, 6, 24) float32: J_c in u = [root_lin, root_ang, qd], rows [linear; angular] in world axes.
        jminv (N, 5, 6, 24): J_c M^-1.  w (N, 30, 30): J_E M^-1 J_E^T, block (a, b) 6 x 6 in chain order, bitwise symmetric.  lam
        (N, 5, 6, 6): W_cc^-1.  `fixed_base`: hold the root (M becomes M[6:, 6:]; the off-diagonal blocks of w and jminv[..., 0:6] are
        zero); W_cc is then singular by structure and "lambda" must not be wanted.  `want`: which of the four to compute; an output that
        is not wanted is None in the result and is not written.  `jac`, `jminv`, `w`, `lam`: contiguous float32 tensors on the sim's device
        to write into (a given tensor is wanted); None: one buffer of each kind per sim, allocated by the first call that needs it and
        overwritten by every later one.  Everything is checked before the library is called."""
        n = self.num_envs
        shapes = {"jac": (n, abi.IK_CHAINS, 6, abi.NUM_GEN), "jminv": (n, abi.IK_CHAINS, 6, abi.NUM_GEN),
                  "w": (n, 6 * abi.IK_CHAINS, 6 * abi.IK_CHAINS), "lambda": (n, abi.IK_CHAINS, 6, 6)}
        try:
            params = abi.op_space_params(offsets, fixed_base)
        except ValueError as e:
            raise BezSimError("operational_space: %s" % e)
        held = ("lambda", "'lambda' with fixed_base (W_cc of a held root is singular by structure)") if fixed_base else None
        out, ptrs = self._wanted("operational_space", shapes, (("jac", jac), ("jminv", jminv), ("w", w), ("lam", lam)), want, "operational_space_", held)
        self._check(self.lib.bez_sim_operational_space(self.h, C.byref(params), *ptrs, self._stream()))
        return out["jac"], out["jminv"], out["w"], out["lambda"]

    # ---- centroidal dynamics: centre of mass, momentum about it, the momentum matrix A_G, mechanical energy
    def centroidal(self, state=None, matrix=None, want_matrix=False):
        """(state, matrix) of the current state in one launch on the current stream (include/bez_sim.h "Centroidal dynamics").
        state (N, 16) float32: the abi.CM_* words -- COM 0:3, COM_VEL 3:6, LIN_MOM 6:9, ANG_MOM (about the centre of mass) 9:12, MASS,
        KINETIC, POTENTIAL.  matrix (N, 6, 24) float32: A_G with matrix @ u == [LIN_MOM; ANG_MOM], u = [root_lin, root_ang, qd]; it is
        written only when a `matrix` tensor is given or want_matrix is set, and is None in the result otherwise.  `state`, `matrix`:
        contiguous float32 tensors on the sim's device to write into; None: one buffer of each kind per sim, allocated by the first
        call that needs it and overwritten by every later one."""
        state = self._out("state", state, "centroidal_state", (self.num_envs, abi.CM_WORDS))
        if matrix is not None or want_matrix:
            matrix = self._out("matrix", matrix, "centroidal_matrix", (self.num_envs, 6, abi.NUM_GEN))
        self._check(self.lib.bez_sim_centroidal(self.h, self._f32(state), self._f32(matrix), self._stream()))
        return state, matrix

    # ---- body accelerations: J udot + Jdot u of every rigid body of the robot, and what an accelerometer on it reads
    def body_accelerations(self, udot=None, terms=abi.ACC_MOTION, space=abi.SPACE_ENV, out=None):
        """(N, NB, 6) float32: the sum of the terms selected by `terms` (abi.ACC_UDOT | ACC_VELOCITY | ACC_GRAVITY) for the robot's NB
        bodies in RIGID_BODY_STATE order, no ball row (include/bez_sim.h "Body accelerations").  Rows 0:3: the acceleration of the body's
        origin, rows 3:6: its angular acceleration -- the time derivatives of RIGID_BODY_STATE[:, 7:10] and [:, 10:13] for ACC_MOTION;
        ACC_UDOT alone is J @ udot, ACC_VELOCITY alone Jdot @ u, ACC_GRAVITY adds -g to rows 0:3.  `udot`: (N, 24) float32 on the sim's
        device, contiguous, or None for zero.  `space`: abi.SPACE_ENV / abi.SPACE_LOCAL or "env" / "local" (world axes / the body's own
        frame).  `out`: a tensor of the result's kind to write into; None: one buffer per sim, allocated by the first such call and
        overwritten by every later one.  One launch on the current stream."""
        space = abi.body_force_space(space)
        n, nb = self.num_envs, self.num_bodies - (1 if self.has_ball else 0)
        udot, out = self._in("udot", udot, (n, abi.NUM_GEN)), self._out("out", out, "body_accelerations", (n, nb, 6))
        self._check(self.lib.bez_sim_body_accelerations(self.h, self._f32(udot), int(terms), space, self._f32(out), self._stream()))
        return out

    # ---- generalised forces: sum over bodies of J_b^T [f; t], the map from wrenches on rigid bodies to forces on u
    def generalized_forces(self, forces=None, torques=None, positions=None, space=abi.SPACE_ENV, at="com", out=None):
        """(N, 24) float32: the generalised force of wrenches on the rigid bodies, in u = [root_lin, root_ang, qd] -- rows 0:3 the total
        force, 3:6 the total moment about the root origin (world axes), 6:24 the joint torques, the rows of inverse_dynamics (include/bez_sim.h
        "Generalised forces").  `forces`, `torques`, `positions`, `space`: what apply_body_forces takes -- float32 on the sim's device,
        contiguous, (N*B, 3) or (N, B, 3) in RIGID_BODY_STATE order (the ball's row included where the task has one, never read), or None;
        forces and torques must not both be None.  `at`: where a wrench acts when `positions` is None: "com", the body's centre of mass
        (as apply_body_forces), or "origin", the body's origin -- the result is then J^T [f; t] with the Jacobian tensor's J.  `out`: a
        tensor of the result's kind to write into; None: one buffer per sim, allocated by the first such call and overwritten by every
        later one.  One launch on the current stream; everything is checked before the library is called."""
        space = abi.generalized_force_space(space, at)
        if forces is None and torques is None:
            raise BezSimError("generalized_forces: forces and torques are both None (nothing to map)")
        if positions is not None and space & abi.GF_AT_ORIGIN:
            raise BezSimError("generalized_forces: at='origin' is the point of application when positions is None")
        ptrs = self._body_vectors(forces, torques, positions)
        out = self._out("out", out, "generalized_forces", (self.num_envs, abi.NUM_GEN))
        self._check(self.lib.bez_sim_generalized_forces(self.h, *ptrs, space, self._f32(out), self._stream()))
        return out

    # ---- limb inverse kinematics: damped least squares on each of the five chains off the torso
    def limb_ik(self, targets, weights, offsets=None, damping=0.05, max_step=0.0, iters=1, space="env", out=None, err_out=None):
        """(q, err): q (N, 18) float32 joint angles in DOF_STATE order after `iters` damped-least-squares iterations per chain from the
        current state's q, err (N, 5, 6) the pose error [position; 2 sin(theta/2) axis] at that q, in the root's axes (include/bez_sim.h
        "Limb inverse kinematics").  `targets`: (N, 5, 7) float32 on the sim's device, contiguous: per chain (abi.IK_CHAIN_NAMES) the wanted
        position and quaternion xyzw of the controlled frame -- space "env": as RIGID_BODY_STATE rows carry them; "root": relative to the
        root origin in the root's axes.  `weights` (5, 2) [w_pos, w_rot] >= 0 per chain, both 0: the chain is left alone; `offsets` (5, 3)
        or None: the controlled frame is the chain's end body (abi.IK_END_BODIES) displaced by this in its own frame; `damping` lambda > 0;
        `max_step` > 0: the largest |dq_i| of one iteration, <= 0: none; `iters` 0 .. abi.IK_MAX_ITERS (0: the pose error of the current
        state).  `out`, `err_out`: tensors of the results' kinds to write into; None: one buffer of each kind per sim, allocated by the
        first such call and overwritten by every later one.  The state is untouched.  One launch on the current stream; everything is
        checked before the library is called."""
        try:
            params = abi.ik_params(weights, offsets, damping, max_step, iters, space)
        except ValueError as e:
            raise BezSimError("limb_ik: %s" % e)
        n = self.num_envs
        self._checked("targets", targets, ((n, abi.IK_CHAINS, 7), (n * abi.IK_CHAINS, 7)))
        out, err_out = self._out("out", out, "limb_ik_q", (n, abi.NUM_DOFS)), self._out("err_out", err_out, "limb_ik_err", (n, abi.IK_CHAINS, 6))
        self._check(self.lib.bez_sim_limb_ik(self.h, self._f32(targets), C.byref(params), self._f32(out), self._f32(err_out), self._stream()))
        return out, err_out

    # ---- proximity: the contact geometry of the step -- ground points, ball against boxes, leg against leg -- as distances
    def proximity(self, ground=None, ball=None, pairs=None, want=("ground", "ball", "pairs")):
        """(ground, ball, pairs) of the current state in one launch on the current stream (include/bez_sim.h "Proximity").
        ground (N, 23, 3) float32: the asset's 22 ground points in env coordinates (abi.PROX_GROUND_NAMES; z < 0 is the step's contact
        decision) and, row abi.PROX_BALL_ROW, the ball's lowest point.  ball (N, 11, 8): per box (abi.PROX_BOX_BODIES) [gap, normal 3,
        point 3, 0] -- the signed distance of the ball's surface to the box, the world normal from the box to the ball, the closest point
        of the box in env coordinates.  pairs (N, 28, 8): per capsule pair (abi.PROX_PAIR_BODIES, a on the left leg) the same words -- the
        signed distance of the two capsules, the normal from b to a, the step's contact point.  `want`: which of the three to compute; an
        output that is not wanted is None in the result and is not written.  `ground`, `ball`, `pairs`: contiguous float32 tensors on
        the sim's device to write into (a given tensor is wanted); None: one buffer of each kind per sim, allocated by the first call
        that needs it and overwritten by every later one."""
        n = self.num_envs
        shapes = {"ground": (n, abi.PROX_GROUND_ROWS, 3), "ball": (n, abi.PROX_BOXES, abi.PROX_WORDS), "pairs": (n, abi.PROX_PAIRS, abi.PROX_WORDS)}
        out, ptrs = self._wanted("proximity", shapes, (("ground", ground), ("ball", ball), ("pairs", pairs)), want, "proximity_")
        self._check(self.lib.bez_sim_proximity(self.h, *ptrs, self._stream()))
        return out["ground"], out["ball"], out["pairs"]

    # ---- query states: the queries above on states the caller supplies (include/bez_sim.h "Query states")
    def query_state(self, rows):
        """A QueryState of `rows` rows (>= 1, independent of N) owned by this sim: fill it with set() or capture(), then ask it what this
        sim is asked -- the live state is never written.  close() frees it; closing the sim frees the ones still open."""
        if isinstance(rows, bool) or not isinstance(rows, int) or rows < 1:
            raise BezSimError("query_state: rows must be an int >= 1, got %r" % (rows,))
        qs = QueryState(self, rows)
        self.__dict__.setdefault("_query_states", []).append(qs)
        return qs

    # ---- env snapshots: whole envs saved and put back (include/bez_sim.h "Env snapshots")
    def snapshot(self, rows):
        """A Snapshot of `rows` rows (>= 1, independent of N) owned by this sim: save() copies envs into it, restore() copies rows back into
        envs of this sim or of another one of the same task and asset.  close() frees it; closing the sim frees the ones still open."""
        if isinstance(rows, bool) or not isinstance(rows, int) or rows < 1:
            raise BezSimError("snapshot: rows must be an int >= 1, got %r" % (rows,))
        snap = Snapshot(self, rows)
        self.__dict__.setdefault("_snapshots", []).append(snap)
        return snap

    def refresh(self, which):
        self._check(self.lib.bez_sim_refresh_tensor(self.h, which, self._stream()))
        return self.tensor(which)

    # ---- gym.set_* equivalents: `src` is the full tensor in the layout of tensor `which`; actor_ids picks the rows an indexed setter takes
    def _set(self, fn, which, src, actor_ids=None):
        args = [self._ptr(src, torch.float32, torch.Size(self._shape[which]).numel())]
        if actor_ids is not None:
            args += [self._ptr(actor_ids, torch.int32), actor_ids.numel()]
        self._check(fn(self.h, *args, self._stream()))

    def set_actor_root_state_tensor_indexed(self, root_states, actor_ids):
        self._set(self.lib.bez_sim_set_actor_root_state_tensor_indexed, abi.TENSOR_ROOT_STATE, root_states, actor_ids)

    def set_dof_state_tensor_indexed(self, dof_state, actor_ids):
        self._set(self.lib.bez_sim_set_dof_state_tensor_indexed, abi.TENSOR_DOF_STATE, dof_state, actor_ids)

    def set_dof_position_target_tensor(self, targets):
        self._set(self.lib.bez_sim_set_dof_position_target_tensor, abi.TENSOR_DOF_TARGET, targets)

    def set_dof_position_target_tensor_indexed(self, targets, actor_ids):
        self._set(self.lib.bez_sim_set_dof_position_target_tensor_indexed, abi.TENSOR_DOF_TARGET, targets, actor_ids)

    def set_net_contact_force_tensor(self, forces):
        self._set(self.lib.bez_sim_set_net_contact_force_tensor, abi.TENSOR_NET_CONTACT_FORCE, forces)

    def set_prev_lin_vel_tensor(self, prev):
        self._set(self.lib.bez_sim_set_prev_lin_vel_tensor, abi.TENSOR_PREV_LIN_VEL, prev)

    def set_goal_tensor(self, goal):
        self._set(self.lib.bez_sim_set_goal_tensor, abi.TENSOR_GOAL, goal)

    def set_flags(self, flags):
        self._check(self.lib.bez_sim_set_flags(self.h, int(flags)))
        asset = abi.FLAG_CLEATS | abi.FLAG_BOX_ASSET   # (the library keeps the creation value of the asset bits)
        self._flags_set = (int(flags) & ~asset) | (int(self.cfg.flags) & asset)   # cfg.flags stays the caller's: callers restore flags from it

    # ---- gym.apply_rigid_body_force_tensors / apply_rigid_body_force_at_pos_tensors
    def apply_body_forces(self, forces=None, torques=None, positions=None, space=abi.SPACE_ENV):
        """External forces / torques on the rigid bodies for the NEXT physics launch only (include/bez_sim.h: bez_sim_apply_body_forces).
        Each tensor: float32 on the sim's device, contiguous, (N*B, 3) or (N, B, 3) in RIGID_BODY_STATE order, or None.  `space`:
        abi.SPACE_ENV / abi.SPACE_LOCAL or "env" / "local".  Everything is checked before the library is called."""
        space = abi.body_force_space(space)
        self._check(self.lib.bez_sim_apply_body_forces(self.h, *self._body_vectors(forces, torques, positions), space, self._stream()))

    # ---- the non-finite guard (abi.FLAG_NONFINITE_GUARD)
    def health(self, clear=False):
        """The health word (abi.HEALTH_* bits), read synchronously on the current stream; `clear` zeroes it after the read."""
        bits = C.c_uint64()
        self._check(self.lib.bez_sim_health(self.h, C.byref(bits), 1 if clear else 0, self._stream()))
        return int(bits.value)

    @property
    def nonfinite_counts(self):
        """(N,) int64 zero-copy view: how often each env tripped the guard (never cleared by the library; writable)."""
        return self.tensor(abi.TENSOR_NONFINITE_COUNT)

    def set_obs_calls(self, n):
        self._check(self.lib.bez_sim_set_obs_calls(self.h, int(n)))

    # ---- the path
    def pre_physics(self, actions):
        self._check(self.lib.bez_sim_pre_physics(self.h, self._ptr(actions, torch.float32, self.num_envs * abi.NUM_DOFS), self._stream()))

    def simulate(self):
        self._check(self.lib.bez_sim_simulate(self.h, self._stream()))

    def post_physics(self):
        self._check(self.lib.bez_sim_post_physics(self.h, self._stream()))

    def observe_reward(self):
        self._check(self.lib.bez_sim_observe_reward(self.h, self._stream()))

    def step(self, actions):
        self._check(self.lib.bez_sim_step(self.h, self._ptr(actions, torch.float32, self.num_envs * abi.NUM_DOFS), self._stream()))

    def step_many(self, actions, n_steps):
        self._check(self.lib.bez_sim_step_many(self.h, self._ptr(actions, torch.float32, n_steps * self.num_envs * abi.NUM_DOFS),
                                               n_steps, self._stream()))

    def time_steps(self, actions, n_steps):
        ms = C.c_float()
        self._check(self.lib.bez_sim_time_steps(self.h, self._ptr(actions, torch.float32, n_steps * self.num_envs * abi.NUM_DOFS),
                                                n_steps, self._stream(), C.byref(ms)))
        return float(ms.value)

    def reset_indexed(self, env_ids):
        self._check(self.lib.bez_sim_reset_indexed(self.h, self._ptr(env_ids, torch.int32), env_ids.numel(), self._stream()))

    def set_env_params(self, param, values):
        ptr = None if values is None else self._ptr(values, torch.float32, self.num_envs * abi.PARAM_WIDTH[param])
        self._check(self.lib.bez_sim_set_env_params(self.h, param, ptr, self._stream()))

    def get_env_params(self, param):
        """current (N, width) array of a domain-randomisation parameter (defaults where never set)"""
        out = torch.empty(self.num_envs, abi.PARAM_WIDTH[param], device=self.device, dtype=torch.float32)
        self._check(self.lib.bez_sim_get_env_params(self.h, param, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def set_randomization(self, dr):
        """device-side VecTask.apply_randomizations: `dr` is an abi.BezDrConfig (abi.dr_config_from_params) or None (off)"""
        self._dr_cfg = dr  # keep the struct alive for the call
        self._check(self.lib.bez_sim_set_randomization(self.h, None if dr is None else C.byref(dr), self._stream()))

    def add_dr_noise(self, x, which, out=None):
        """out = x + mean + std * N(0, 1) with the device-resident noise parameters (which: 0 observations, 1 actions); out=None: in place"""
        out = x if out is None else out
        self._check(self.lib.bez_sim_add_dr_noise(self.h, self._ptr(x, torch.float32), self._ptr(out, torch.float32, x.numel()), x.numel(), int(which), self._stream()))
        return out

    def dr_prelaunch(self):
        """The coming step's randomisation kernel now, on torch's current stream (bez_sim_dr_prelaunch): the step then skips its own."""
        self._check(self.lib.bez_sim_dr_prelaunch(self.h, self._stream()))

    def dr_step_args(self):
        """The coming step's randomisation as an opaque argument block (ctypes buffer, BEZ_DR_STEP_BYTES) for a launch of the caller's that
        executes it itself (PolicyForward.rollout_step(dr_step=)); the step then skips its own kernel.  None without a randomisation."""
        blob = (C.c_uint8 * 512)()
        rc = self.lib.bez_sim_dr_step_args(self.h, blob, 512)
        if rc < 0:
            self._check(rc)
        return blob if rc > 0 else None

    def dr_cancel(self):
        """The consumer of dr_prelaunch() / dr_step_args() did not run: the coming step launches its own randomisation kernel again."""
        self._check(self.lib.bez_sim_dr_cancel(self.h))

    def action_noise_source(self):
        """(device pointer of the action-noise snapshot, seed, env id offset) for a consumer that adds the action noise itself, or None
        when the randomisation has no action noise (bez_sim_action_noise_source)"""
        p, seed, off = C.c_void_p(), C.c_uint64(), C.c_int64()
        rc = self.lib.bez_sim_action_noise_source(self.h, C.byref(p), C.byref(seed), C.byref(off))
        if rc < 0:
            self._check(rc)
        return (p.value, seed.value, off.value) if rc == 1 else None

    def seed(self, seed):
        self._check(self.lib.bez_sim_seed(self.h, int(seed)))


class _BoundLib:
    """The library as a QueryState calls it: an entry point of BOUND_QUERIES runs between bez_query_state_bind(sim, qs) and
    bez_query_state_bind(sim, NULL) -- the unbind also when the call raises --, every other one goes straight through."""

    def __init__(self, lib, sim_h, qs_h):
        self._lib, self._sim_h, self._qs_h = lib, sim_h, qs_h

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in BOUND_QUERIES:
            return fn

        def bound(*args):
            rc = self._lib.bez_query_state_bind(self._sim_h, self._qs_h)
            if rc != 0:
                return rc      # (nothing was bound: the query must not run on the live state in this object's name)
            try:
                return fn(*args)
            finally:
                self._lib.bez_query_state_bind(self._sim_h, None)   # (a successful call leaves the sim's error message alone)
        self.__dict__[name] = bound
        return bound


class QueryState:
    """A state of `rows` rows that the caller supplies, asked what a BezSim is asked (BezSim.query_state; include/bez_sim.h "Query
    states").  set() fills it from Isaac-layout rows, capture() from live envs; the query methods are BezSim's own, with `rows` in
    the place of N in every shape, and their result buffers are this object's.  Each of them binds the state, calls and unbinds."""

    def __init__(self, sim, rows):
        self.sim, self.rows, self.num_envs = sim, rows, rows   # (num_envs: what the shared methods size their tensors by)
        self.cfg, self.device, self.has_ball, self.num_bodies = getattr(sim, "cfg", None), sim.device, sim.has_ball, sim.num_bodies
        self._stream, self._views, self.h = sim._stream, {}, sim.h
        qs = C.c_void_p()
        sim._check(sim.lib.bez_query_state_create(sim.h, rows, C.byref(qs)))
        self.qs = qs
        self.lib = _BoundLib(sim.lib, sim.h, qs)

    # the query calls and the argument machinery under them are BezSim's functions, run on this object: nothing is written twice
    for _name in ("_check", "_ptr", "_checked", "_in", "_out", "_f32", "_wanted", "_body_vectors", "_describe", "_wrap", "inverse_dynamics",
                  "forward_dynamics", "operational_space", "centroidal", "body_accelerations", "generalized_forces", "limb_ik", "proximity"):
        locals()[_name] = getattr(BezSim, _name)
    del _name

    def _forget(self):
        self.qs, self._views = None, {}

    def close(self):
        if getattr(self, "qs", None) is not None:
            self._views = {}
            self._check(self.lib.bez_query_state_destroy(self.h, self.qs))
            self._forget()
            states = self.sim.__dict__.get("_query_states", [])
            if self in states:
                states.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _env_ids(self, env_ids):
        """the pointer of (rows,) int32 env ids on the device, NULL for None"""
        return None if env_ids is None else self._ptr(self._checked("env_ids", env_ids, ((self.rows,),)), torch.int32)

    def set(self, root, dof, ball=None, env_ids=None):
        """Fills every row: `root` (M, 13) as ROOT_STATE rows, `dof` (M, 18, 2) or (M*18, 2) as DOF_STATE rows, `ball` (M, 13) or None --
        None where the task has no ball (a tensor is refused there), the config's ball_init pose at rest on bez_kick.  float32 on the
        sim's device, contiguous; values are copied as given.  `env_ids` (M,) int32 or None: row i takes the mass-scale, gravity and
        joint-limit rows of env env_ids[i] as they are now (ids may repeat; an id outside 0 .. N-1: the default rows); None: the asset's
        nominal parameters for every row.  One launch on the current stream; everything is checked before the library is called."""
        m = self.rows
        root, dof = self._checked("root", root, ((m, 13),)), self._checked("dof", dof, ((m, abi.NUM_DOFS, 2), (m * abi.NUM_DOFS, 2)))
        ball = self._in("ball", ball, (m, 13))
        if ball is not None and not self.has_ball:
            raise BezSimError("query state set: ball given, but this task has no ball")
        ptrs = [self._f32(root), self._f32(dof), self._f32(ball), self._env_ids(env_ids)]
        self._check(self.lib.bez_query_state_set(self.h, self.qs, *ptrs, self._stream()))

    def capture(self, env_ids=None):
        """Row i becomes the live state of env env_ids[i] -- root, joints, ball -- with its parameter rows; `env_ids` (M,) int32 on the
        sim's device, or None for row i <- env i (needs M == N).  A row whose id is outside 0 .. N-1 is left as it was.  One launch on
        the current stream."""
        if env_ids is None and self.rows != self.sim.num_envs:
            raise BezSimError("query state capture: env_ids is None (row i <- env i), which needs rows == num_envs (%d != %d)"
                              % (self.rows, self.sim.num_envs))
        self._check(self.lib.bez_query_state_capture(self.h, self.qs, self._env_ids(env_ids), self._stream()))

    # ---- the tensors of its own: RIGID_BODY_STATE rows, Jacobian, mass matrix; each allocated by its first acquisition
    def _tensor(self, which):
        return self._wrap(("query", which), lambda h, w, *out: self.lib.bez_query_state_tensor(h, self.qs, w, *out), which)

    def dynamics_tensor(self, which):
        """BezSim.dynamics_tensor of this state: the Jacobian (M*NB, 6, 24) or the mass matrix (M, 24, 24); refresh_dynamics_tensors() fills it."""
        return self._tensor((abi.QUERY_JACOBIAN, abi.QUERY_MASS_MATRIX)[abi.dynamics_tensor_id(which)])

    def refresh_dynamics_tensors(self, which=None):
        """BezSim.refresh_dynamics_tensors of this state: one tensor, a sequence of them, or None for every one acquired so far."""
        if which is None:
            ids = [k[1] for k in self._views if k[1] != abi.QUERY_RIGID_BODY_STATE]
        else:
            ids = [(abi.QUERY_JACOBIAN, abi.QUERY_MASS_MATRIX)[abi.dynamics_tensor_id(w)] for w in ([which] if isinstance(which, (str, int)) else which)]
        mask = 0
        for k in ids:
            mask |= 1 << k
        self._check(self.lib.bez_query_state_refresh(self.h, self.qs, mask, self._stream()))

    def refresh(self, which):
        """BezSim.refresh(abi.TENSOR_RIGID_BODY_STATE) of this state: its (M*NBE, 13) rigid-body rows, refreshed.  A query state has no
        other Isaac-layout tensor: its root, DOF and ball rows are what set() or capture() were given."""
        if which != abi.TENSOR_RIGID_BODY_STATE:
            raise BezSimError("a query state refreshes abi.TENSOR_RIGID_BODY_STATE only, got tensor id %r" % (which,))
        view = self._tensor(abi.QUERY_RIGID_BODY_STATE)
        self._check(self.lib.bez_query_state_refresh(self.h, self.qs, 1 << abi.QUERY_RIGID_BODY_STATE, self._stream()))
        return view


class Snapshot:
    """`rows` whole envs of a BezSim, saved and put back (BezSim.snapshot; include/bez_sim.h "Env snapshots"): everything that decides how
    an env continues -- the state with targets, contact rows and goal, obs / rew / reset / progress / timeout, the episode counter that
    keys the reset noise, randomize, the statistics, the parameter rows the sim has, the actuator record -- and, per save, the sim-global
    counters and randomisation clock.  A restored env keeps the destination's random identity (seed, global env id)."""

    def __init__(self, sim, rows):
        self.sim, self.rows, self.device, self.lib, self.h = sim, rows, sim.device, sim.lib, sim.h
        self._stream = sim._stream
        snap = C.c_void_p()
        sim._check(sim.lib.bez_snapshot_create(sim.h, rows, C.byref(snap)))
        self.snap = snap

    for _name in ("_check", "_ptr", "_checked"):
        locals()[_name] = getattr(BezSim, _name)
    del _name

    def _forget(self):
        self.snap = None

    def close(self):
        if getattr(self, "snap", None) is not None:
            self._check(self.lib.bez_snapshot_destroy(self.h, self.snap))
            self._forget()
            snaps = self.sim.__dict__.get("_snapshots", [])
            if self in snaps:
                snaps.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _open(self, what):
        if getattr(self, "snap", None) is None:
            raise BezSimError("snapshot %s: the snapshot is closed" % what)

    def _ids(self, name, ids, count):
        """the pointer of (count,) int32 ids on the device, NULL for None"""
        return None if ids is None else self._ptr(self._checked(name, ids, ((count,),)), torch.int32)

    def save(self, env_ids=None):
        """Row i becomes env env_ids[i] as it is now; `env_ids` (rows,) int32 on the sim's device, contiguous, or None for row i <- env i.
        Ids may repeat; a row whose id is outside 0 .. N-1 keeps what it held.  Also records the sim-global counters and randomisation
        clock.  One launch on the current stream."""
        self._open("save")
        self._check(self.lib.bez_snapshot_save(self.h, self.snap, self._ids("env_ids", env_ids, self.rows), self._stream()))

    def restore(self, sim=None, env_ids=None, row_ids=None, count=None, globals_=False):
        """Env env_ids[i] of `sim` (None: the owning sim) becomes row row_ids[i], i < count.  `env_ids`, `row_ids`: (count,) int32 on the
        sim's device, contiguous, or None for env i / row i; `count` None: the length of the ids given, else the snapshot's rows.  Valid
        env ids must be distinct; an entry with either id out of range is skipped.  `globals_`: also give the sim the snapshot's global
        block (a rewind of the whole sim); False leaves the sim's own alone.  The Isaac-layout tensors are stale afterwards as after a
        set_*_indexed call: refresh them.  Everything is checked before the library is called."""
        self._open("restore")
        dst = self.sim if sim is None else sim
        if not isinstance(dst, BezSim):
            raise BezSimError("snapshot restore: sim must be a BezSim, got %s" % type(dst).__name__)
        if dst.device != self.device:
            raise BezSimError("snapshot restore: the destination sim is on %s, the snapshot on %s" % (dst.device, self.device))
        given = [t for t in (env_ids, row_ids) if isinstance(t, torch.Tensor)]
        if count is None:
            count = given[0].numel() if given else self.rows
        if isinstance(count, bool) or not isinstance(count, int) or count < 0:
            raise BezSimError("snapshot restore: count must be an int >= 0, got %r" % (count,))
        if row_ids is None and count > self.rows:
            raise BezSimError("snapshot restore: count %d exceeds the snapshot's %d rows (row_ids is None: row i)" % (count, self.rows))
        ptrs = [self._ids("env_ids", env_ids, count), self._ids("row_ids", row_ids, count)]
        what = abi.SNAPSHOT_ENVS | (abi.SNAPSHOT_GLOBALS if globals_ else 0)
        dst._check(self.lib.bez_snapshot_restore(dst.h, self.snap, *ptrs, count, what, self._stream()))

    # ---- the snapshot as host data: one self-describing blob (include/bez_sim.h), here cut into its sections
    def _blob_words(self):
        size = C.c_int64(0)
        self._check(self.lib.bez_snapshot_export(self.h, self.snap, None, C.byref(size), self._stream()))
        return size.value // 4

    def state_dict(self):
        """{"header": (SNAPSHOT_HEADER_WORDS,), <section>: (width, rows) for every name of abi.SNAPSHOT_SECTIONS, "globals":
        (SNAPSHOT_GLOBAL_WORDS,)}: int32 CPU tensors holding the 32-bit words of the snapshot (a 64-bit item is two rows of its section,
        low then high), copies that stay valid.  Waits for the current stream."""
        self._open("state_dict")
        words = self._blob_words()
        blob = torch.empty(words, dtype=torch.int32)
        size = C.c_int64(words * 4)
        self._check(self.lib.bez_snapshot_export(self.h, self.snap, C.c_void_p(blob.data_ptr()), C.byref(size), self._stream()))
        hw = abi.SNAPSHOT_HEADER_WORDS
        out, at = {"header": blob[:hw].clone()}, hw
        for k, name in enumerate(abi.SNAPSHOT_SECTIONS):
            width = int(blob[8 + k])
            out[name] = blob[at:at + width * self.rows].view(width, self.rows).clone()
            at += width * self.rows
        out["globals"] = blob[at:at + abi.SNAPSHOT_GLOBAL_WORDS].clone()
        return out

    def load_state_dict(self, d):
        """Fills the snapshot from a state_dict() of a snapshot with the same rows and widths (of this sim or another one of the same
        task and asset); the library refuses what does not fit and leaves the snapshot as it was."""
        self._open("load_state_dict")
        names = ("header",) + abi.SNAPSHOT_SECTIONS + ("globals",)
        for name in names:
            if name not in d or not isinstance(d[name], torch.Tensor) or d[name].dtype != torch.int32 or d[name].device.type != "cpu":
                raise BezSimError("snapshot load_state_dict: %r must be an int32 CPU tensor" % name)
        blob = torch.cat([d[name].reshape(-1) for name in names]).contiguous()
        self._check(self.lib.bez_snapshot_import(self.h, self.snap, C.c_void_p(blob.data_ptr()), blob.numel() * 4, self._stream()))
