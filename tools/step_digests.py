#!/usr/bin/env python3
"""SHA-256 digests of what the step kernels write: one line per configuration, after 3 control steps from the seeded states of the GPU tests
(tests/state_sets.generate_states) with actions from a seeded generator.  Two builds that print the same lines compute the same bits:

  BEZ_SIM_LIB=build_ab/parent.so python tools/step_digests.py        (one process per library; profiles/step_df_template_digests.txt)

Hashed: ROOT_STATE, DOF_STATE, RIGID_BODY_STATE, NET_CONTACT_FORCE, obs, reward and reset; with abi.FLAG_DOF_FORCE also the three actuator
tensors after refresh_actuator_tensors.  Configurations, each crossed with the others: BEZ_SIM_KERNEL in ws8q / ws8 / lane, the flag off and
on, the assets of tests.gpu_util.ASSETS, bez_kick and bez_walk, per-env parameters off and on (one set_env_params row of mass scales),
external wrenches off and on (one apply_body_forces before each step), num_envs 17 and 65 (one ragged 16-env workgroup of the lane-group
form, one ragged 64-env workgroup of the other two); for the lane kernel without the flag also the split path pre_physics, simulate,
post_physics and a closing observe_reward."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bez_isaacgym_amd   # noqa: E402,F401  (before anything initialises HIP: DESIGN.md 6.2)
import numpy as np   # noqa: E402
import torch   # noqa: E402

from bez_isaacgym_amd import abi   # noqa: E402
from tests.gpu_util import ASSETS, _dev, _sim, _write_states   # noqa: E402
from tests.sim_cfg import make_cfg   # noqa: E402
from tests.state_sets import ball_states, generate_states   # noqa: E402

SIZES = (17, 65)
STEPS = 3
STATE = (abi.TENSOR_ROOT_STATE, abi.TENSOR_DOF_STATE, abi.TENSOR_RIGID_BODY_STATE, abi.TENSOR_NET_CONTACT_FORCE)
OUT = (abi.TENSOR_OBS, abi.TENSOR_REW, abi.TENSOR_RESET)


def digest(tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def run(kernel, df, asset, task, params, ext, n, split):
    os.environ["BEZ_SIM_KERNEL"] = kernel   # read per sim, at its creation
    cfg = make_cfg(n, task=task, seed=5, **ASSETS[asset])
    if df:
        cfg.flags |= abi.FLAG_DOF_FORCE
    sim = _sim(cfg)
    root, dof, _ = generate_states(n)
    _write_states(sim, root, dof, ball_states(n))
    rng = np.random.default_rng(31)
    if params:
        sim.set_env_params(abi.PARAM_MASS_SCALE, _dev(rng.uniform(0.5, 1.5, (n, abi.PARAM_WIDTH[abi.PARAM_MASS_SCALE]))))
    actions = _dev(rng.uniform(-1.0, 1.0, (STEPS, n, abi.NUM_DOFS))).view(STEPS, n * abi.NUM_DOFS)
    forces = _dev(rng.uniform(-5.0, 5.0, (STEPS, n, sim.num_bodies, 3))).view(STEPS, n, sim.num_bodies, 3)
    torques = _dev(rng.uniform(-0.5, 0.5, (STEPS, n, sim.num_bodies, 3))).view(STEPS, n, sim.num_bodies, 3)
    for k in range(STEPS):
        if ext:
            sim.apply_body_forces(forces[k].contiguous(), torques[k].contiguous())
        if split:
            sim.pre_physics(actions[k])
            sim.simulate()
            sim.post_physics()
        else:
            sim.step(actions[k])
    if split:
        sim.observe_reward()
    out = [sim.refresh(w).clone() for w in STATE] + [sim.tensor(w).clone() for w in OUT]
    if df:
        sim.refresh_actuator_tensors()
        out += [sim.actuator_tensor(w).clone() for w in (abi.ACTUATOR_DOF_FORCE, abi.ACTUATOR_DRIVE_TORQUE, abi.ACTUATOR_STATUS)]
    d = digest(out)
    sim.close()
    return d


def main():
    for kernel in ("ws8q", "ws8", "lane"):
        for df in (False, True):
            for split in ((False, True) if kernel == "lane" and not df else (False,)):
                for asset in ASSETS:
                    for task in ("bez_kick", "bez_walk"):
                        for params in (False, True):
                            for ext in (False, True):
                                ds = " ".join("n=%d:%s" % (n, run(kernel, df, asset, task, params, ext, n, split)) for n in SIZES)
                                print("%-4s %-5s df=%d %-7s %-8s params=%d ext=%d %s"
                                      % (kernel, "split" if split else "fused", df, asset, task, params, ext, ds), flush=True)


if __name__ == "__main__":
    main()
