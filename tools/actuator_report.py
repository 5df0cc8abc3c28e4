#!/usr/bin/env python3
"""What the actuators do (GPU; BEZ_FLAG_DOF_FORCE): uniform random actions and the shipped reference policy
(tests/golden/bez_kick_33_policy.npz) in 4096 envs -- per joint the RMS and maximum of the drive torque, the share of control steps in
which a substep saturated the drive / locked the joint on its speed limit, and the mean positive mechanical power; the same over the 16
driven joints; and the device time of one bez_sim_refresh_actuator_tensors launch.  Samples of envs that the step reset are left out
(their row describes the discarded step).  The lock share stands beside profiles/r06_vlimit_probe.txt (tools/vlimit_probe.py, CPU
oracle): that probe counts joint samples whose |qd| ENDS a control step within 2 % of the limit, this one control steps in which ANY
substep locked the joint.

    python tools/actuator_report.py > profiles/actuator_report.txt
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bez_isaacgym_amd import abi  # noqa: E402
from bez_isaacgym_amd.sim import BezSim  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "bez_kick_33_policy.npz")


def run(policy, n, steps, seed=1):
    cfg = abi.default_config(n, seed=seed)
    cfg.flags |= abi.FLAG_DOF_FORCE
    sim = BezSim(cfg, 0)
    dev = sim.device
    obs, prog = sim.tensor(abi.TENSOR_OBS), sim.tensor(abi.TENSOR_PROGRESS)
    player = None
    if policy == "reference":
        from bez_isaacgym_amd.utils.player import PpoPlayerContinuous
        player = PpoPlayerContinuous(FIXTURE, "cuda:0")
    gen = torch.Generator(device=dev).manual_seed(seed)
    sim.step(torch.zeros(n * 18, device=dev))
    f64 = dict(device=dev, dtype=torch.float64)
    sq, mx, sat, lock, power, end_on = (torch.zeros(18, **f64) for _ in range(6))
    count = torch.zeros((), **f64)
    vl = float(cfg.vel_limit)
    for _ in range(steps):
        a = player.get_action(obs) if player is not None else torch.rand(n, 18, device=dev, generator=gen) * 2 - 1
        sim.step(a.reshape(-1).contiguous())
        sim.refresh_actuator_tensors()
        drive = sim.actuator_tensor(abi.ACTUATOR_DRIVE_TORQUE).view(n, 18).double()
        status = sim.actuator_tensor(abi.ACTUATOR_STATUS).view(n, 18)
        qd = sim.refresh(abi.TENSOR_DOF_STATE).view(n, 18, 2)[:, :, 1].double()
        live = (prog > 0).double()[:, None]   # an env with progress 0 was reset behind the step
        sq += (drive * drive * live).sum(0); mx = torch.maximum(mx, (drive.abs() * live).max(0).values)
        sat += (((status & abi.ACTUATOR_SATURATED) != 0).double() * live).sum(0)
        lock += (((status & abi.ACTUATOR_LOCKED) != 0).double() * live).sum(0)
        power += ((drive * qd).clamp_min(0) * live).sum(0)
        r = qd.abs() / vl
        end_on += (((r > 0.98) & (r <= 1.02)).double() * live).sum(0)   # tools/vlimit_probe.py's "on_limit", on the same samples
        count += live.sum()
    # one refresh launch, timed with events over 200 launches
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        sim.refresh_actuator_tensors()
    e0.record()
    for _ in range(200):
        sim.refresh_actuator_tensors()
    e1.record(); torch.cuda.synchronize()
    c = float(count.item())
    per = dict(rms=(sq / c).sqrt().tolist(), max=mx.tolist(), saturated=(sat / c).tolist(), locked=(lock / c).tolist(),
               power=(power / c).tolist())
    d = slice(2, 18)
    summary = dict(policy=policy, envs=n, steps=steps, env_step_samples=int(c), driven_joint_samples=int(c) * 16,
                   rms_drive=float((sq[d].sum() / (16 * c)).sqrt()), max_drive=float(mx[d].max()),
                   saturated_share=float(sat[d].sum() / (16 * c)), locked_share=float(lock[d].sum() / (16 * c)),
                   ends_on_limit_share=float(end_on[d].sum() / (16 * c)), mean_positive_power_w=float(power[d].sum() / (16 * c)),
                   refresh_us=e0.elapsed_time(e1) * 1e3 / 200)
    return summary, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    names = json.load(open(os.path.join(ROOT, "bez_isaacgym_amd", "model", "bez_model.json")))["dof_names"]
    for policy in ("random", "reference"):
        summary, per = run(policy, a.envs, a.steps)
        print("== policy %s" % policy)
        print(json.dumps(summary))
        print("%-28s %9s %9s %10s %8s %9s" % ("joint", "rms N m", "max N m", "saturated", "locked", "power W"))
        for j, name in enumerate(names):
            print("%-28s %9.3f %9.2f %10.4f %8.4f %9.4f" % (name, per["rms"][j], per["max"][j], per["saturated"][j], per["locked"][j], per["power"][j]))


if __name__ == "__main__":
    main()
