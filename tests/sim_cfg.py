"""The BezConfig every test and tool builds its simulations from: task, asset flags and seed by name."""
from bez_isaacgym_amd import abi


def make_cfg(n, task="bez_kick", cleats=False, seed=42, box=False, **kw):
    c = abi.default_config(n, seed=seed, **kw)
    c.task = abi.TASK_IDS[task]
    if task != "bez_kick":
        c.max_episode_length = 600      # bez_walk.yaml / bez_orient.yaml: episodeLength_s 10
        c.goal[:] = [2.0, 0.0]
        c.goal_angle = 1.5708
    if cleats:
        c.flags |= abi.FLAG_CLEATS
    if box:
        c.flags |= abi.FLAG_BOX_ASSET
    return c


def oracle(n, **kw):
    from oracle.bez_oracle import Oracle
    return Oracle(make_cfg(n, **kw))
