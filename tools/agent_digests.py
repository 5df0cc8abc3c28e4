#!/usr/bin/env python3
"""SHA-256 digests of what five PPO epochs leave behind (2 eager epochs, the capturing one, 2 replays): the model parameters, both running
normalisers and Adam's moments.  Two builds that print the same line for a configuration train bit-identically in it:

  python tools/agent_digests.py [--randomize] [--train] [--dist] [switch=value ...]      e.g.  fused_ops=False hip_graphs=False

The agent is tests.gpu_util._agent(512, 4096, **switches).  --train: the epochs run through train(max_epochs=5) (pipelined epochs)
instead of train_epoch(); --dist: a 1-rank RCCL process group with BEZ_PPO_FORCE_DIST=1 (the data-parallel path on one GPU).  One
configuration per process (profiles/agent_refactor_digests.txt)."""
import ast
import hashlib
import os
import socket
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bez_isaacgym_amd   # noqa: E402,F401  (before anything initialises HIP: DESIGN.md 6.2)
import torch   # noqa: E402


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:32]


def main(argv):
    flags = [a for a in argv if a.startswith("--")]
    over = {}
    for a in argv:
        if not a.startswith("--"):
            k, v = a.split("=", 1)
            over[k] = ast.literal_eval(v)
    if "--dist" in flags:
        import torch.distributed as dist
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", BEZ_PPO_FORCE_DIST="1")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from tests.gpu_util import _agent
    a = _agent(512, 4096, randomize="--randomize" in flags, **over)
    if "--train" in flags:
        a.train(max_epochs=5, log=lambda line: None)
    else:
        a.obs = a.env_reset()
        for _ in range(5):
            a.train_epoch()
    torch.cuda.synchronize()
    params = list(a.model.parameters())
    rms = [t for m in (a.running_mean_std, a.value_mean_std) if m is not None for t in (m.running_mean, m.running_var, m.count)]
    adam = [a.optimizer.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq")]
    print("%-52s graphs=%d params=%s normalisers=%s adam=%s" % (" ".join(argv) or "defaults", int(a._g_update is not None or a._seg is not None),
                                                                 digest(params), digest(rms), digest(adam)), flush=True)
    if "--dist" in flags:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
