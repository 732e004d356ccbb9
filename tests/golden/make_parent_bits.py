"""Record the step kernels' raw output bits for tests/test_gpu_parent_bits.py.

parent_bits.npz was made by this script on an MI355X with the library built from commit
42f1e2a ("Add a device-resident RolloutBuffer: add, GAE, shuffled minibatches"), the parent of the
change that moved the 7x7 Cholesky of the dynamics and of the IK to one row per lane.  That change
has no switch inside one library, so the parent's bits are kept here: the claim is that every
product and every accumulation order stayed what chol7 / chol7_solve did.

    python tests/golden/make_parent_bits.py [OUT.npz]      (on the GPU box; PGX_LIB picks the library)

For PandaReach-v3 and PandaReachJoints-v3 (the two control modes' kernels): 64 envs, seed 9, the
pressing-down policy (press() below), 16 lanes per env, launch order = env order; after steps 5,
10, 20 and 30 the bits of the observation, q and qd as uint32.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ENV_IDS = ("PandaReach-v3", "PandaReachJoints-v3")
N_ENVS, SEED, RECORD = 64, 9, (5, 10, 20, 30)
GOLDEN = os.path.join(HERE, "parent_bits.npz")


def key(env_id, step, name):
    return f"{env_id}/{step}/{name}"


def press(v, t):
    """The pressing-down policy.  End-effector control: z = -1, x / y random (as
    tests/test_gpu_merged_rows.py).  Joint control has no z: the shoulder joint (dof 1) turns
    towards the table at full rate and the base joint (dof 0) is random -- on the fp64 oracle the
    tool reaches the table at step 18, two points per env with idle second points among them."""
    import torch

    a = torch.zeros((v.num_envs, v.action_dim), device="cuda:0")
    r = v.sample_actions(t)
    if v.action_dim >= 7:
        a[:, 1] = 1.0
        a[:, 0] = r[:, 0]
    else:
        a[:, 2] = -1.0
        a[:, :2] = r[:, :2]
    return a


def run(pg, env_id):
    """{key: uint32 bits} of obs, q and qd after each step of RECORD."""
    old = os.environ.get("PGX_SORT_ENVS")
    os.environ["PGX_SORT_ENVS"] = "0"   # read when the handle is created
    try:
        v = pg.PandaVecEnv(env_id, num_envs=N_ENVS, device="cuda:0", seed=SEED, lanes_per_env=16)
    finally:
        if old is None:
            del os.environ["PGX_SORT_ENVS"]
        else:
            os.environ["PGX_SORT_ENVS"] = old
    v.reset_tensors(seed=SEED)
    out = {}
    for t in range(max(RECORD)):
        v.step_tensors(press(v, t))
        if t + 1 in RECORD:
            st = v.state()
            for name, x in (("obs", v.obs), ("q", st["q"]), ("qd", st["qd"])):
                out[key(env_id, t + 1, name)] = x.contiguous().cpu().numpy().view(np.uint32).copy()
    v.close()
    return out


def main():
    import panda_gym_amd as pg

    pg.load_native()
    out = {}
    for env_id in ENV_IDS:
        out.update(run(pg, env_id))
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
