"""Record the arm step kernels' raw output bits for tests/test_gpu_table_normal_bits.py.

table_normal_bits.npz was made by this script on an MI355X with the library built from commit
ccace18 ("Fold the batch-row launches' repeats into the shared policy layer"), the parent of the
change that made the table's normal a compile-time constant in the arm kernels' contact rows: there
a robot point's normal (0, 0, 1), its g1rb and its g1w are no longer stored by the candidate lane
nor read back, plane_space is not evaluated, and the three Jacobian entries dot(u, Jv) are Jv.z,
-Jv.y and Jv.x with the signed zeros the three-term sums gave.  That change has no switch inside
the shipped library, so the parent's words are kept here.

    python tests/golden/make_table_normal_bits.py [OUT.npz]   (on the GPU box; PGX_LIB picks the library)

Four cases, 16 lanes per env (one wave is 4 envs), launch order = env order (PGX_SORT_ENVS=0):

    fingers_table   PandaReach-v3, 8 envs from start poses that differ per env (start_q), the end
                    effector driven down onto the table (the drive of test_gpu_contacts'
                    table test, a per-env offset): the hand capsules' end spheres press on the
                    table top, 30 steps
    limit_touch     PandaReachJoints-v3, 8 envs started with the elbow (dof 3) 0.03 to 0.10 rad
                    below its upper limit (0) and the arm stretched forward over the table, the
                    shoulder (dof 1) driven down and the elbow into its limit: the hand comes down
                    on the table while dof 3 sits at the limit, so the motor bound cannot clear
                    that pair (the partial solve) and contact impulses stand beside it, 25 steps.
                    Chosen on the fp64 oracle: start poses swept until every env touched with
                    upper[3] - q[3] < 0.02 at a recorded step.
    off_table       PandaReachJoints-v3, 8 envs started with the arm turned sideways (dof 0 at
                    +-pi/2, alternating), the wrist straight and the elbow at -1.0 to -1.55 rad, the
                    shoulder driven down: the hand passes the table's edge (|y| > 0.35) and comes
                    down on the plane beside the table (z = -0.4), robot points with on_table
                    false, 15 steps.  Chosen on the fp64 oracle: elbow angles swept, those kept
                    whose hand reaches the plane (a flatter elbow stays above it, a sharper one
                    puts an end sphere deep under the table top).
    reach_random    PandaReach-v3, 64 envs, seeded random actions with staggered episode phases,
                    60 steps, every 10th recorded: contact-free waves (the far mode), early exits
                    and the iteration cap

After the steps of RECORD[case]: the bits of the observation, q, qd, and of the robot slots' cached
feature ids (2 * capsule + end; -1 = empty) and normal impulses, as uint32.  main() refuses to
write a file that does not meet coverage() -- what the test asserts again from the file.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 23
CASES = ("fingers_table", "limit_touch", "off_table", "reach_random")
ENV_OF = {"fingers_table": "PandaReach-v3", "limit_touch": "PandaReachJoints-v3", "off_table": "PandaReachJoints-v3",
          "reach_random": "PandaReach-v3"}
N_ENVS = {"fingers_table": 8, "limit_touch": 8, "off_table": 8, "reach_random": 64}
RECORD = {"fingers_table": (10, 20, 30), "limit_touch": (16, 19, 22, 25), "off_table": (6, 9, 12, 15),
          "reach_random": (10, 20, 30, 40, 50, 60)}
NAMES = ("obs", "q", "qd", "ids", "imp")
GOLDEN = os.path.join(HERE, "table_normal_bits.npz")
NEUTRAL_Q = (0.0, 0.41, 0.0, -1.85, 0.0, 2.26, 0.79)   # abi.NEUTRAL_Q's arm
ELBOW_UPPER = 0.0       # dof 3's upper limit (the model's)
PLANE_EE_Z = -0.25      # an end effector below this is beside the table: the table top is z = 0, the plane z = -0.4


def key(case, step, name):
    return f"{case}/{step}/{name}"


def start_q(case, n):
    """Per-env start pose [n, 7] (None: the reset's)."""
    rng = np.random.default_rng(SEED)
    if case == "fingers_table":
        return (np.array(NEUTRAL_Q) + rng.uniform(-0.15, 0.15, (n, 7))).astype(np.float32)
    if case == "limit_touch":
        q = np.tile(np.array([0.0, 0.55, 0.0, 0.0, 0.0, 1.2, 0.79]), (n, 1))
        q[:, 0] = rng.uniform(-0.25, 0.25, n)
        q[:, 1] += rng.uniform(-0.05, 0.05, n)
        q[:, 3] = ELBOW_UPPER - np.linspace(0.03, 0.10, n)
        q[:, 5] += rng.uniform(-0.3, 0.3, n)
        return q.astype(np.float32)
    if case == "off_table":
        q = np.tile(np.array([np.pi / 2, 1.2, 0.0, 0.0, 0.0, np.pi, 0.79]), (n, 1))
        q[1::2, 0] *= -1.0
        q[:, 3] = -np.linspace(1.0, 1.55, n)
        q[:, 6] += rng.uniform(-0.3, 0.3, n)
        return q.astype(np.float32)
    return None


def actions(case, n, ad, t):
    """The drive's actions at step t, [n, ad] float32 (None: the handle's seeded random policy)."""
    rng = np.random.default_rng(SEED + 1)
    i = np.arange(n)
    if case == "fingers_table":
        off = rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32)
        off[:, 2] = 0.0
        return np.clip(np.array([0.3, -0.2, -1.0], np.float32) + off, -1, 1).astype(np.float32)
    if case == "limit_touch":
        a = np.zeros((n, ad), np.float32)
        a[:, 1] = 1.0                                  # the shoulder down
        a[:, 3] = 1.0                                  # the elbow into its upper limit
        a[:, 5] = np.where(i % 2 == 0, 0.3, -0.3)
        return a
    if case == "off_table":
        a = np.zeros((n, ad), np.float32)
        a[:, 1] = 1.0                                  # the shoulder down
        a[:, 4] = np.where(i % 2 == 0, 0.2, -0.2)
        return a
    return None


def coverage(out):
    """What the recorded cache words show, as a dict of flags: in one wave (4 consecutive envs) an
    env with exactly 2 robot points, one with exactly 1 and one with 0; both end spheres of a
    two-sphere capsule in one env; a point recorded at the plane's height (an end-effector
    capsule's, 9-13, with the end effector below PLANE_EE_Z); the elbow within 0.02 rad of its limit
    in an env that holds a point (limit_touch)."""
    f = {"wave_2_1_0": False, "both_ends": False, "plane_point": False, "limit_and_point": False}
    for case in CASES:
        for step in RECORD[case]:
            if key(case, step, "ids") not in out:
                continue
            ids = out[key(case, step, "ids")].view(np.float32)        # [slots, n]
            obs = out[key(case, step, "obs")].view(np.float32)        # [n, od]
            q = out[key(case, step, "q")].view(np.float32)            # [7, n]
            cnt = (ids >= 0).sum(axis=0)
            for w in range(0, ids.shape[1], 4):
                c4 = set(cnt[w:w + 4].tolist())
                f["wave_2_1_0"] |= {0, 1, 2} <= c4
            for e in range(ids.shape[1]):
                have = {int(x) for x in ids[:, e] if x >= 0}
                f["both_ends"] |= any(x % 2 == 0 and x + 1 in have for x in have)
                hand = any(9 <= x // 2 <= 13 for x in have)
                f["plane_point"] |= hand and obs[e, 2] < PLANE_EE_Z
                if case == "limit_touch":
                    f["limit_and_point"] |= bool(have) and ELBOW_UPPER - q[3, e] < 0.02
    return f


def run(pg, case):
    """{key: uint32 bits} of obs, q, qd and the robot slots' feature ids and impulses after each step
    of RECORD[case]."""
    import torch

    from panda_gym_amd import abi

    n = N_ENVS[case]
    old = os.environ.get("PGX_SORT_ENVS")
    os.environ["PGX_SORT_ENVS"] = "0"   # read when the handle is created
    try:
        v = pg.PandaVecEnv(ENV_OF[case], num_envs=n, device="cuda:0", seed=SEED, lanes_per_env=16)
    finally:
        if old is None:
            del os.environ["PGX_SORT_ENVS"]
        else:
            os.environ["PGX_SORT_ENVS"] = old
    v.reset_tensors(seed=SEED, episode_phase="staggered" if case == "reach_random" else None)
    q0 = start_q(case, n)
    if q0 is not None:
        st = v.state()
        qt = torch.as_tensor(q0.T.copy(), dtype=torch.float32, device="cuda:0")
        st["q"].copy_(qt)
        st["qc"].copy_(qt)
        st["qd"].zero_()
    budget = v.robot_contact_budget()
    out = {}
    for t in range(max(RECORD[case])):
        a = actions(case, n, v.action_dim, t)
        v.step_tensors(v.sample_actions(t).clone() if a is None else torch.as_tensor(a, device="cuda:0"))
        if t + 1 in RECORD[case]:
            st = v.state()
            rows = st["contacts"][2 * abi.OBJECT_POINTS:2 * (abi.OBJECT_POINTS + budget)]
            for name, x in (("obs", v.obs), ("q", st["q"]), ("qd", st["qd"]), ("ids", rows[0::2]), ("imp", rows[1::2])):
                out[key(case, t + 1, name)] = x.contiguous().cpu().numpy().view(np.uint32).copy()
    v.close()
    return out


def main():
    import panda_gym_amd as pg

    pg.load_native()
    out = {}
    for case in CASES:
        r = run(pg, case)
        for step in RECORD[case]:
            ids = r[key(case, step, "ids")].view(np.float32)
            print(case, step, "points per env", (ids >= 0).sum(axis=0).tolist(),
                  "features", sorted({int(x) for x in ids.ravel() if x >= 0}),
                  "ee z min", float(r[key(case, step, "obs")].view(np.float32)[:, 2].min()), flush=True)
        out.update(r)
    cov = coverage(out)
    print("coverage", cov)
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    if not all(cov.values()):
        path += ".rejected.npz"
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert all(cov.values()), "the drives do not reach the coverage the test asserts"


if __name__ == "__main__":
    main()
