"""Shared pieces of the whole-range and tumbling-cube tests (test_gpu_whole_range.py and
test_gpu_tumbling_cube.py on the device, test_whole_range_oracle.py on the CPU): the start states,
the actions, the row classes, the restated mat_to_quat branch test and the Euler / quaternion
rotations the cube tests compare.

Arm start state: every arm dof uniform in [lower + EDGE, upper - EDGE], joint velocities U(-1, 1)
rad/s, rounded to float32 (what the device state holds), qc = q.  One env step from there runs the
IK from a pose whose EE rotation is anywhere (all four branches of mat_to_quat, the angle > pi wrap,
the step clamp and all 20 iterations), and FK, the mass matrix and the bias forces over the whole
joint range.

Cube start state: 1 m above the table, a uniformly random orientation, linear velocity U(-1, 1) m/s
and an angular velocity of random direction in four bands of |w| (the exponential map's small-angle
branch, its plain branch twice, and its clamp at |w| dt > pi / 8)."""
import numpy as np

import limp_arm as L

N, SEED, ACTION_SEED = 512, 11, 5
EDGE = 0.05
# (env id, contacts) under EE control; joint control: PandaReachJoints-v3
EE_CASES = [("PandaReach-v3", True), ("PandaReach-v3", False), ("PandaPush-v3", True), ("PandaPickAndPlace-v3", True)]
JOINTS_ENV = "PandaReachJoints-v3"
BRANCHES = ("x", "y", "z", "trace>0")

CUBE_N, CUBE_SEED, CUBE_BAND = 256, 9, 64
CUBE_ENVS = ("PandaPush-v3", "PandaPickAndPlace-v3")
W_BANDS = ((0.0, 9e-4), (0.5, 20.0), (20.0, 190.0), (200.0, 400.0))
BAND_NAMES = ("small angle", "0.5-20", "20-190", "clamp")
GIMBAL_N, GIMBAL_SIN = 16, 0.99
VEL_TOL = 1e-4          # x max(1, |value64|): linear and angular velocity of the cube


def start_state(cfg, n=N, seed=SEED):
    """(q, qd) [n, n_dofs] of the whole-range start state, float32 values held in doubles."""
    lo, hi = L.limits(cfg)
    rng = np.random.default_rng(seed)
    q = rng.uniform(lo + EDGE, hi - EDGE, (n, len(lo)))
    qd = rng.uniform(-1.0, 1.0, (n, len(lo)))
    return q.astype(np.float32).astype(np.float64), qd.astype(np.float32).astype(np.float64)


def actions(n, action_dim, zero=False, seed=ACTION_SEED):
    if zero:
        return np.zeros((n, action_dim), np.float32)
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, action_dim)).astype(np.float32)


def quat_branch(R):
    """The branch btMatrix3x3::getRotation (mat_to_quat in pgx_kernels.hip and pgx_oracle.c) takes for
    the rotations R [n, 3, 3]: 3 where the trace is positive, else the index of the largest diagonal
    entry by the kernels' comparisons (0 = x: m0 >= m4 and m0 >= m8; 1 = y: m0 < m4 and m4 >= m8;
    2 = z otherwise)."""
    m0, m4, m8 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    i = np.where(~(m0 < m4) & ~(m0 < m8), 0, np.where((m0 < m4) & ~(m4 < m8), 1, 2))
    return np.where(m0 + m4 + m8 > 0.0, 3, i)


def ee_branches(O, cfg, q):
    """quat_branch of the EE link's rotation at every row of q (the IK's first iteration)."""
    m = cfg.model.contents
    R = np.stack([O.fk(m, qi, tuple(cfg.base_pos))[1][m.ee_link] for qi in q])
    return quat_branch(R)


def classes(O, cfg, r64, o64, also_done=None):
    """(free, limit, points) row masks by the fp64 oracle after the step: free = no robot contact
    point, no dof within LIMIT_TOL of a limit, not ended; limit = a dof at a limit, no robot point,
    not ended; points = rows with a robot point (left out of every comparison)."""
    pts = L.robot_points(O, r64) > 0
    lim = L.at_limit(cfg, r64.q).any(axis=1)
    done = (o64["truncated"] | o64["terminated"]) != 0
    if also_done is not None:
        done = done | (also_done != 0)
    return ~pts & ~lim & ~done, lim & ~pts & ~done, pts


def slack_rule(ratio, start):
    """The slack of a measured device / fp32-oracle ratio (limp_arm.py's rule): the starting value
    where it holds, else 1.5 x the largest measured ratio, capped at 8."""
    return start if ratio <= start else min(1.5 * ratio, 8.0)


# ------------------------------------------------------------------ cube
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def cube_state(n=CUBE_N, seed=CUBE_SEED):
    """obj [n, 13] (pos, quat (x, y, z, w), linvel, angvel) of the tumbling cubes, float32 values held
    in doubles: z = 1, x spread over [-0.2, 0.1], band k of |w| in rows [k * CUBE_BAND, (k + 1) * CUBE_BAND)."""
    assert n == CUBE_BAND * len(W_BANDS)
    rng = np.random.default_rng(seed)
    obj = np.zeros((n, 13))
    obj[:, 0] = np.linspace(-0.2, 0.1, n)
    obj[:, 2] = 1.0
    obj[:, 3:7] = _unit(rng.standard_normal((n, 4)))
    obj[:, 7:10] = rng.uniform(-1.0, 1.0, (n, 3))
    mag = np.concatenate([rng.uniform(lo, hi, CUBE_BAND) for lo, hi in W_BANDS])
    obj[:, 10:13] = _unit(rng.standard_normal((n, 3))) * mag[:, None]
    return obj.astype(np.float32).astype(np.float64)


def band(k):
    return slice(k * CUBE_BAND, (k + 1) * CUBE_BAND)


def euler_quat(rpy):
    """(x, y, z, w) of pybullet's getQuaternionFromEuler: R = Rz(yaw) Ry(pitch) Rx(roll)."""
    r, p, y = (0.5 * rpy[:, i] for i in range(3))
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], axis=1)


def gimbal_state(n=GIMBAL_N, seed=CUBE_SEED):
    """obj [n + 2, 13] of cubes at rest, roll and yaw anywhere: n rows whose pitch is U(0, 1e-3) inside
    +-pi/2, then one row each at +pi/2 and -pi/2 themselves.  There sin(pitch) reaches 1 (the clamp
    of quat_euler) and both arguments of roll's and yaw's atan2 vanish: the reference's formula
    returns rounding noise for them, in fp64 too, so those two rows are checked for finite angles
    and the pitch bound only."""
    rng = np.random.default_rng(seed + 1)
    off = np.concatenate([rng.uniform(0.0, 1e-3, n), [0.0, 0.0]])
    n += 2
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    rpy = np.stack([rng.uniform(-np.pi, np.pi, n), sign * (0.5 * np.pi - off), rng.uniform(-np.pi, np.pi, n)], axis=1)
    obj = np.zeros((n, 13))
    obj[:, 0] = np.linspace(-0.2, 0.1, n)
    obj[:, 2] = 1.0
    obj[:, 3:7] = euler_quat(rpy)
    return obj.astype(np.float32).astype(np.float64)


def quat_rot(q):
    """R [n, 3, 3] of the quaternions q [n, 4] (x, y, z, w), normalised first."""
    x, y, z, w = _unit(np.asarray(q, np.float64)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def euler_rot(rpy):
    return quat_rot(euler_quat(np.asarray(rpy, np.float64)))


def angle_diff(a, b):
    """|a - b| modulo 2 pi (roll and yaw across the +-pi seam)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2.0 * np.pi)
    return np.minimum(d, 2.0 * np.pi - d)


def quat_diff(a, b):
    """max |a -+ b| per row: the quaternions up to sign."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1))


def cube_inject(ref, obj):
    """obj [n, 13] into an oracle env, the contact cache and the manifolds cleared."""
    from oracle import oracle as O

    ref.obj[:, :13] = obj
    ref.obj[:, O.OBJ_CACHE:O.OBJ_AO:2] = -1.0
    ref.obj[:, O.OBJ_CACHE + 1:O.OBJ_AO:2] = 0.0
    ref.obj[:, O.OBJ_MAN:O.OBJ_N] = 0.0


def cube_points(O, ref):
    """Contact points per env in the oracle's cache after the step, object-scene and robot slots."""
    return (ref.obj[:, O.OBJ_CACHE:O.OBJ_AO:2] >= 0).sum(axis=1)


def vel_bar(v64):
    return VEL_TOL * np.maximum(1.0, np.abs(v64))
