"""A tumbling cube in free flight against the fp64 oracle: object_integrate and quat_euler.

No other cube comparison starts away from the identity orientation (but for a yaw of 0.3 rad), and the
free-fall test releases the cube at rest.  Here 256 cubes start 1 m above the table with a uniformly
random orientation, a linear velocity in (-1, 1) m/s and an angular velocity of random direction in
four bands of |w| (whole_range.cube_state): (0, 9e-4) rad/s, the exponential map's small-angle branch
in every substep; (0.5, 20) and (20, 190), its plain branch (__sinf, __cosf, the hardware rcp and
rsq); (200, 400), its clamp at |w| dt > pi / 8.  One env step with a zero action, no contact (the
oracle's cache stays empty: test_whole_range_oracle.py), so the step is gravity, the base bias term
cross(w, v), the linear and quadratic damping, the integration and quat_euler's three angles.

Per band, against the fp64 oracle stepped from the same state: cube position and the state
quaternion (up to sign) within OBS_TOL = 1e-4; the Euler columns of the observation within 1e-4
(modulo 2 pi) on rows with |sin(pitch64)| <= 0.99; linear and angular velocity within
1e-4 x max(1, |value64|) (they reach 24 m/s and 224 rad/s in the clamped band).  The bars are the
project's absolute ones: the kernel's hardware sin / cos may sit above the fp32 oracle's envelope, and
the device / fp32-oracle ratios are printed per band and quantity.  test_whole_range_oracle.py shows
that ang_damping or lin_damping 0.05 instead of 0.04 misses the velocity bar by 565 x and 14.7 x.

Near the gimbal (whole_range.gimbal_state: 16 cubes within 1e-3 of pitch +-pi/2, and one each at
+-pi/2): finite angles, |pitch| <= pi/2 to one float32 spacing, and the rotation rebuilt from the
device's (roll, pitch, yaw) within SLACK_R x the fp32 oracle's figure of the fp64 oracle's rotation.

Measured (profiles/r12/pytest_gpu_tumbling_cube.log; both tasks and both layouts run the same object
code and give the same figures), the device's largest deviation per band (small angle / 0.5-20 /
20-190 / clamp) and its ratio to the fp32 oracle's at p50 / p99 / max in the band where it is largest:

    position      3.8e-7 / 3.4e-7 / 3.9e-7 / 3.5e-7     ratio <= 1.29 / 1.04 / 1.13
    quaternion    8.7e-7 / 3.5e-7 / 7.0e-7 / 9.3e-7     20-190: 2.02 / 1.79 / 2.04 (__sinf, __cosf, rcp, rsq)
    Euler angles  3.7e-6 / 2.2e-6 / 2.2e-6 / 1.9e-6     20-190: 1.50 / 1.84 / 2.00
    linvel        4.5e-7 / 2.7e-7 / 1.0e-6 / 2.7e-5     clamp: 1.38 / 1.45 / 1.99; 0.11 of the bar at most
    angvel        1.0e-10 / 2.5e-6 / 2.0e-5 / 5.4e-5    ratio <= 1.04; 0.004 of the bar at most

so the hardware transcendentals cost the quaternion a factor of two over the fp32 oracle, 100 x inside
the bar.  Gimbal rows: device pitch equal to the clamp constant or to one of a few float32 values of
asinf next to 1; rebuilt rotation p50 / max 5.9e-5 / 3.1e-4 against the fp32 oracle's 6.7e-5 / 3.1e-4
(ratio 0.88 / 1.00): SLACK_R stays at 1.25.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import limp_arm as L  # noqa: E402
import whole_range as W  # noqa: E402
from test_gpu_fp32_envelope import _copy_state  # noqa: E402
from test_gpu_limp_arm import _held, _oracles  # noqa: E402
from test_gpu_parity import OBS_TOL, _state_to_oracle  # noqa: E402

SLACK_R = L.SLACK     # the gimbal rows' rebuilt rotation (whole_range.slack_rule from this start)


@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    pg.load_native()
    return pg


def _step_cubes(pg, oracle, env_id, obj, lanes):
    """One zero-action step of the device and both oracles from the injected cube state: (r64, r32,
    o64, o32, device object state [n, 13] as doubles, device observation)."""
    n = len(obj)
    v = pg.PandaVecEnv(env_id, num_envs=n, device="cuda:0", seed=3, lanes_per_env=lanes)
    v.reset_tensors()
    st = v.state()
    st["object"].copy_(torch.as_tensor(obj.T.copy(), dtype=torch.float32, device="cuda:0"))
    st["contacts"][0::2] = -1.0
    st["contacts"][1::2] = 0.0
    if "manifolds" in st:
        st["manifolds"].zero_()
    r64, r32 = _oracles(oracle, v)
    _state_to_oracle(v, r64)
    _copy_state(r64, r32)
    assert np.array_equal(r64.obj[:, :13], obj)      # the state is float32 values: nothing was rounded
    a = torch.zeros((n, v.action_dim), device="cuda:0")
    v.step_tensors(a)
    o64, o32 = r64.step(a.cpu().numpy()), r32.step(a.cpu().numpy())
    dev = v.state()["object"].double().cpu().numpy().T
    obs = v.obs.cpu().numpy()
    ended = v.truncated.cpu().numpy() | v.terminated.cpu().numpy() | o64["truncated"] | o64["terminated"]
    v.close()
    assert not ended.any()
    assert W.cube_points(oracle, r64).max() == 0
    return r64, r32, o64, o32, dev, obs


def _ratio(name, dev, f32):
    d, f = L.pcts(dev), L.pcts(f32)
    print(f"    {name}: device {L.fmt(d)} | fp32 oracle {L.fmt(f)} | ratio "
          + " / ".join(f"{x / y:.2f}" if y > 0 else "-" for x, y in zip(d, f)))
    return d[-1]


@pytest.mark.parametrize("env_id", W.CUBE_ENVS)
def test_tumbling_cube_one_step(pg, oracle, env_id, lanes):
    obj = W.cube_state()
    r64, r32, o64, o32, dev, obs = _step_cubes(pg, oracle, env_id, obj, lanes)
    k = obs.shape[1] - 12          # obs: ..., cube position, euler, linear velocity, angular velocity
    assert np.all(np.isfinite(dev)) and np.all(np.isfinite(obs))
    # the observation's position and velocity columns are the state's
    assert np.array_equal(obs[:, k:k + 3], dev[:, 0:3].astype(np.float32))
    assert np.array_equal(obs[:, k + 6:k + 12], dev[:, 7:13].astype(np.float32))
    e64 = o64["obs"][:, k + 3:k + 6].astype(np.float64)
    clear = np.abs(np.sin(e64[:, 1])) <= W.GIMBAL_SIN
    print(f"\n{env_id} lanes {lanes}: gimbal share {1.0 - clear.mean():.3f}")
    assert 1.0 - clear.mean() <= 0.05
    bad = []
    for b, name in enumerate(W.BAND_NAMES):
        s = W.band(b)
        c = clear[s]
        print(f"  |w| band {name} (p50 / p99 / max):")
        pos = _ratio("position  ", np.abs(dev[s, 0:3] - r64.obj[s, 0:3]), np.abs(r32.obj[s, 0:3] - r64.obj[s, 0:3]))
        quat = _ratio("quaternion", W.quat_diff(dev[s, 3:7], r64.obj[s, 3:7]), W.quat_diff(r32.obj[s, 3:7], r64.obj[s, 3:7]))
        eul = _ratio("euler     ", W.angle_diff(obs[s, k + 3:k + 6], e64[s])[c],
                     W.angle_diff(o32["obs"][s, k + 3:k + 6], e64[s])[c])
        ev, ew = np.abs(dev[s, 7:10] - r64.obj[s, 7:10]), np.abs(dev[s, 10:13] - r64.obj[s, 10:13])
        _ratio("linvel    ", ev, np.abs(r32.obj[s, 7:10] - r64.obj[s, 7:10]))
        _ratio("angvel    ", ew, np.abs(r32.obj[s, 10:13] - r64.obj[s, 10:13]))
        rv, rw = (ev / W.vel_bar(r64.obj[s, 7:10])).max(), (ew / W.vel_bar(r64.obj[s, 10:13])).max()
        print(f"    largest |v - v64| / bar {rv:.3f}, |w - w64| / bar {rw:.3f}")
        bad += [(name, what, x) for what, x, tol in (("position", pos, OBS_TOL), ("quaternion", quat, OBS_TOL),
                                                      ("euler", eul, 1e-4), ("linvel / bar", rv, 1.0),
                                                      ("angvel / bar", rw, 1.0)) if not x <= tol]
    assert not bad, bad


def test_euler_angles_near_the_gimbal(pg, oracle, lanes):
    obj = W.gimbal_state()
    r64, r32, o64, o32, dev, obs = _step_cubes(pg, oracle, "PandaPush-v3", obj, lanes)
    k = obs.shape[1] - 12
    rpy = obs[:, k + 3:k + 6]
    print(f"\ngimbal lanes {lanes}: device pitch {rpy[:, 1].tolist()}")
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(dev))
    half_pi = np.float32(0.5 * np.pi)
    assert np.all(np.abs(rpy[:, 1]) <= half_pi + np.spacing(half_pi)), np.abs(rpy[:, 1]).max()
    assert np.all(np.sign(rpy[:, 1]) == np.sign(obj[:, 4] * obj[:, 6] - obj[:, 3] * obj[:, 5]))
    n = W.GIMBAL_N
    R64 = W.quat_rot(r64.obj[:n, 3:7])
    e_dev = np.abs(W.euler_rot(rpy[:n]) - R64).max(axis=(1, 2))
    e_32 = np.abs(W.euler_rot(o32["obs"][:n, k + 3:k + 6]) - R64).max(axis=(1, 2))
    bad = _held("rebuilt rotation", e_dev, e_32, (50, 100), SLACK_R)
    # the quaternion itself: a cube at rest keeps it (renormalised)
    assert W.quat_diff(dev[:, 3:7], r64.obj[:, 3:7]).max() <= OBS_TOL
    assert not bad, bad
