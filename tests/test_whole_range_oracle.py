"""The conditions and the bite of test_gpu_whole_range.py and test_gpu_tumbling_cube.py: oracle-only
checks that run without a GPU.

Whole-range arm states (whole_range.start_state: every dof U[lower + 0.05, upper - 0.05], qd U(-1, 1),
512 envs, seed 11; actions U(-1, 1), seed 5; one env step).  Measured on the fp64 oracle, rows classed
after the step (free: no robot point, no dof at a limit, not ended; limit: a dof at a limit, no point):

    EE control   Reach (table)   free 0.635  limit 0.344  robot points 0.021
                 Reach (no table)     0.645        0.355               0
                 Push                 0.635        0.344               0.021
                 PickAndPlace         0.629        0.346               0.025
    joint control, stock motors  free 0.994;  limp  free 0.977
    mat_to_quat branch of the start pose's EE rotation, x / y / z / trace > 0: 111 / 94 / 103 / 204 of
    512 rows, 15-38 % of the free rows each (limp_arm.start_state: all in x)
    fp32 oracle |q - q64| on the free rows p50 / p99 / max 3.7e-7 / 2.9e-5 / 1.8e-4, qd 9.9e-6 /
    7.7e-4 / 8.5e-3; its at-limit dof sets equal the fp64 oracle's on every limit row

The bar of the device test bites: the fp64 oracle steps the same states with a slightly wrong IK and
its median |q - q64| over the free rows must be at least 10 x (SLACK x the fp32 envelope's p50 =
4.6e-7).  Measured medians (Reach with the table; the other cases within 5 %):

    ik_max_iters 20 -> 19     2.3e-3   (5100 x the bar)
    ik_damping 0.5 -> 0.55    4.5e-3   (9700 x)
    ik_max_angle x 0.9        7.2e-5   (156 x: the step clamp is live from these states)

Tumbling cube (whole_range.cube_state, 256 envs, seed 9, zero action, one env step): no contact point
in any env, |sin(pitch64)| > 0.99 in 2.0 % of the rows.  The fp32 oracle against fp64 by |w| band
(small angle / 0.5-20 / 20-190 / clamp), maxima: position 3.8e-7 / 3.4e-7 / 3.9e-7 / 3.1e-7, quaternion
9.1e-7 / 4.0e-7 / 3.4e-7 / 5.0e-7, linear velocity 4.5e-7 / 2.9e-7 / 7.5e-7 / 1.3e-5 (|v64| up to 24 m/s),
angular velocity 1.0e-10 / 2.5e-6 / 2.0e-5 / 5.2e-5 (|w64| up to 224 rad/s).  The velocity bar of the
device test, 1e-4 x max(1, |value64|) on every row, bites in the 20-190 band: per row, the worst
component's |mutant - fp64| / bar is

    ang_damping 0.04 -> 0.05   min 85, median 337, max 565
    lin_damping 0.04 -> 0.05   min 0.7, median 7.8, max 14.7

The device test holds every row, so a kernel wrong by as much fails it by the band's largest ratio:
both clear 10 x (the linear one on its fastest cubes only: the damping acts on |v| <= 2.4 m/s there).
Near the gimbal (whole_range.gimbal_state: 16 rows within 1e-3 of +-pi/2) the fp64 oracle's own Euler
angles rebuild its rotation to 1.1e-7; the fp32 oracle's to 8.0e-6-2.7e-4 (asin's slope at 1)."""
import numpy as np
import pytest

import limp_arm as L
import whole_range as W
from oracle import count_flops as CF

ARM_CASES = [(e, c, "stock") for e, c in W.EE_CASES] + [(W.JOINTS_ENV, True, "stock"), (W.JOINTS_ENV, True, "limp")]
IK_MUTANTS = (("ik_max_iters 19", "ik_max_iters", lambda p: 19), ("ik_damping 0.55", "ik_damping", lambda p: 0.55),
              ("ik_max_angle x 0.9", "ik_max_angle", lambda p: 0.9 * p.ik_max_angle))


def _cfg(env_id, contacts, n, motors="stock"):
    cfg, keep = CF.make_cfg(env_id, n, contacts, 3)
    if motors == "limp":
        L.set_forces(cfg, L.forces(0.0))
    return cfg, keep


def _with_param(cfg, keep, field, value):
    """cfg with one pgx_sim_params field changed (and the copies it points to, to be kept alive)."""
    p = type(keep[1]).from_buffer_copy(keep[1])
    setattr(p, field, value)
    c = type(cfg).from_buffer_copy(cfg)
    c.params = type(cfg.params)(p)
    return c, p


def _arm_step(O, cfg, zero, fp32=True):
    r64, r32 = L.oracles(O, cfg, W.N)
    r64.reset()
    q0, qd0 = W.start_state(cfg)
    L.inject(r64, q0, qd0)
    L.copy_state(r64, r32)
    a = W.actions(W.N, r64.ad, zero)
    o64 = r64.step(a)
    if fp32:
        r32.step(a)
    return r64, r32, o64, q0


@pytest.fixture(scope="module")
def arm(oracle):
    """One step of both oracles per case, computed once: case -> (cfg, keep, r64, r32, o64, q0)."""
    out = {}
    for env_id, contacts, motors in ARM_CASES:
        cfg, keep = _cfg(env_id, contacts, W.N, motors)
        out[env_id, contacts, motors] = (cfg, keep) + _arm_step(oracle, cfg, motors == "limp")
    return out


@pytest.mark.parametrize("case", ARM_CASES, ids=lambda c: f"{c[0]}-{'table' if c[1] else 'no_table'}-{c[2]}")
def test_whole_range_conditions(oracle, arm, case):
    cfg, _, r64, r32, o64, q0 = arm[case]
    free, lim, pts = W.classes(oracle, cfg, r64, o64)
    fq, fqd = np.abs(r32.q - r64.q), np.abs(r32.qd - r64.qd)
    print(f"\n{case}: free {free.mean():.3f}, limit {lim.mean():.3f}, robot points {pts.mean():.3f}; fp32 oracle on "
          f"the free rows q {L.fmt(L.pcts(fq[free]))}, qd {L.fmt(L.pcts(fqd[free]))}")
    lo, hi = L.limits(cfg)
    assert np.all(q0 >= lo + W.EDGE - 1e-6) and np.all(q0 <= hi - W.EDGE + 1e-6)
    assert (q0.max(axis=0) - q0.min(axis=0) >= 0.9 * (hi - lo - 2 * W.EDGE)).all()     # the whole range
    if case[0] == W.JOINTS_ENV:
        assert free.mean() >= 0.9, free.mean()
        return
    assert free.mean() >= 0.5 and lim.mean() >= 0.2 and pts.mean() <= 0.05, (free.mean(), lim.mean(), pts.mean())
    br = W.ee_branches(oracle, cfg, q0)
    share = np.bincount(br[free], minlength=4) / free.sum()
    print(f"  mat_to_quat branch {W.BRANCHES}: all rows {np.bincount(br, minlength=4).tolist()}, share of the free rows "
          + " / ".join(f"{s:.3f}" for s in share))
    assert share.min() >= 0.10, share
    # the limit rows' dof sets: the fp32 evaluation of the algorithm agrees with fp64 on every row
    same = (L.at_limit(cfg, r32.q) == L.at_limit(cfg, r64.q)).all(axis=1)
    assert same[lim].all(), int((~same[lim]).sum())


def test_neutral_start_state_takes_one_branch(oracle):
    """Why the whole range: every row of the limp-arm start state (neutral +- 0.4 rad) takes the x
    branch of mat_to_quat."""
    cfg, keep = _cfg("PandaReach-v3", True, W.N)
    q0, _ = L.start_state(cfg, W.N, 7)
    assert np.all(W.ee_branches(oracle, cfg, q0) == 0)
    del keep


@pytest.mark.parametrize("case", [c for c in ARM_CASES if c[0] != W.JOINTS_ENV],
                         ids=lambda c: f"{c[0]}-{'table' if c[1] else 'no_table'}")
def test_ik_mutants_exceed_ten_times_the_bar(oracle, arm, case):
    cfg, keep, r64, r32, o64, _ = arm[case]
    free, _, _ = W.classes(oracle, cfg, r64, o64)
    env_p50 = float(np.median(np.abs(r32.q - r64.q)[free]))
    bar = L.SLACK * env_p50
    print(f"\n{case}: fp32 envelope q p50 {env_p50:.2e}, bar {bar:.2e}")
    assert 5e-8 < env_p50 < 2e-6, env_p50
    for name, field, value in IK_MUTANTS:
        c, alive = _with_param(cfg, keep, field, value(keep[1]))
        rm, _, _, _ = _arm_step(oracle, c, False, fp32=False)
        med = float(np.median(np.abs(rm.q - r64.q)[free]))
        print(f"  {name}: median |q - q64| {med:.2e} = {med / bar:.0f} x the bar")
        assert med >= 10.0 * bar, (name, med, bar)
        del alive


# ------------------------------------------------------------------ cube
def _cube_step(O, cfg, obj, fp32=True):
    n = len(obj)
    r64, r32 = L.oracles(O, cfg, n)
    r64.reset()
    W.cube_inject(r64, obj)
    L.copy_state(r64, r32)
    a = np.zeros((n, r64.ad), np.float32)
    o64 = r64.step(a)
    o32 = r32.step(a) if fp32 else None
    return r64, r32, o64, o32


@pytest.mark.parametrize("env_id", W.CUBE_ENVS)
def test_tumbling_cube_conditions_and_bite(oracle, env_id):
    cfg, keep = _cfg(env_id, True, W.CUBE_N)
    obj = W.cube_state()
    wn = np.linalg.norm(obj[:, 10:13], axis=1)
    for b, (lo, hi) in enumerate(W.W_BANDS):
        assert np.all((wn[W.band(b)] > lo) & (wn[W.band(b)] < hi)), b
    assert np.abs(np.linalg.norm(obj[:, 3:7], axis=1) - 1.0).max() < 1e-6
    r64, r32, o64, o32 = _cube_step(oracle, cfg, obj)
    k = r64.od - 12
    assert W.cube_points(oracle, r64).max() == 0 and L.robot_points(oracle, r64).max() == 0
    gimbal = np.abs(np.sin(o64["obs"][:, k + 4].astype(np.float64))) > W.GIMBAL_SIN
    print(f"\n{env_id}: gimbal share {gimbal.mean():.3f}")
    assert gimbal.mean() <= 0.05
    dt = float(keep[1].dt)
    w64 = np.linalg.norm(r64.obj[:, 10:13], axis=1)
    # the branches of the exponential map: small angle in every substep of band 0 (damping only
    # slows the cube), never in the others; the clamp in the first substep of every row of band 3
    assert wn[W.band(0)].max() < 1e-3 and w64[W.band(1)].min() > 1e-3
    assert wn[W.band(2)].max() * dt < np.pi / 8 < wn[W.band(3)].min() * dt
    for b, name in enumerate(W.BAND_NAMES):
        s = W.band(b)
        print(f"  {name}: |v64| <= {np.abs(r64.obj[s, 7:10]).max():.3g}, |w64| <= {np.abs(r64.obj[s, 10:13]).max():.3g}; "
              f"fp32 oracle max: pos {np.abs(r32.obj[s, :3] - r64.obj[s, :3]).max():.2e}, quat "
              f"{W.quat_diff(r32.obj[s, 3:7], r64.obj[s, 3:7]).max():.2e}, v "
              f"{np.abs(r32.obj[s, 7:10] - r64.obj[s, 7:10]).max():.2e}, w "
              f"{np.abs(r32.obj[s, 10:13] - r64.obj[s, 10:13]).max():.2e}")
        # the fp32 evaluation of the algorithm itself meets the device test's bars
        assert np.all(np.abs(r32.obj[s, 7:13] - r64.obj[s, 7:13]) <= W.vel_bar(r64.obj[s, 7:13]))
    s = W.band(2)
    for field, cols in (("ang_damping", slice(10, 13)), ("lin_damping", slice(7, 10))):
        assert getattr(keep[1], field) == 0.04
        c, alive = _with_param(cfg, keep, field, 0.05)
        rm, _, _, _ = _cube_step(oracle, c, obj, fp32=False)
        ratio = (np.abs(rm.obj[s, cols] - r64.obj[s, cols]) / W.vel_bar(r64.obj[s, cols])).max(axis=1)
        print(f"  {field} 0.05, band 20-190: |mutant - fp64| / bar per row min {ratio.min():.1f}, median "
              f"{np.median(ratio):.1f}, max {ratio.max():.1f}")
        # the device test holds every row to the bar: it fails by the band's largest ratio
        assert ratio.max() >= 10.0, (field, ratio.max())
        del alive


def test_gimbal_rows_rebuild_the_oracle_rotation(oracle):
    cfg, keep = _cfg("PandaPush-v3", True, W.GIMBAL_N + 2)
    obj = W.gimbal_state()
    r64, r32, o64, o32 = _cube_step(oracle, cfg, obj)
    k = r64.od - 12
    pitch = o64["obs"][:, k + 4].astype(np.float64)
    assert W.cube_points(oracle, r64).max() == 0
    assert np.all(np.abs(np.abs(pitch) - 0.5 * np.pi) <= 1e-3 + 1e-6), pitch
    assert np.all(np.sign(pitch[:W.GIMBAL_N:2]) == 1.0) and np.all(np.sign(pitch[1:W.GIMBAL_N:2]) == -1.0)
    R64 = W.quat_rot(r64.obj[:, 3:7])
    e64 = np.abs(W.euler_rot(o64["obs"][:, k + 3:k + 6]) - R64).max(axis=(1, 2))
    e32 = np.abs(W.euler_rot(o32["obs"][:, k + 3:k + 6]) - R64).max(axis=(1, 2))
    print(f"\ngimbal rows: rotation rebuilt from the Euler angles, fp64 oracle max {e64[:W.GIMBAL_N].max():.2e}, fp32 "
          f"oracle {L.fmt(L.pcts(e32[:W.GIMBAL_N]))}; the two rows at +-pi/2: {e64[W.GIMBAL_N:]}")
    assert e64[:W.GIMBAL_N].max() <= 1e-6
    assert 1e-6 < e32[:W.GIMBAL_N].max() < 1e-2     # asin's slope near 1 amplifies fp32 rounding: the envelope is wide
    del keep
