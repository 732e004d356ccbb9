"""The limp-arm bar of test_gpu_limp_arm.py bites: oracle-only checks that run without a GPU.

test_gpu_limp_arm.py holds the device's qd after one ballistic env step (motors limp, zero
action, limp_arm.start_state) to SLACK_QD x the fp32 oracle's own deviation from the fp64 oracle.
Here the fp64 oracle steps the same state with a slightly wrong robot or damping, and each mutant's
median |qd - qd64| must be at least 10 x that bar (SLACK_QD x the fp32 envelope's p50 = 6.3e-7): a
kernel wrong by as much would fail the device test by an order of magnitude.  Measured (256 envs,
seed 7; fp32 envelope qd p50 7.9e-8, p99 5.7e-7):

    link 4 mass x 1.01            median 4.2e-4   (5300 x the envelope's p50, 670 x the bar)
    link 2 COM shifted 1 mm       median 5.8e-4   (7300 x, 910 x the bar)
    ang_damping 0.04 -> 0.05      median 1.2e-4   (1600 x, 190 x the bar)

so all three clear 10 x the bar, at the cap of 8 the slack stands at.  With the stock
motors (joint_forces x 1) the mass mutant's median is 7.0e-6 against an envelope p50 of 9.1e-7:
the motor impulse makes up most of the difference, which is why the arm is limp here.
"""
import numpy as np

import limp_arm as L
from oracle import count_flops as CF

N, SEED = 256, 7


def _step(O, cfg, n=N, seed=SEED, spread=L.SPREAD, fp32=False):
    """One zero-action env step of the fp64 (and fp32) oracle from the start state."""
    r64, r32 = L.oracles(O, cfg, n)
    r64.reset()
    q, qd = L.start_state(cfg, n, seed, spread)
    L.inject(r64, q, qd)
    L.copy_state(r64, r32)
    a = np.zeros((n, r64.ad), np.float32)
    o64 = r64.step(a)
    if fp32:
        r32.step(a)
    return r64, r32, o64


def _limp_cfg(env_id="PandaReachJoints-v3", scale=0.0):
    cfg, keep = CF.make_cfg(env_id, N, True, 3)
    L.set_forces(cfg, L.forces(scale))
    return cfg, keep


def _mutants(cfg, keep):
    """(name, cfg, the model and parameters it points to) of the wrong robots / parameters."""
    model, params = keep
    out = []
    for name in ("link 4 mass x 1.01", "link 2 COM + 1 mm", "ang_damping 0.05"):
        m, p = type(model).from_buffer_copy(model), type(params).from_buffer_copy(params)
        if name.startswith("link 4"):
            assert m.mass[4] > 0.0
            m.mass[4] *= 1.01
        elif name.startswith("link 2"):
            assert m.mass[2] > 0.0
            m.com[2][0] += 1e-3
        else:
            assert p.ang_damping == 0.04
            p.ang_damping = 0.05
        c = type(cfg).from_buffer_copy(cfg)
        c.model, c.params = type(cfg.model)(m), type(cfg.params)(p)
        out.append((name, c, (m, p)))
    return out


def test_mutants_exceed_ten_times_the_limp_bar(oracle):
    cfg, keep = _limp_cfg()
    r64, r32, _ = _step(oracle, cfg, fp32=True)
    env_p50 = float(np.median(np.abs(r32.qd - r64.qd)))
    bar = L.SLACK_QD * env_p50
    print(f"\nfp32 envelope qd p50 {env_p50:.2e}, bar {bar:.2e}")
    assert 2e-8 < env_p50 < 3e-7, env_p50            # rounding level: a few fp32 ulps of 1 rad/s
    for name, c, _alive in _mutants(cfg, keep):
        rm, _, _ = _step(oracle, c)
        med = float(np.median(np.abs(rm.qd - r64.qd)))
        print(f"{name}: median |qd - qd64| {med:.2e} = {med / env_p50:.0f} x the envelope's p50")
        assert med >= 10.0 * bar, (name, med, bar)


def test_start_state_is_ballistic(oracle):
    """The rows test_gpu_limp_arm.py keeps (no robot point, no dof at a limit, no truncation after
    the step): every row of Reach / Push, and of ReachAO -- whose obstacles the arm may touch --
    at least 90 % at its smaller pose spread."""
    for env_id in L.BALLISTIC_ENVS:
        for scale in (0.0, 1.0):
            cfg, keep = _limp_cfg(env_id, scale)
            r64, _, o64 = _step(oracle, cfg, spread=L.spread(env_id))
            ok = (L.robot_points(oracle, r64) == 0) & ~L.at_limit(cfg, r64.q).any(axis=1) & (o64["truncated"] == 0)
            print(f"\n{env_id} x{scale:g}: kept {ok.mean():.3f}, largest |qd| {np.abs(r64.qd).max():.1f}")
            assert ok.mean() >= (0.9 if env_id == "PandaReachAO-v3" else 1.0), (env_id, scale, ok.mean())
            del keep
