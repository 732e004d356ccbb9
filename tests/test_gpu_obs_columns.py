"""Per-step oracle parity of every observation column under contact.

The position bars of test_gpu_contacts.py and test_gpu_reach_ao.py barely see a velocity error: from
a shared start state an error e in a substep's velocity moves a position by at most e x 0.04 s, and
the velocity the last substep leaves does not enter the position at all.  Here the device free-runs,
its state is copied into the fp64 oracle and the fp32 oracle before every step, all three step with
the same action (obs_columns.cube_run / ao_run), and every column the position bars leave out is
held to the fp32 oracle's own deviation from fp64 on the same rows, percentile for percentile:

  Push / PickAndPlace under the scripted push (128 envs x 50 steps, both layouts): the EE velocity
  (obs 3:6), the cube's rotation (rebuilt from the Euler columns, the columns themselves off the
  gimbal rows, the state quaternion), its linear and angular velocity; on the rows with a robot-cube
  point (touched: p50 / p90 / p99, slack 1), on the rows where the cube slides on the table alone
  (sliding: the velocities' p50 / p90, slack limp_arm.SLACK) and on all rows (p99 / p99.9, slack 1);
  the cube's position and velocity columns are the state's own bits and PickAndPlace's width the
  oracle's.  (EE position 0:3 and cube position: test_gpu_contacts.py.)
  ReachAO under the random policy (512 envs x 12 steps) and driven into a sphere (64 envs x 14
  steps, >= 50 % contact rows): EE velocity, q and qd (obs 3:20) at slack 1.25, every q sample within
  OBS_TOL, the 27 unit-vector columns per (env, link) pair by obs_columns.assert_unit_vectors, the
  distance columns at the existing bars.

test_obs_columns_oracle.py asserts the same row-class conditions on the oracle alone and shows which
wrong parameters miss these bars by >= 10 x.  Measured device / fp32-oracle ratios:
profiles/r14/pytest_gpu_obs_columns.log.

Measured (device | fp32 oracle; the velocities relative to max(1, |value64|)):

  cube tasks, device / fp32-oracle ratios over Push and PickAndPlace (shares of the touched / sliding /
  gimbal rows 0.098-0.120 / 0.158-0.177 / 0.075-0.129):
    touched p50 / p90 / p99   wide   EE velocity 0.03 / 0.04 / 0.19, rotation 0.02 / 0.07 / 0.26, Euler
                                     0.02 / 0.07 / 0.26, quaternion 0.02 / 0.07 / 0.28, linvel 0.03 / 0.07 /
                                     0.26, angvel 0.04 / 0.07 / 0.36
                              narrow every quantity <= 0.04 / 0.08 / 0.20
      in absolute terms, Push wide: EE velocity 9.8e-6 / 6.1e-5 / 8.5e-4 | 3.1e-4 / 1.5e-3 / 5.5e-3, linvel
      1.1e-5 / 1.5e-4 / 3.0e-3 | 3.6e-4 / 2.2e-3 / 1.2e-2, angvel 1.8e-4 / 4.3e-3 / 1.3e-1 | 4.3e-3 / 5.9e-2 / 3.7e-1
    sliding p50 / p90         linvel 0.99-1.00 / 0.05-0.07 (3.7e-7 | 3.7e-7 at p50: rounding level), angvel
                              1.02-1.26 / 0.07-0.12 (4.4e-7-1.5e-6 | 4.3e-7-1.2e-6)
    all rows p99 / p99.9      every quantity <= 0.10 / 0.37
  The IK amplifies the fp32 oracle's rounding under robot contact and the device sits 3-50 x inside;
  where the cube slides on the table alone both sit at rounding level and the medians coincide.  One
  ratio passes its starting slack: PickAndPlace wide, sliding angvel p50 1.26 (1.50e-6 | 1.19e-6) ->
  obs_columns.CUBE_SLACKS, 1.5 x 1.26 = 1.89 by limp_arm.py's rule.

  ReachAO random policy, p50 / p99 / p99.9, wide: EE velocity 2.7e-6 / 1.1e-5 / 4.3e-5 | 2.7e-6 / 1.1e-5 /
  4.4e-5, q 1.6e-7 / 4.6e-7 / 7.4e-7 | 1.6e-7 / 4.5e-7 / 6.1e-7, qd 7.4e-6 / 2.2e-5 / 9.9e-5 | 7.4e-6 / 2.2e-5 /
  1.1e-4; ratios 0.94-1.21 (narrow 0.86-1.22); largest |q - q64| 3.5e-6; 0.045 % of 55242 pairs
  ambiguous, clear pairs p99 8.6e-7, max 9.4e-6 (narrow 8.9e-6).
  ReachAO driven into the sphere: 775 contact rows of 884 kept (0.88); contact rows p50 / p99, wide: EE
  velocity 8.1e-6 / 8.1e-5 | 7.9e-6 / 9.0e-5, q 3.6e-7 / 7.1e-6 | 3.7e-7 / 8.9e-6, qd 4.6e-5 / 7.6e-4 | 4.7e-5 /
  8.6e-4; ratios 0.80-1.03, narrow 0.90-1.17 but qd p99 1.2537 (8.29e-4 | 6.61e-4, the 8th largest of
  775 samples; the wide run of the same case has 7.6e-4 | 8.6e-4) -> obs_columns.AO_SLACKS, 1.89.
  0.54 % of the pairs ambiguous, clear pairs p99 2.3e-6, max 4.4e-5 (narrow 9.9e-5).

No kernel finding: the last substep's velocity write-back, the cube's damping and cross(w, v) under
contact and ReachAO's epilogue columns all sit inside the fp32 evaluation of the same algorithm.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import limp_arm as L  # noqa: E402
import obs_columns as C  # noqa: E402
from test_gpu_parity import OBS_TOL, _state_to_oracle  # noqa: E402


@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    pg.load_native()
    return pg


class DeviceLead:
    """The device as the free-running leader of obs_columns.cube_run / ao_run."""

    def __init__(self, venv):
        self.v = venv

    def obs(self):
        return self.v.obs.cpu().numpy()

    def sync(self, r64):
        _state_to_oracle(self.v, r64)

    def step(self, a):
        v = self.v
        v.step_tensors(torch.as_tensor(a, device="cuda:0"))
        st = v.state()
        obj = st["object"].cpu().numpy().T.copy() if "object" in st else None
        ended = (v.truncated | v.terminated).cpu().numpy() != 0
        return (v.obs.cpu().numpy(), obj, st["q"].double().cpu().numpy().T, st["qd"].double().cpu().numpy().T,
                ended)


def _oracles(oracle, v):
    return L.oracles(oracle, v._cfg, v.num_envs, v.robot_contact_budget() or -1)


@pytest.mark.parametrize("env_id", C.CUBE_ENVS)
def test_cube_columns_under_the_scripted_push(pg, oracle, env_id, lanes):
    v = pg.PandaVecEnv(env_id, num_envs=C.CUBE_N, device="cuda:0", seed=C.cube_seed(env_id, lanes),
                       lanes_per_env=lanes)
    v.reset_tensors()
    pool = "manifolds" in v.state()
    assert pool == (lanes == 16)            # Bullet's persistent manifolds: the per-pair budget's kernels
    r64, r32 = _oracles(oracle, v)
    run = C.cube_run(oracle, env_id, DeviceLead(v), r64, r32, C.cube_policy(env_id), pool=pool)
    v.close()
    print(f"\n{env_id} lanes {lanes}:")
    C.assert_cube_conditions(run)
    bad = []
    for cls, (rows, ps, qs) in C.cube_classes(run).items():
        for q in qs:
            bad += C.held(f"{cls:8s} {q:7s}", run["lead"][q][rows], run["fp32"][q][rows], ps,
                          C.cube_slack(env_id, lanes, cls, q))
    assert not bad, bad


def _ao_bars(case, lanes, run, rows, ps):
    bad = []
    for q in C.AO_QUANTITIES:
        bad += C.held(f"{q:6s}", run["lead"][q][rows], run["fp32"][q][rows], ps, C.ao_slack(case, lanes, q))
    ee = run["lead"]["ee"]
    print(f"  EE position p99 {np.percentile(ee, 99):.2e} max {ee.max():.2e}; q max {run['lead']['q'].max():.2e}")
    assert np.percentile(ee, 99) <= 1e-5 and ee.max() <= 1e-3           # the existing position bar
    C.assert_unit_vectors(run)
    return bad


def test_reach_ao_columns_random_policy(pg, oracle, lanes):
    v = pg.PandaVecEnv(C.AO_ENV, num_envs=C.AO_N, device="cuda:0", seed=21, lanes_per_env=lanes)
    v.reset_tensors(seed=C.AO_RESET_SEED)
    r64, r32 = _oracles(oracle, v)
    run = C.ao_run(oracle, v._cfg, DeviceLead(v), r64, r32, lambda t: v.sample_actions(t).cpu().numpy(), C.AO_STEPS)
    v.close()
    print(f"\nReachAO random policy lanes {lanes}: {len(run['contact'])} kept rows, {run['ended']} ended, contact rows "
          f"{run['contact'].mean() * 100:.2f} %")
    bad = _ao_bars("random", lanes, run, slice(None), C.AO_PS)
    assert run["lead"]["q"].max() <= OBS_TOL, run["lead"]["q"].max()
    assert not bad, bad


def test_reach_ao_columns_driven_into_a_sphere(pg, oracle, lanes):
    v = pg.PandaVecEnv(C.AO_ENV, num_envs=C.AO_DRIVEN_N, device="cuda:0", seed=1, lanes_per_env=lanes)
    com, _, _ = oracle.fk(v._cfg.model.contents, np.array(pg.abi.NEUTRAL_Q[:7]))
    goals, obst, act = C.driven_case(com[11])
    v.reset_tensors(goals=goals, objects=obst)
    r64, r32 = _oracles(oracle, v)
    run = C.ao_run(oracle, v._cfg, DeviceLead(v), r64, r32, lambda t: act, C.AO_DRIVEN_STEPS)
    v.close()
    c = run["contact"]
    print(f"\nReachAO driven into the sphere lanes {lanes}: {int(c.sum())} contact rows of {len(c)} kept "
          f"({c.mean():.2f}), {run['ended']} ended")
    assert c.mean() >= C.AO_CONTACT_MIN, c.mean()
    bad = _ao_bars("driven", lanes, run, c, C.AO_CONTACT_PS)
    assert not bad, bad
