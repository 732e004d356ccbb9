"""The conditions and the bite of test_gpu_obs_columns.py: oracle-only checks that run without a GPU.

The fp64 oracle free-runs (obs_columns.OracleLead); before every step its state is copied into the
fp32 oracle and into fp64 oracles with one parameter wrong, and all step with the same action
(obs_columns.cube_run / ao_run).  The device test holds the device to slack x the fp32 oracle's
percentiles on the same rows; here the row classes are shown to be populated and the mutants to miss
those bars by >= 10 x.  The figures below are profiles/r14/pytest_obs_columns_oracle.log.

Cube tasks, 128 envs x 50 steps of the scripted push (obs_columns.cube_policy), 6272 kept rows.  Shares
of the touched / sliding / gimbal rows (caps: >= 0.08, >= 0.10, <= 0.15), the fp64 oracle alone:

    Push          per-pair budget, seed 3   0.120 / 0.158 / 0.072      one-lane budget, seed 3   0.099 / 0.162 / 0.075
    PickAndPlace  per-pair budget, seed 3   0.108 / 0.176 / 0.127      one-lane budget, seed 6   0.118 / 0.164 / 0.079
    (PickAndPlace at the one-lane budget and seed 3: gimbal 0.166, past the cap: obs_columns.CUBE_SEEDS)

Nearly every gimbal row is a cube lying flat on a side (obs_columns.flat_rows: 0.066 of 0.072); there
the oracle's own Euler columns rebuild its own rotation to 0.05-0.2 only, on every other row to 2.2e-7.

The fp32 oracle's envelope, Push, p50 / p90 / p99 (the velocities relative to max(1, |value64|)):

    rows      EE velocity                   rotation                      linvel                        angvel
    touched   2.9e-4 / 1.6e-3 / 7.0e-3      2.2e-4 / 1.3e-3 / 6.8e-3      3.1e-4 / 2.1e-3 / 9.1e-3      4.2e-3 / 4.8e-2 / 3.3e-1
    sliding   -                             -                             2.4e-7 / 3.7e-4               3.0e-7 / 2.7e-3
    all, p99 / p99.9   1.0e-2 / 4.0e-2      2.0e-3 / 9.9e-3               3.0e-3 / 1.3e-2               8.8e-2 / 4.5e-1

Bite: the fp64 oracle stepped from the same states with one parameter wrong, as a multiple of the
device test's bar (slack x the envelope):

    friction x 1.1        touched p50: EE velocity 13.3, rotation 13.5, linvel 17.5, angvel 14.5;
                          sliding linvel p50 9.8e-3 = 3.2e4
    link_friction x 1.1   touched p99: EE velocity 25, linvel 10.9 (rotation 9.8 and angvel 8.1: not claimed)
    ang_damping 0.05      sliding angvel p50 1.0e-4 = 270

These clear 10 x at this seed; over the handle seeds 3-8 the link_friction claim on linvel ranges 6.3-10.9
(a p99 of ~750 rows), on the EE velocity 8.9-30.  Two 10 % errors do not clear the bar and the test
does not claim them: contact_erp 0.2 -> 0.22 stays within 2.8 x on the touched rows (2.6 x on all
rows), warmstart 0.85 -> 0.8 within 4.1 x (3.8 x): under robot contact the fp32 oracle is a loose
yardstick.  The device needs no slack above 1 on the touched rows (it sits 3-50 x inside).

ReachAO.  Random policy from the seeded resets 1000.. (256 envs x 8 steps here, 2047 kept rows): the
fp32 oracle alone has 0.027 % ambiguous pairs, clear-pair p99 1.0e-6, p99.9 1.4e-4, none of 18423
above 1e-3; its envelope p50 / p99 / p99.9 / max: q 1.6e-7 / 4.6e-7 / 5.9e-7 / 7.9e-6, qd 7.5e-6 /
2.2e-5 / 6.2e-5 / 9.9e-4, EE velocity 2.8e-6 / 1.1e-5 / 1.5e-5 / 1.7e-4.  Driven into a sphere
(obs_columns.driven_case, 64 envs x 14 steps): 773 contact rows of 880 kept (0.88), 16 ended; on the
contact rows p50 / p99: q 3.7e-7 / 7.9e-6, qd 4.5e-5 / 8.6e-4, EE velocity 7.3e-6 / 9.1e-5; 0.53 % of
the pairs ambiguous.  motor_kd x 1.1 misses the qd bar (1.25 x the envelope) by 451 / 341 x at p50 /
p99, motor_kp x 1.1 by 473 / 323 x; q and the EE velocity by 296-2900 x.
"""
import numpy as np
import pytest

import limp_arm as L
import obs_columns as C
from oracle import count_flops as CF

# (name, pgx_sim_params field, value or function of the current value)
CUBE_MUTANTS = (("friction x 1.1", "friction", lambda v: 1.1 * v),
                ("link_friction x 1.1", "link_friction", lambda v: 1.1 * v),
                ("ang_damping 0.05", "ang_damping", 0.05),
                ("contact_erp 0.22", "contact_erp", 0.22),
                ("warmstart 0.8", "warmstart", 0.8))
# mutant -> [(row class, percentile, quantities)] it is claimed for: >= BITE x the device test's bar
BITE = 10.0
CUBE_CLAIMS = {"friction x 1.1": [("touched", 50, ("ee_vel", "rot", "linvel", "angvel")), ("sliding", 50, ("linvel",))],
               "link_friction x 1.1": [("touched", 99, ("ee_vel", "linvel"))],
               "ang_damping 0.05": [("sliding", 50, ("angvel",))]}
# the 10 % errors the fp32 yardstick does not catch under robot contact: every touched-row ratio below this
UNCAUGHT = {"contact_erp 0.22": 10.0, "warmstart 0.8": 10.0}


def _oracle_run(O, env_id, mutants):
    cfg, keep = CF.make_cfg(env_id, C.CUBE_N, True, C.CUBE_SEED)
    r64, r32 = L.oracles(O, cfg, C.CUBE_N)
    lead = O.OracleVecEnv(cfg, C.CUBE_N)
    alive, ms = [], []
    for name, field, value in mutants:
        c, p = C.with_param(cfg, keep[1], field, value)
        alive.append((c, p))
        ms.append((name, O.OracleVecEnv(c, C.CUBE_N)))
    run = C.cube_run(O, env_id, C.OracleLead(lead, lead.reset()), r64, r32, C.cube_policy(env_id), mutants=ms)
    del alive, keep
    return run


@pytest.fixture(scope="module")
def push(oracle):
    return _oracle_run(oracle, "PandaPush-v3", CUBE_MUTANTS)


def _envelope(run):
    for cls, (rows, ps, qs) in C.cube_classes(run).items():
        for q in C.CUBE_QUANTITIES if cls != "sliding" else qs:
            print(f"  {cls:8s} {q:7s} fp32 oracle p{ps}: {L.fmt(C.pcts(run['fp32'][q][rows], ps))}, max "
                  f"{np.nanmax(run['fp32'][q][rows]):.2e}")


def test_push_conditions_and_envelope(push):
    print("\nPandaPush-v3, the fp64 oracle under the scripted push:")
    C.assert_cube_conditions(push)
    _envelope(push)
    assert len(push["touched"]) >= 6000
    g = push["gimbal"]
    for q in C.CUBE_QUANTITIES:     # the leader is the fp64 oracle itself: the float32 rounding of its observation
        print(f"  fp64 oracle against itself, {q}: max {np.nanmax(push['lead'][q]):.2e}, off the gimbal rows "
              f"{np.nanmax(push['lead'][q][~g]):.2e}")
        assert np.nanmax(push["lead"][q][~g]) <= 1e-6, q
        assert q == "rot" or np.nanmax(push["lead"][q]) <= 1e-6, q
    # the rotation rebuilt from the Euler columns is as close as the columns themselves off the gimbal
    # and stays bounded on it: the fp32 oracle's own figures on the gimbal rows
    near = g & ~push["flat"]
    print(f"  fp32 oracle rot p50 / p99 / max: the {int(near.sum())} gimbal rows not flat on a side "
          f"{L.fmt(L.pcts(push['fp32']['rot'][near]))}, the rest {L.fmt(L.pcts(push['fp32']['rot'][~g]))}")
    assert np.isnan(push["fp32"]["rot"][push["flat"]]).all() and np.isfinite(push["fp32"]["rot"][~push["flat"]]).all()
    assert np.isnan(push["fp32"]["euler"][g]).all() and np.isfinite(push["fp32"]["euler"][~g]).all()


def test_pick_and_place_conditions(oracle, push):
    run = _oracle_run(oracle, "PandaPickAndPlace-v3", ())
    print("\nPandaPickAndPlace-v3, the fp64 oracle under the scripted push:")
    C.assert_cube_conditions(run)
    _envelope(run)
    t, t0 = C.shares(run)[0], C.shares(push)[0]
    assert abs(t - t0) <= 0.02, (t, t0)     # the same script meets the cube as often


@pytest.mark.parametrize("full", [True, False], ids=["per-pair budget", "one-lane budget"])
@pytest.mark.parametrize("env_id", C.CUBE_ENVS)
def test_conditions_hold_at_both_budgets(oracle, env_id, full):
    """The fp64 oracle alone at the wide layout's per-pair budget (persistent manifolds: touched by the
    pool) and at the one-lane layout's 4 points (touched by the cache's cube ids)."""
    from panda_gym_amd import abi, envs

    seed = C.cube_seed(env_id, 16 if full else 1)
    _, keep = CF.make_cfg(env_id, C.CUBE_N, True, seed)
    cfg = abi.make_config(envs.spec(env_id), C.CUBE_N, keep[0], keep[1], seed=seed, contacts=True, full_manifold=full)
    oracle.set_robot_budget(-1)
    print(f"\n{env_id}, {'per-pair' if full else 'one-lane'} budget, seed {seed}, the fp64 oracle alone:")
    rows = C.cube_rows_oracle_alone(oracle, cfg, env_id, full)
    C.assert_cube_conditions(rows)
    # why "rot" leaves the flat rows out: there the fp64 oracle's own columns do not rebuild its own
    # rotation; on every other row, the other gimbal rows included, they do to float32 rounding
    flat, near = rows["flat"], rows["gimbal"] & ~rows["flat"]
    print(f"  the oracle's Euler columns against its own rotation: flat rows max {rows['self_rot'][flat].max():.2e}, "
          f"the other {int(near.sum())} gimbal rows {rows['self_rot'][near].max():.2e}, the rest "
          f"{rows['self_rot'][~rows['gimbal']].max():.2e}")
    assert rows["self_rot"][~flat].max() <= 1e-6 and rows["self_rot"][flat].max() > 1e-3


def test_cube_mutants_miss_the_bars(push):
    """Each mutant misses the bars it is claimed for by >= 10 x; two 10 % errors do not (printed with
    their ratios, and asserted to stay below 10 x: the test must not claim more than it catches)."""
    classes = C.cube_classes(push)
    print()
    for name, _, _ in CUBE_MUTANTS:
        worst = 0.0
        for cls, (rows, ps, qs) in classes.items():
            slack = L.SLACK if cls == "sliding" else 1.0
            for q in qs:
                m, f = C.pcts(push[name][q][rows], ps), C.pcts(push["fp32"][q][rows], ps)
                ratio = [x / (slack * y) for x, y in zip(m, f)]
                print(f"  {name:20s} {cls:8s} {q:7s} p{ps}: {L.fmt(m)} = " + " / ".join(f"{r:.3g}" for r in ratio)
                      + " x the bar")
                if cls == "touched":
                    worst = max(worst, max(ratio))
        for cls, p, qs in CUBE_CLAIMS.get(name, ()):
            rows, _, _ = classes[cls]
            slack = L.SLACK if cls == "sliding" else 1.0
            for q in qs:
                m, f = C.pcts(push[name][q][rows], (p,))[0], C.pcts(push["fp32"][q][rows], (p,))[0]
                assert m >= BITE * slack * f, (name, cls, p, q, m, f)
        if name in UNCAUGHT:
            assert worst < UNCAUGHT[name], (name, worst)


# ------------------------------------------------------------------ ReachAO
AO_MUTANTS = (("motor_kd x 1.1", "motor_kd", lambda v: 1.1 * v), ("motor_kp x 1.1", "motor_kp", lambda v: 1.1 * v))


def _ao(O, n, mutants=()):
    cfg, keep = CF.make_cfg(C.AO_ENV, n, True, 21)
    r64, r32 = L.oracles(O, cfg, n)
    lead = O.OracleVecEnv(cfg, n)
    alive, ms = [], []
    for name, field, value in mutants:
        c, p = C.with_param(cfg, keep[1], field, value)
        alive.append((c, p))
        ms.append((name, O.OracleVecEnv(c, n)))
    return cfg, keep, r64, r32, lead, ms, alive


def test_reach_ao_random_policy_conditions(oracle):
    """256 envs x 8 steps of the random policy from the seeded resets 1000..: the fp32 oracle alone
    meets the unit-vector rule and the ambiguous pairs are rare."""
    import panda_gym_amd as pg

    n, steps = 256, 8
    cfg, keep, r64, r32, lead, _, _ = _ao(oracle, n)
    draws = [pg.seeded_reset(pg.spec(C.AO_ENV), C.AO_RESET_SEED + i) for i in range(n)]
    first = lead.reset(inject_goal=np.array([g for g, _ in draws]), inject_obj=np.array([o for _, o in draws]))
    run = C.ao_run(oracle, cfg, C.OracleLead(lead, first), r64, r32, lead.sample_actions, steps)
    print(f"\nReachAO random policy, {len(run['contact'])} kept rows, {run['ended']} ended, contact rows "
          f"{run['contact'].mean() * 100:.2f} %")
    for q in C.AO_QUANTITIES:
        print(f"  {q:6s} fp32 oracle p{C.AO_PS} / max: {L.fmt(C.pcts(run['fp32'][q], C.AO_PS + (100,)))}")
    C.assert_unit_vectors(run, "fp32")
    assert run["lead"]["unit"].max() == 0.0
    del keep


def test_reach_ao_driven_contact_conditions_and_bite(oracle):
    from panda_gym_amd import abi

    n = C.AO_DRIVEN_N
    cfg, keep, r64, r32, lead, ms, alive = _ao(oracle, n, AO_MUTANTS)
    com, _, _ = oracle.fk(cfg.model.contents, np.array(abi.NEUTRAL_Q[:7]))
    goals, obst, act = C.driven_case(com[11])
    first = lead.reset(inject_goal=goals, inject_obj=obst)
    run = C.ao_run(oracle, cfg, C.OracleLead(lead, first), r64, r32, lambda t: act, C.AO_DRIVEN_STEPS, mutants=ms)
    c = run["contact"]
    print(f"\nReachAO driven into the sphere: {int(c.sum())} contact rows of {len(c)} kept ({c.mean():.2f}), "
          f"{run['ended']} ended")
    assert c.mean() >= C.AO_CONTACT_MIN, c.mean()
    for q in C.AO_QUANTITIES:
        print(f"  {q:6s} contact rows, fp32 oracle p{C.AO_CONTACT_PS}: {L.fmt(C.pcts(run['fp32'][q][c], C.AO_CONTACT_PS))}")
    C.assert_unit_vectors(run, "fp32")
    bit = {}
    for name, _, _ in AO_MUTANTS:
        for q in C.AO_QUANTITIES:
            m, f = C.pcts(run[name][q][c], C.AO_CONTACT_PS), C.pcts(run["fp32"][q][c], C.AO_CONTACT_PS)
            ratio = [x / (C.AO_SLACK * y) for x, y in zip(m, f)]
            print(f"  {name:15s} {q:6s} p{C.AO_CONTACT_PS}: {L.fmt(m)} = " + " / ".join(f"{r:.3g}" for r in ratio)
                  + " x the bar")
            bit[name, q] = max(ratio)
    assert max(bit[name, "qd"] for name, _, _ in AO_MUTANTS) >= BITE, bit
    del keep, alive
