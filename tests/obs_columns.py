"""Shared pieces of the per-step comparison of every observation column (test_gpu_obs_columns.py on
the device, test_obs_columns_oracle.py on the CPU): the leader that free-runs, the two oracles
stepped from its state, the row classes, the per-row quantities and the bars.

The comparison is per step.  A leader free-runs (the device; on the CPU the fp64 oracle itself).
Before every step its state is copied into the fp64 oracle and from there into the fp32 oracle
(limp_arm.copy_state) and into every mutant (an fp64 oracle with one parameter wrong); all step with
the same action.  A row is kept when none of them ended the episode on that step; rows are classed on
the fp64 oracle after the step.

Cube tasks (Push: obs 18 = EE position 0:3, EE velocity 3:6, cube position 6:9, Euler angles 9:12,
linear velocity 12:15, angular velocity 15:18; PickAndPlace: 19, the fingers' width at 6 and the
cube's columns one further), under tests/scripted_push.py, 128 envs x 50 steps:

    touched   a robot-cube point after the step: the oracle's manifold pool count (obj[:, OBJ_MAN])
              > 0 where Bullet's persistent manifolds run (the per-pair budget: the pool holds
              robot-cube points only), else a robot slot of the contact cache with a cube id (>= 32)
    sliding   no such point, max |v, w| of the cube > 1e-2 and |z - 0.02| < 2e-3: the cube on the
              table top, the cube-table rows alone live
    gimbal    |sin(pitch64)| > whole_range.GIMBAL_SIN: a cube that left the table and landed on a
              side; the Euler columns themselves are compared on the other rows, the rotation
              rebuilt from them on every row

Per row: "ee_vel" max |obs[3:6] - obs64|; "rot" max |R(roll, pitch, yaw) - R(quat64)|; "euler"
whole_range.angle_diff of the three columns (NaN on gimbal rows); "quat" the state quaternion up to
sign; "linvel", "angvel" max |value - value64| / whole_range.vel_bar(value64), x VEL_TOL: the error
relative to max(1, |value64|).  On the rows where the cube lies flat on a side (flat_rows) sin(pitch)
reaches the clamp of quat_euler and both arguments of roll's and yaw's atan2 vanish
(whole_range.gimbal_state: the reference's formula returns rounding noise there, in fp64 too): the
fp64 oracle's own float32 Euler columns rebuild its own rotation to 0.05-0.2 only, so "rot" is NaN on
those rows -- they are held to finite angles and the pitch bound, as whole_range.gimbal_state's two
rows at +-pi/2 are, and the quaternion covers their rotation; on every other row, the rest of the
gimbal rows included, the oracle's columns rebuild its rotation to 2e-7 and "rot" is compared.

ReachAO (obs 56 = EE position 0:3, EE velocity 3:6, q 6:13, qd 13:20, link distances 20:29, unit
vectors 29:56): "ee_vel", "q", "qd" per row against the fp64 oracle's state, and per (env, link) pair
the unit vector's largest component error, with the pairs classed clear / ambiguous (ambiguous_pairs).

Slacks.  The bars are the project's rule -- the device at least as close to fp64 as the fp32
evaluation of the same algorithm from the same state, percentile for percentile -- times a slack:
1 for the IK tasks' touched and all rows, limp_arm.SLACK on the sliding rows and for ReachAO.  Where
the device sits above a bar at rounding level the slack is limp_arm.py's written rule, 1.5 x the
largest measured device / fp32-oracle ratio, capped at 8 (whole_range.slack_rule); CUBE_SLACKS and
AO_SLACKS hold the measured ratios that needed it, with the log that has them."""
import numpy as np

import limp_arm as L
import whole_range as W

CUBE_ENVS = ("PandaPush-v3", "PandaPickAndPlace-v3")
# The handle's seed (the cubes' and goals' reset draws): 3, but for PickAndPlace at the one-lane layout's
# budget of 4 robot points, where the fp64 oracle alone has 16.6 % gimbal rows at seed 3 (more cubes
# are kicked over and lie on a side) -- past the cap below, so the Euler columns would be compared on
# too few rows.  There the seed is 6, chosen on the oracle alone among 3-8 as the one with the most
# room on both sides (touched 0.118, gimbal 0.079); test_obs_columns_oracle.py asserts the conditions
# for all four (task, budget) pairs at the seeds used here.
CUBE_N, CUBE_STEPS, CUBE_SEED, POLICY_SEED = 128, 50, 3, 11
CUBE_SEEDS = {("PandaPickAndPlace-v3", 1): 6}
TOUCHED_MIN, SLIDING_MIN, GIMBAL_MAX = 0.08, 0.10, 0.15
SLIDE_V, SLIDE_Z = 1e-2, 2e-3
CUBE_REST_Z = 0.02
# sin(pitch) = 2 (w y - z x) carries a few fp32 spacings (6e-8 each) of the quaternion's rounding, and
# roll's and yaw's atan2 arguments are of size cos(pitch) = sqrt(2 (1 - |sin|)): below 1 - |sin| = 1e-6
# (arguments of 1.4e-3 with noise of 1e-7, angles good to 1e-4) an fp32 evaluation reaches the clamp
# of quat_euler, where both arguments vanish and roll and yaw are rounding noise -- in the fp64
# oracle's float32 observation too.  A cube lying flat on a side sits there (1 - |sin| < 1e-8).
FLAT_SIN = 1e-6
PITCH_MAX = float(np.float32(0.5 * np.pi))     # (float32 rounds pi / 2 up)
CUBE_ID0 = 32            # robot slots of the contact cache: ids from here on are capsule x cube points
CUBE_QUANTITIES = ("ee_vel", "rot", "euler", "quat", "linvel", "angvel")
SLIDING_QUANTITIES = ("linvel", "angvel")
TOUCHED_PS, SLIDING_PS, ALL_PS = (50, 90, 99), (50, 90), (99, 99.9)

AO_ENV = "PandaReachAO-v3"
AO_N, AO_STEPS, AO_RESET_SEED = 512, 12, 1000
AO_SLACK = 1.25          # test_gpu_fp32_envelope.SLACK["PandaReachAO-v3"]
AO_PS = (50, 99, 99.9)
AO_DRIVEN_N, AO_DRIVEN_STEPS, AO_DRIVEN_SEED = 64, 14, 5
AO_CONTACT_MIN, AO_CONTACT_PS = 0.5, (50, 99)
AO_QUANTITIES = ("ee_vel", "q", "qd")
UNIT_TOL, UNIT_OUTLIER, UNIT_TOUCH, UNIT_REL, UNIT_TRIALS = 1e-5, 1e-3, 1e-4, 1e-6, 4
AMBIGUOUS_MAX = 0.01

# (env id, lanes, row class, quantity) -> the largest measured device / fp32-oracle ratio that sits
# above the starting slack (1 on the touched and all rows, limp_arm.SLACK on the sliding rows); the bar
# there is whole_range.slack_rule of it.  Filled from profiles/r14/pytest_gpu_obs_columns.log.
CUBE_SLACKS = {
    # sliding medians sit at rounding level (device 1.50e-6 against 1.19e-6 of a velocity ~1): x 1.5 = 1.89
    ("PandaPickAndPlace-v3", 16, "sliding", "angvel"): 1.26,
}
# (case, lanes, quantity): the same for ReachAO (starting slack AO_SLACK)
AO_SLACKS = {
    # p99 of 775 contact rows, the 8th largest sample: 8.29e-4 against 6.61e-4 (the wide layout's run of
    # the same case: 7.59e-4 against 8.58e-4); 1.2537 rounded up, x 1.5 = 1.89
    ("driven", 1, "qd"): 1.26,
}


def cube_seed(env_id, lanes):
    return CUBE_SEEDS.get((env_id, lanes), CUBE_SEED)


def cube_slack(env_id, lanes, cls, quantity):
    start = L.SLACK if cls == "sliding" else 1.0
    return W.slack_rule(CUBE_SLACKS.get((env_id, lanes, cls, quantity), 0.0), start)


def ao_slack(case, lanes, quantity):
    return W.slack_rule(AO_SLACKS.get((case, lanes, quantity), 0.0), AO_SLACK)


def obj_col(env_id):
    """The first cube column of env_id's observation."""
    return 7 if "PickAndPlace" in env_id else 6


def cube_policy(env_id, n=CUBE_N, seed=POLICY_SEED):
    """The scripted push as a function of (observation before the step, t) -> actions [n, action_dim];
    PickAndPlace's gripper action is 0."""
    from scripted_push import ScriptedPush

    pol = ScriptedPush(n, seed=seed, obj_col=obj_col(env_id))
    if "PickAndPlace" in env_id:
        return lambda obs, t: np.concatenate([pol(obs, t), np.zeros((n, 1), np.float32)], axis=1)
    return pol


def with_param(cfg, params, field, value):
    """cfg with one pgx_sim_params field changed; (cfg, the params copy it points to: keep it alive).
    value: a number, or a function of the field's current value."""
    p = type(params).from_buffer_copy(params)
    cur = getattr(p, field)
    if callable(value):
        if hasattr(cur, "__len__"):
            for i in range(len(cur)):
                cur[i] = value(cur[i])
        else:
            setattr(p, field, value(cur))
    else:
        setattr(p, field, value)
    c = type(cfg).from_buffer_copy(cfg)
    c.params = type(cfg.params)(p)
    return c, p


class OracleLead:
    """The fp64 oracle as the free-running leader (the CPU file): its own state is the shared state."""

    def __init__(self, ref, first):
        self.ref, self._obs = ref, first["obs"]

    def obs(self):
        return self._obs

    def sync(self, r64):
        L.copy_state(self.ref, r64)

    def step(self, a):
        out = self.ref.step(a)
        self._obs = out["obs"]
        return out["obs"], self.ref.obj[:, :13].copy(), self.ref.q.copy(), self.ref.qd.copy(), \
            (out["truncated"] | out["terminated"]) != 0


def _finite(name, **arrays):
    for k, v in arrays.items():
        assert np.all(np.isfinite(v)), f"{name}: non-finite {k}"


def touched_rows(O, ref, pool):
    if pool:
        return ref.obj[:, O.OBJ_MAN] > 0
    return (ref.obj[:, O.OBJ_CACHE1:O.OBJ_AO:2] >= CUBE_ID0).any(axis=1)


def flat_rows(ref):
    """Rows whose cube lies flat on a side by the fp64 state: 1 - |sin(pitch64)| < FLAT_SIN."""
    x, y, z, w = W._unit(ref.obj[:, 3:7]).T
    return 1.0 - np.abs(2.0 * (w * y - z * x)) < FLAT_SIN


def cube_quantities(env_id, obs, obj, o64, r64, name="device"):
    """The per-row quantities (module docstring) of one candidate -- obs [n, od] and its cube state
    obj [n, 13] -- against the fp64 oracle's step (o64, r64).  Asserts the candidate finite first."""
    _finite(name, obs=obs, state=obj)
    k = obj_col(env_id)
    obs = np.asarray(obs, np.float64)
    ref = r64.obj
    R64 = W.quat_rot(ref[:, 3:7])
    rpy64 = o64["obs"][:, k + 3:k + 6].astype(np.float64)
    gimbal = np.abs(np.sin(rpy64[:, 1])) > W.GIMBAL_SIN
    flat = flat_rows(r64)
    # every row, the flat ones included: finite angles (above) and the pitch inside asin's range
    assert np.all(np.abs(obs[:, k + 4]) <= PITCH_MAX), (name, np.abs(obs[:, k + 4]).max())
    out = {"ee_vel": np.abs(obs[:, 3:6] - o64["obs"][:, 3:6]).max(axis=1),
           "rot": np.where(flat, np.nan, np.abs(W.euler_rot(obs[:, k + 3:k + 6]) - R64).max(axis=(1, 2))),
           "euler": np.where(gimbal, np.nan, W.angle_diff(obs[:, k + 3:k + 6], rpy64).max(axis=1)),
           "quat": W.quat_diff(obj[:, 3:7], ref[:, 3:7]),
           "linvel": W.VEL_TOL * (np.abs(obs[:, k + 6:k + 9] - ref[:, 7:10]) / W.vel_bar(ref[:, 7:10])).max(axis=1),
           "angvel": W.VEL_TOL * (np.abs(obs[:, k + 9:k + 12] - ref[:, 10:13]) / W.vel_bar(ref[:, 10:13])).max(axis=1)}
    return out, gimbal


def cube_bits(env_id, obs, obj, o64):
    """The bit equalities of a candidate's observation: the cube's position and velocity columns are
    the state's own bits, PickAndPlace's width column the oracle's."""
    k = obj_col(env_id)
    st = np.asarray(obj, np.float32)
    assert np.array_equal(obs[:, k:k + 3].view(np.uint32), st[:, 0:3].view(np.uint32)), "cube position bits"
    assert np.array_equal(obs[:, k + 6:k + 12].view(np.uint32), np.ascontiguousarray(st[:, 7:13]).view(np.uint32)), \
        "cube velocity bits"
    if k == 7:
        assert np.array_equal(obs[:, 6].view(np.uint32), o64["obs"][:, 6].view(np.uint32)), "width bits"


def cube_run(O, env_id, lead, r64, r32, policy, steps=CUBE_STEPS, mutants=(), pool=True, bits=True):
    """The per-step loop of the cube tasks.  Returns {"touched", "sliding", "gimbal": row masks,
    "lead", "fp32", mutant names...: {quantity: per-row array}} over the kept rows of every step."""
    rows = {"touched": [], "sliding": [], "gimbal": [], "flat": []}
    names = ["lead", "fp32"] + [m[0] for m in mutants]
    res = {nm: {q: [] for q in CUBE_QUANTITIES} for nm in names}
    for t in range(steps):
        a = np.asarray(policy(lead.obs(), t), np.float32)
        lead.sync(r64)
        L.copy_state(r64, r32)
        for _, rm in mutants:
            L.copy_state(r64, rm)
        obs, obj, _, _, ended = lead.step(a)
        _finite("lead", obs=obs, state=obj)
        o64, o32 = r64.step(a), r32.step(a)
        cand = [("lead", obs, obj), ("fp32", o32["obs"], r32.obj[:, :13])]
        keep = ~ended & ((o64["truncated"] | o64["terminated"] | o32["truncated"] | o32["terminated"]) == 0)
        for nm, rm in mutants:
            om = rm.step(a)
            cand.append((nm, om["obs"], rm.obj[:, :13]))
            keep &= (om["truncated"] | om["terminated"]) == 0
        if not keep.any():
            continue
        if bits:
            cube_bits(env_id, obs[keep], obj[keep], {"obs": o64["obs"][keep]})
        touched = touched_rows(O, r64, pool)
        sliding = ~touched & (np.abs(r64.obj[:, 7:13]).max(axis=1) > SLIDE_V) & \
            (np.abs(r64.obj[:, 2] - CUBE_REST_Z) < SLIDE_Z)
        for nm, ob, st in cand:
            qs, gimbal = cube_quantities(env_id, ob, st, o64, r64, nm)
            for q in CUBE_QUANTITIES:
                res[nm][q].append(qs[q][keep])
        rows["touched"].append(touched[keep])
        rows["sliding"].append(sliding[keep])
        rows["gimbal"].append(gimbal[keep])
        rows["flat"].append(flat_rows(r64)[keep])
    out = {k: np.concatenate(v) for k, v in rows.items()}
    for nm in names:
        out[nm] = {q: np.concatenate(v) for q, v in res[nm].items()}
    return out


def cube_rows_oracle_alone(O, cfg, env_id, pool, n=CUBE_N, steps=CUBE_STEPS):
    """The row masks of cube_run for the fp64 oracle free-running on its own (cfg: either budget), and
    "self_rot": how far its own Euler columns rebuild its own rotation, per row."""
    ref = O.OracleVecEnv(cfg, n)
    obs, policy, k = ref.reset()["obs"], cube_policy(env_id, n), obj_col(env_id)
    rows = {"touched": [], "sliding": [], "gimbal": [], "flat": [], "self_rot": []}
    for t in range(steps):
        out = ref.step(policy(obs, t))
        obs = out["obs"]
        keep = (out["truncated"] | out["terminated"]) == 0
        touched = touched_rows(O, ref, pool)
        sliding = ~touched & (np.abs(ref.obj[:, 7:13]).max(axis=1) > SLIDE_V) & \
            (np.abs(ref.obj[:, 2] - CUBE_REST_Z) < SLIDE_Z)
        gimbal = np.abs(np.sin(obs[:, k + 4].astype(np.float64))) > W.GIMBAL_SIN
        # the oracle's own float32 Euler columns against its own rotation
        self_rot = np.abs(W.euler_rot(obs[:, k + 3:k + 6]) - W.quat_rot(ref.obj[:, 3:7])).max(axis=(1, 2))
        for key, m in (("touched", touched), ("sliding", sliding), ("gimbal", gimbal), ("flat", flat_rows(ref)),
                       ("self_rot", self_rot)):
            rows[key].append(m[keep])
    return {key: np.concatenate(v) for key, v in rows.items()}


def cube_classes(run):
    """name -> (row mask, percentiles, quantities) of the cube bars."""
    return {"touched": (run["touched"], TOUCHED_PS, CUBE_QUANTITIES),
            "sliding": (run["sliding"], SLIDING_PS, SLIDING_QUANTITIES),
            "all": (np.ones(len(run["touched"]), bool), ALL_PS, CUBE_QUANTITIES)}


def pcts(x, ps):
    x = np.asarray(x, np.float64).ravel()
    x = x[~np.isnan(x)]           # "euler" on gimbal rows, "rot" on flat rows (the inputs were asserted finite)
    return [float(np.percentile(x, p)) for p in ps]


def shares(run):
    return float(run["touched"].mean()), float(run["sliding"].mean()), float(run["gimbal"].mean())


def assert_cube_conditions(run):
    t, s, g = shares(run)
    print(f"  {len(run['touched'])} kept rows: touched {t:.3f}, sliding {s:.3f}, gimbal {g:.3f} (flat on a side "
          f"{run['flat'].mean():.3f})")
    assert t >= TOUCHED_MIN and s >= SLIDING_MIN and g <= GIMBAL_MAX, (t, s, g)
    assert not (run["flat"] & ~run["gimbal"]).any()


def held(label, dev, f32, ps, slack):
    """dev <= slack x f32 at the percentiles ps, everything printed first; the list of misses."""
    d, f = pcts(dev, ps), pcts(f32, ps)
    ratio = [x / y if y > 0 else (1.0 if x == 0 else np.inf) for x, y in zip(d, f)]
    print(f"  {label} p{ps}: lead {L.fmt(d)} | fp32 oracle {L.fmt(f)} | ratio " + " / ".join(f"{r:.2f}" for r in ratio)
          + (f" | slack {slack:.2f}" if slack != 1.0 else "")
          + f" | max (printed only) {np.nanmax(dev):.2e} | {np.nanmax(f32):.2e}")
    return [(label, p, x, y, slack) for p, x, y in zip(ps, d, f) if not x <= slack * y]


# ------------------------------------------------------------------ ReachAO
def in_path_sphere(ee):
    """Obstacle centres [6, 3] with sphere 0 at EE height, 0.14 m towards +y -- in the path of
    panda_hand when joint 1 swings that way (test_gpu_reach_ao._in_path, kind 0) -- the rest parked."""
    obst = np.array([[99.9, 99.9, -99.9]] * 6)
    obst[0] = np.asarray(ee) + np.array([0.0, 0.14, 0.0])
    return obst


def driven_case(ee, n=AO_DRIVEN_N, seed=AO_DRIVEN_SEED):
    """(goals [n, 3], obstacles [n, 6, 3], action [n, 7]) of the obstacle-contact case: the sphere of
    in_path_sphere moved by U(-0.02, 0.02)^3 per env, joint 1 driven at 1 with U(-0.2, 0.2) on every
    joint, clipped -- one action per env, held over the run."""
    rng = np.random.default_rng(seed)
    obst = np.tile(in_path_sphere(ee)[None], (n, 1, 1))
    obst[:, 0] += rng.uniform(-0.02, 0.02, (n, 3))
    a = rng.uniform(-0.2, 0.2, (n, 7))
    a[:, 0] += 1.0
    return np.tile([[0.5, 0.3, 0.3]], (n, 1)), obst, np.clip(a, -1.0, 1.0).astype(np.float32)


def unit_vectors(O, cfg, q, obstacles):
    """u [9, 3] = (pb - pa) / |pb - pa| of ReachAO's nine links at q: the observation's unit vectors."""
    _, pa, pb, _ = O.ao_link_distances(cfg, q, obstacles)
    d = pb - pa
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def ambiguous_pairs(O, cfg, r64, o64, rows, rng):
    """[len(rows), 9] mask of the (env, link) pairs whose direction the fp64 oracle itself does not pin:
    |distance64| < UNIT_TOUCH (a touching link has no direction), or the oracle's own unit vector
    moves by more than UNIT_TOUCH under any of UNIT_TRIALS perturbations of the post-step q, each
    UNIT_REL relative (where a capsule runs parallel to a cuboid face the closest pair is not unique)."""
    amb = np.abs(o64["obs"][rows, 20:29].astype(np.float64)) < UNIT_TOUCH
    obst = r64.obstacles
    for j, e in enumerate(rows):
        u0 = unit_vectors(O, cfg, r64.q[e], obst[e])
        for _ in range(UNIT_TRIALS):
            u = unit_vectors(O, cfg, r64.q[e] * (1.0 + UNIT_REL * rng.standard_normal(7)), obst[e])
            amb[j] |= ~(np.abs(u - u0).max(axis=1) <= UNIT_TOUCH)
    return amb


def ao_quantities(obs, o64, r64, name="device"):
    _finite(name, obs=obs)
    obs = np.asarray(obs, np.float64)
    return {"ee_vel": np.abs(obs[:, 3:6] - o64["obs"][:, 3:6]).max(axis=1),
            "q": np.abs(obs[:, 6:13] - r64.q).max(axis=1), "qd": np.abs(obs[:, 13:20] - r64.qd).max(axis=1),
            "ee": np.abs(obs[:, 0:3] - o64["obs"][:, 0:3]).max(axis=1),
            "dist": np.abs(obs[:, 20:29] - o64["obs"][:, 20:29]),
            "unit": np.abs(obs[:, 29:56] - o64["obs"][:, 29:56]).reshape(len(obs), 9, 3).max(axis=2),
            "norm": np.linalg.norm(obs[:, 29:56].reshape(len(obs), 9, 3), axis=2)}


def ao_run(O, cfg, lead, r64, r32, actions, steps, mutants=(), seed=0):
    """The per-step loop of ReachAO; actions(t) -> [n, 7].  Returns {"contact": rows with a robot
    point after the step, "ambiguous": [rows, 9], "reproduced": the largest |u(ao_link_distances) -
    obs64| seen, "lead", "fp32", mutants...: {quantity: array}} over the kept rows."""
    names = ["lead", "fp32"] + [m[0] for m in mutants]
    keys = AO_QUANTITIES + ("ee", "dist", "unit", "norm")
    res = {nm: {q: [] for q in keys} for nm in names}
    contact, amb, ended_n = [], [], 0
    rng = np.random.default_rng(seed)
    for t in range(steps):
        a = np.asarray(actions(t), np.float32)
        lead.sync(r64)
        L.copy_state(r64, r32)
        for _, rm in mutants:
            L.copy_state(r64, rm)
        obs, _, _, _, ended = lead.step(a)
        o64, o32 = r64.step(a), r32.step(a)
        cand = [("lead", obs), ("fp32", o32["obs"])]
        keep = ~ended & ((o64["truncated"] | o64["terminated"] | o32["truncated"] | o32["terminated"]) == 0)
        for nm, rm in mutants:
            om = rm.step(a)
            cand.append((nm, om["obs"]))
            keep &= (om["truncated"] | om["terminated"]) == 0
        ended_n += int((~keep).sum())
        rows = np.flatnonzero(keep)
        if not len(rows):
            continue
        for nm, ob in cand:
            qs = ao_quantities(ob, o64, r64, nm)
            for q in keys:
                res[nm][q].append(qs[q][keep])
        contact.append(L.robot_points(O, r64)[keep] > 0)
        amb.append(ambiguous_pairs(O, cfg, r64, o64, rows, rng))
    out = {"contact": np.concatenate(contact), "ambiguous": np.concatenate(amb), "ended": ended_n}
    for nm in names:
        out[nm] = {q: np.concatenate(v) for q, v in res[nm].items()}
    return out


def assert_unit_vectors(run, name="lead"):
    """Rule 2: the unit vectors of the clear pairs, the conditions on the ambiguous ones."""
    amb, r = run["ambiguous"], run[name]
    clear = r["unit"][~amb]
    above = int((clear > UNIT_OUTLIER).sum())
    p99, p999 = pcts(clear, (99, 99.9))
    print(f"  unit vectors ({name}): {amb.mean() * 100:.3f} % of {amb.size} pairs ambiguous; clear pairs p99 "
          f"{p99:.2e} p99.9 {p999:.2e} max {clear.max():.2e}, {above} above {UNIT_OUTLIER:g}; distances p99 "
          f"{pcts(r['dist'].max(axis=1), (99,))[0]:.2e} max {r['dist'].max():.2e}")
    assert amb.mean() <= AMBIGUOUS_MAX, amb.mean()
    assert p99 <= UNIT_TOL, p99
    assert above <= clear.size // 2000, (above, clear.size)
    assert np.abs(r["norm"] - 1.0).max() <= 1e-5, np.abs(r["norm"] - 1.0).max()      # clear and ambiguous alike
    # the distance column: the existing bars of test_gpu_reach_ao.py, the ambiguous pairs included
    assert pcts(r["dist"].max(axis=1), (99,))[0] <= 1e-5 and r["dist"].max() <= 1e-3, r["dist"].max()
