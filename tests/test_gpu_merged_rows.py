"""The arm kernels' merged-register sweeps (substep_g, MERGE): waves holding 1 or 2 robot points and
no extra points keep the 7 dofs' velocity deltas, the partial solve's slot and the 6 contact rows'
velocities in one register, so a PGS row is one fma.  Per lane it is the fma the two registers
did, so the claim is bit-exact equality with the two-register sweeps, which PGX_PGS_MODE=4 ("auto,
but never merge") keeps in the same library; modes 2 (all rows) and 3 (always redo) never merge
their final solve either."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NEVER_MERGE = "4"
PRESS_STEPS = 12
DOF = 6   # the dof put at its lower limit: the last wrist joint (turning it keeps the tool on the table)


@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    pg.load_native()
    return pg


def _make(pg, mode, n, seed=9, **kw):
    with pytest.MonkeyPatch.context() as mp:   # the hook is read when the handle is created
        mp.setenv("PGX_PGS_MODE", mode)
        if n <= 256:   # never sorted, launch order = env order: envs 4w .. 4w + 3 share wave w
            mp.setenv("PGX_SORT_ENVS", "0")
        return pg.PandaVecEnv("PandaReach-v3", num_envs=n, device="cuda:0", seed=seed, lanes_per_env=16, **kw)


def _press(v, t):
    """The pressing-down policy of test_speculative_limit_skip_is_exact: z = -1, x / y random."""
    a = torch.zeros((v.num_envs, v.action_dim), device="cuda:0")
    a[:, 2] = -1.0
    a[:, :2] = v.sample_actions(t)[:, :2]
    return a


def _points(v):
    """Robot contact points per env after the last step (the warm-start cache's live robot slots,
    as tools/point_hist.py reads them)."""
    from panda_gym_amd import abi

    c = v.state()["contacts"]
    ids = c[2 * abi.OBJECT_POINTS::2][:v.robot_contact_budget()]
    return (ids >= 0).sum(0).cpu().numpy()


def _out(v):
    o = torch.cat([v.obs, v.state()["qd"].T], 1).cpu().numpy().copy()
    assert np.all(np.isfinite(o))
    return o


def _pressed_run(pg, mode, n, steps=25):
    v = _make(pg, mode, n)
    v.reset_tensors(seed=9)
    outs, pts = [], []
    for t in range(steps):
        v.step_tensors(_press(v, t))
        outs.append(_out(v))
        pts.append(_points(v))
    v.close()
    return np.stack(outs), np.stack(pts)


def test_merged_sweeps_are_exact_pressing_down(pg):
    """256 envs pressed onto the table for 25 steps: the default solve (merged sweeps in the waves
    with 1 or 2 points) against all rows, always redo (the columns split again for the all-rows
    solve) and never merge."""
    runs = {mode: _pressed_run(pg, mode, 256) for mode in ("0", "2", "3", NEVER_MERGE)}
    pts = runs["0"][1]
    # the merged copy ran: on some step every env holds at most 2 points and one holds some
    assert any(1 <= p.max() <= 2 for p in pts), [int(p.max()) for p in pts]
    for mode in ("2", "3", NEVER_MERGE):
        assert np.array_equal(runs["0"][0], runs[mode][0]), mode


def test_merged_sweeps_are_exact_two_waves_per_simd(pg):
    """The same run at 8192 envs: the two-waves-per-SIMD build, another register allocation (it
    keeps the two-register sweeps for now, DESIGN.md section 8 D: the check stands for the day
    it merges)."""
    a, pts = _pressed_run(pg, "0", 8192)
    b, _ = _pressed_run(pg, NEVER_MERGE, 8192)
    assert any(np.any((p >= 1) & (p <= 2)) for p in pts)
    assert np.array_equal(a, b)


@pytest.fixture(scope="module")
def pressed_state(pg):
    """256 envs after PRESS_STEPS pressing-down steps, solved with all rows (no speculation, no
    merged sweeps): the state views on the host, and the points per env."""
    v = _make(pg, "2", 256)
    v.reset_tensors(seed=9)
    for t in range(PRESS_STEPS):
        v.step_tensors(_press(v, t))
    st = {k: x.cpu().clone() for k, x in v.state().items() if k != "env_order"}
    pts = _points(v)
    v.close()
    return st, pts


def _from_state(pg, mode, st, n=None, **kw):
    """A handle in `mode` holding the first n envs of the state st."""
    n = n or st["q"].shape[-1]
    v = _make(pg, mode, n, **kw)
    v.reset_tensors(seed=9)
    dst = v.state()
    for k in ("q", "qd", "qc", "goal", "object", "contacts", "elapsed", "episode"):
        dst[k].copy_(st[k][..., :n].to(dst[k].device))
    return v


def _clear_robot_cache(st, e):
    from panda_gym_amd import abi

    st["contacts"][2 * abi.OBJECT_POINTS::2, e] = -1.0
    st["contacts"][2 * abi.OBJECT_POINTS + 1::2, e] = 0.0


def _oracle_wave(oracle, v, st, envs, act):
    """One fp64 oracle step of the envs `envs` from the state st: (env-substeps ending with a live
    limit row and robot points at once, the points per env after the step)."""
    oracle.set_robot_budget(v.robot_contact_budget() or -1)
    ref = oracle.OracleVecEnv(v._cfg, len(envs))
    ref.q[:] = st["q"].double().numpy().T[envs]
    ref.qd[:] = st["qd"].double().numpy().T[envs]
    ref.qc[:] = st["qc"].double().numpy().T[envs]
    ref.goal[:] = st["goal"].numpy().T[envs]
    ref.elapsed[:] = st["elapsed"].numpy()[envs]
    ref.episode[:] = st["episode"].numpy().view(np.uint32)[envs]
    ref.obj[:, :13] = st["object"].double().numpy().T[envs]
    oracle.set_contact_cache(ref.obj, st["contacts"].double().numpy().T[envs])
    oracle.set_manifolds(ref.obj, np.zeros((len(envs), 1)))
    diag = np.zeros(128, np.int64)
    oracle.lib().pgxo_diag_read(diag.ctypes.data_as(C.c_void_p), 1)
    ref.step(act[envs])
    oracle.lib().pgxo_diag_read(diag.ctypes.data_as(C.c_void_p), 1)
    oracle.set_robot_budget(-1)
    ids = ref.obj[:, oracle.OBJ_CACHE1:oracle.OBJ_AO:2]
    return int(diag[114]), (ids >= 0).sum(1)


def test_merged_sweeps_with_a_limit_pair_in_the_wave(pg, oracle, pressed_state):
    """Contact rows and a running limit pair (the partial solve's mirrored slot) in one register:
    in waves that hold a table point, one env starts 0.005 rad inside the last wrist joint's lower
    limit, turning into it at 2 rad/s (the tool keeps pressing on the table).  The waves are those
    in which the fp64 oracle, stepping the wave's 4 envs from that state, sees substeps that end
    with a limit impulse and hold robot points at once, and no env with more than 2 points.
    Random policy, 6 steps."""
    st0, pts = pressed_state
    st = {k: x.clone() for k, x in st0.items()}
    probe = _make(pg, "2", 256)
    act = probe.sample_actions(PRESS_STEPS).cpu().numpy().copy()
    lower = float(probe._cfg.model.contents.lower[DOF])
    chosen = []
    for w in range(256 // 4):
        envs = list(range(4 * w, 4 * w + 4))
        if not 1 <= pts[envs].max() <= 2:
            continue
        keep = envs[int(np.argmax(pts[envs]))]
        mate = min((e for e in envs if e != keep), key=lambda e: pts[e])
        trial = {k: x.clone() for k, x in st.items()}
        trial["q"][DOF, mate] = trial["qc"][DOF, mate] = lower + 0.005
        trial["qd"][DOF, mate] = -2.0
        _clear_robot_cache(trial, mate)
        both, after = _oracle_wave(oracle, probe, trial, envs, act)
        if both > 0 and after.max() <= 2:
            st = trial
            chosen.append(w)
        if len(chosen) == 3:
            break
    probe.close()
    assert chosen, "no wave with a table point and a live limit row in the oracle"
    runs = {}
    for mode in ("0", "2", NEVER_MERGE):
        v = _from_state(pg, mode, st)
        outs = []
        for t in range(6):
            v.step_tensors(v.sample_actions(PRESS_STEPS + t))
            outs.append(_out(v))
        runs[mode] = np.stack(outs)
        v.close()
    assert np.array_equal(runs["0"], runs["2"])
    assert np.array_equal(runs["0"], runs[NEVER_MERGE])


def test_wave_with_three_points_keeps_two_registers(pg, pressed_state):
    """64 envs, one forced to the hand-and-finger-on-the-table pose (5 points): its wave takes the
    two-register 4-point or extra-row copy while its neighbours merge.  Bit-identical to never
    merge, and every other env, its three wave mates included, to a run without the pose change (an
    env's result does not depend on the envs it shares a wave or a launch with).  One substep per
    env step, as in test_contact_budget_cases_keep_all_points, so that the cache after a step
    shows the points of the substep that ran; the posed env holds still (zero action)."""
    from test_oracle_contacts import TWO_LINKS_ON_TABLE_REL_Q

    n, k = 64, 21
    st0, pts = pressed_state
    assert np.any((pts[:n] >= 1) & (pts[:n] <= 2))
    st = {x: y.clone() for x, y in st0.items()}
    q = torch.tensor(TWO_LINKS_ON_TABLE_REL_Q, dtype=torch.float32)
    st["q"][:, k] = q
    st["qc"][:, k] = q
    st["qd"][:, k] = 0.0
    _clear_robot_cache(st, k)
    runs = {}
    for name, mode, s in (("merged", "0", st), ("never", NEVER_MERGE, st), ("plain", "0", st0)):
        v = _from_state(pg, mode, s, n, n_substeps=1)
        outs, cnt = [], []
        for t in range(5):
            a = _press(v, PRESS_STEPS + t)
            a[k] = 0.0
            v.step_tensors(a)
            outs.append(_out(v))
            cnt.append(_points(v))
        runs[name] = (np.stack(outs), np.stack(cnt))
        v.close()
    cnt = runs["merged"][1]
    assert cnt[0][k] >= 3, cnt[0][k]
    others = np.arange(n) != k
    assert any(1 <= c[others].max() <= 2 for c in cnt)
    assert np.array_equal(runs["merged"][0], runs["never"][0])
    assert np.array_equal(runs["merged"][0][:, others], runs["plain"][0][:, others])
