"""The arm kernels' two-point instance of the contact substep (substep_g): a wave whose envs hold at
most 2 robot points and no extra points runs a copy of the contact part in which every per-point
object has two entries, so nothing of points 2.. is computed, loaded or stored.  An absent point's
rows are zero rows in the general instance (J = R = 0, lambda = 0, bounds [0, 0]), so the claim is
bit equality with the general instance, which PGX_PGS_MODE=4 ("the general instance, never merged")
keeps in the same library; modes 2 (all rows) and 3 (always redo) take the two-point instance's
all-rows copy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GENERAL = "4"


@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    pg.load_native()
    return pg


def _make(pg, env_id, mode, n, **kw):
    with pytest.MonkeyPatch.context() as mp:   # the hooks are read when the handle is created
        mp.setenv("PGX_PGS_MODE", mode)
        mp.setenv("PGX_SORT_ENVS", "0")        # launch order = env order: envs 4w .. 4w + 3 share wave w
        return pg.PandaVecEnv(env_id, num_envs=n, device="cuda:0", seed=9, lanes_per_env=16, **kw)


def _press(v, t):
    """The pressing-down policy of tests/test_gpu_merged_rows.py: z = -1, x / y random.  Joint control
    has no z: the shoulder joint (dof 1) turns towards the table at full rate, the base joint (dof 0)
    is random (fp64 oracle: the tool reaches the table at step 18, two points per env, idle second
    points among them)."""
    a = torch.zeros((v.num_envs, v.action_dim), device="cuda:0")
    r = v.sample_actions(t)
    if v.action_dim >= 7:
        a[:, 1] = 1.0
        a[:, 0] = r[:, 0]
    else:
        a[:, 2] = -1.0
        a[:, :2] = r[:, :2]
    return a


def _cache(v):
    return v.state()["contacts"].cpu().numpy().copy()


def _points(v, cache):
    from panda_gym_amd import abi

    ids = cache[2 * abi.OBJECT_POINTS::2][:v.robot_contact_budget()]
    return (ids >= 0).sum(0)


def _out(v):
    """(obs | qd, contact cache) of the step just run."""
    o = torch.cat([v.obs, v.state()["qd"].T], 1).cpu().numpy().copy()
    assert np.all(np.isfinite(o))
    return o, _cache(v)


def _pressed_run(pg, env_id, mode, n=256, steps=25):
    v = _make(pg, env_id, mode, n)
    v.reset_tensors(seed=9)
    outs, caches, pts = [], [], []
    for t in range(steps):
        v.step_tensors(_press(v, t))
        o, c = _out(v)
        outs.append(o)
        caches.append(c)
        pts.append(_points(v, c))
    v.close()
    return np.stack(outs), np.stack(caches), np.stack(pts)


def _check_pressing_down(pg, env_id):
    runs = {mode: _pressed_run(pg, env_id, mode) for mode in ("0", "2", "3", GENERAL)}
    pts = runs["0"][2]
    print(env_id, "largest point count per step:", [int(p.max()) for p in pts])
    print(env_id, "one-point envs per step:", [int((p == 1).sum()) for p in pts])
    # the run crosses from the no-point case into the two-point one
    assert int(pts[0].max()) == 0, int(pts[0].max())
    assert any(int(p.max()) == 2 for p in pts), [int(p.max()) for p in pts]
    for mode in ("2", "3", GENERAL):
        for t in range(len(pts)):
            assert np.array_equal(runs["0"][0][t], runs[mode][0][t]), (mode, t, "obs / qd")
            assert np.array_equal(runs["0"][1][t], runs[mode][1][t]), (mode, t, "contact cache")


def test_two_point_instance_is_exact_pressing_down(pg):
    """256 envs pressed onto the table for 25 steps, the cache compared too: no points at first,
    then waves whose largest count is 2 with idle second points among them."""
    _check_pressing_down(pg, "PandaReach-v3")


def test_two_point_instance_is_exact_joint_control(pg):
    """The same run under joint control: the other control mode's kernel."""
    _check_pressing_down(pg, "PandaReachJoints-v3")


@pytest.fixture(scope="module")
def pressed_state(pg):
    """64 envs after 12 pressing-down steps, solved with all rows: the state views on the host."""
    v = _make(pg, "PandaReach-v3", "2", 64)
    v.reset_tensors(seed=9)
    for t in range(12):
        v.step_tensors(_press(v, t))
    st = {k: x.cpu().clone() for k, x in v.state().items() if k != "env_order"}
    pts = _points(v, _cache(v))
    v.close()
    return st, pts


def _from_state(pg, mode, st, **kw):
    n = st["q"].shape[-1]
    v = _make(pg, "PandaReach-v3", mode, n, **kw)
    v.reset_tensors(seed=9)
    dst = v.state()
    for k in ("q", "qd", "qc", "goal", "object", "contacts", "elapsed", "episode"):
        dst[k].copy_(st[k].to(dst[k].device))
    return v


@pytest.mark.parametrize("substeps", [1, None], ids=["one-substep", "default-substeps"])
def test_heavy_env_among_two_point_waves(pg, pressed_state, substeps):
    """One env forced to the hand-and-finger-on-the-table pose (5 points): its wave takes the general
    instance, its neighbours the two-point one.  Bit-identical to the general instance everywhere,
    and every other env to a run without the pose change."""
    from panda_gym_amd import abi
    from test_oracle_contacts import TWO_LINKS_ON_TABLE_REL_Q

    k = 21
    st0, pts = pressed_state
    assert np.any((pts >= 1) & (pts <= 2))
    st = {x: y.clone() for x, y in st0.items()}
    q = torch.tensor(TWO_LINKS_ON_TABLE_REL_Q, dtype=torch.float32)
    st["q"][:, k] = q
    st["qc"][:, k] = q
    st["qd"][:, k] = 0.0
    st["contacts"][2 * abi.OBJECT_POINTS::2, k] = -1.0
    st["contacts"][2 * abi.OBJECT_POINTS + 1::2, k] = 0.0
    kw = {} if substeps is None else {"n_substeps": substeps}
    runs = {}
    for name, mode, s in (("default", "0", st), ("general", GENERAL, st), ("plain", "0", st0)):
        v = _from_state(pg, mode, s, **kw)
        outs, caches, cnt = [], [], []
        for t in range(5):
            a = _press(v, 12 + t)
            a[k] = 0.0
            v.step_tensors(a)
            o, c = _out(v)
            outs.append(o)
            caches.append(c)
            cnt.append(_points(v, c))
        runs[name] = (np.stack(outs), np.stack(caches), np.stack(cnt))
        v.close()
    cnt = runs["default"][2]
    others = np.arange(st["q"].shape[-1]) != k
    print("posed env's points per step:", [int(c[k]) for c in cnt], "others' largest:", [int(c[others].max()) for c in cnt])
    if substeps == 1:   # the cache after a step shows the points of the one substep that ran
        assert cnt[0][k] >= 3, cnt[0][k]
    assert any(1 <= c[others].max() <= 2 for c in cnt)
    assert np.array_equal(runs["default"][0], runs["general"][0])
    assert np.array_equal(runs["default"][1], runs["general"][1])
    assert np.array_equal(runs["default"][0][:, others], runs["plain"][0][:, others])
    assert np.array_equal(runs["default"][1][..., others], runs["plain"][1][..., others])
