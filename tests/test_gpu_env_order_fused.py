"""GPU: the heavy-first env order derived inside the step kernel (the previous step's key bytes,
order_env in pgx_kernels.hip) against the sort kernel's.  Every case steps two
handles of one process with the same actions, both with the order forced on (PGX_SORT_ENVS=1): one
derives the order in the step kernel's prologue, the other (PGX_SORT_FUSED=0) launches
env_sort_segment_kernel before every step.  The order of every launch, the state and the outputs
are the same bits; after a restore or a reset the next step sorts from the state as it stands; a
captured step loop replays to the eager steps' bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STATE = ("q", "qd", "qc", "goal", "object", "contacts", "obstacles", "manifolds", "elapsed", "episode")
OUT = ("obs", "achieved_goal", "desired_goal", "reward", "success", "terminated", "truncated", "terminal_obs",
       "terminal_ag", "terminal_dg", "task_trunc", "nonfinite_t")


@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    pg.load_native()
    return pg


def _pair(pg, monkeypatch, env_id, n, seed=5, **kw):
    """(fused, sorted by the kernel): the hooks are read when the handle is created."""
    monkeypatch.setenv("PGX_SORT_ENVS", "1")
    monkeypatch.setenv("PGX_SORT_FUSED", "1")
    a = pg.PandaVecEnv(env_id, num_envs=n, device="cuda:0", seed=seed, **kw)
    monkeypatch.setenv("PGX_SORT_FUSED", "0")
    b = pg.PandaVecEnv(env_id, num_envs=n, device="cuda:0", seed=seed, **kw)
    a.reset_tensors(seed=seed)
    b.reset_tensors(seed=seed)
    return a, b


def _keys(v):
    """The sort key of every env as the state stands: the robot slots its cache row holds."""
    c = v.state()["contacts"].cpu().numpy()
    return (c[8:8 + 2 * 12:2] >= 0).sum(0)


def _heavy_first(keys, segs):
    S = len(keys) // segs
    return np.concatenate([x * S + np.argsort(-keys[x * S:(x + 1) * S], kind="stable") for x in range(segs)])


def _same_bits(a, b, what):
    sa, sb = a.state(), b.state()
    for k in STATE:
        if k in sa:
            assert np.array_equal(sa[k].cpu().numpy().view(np.uint8), sb[k].cpu().numpy().view(np.uint8)), (what, k)
    for k in OUT:
        assert np.array_equal(getattr(a, k).cpu().numpy().view(np.uint8),
                              getattr(b, k).cpu().numpy().view(np.uint8)), (what, k)


CASES = [("PandaReach-v3", 130, None, {}),            # ragged, one segment
         ("PandaReach-v3", 1024, None, {}),           # a full 1024-env segment: 16 keys in every lane
         ("PandaReach-v3", 2048, None, {}),           # eight per-XCD segments of 256
         ("PandaReach-v3", 130, "2", {}),             # the two-wave build
         ("PandaPush-v3", 67, None, {}),
         ("PandaReachAO-v3", 130, None, {}),
         ("PandaReachAO-v3", 130, None, {"nonfinite": "reset"})]


@pytest.mark.parametrize("env_id,n,waves,kw", CASES)
def test_same_order_same_bits(pg, monkeypatch, env_id, n, waves, kw):
    if waves:
        monkeypatch.setenv("PGX_WAVES_PER_SIMD", waves)
    a, b = _pair(pg, monkeypatch, env_id, n, **kw)
    segs = 8 if n % 2048 == 0 else 1
    S = n // segs
    try:
        moved, heavy = 0, 0
        for t in range(40):
            keys0 = _keys(a)
            acts = a.sample_actions(t).clone()
            a.step_tensors(acts)
            b.step_tensors(acts)
            pa, pb = a.state()["env_order"].cpu().numpy(), b.state()["env_order"].cpu().numpy()
            assert np.array_equal(pa, pb), t
            for x in range(segs):   # a permutation, segment by segment
                assert np.array_equal(np.sort(pa[x * S:(x + 1) * S]), np.arange(x * S, (x + 1) * S)), (t, x)
            assert np.array_equal(pa, _heavy_first(keys0, segs)), t
            _same_bits(a, b, t)
            moved += int((pa != np.arange(n)).any())
            heavy = max(heavy, int(_keys(a).max()))
        assert heavy >= 1   # some env held robot points
        assert moved >= 1   # and some launch read its envs in an order other than the identity
    finally:
        a.close()
        b.close()


def test_a_restore_and_a_reset_sort_from_the_state_as_it_stands(pg, monkeypatch):
    a, b = _pair(pg, monkeypatch, "PandaReach-v3", 130)
    try:
        def step(t):
            acts = a.sample_actions(t).clone()
            a.step_tensors(acts)
            b.step_tensors(acts)

        for t in range(20):
            step(t)
        sid_a, sid_b = a.save_state(), b.save_state()
        for t in range(20, 25):
            step(t)
        a.restore_state(sid_a)
        b.restore_state(sid_b)
        keys0 = _keys(a)
        step(25)
        order = a.state()["env_order"].cpu().numpy()
        assert np.array_equal(order, _heavy_first(keys0, 1))
        assert np.array_equal(order, b.state()["env_order"].cpu().numpy())
        _same_bits(a, b, "restore")
        for t in range(26, 36):
            step(t)
        mask = torch.zeros(130, dtype=torch.bool, device="cuda:0")
        mask[::3] = True
        a.reset_tensors(seed=11, mask=mask)
        b.reset_tensors(seed=11, mask=mask)
        keys0 = _keys(a)
        step(36)
        order = a.state()["env_order"].cpu().numpy()
        assert np.array_equal(order, _heavy_first(keys0, 1))
        assert np.array_equal(order, b.state()["env_order"].cpu().numpy())
        _same_bits(a, b, "reset")
    finally:
        a.close()
        b.close()


def test_the_step_kernel_reads_the_keys_of_the_last_step(pg, monkeypatch):
    """pgx.h: a caller that writes `contacts` through the state view gets an order one step stale
    from the fused path (the keys are the last step's epilogue's), the right one from the sort
    kernel -- and the same results from both, whatever the order.  (That the two differ here is
    what shows the fused handle took the fused path.)"""
    a, b = _pair(pg, monkeypatch, "PandaReach-v3", 130)
    try:
        for t in range(3):
            acts = a.sample_actions(t).clone()
            a.step_tensors(acts)
            b.step_tensors(acts)
        keys_last = _keys(a)
        j = 129 - int(np.argmin(keys_last[::-1]))   # the last of the lightest envs: one more point moves it up
        for v in (a, b):   # its first robot slot now holds a (cold) point
            v.state()["contacts"][8, j] = 0.0
        keys_now = _keys(a)
        assert not np.array_equal(_heavy_first(keys_now, 1), _heavy_first(keys_last, 1))
        acts = a.sample_actions(3).clone()
        a.step_tensors(acts)
        b.step_tensors(acts)
        assert np.array_equal(a.state()["env_order"].cpu().numpy(), _heavy_first(keys_last, 1))
        assert np.array_equal(b.state()["env_order"].cpu().numpy(), _heavy_first(keys_now, 1))
        _same_bits(a, b, "view write")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("env_id", ["PandaReach-v3", "PandaReachAO-v3"])
def test_captured_steps_equal_eager_steps(pg, monkeypatch, env_id):
    n, k = 96, 5   # (an odd count: a replay's first launch reads keys one step stale -- still a bijection)
    graphed, eager = _pair(pg, monkeypatch, env_id, n, seed=9)
    try:
        for t in range(3):
            acts = eager.sample_actions(t).clone()
            eager.step_tensors(acts)
            graphed.step_tensors(acts)
        acts = torch.empty((k, n, eager.action_dim), device="cuda:0")
        g = graphed.capture_steps(k, acts)
        for rep in range(2):
            for i in range(k):
                acts[i].copy_(eager.sample_actions(100 * rep + i))
            for i in range(k):
                eager.step_tensors(acts[i])
            g.replay()
            torch.cuda.synchronize()
            _same_bits(graphed, eager, rep)
            assert np.array_equal(np.sort(graphed.state()["env_order"].cpu().numpy()), np.arange(n)), rep
    finally:
        graphed.close()
        eager.close()
