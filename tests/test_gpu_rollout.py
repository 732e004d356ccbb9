"""GPU tests of the device RolloutBuffer (pgx_rollout.hip, panda_gym_amd/rollout.py) against RefRollout,
the numpy restatement of SB3's RolloutBuffer, and ref_permutation, the restatement of the minibatch
order, that tests/test_rollout_abi.py writes from the rules of include/pgx.h and pins by hand.

The bar is bit-exactness everywhere: every stored plane, advantage and return, the carry, gathered
rows and permutations compare through integer views (a NaN is compared as "NaN in the same places":
the payload of a NaN is not part of the rules).  The arithmetic is f32 with every operation rounded on
its own on both sides, so there is no tolerance to choose.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import panda_gym_amd as pg  # noqa: E402
from panda_gym_amd import abi  # noqa: E402
from panda_gym_amd.rollout import terminal_observation  # noqa: E402
from test_rollout_abi import EPOCHS, ERR_INDEX, ERR_NOT_FULL, ERR_OVERFLOW, RefRollout, ref_permutation  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
KEYS = ("observation", "achieved_goal", "desired_goal")
STORED = KEYS + ("action", "reward", "episode_start", "value", "log_prob")
GAE = ("advantage", "return")
GAMMA, LAMBDA = 0.99, 0.95


def assert_same(got, want, what):
    """Bit for bit (floats through their integer views), NaN matching NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = got[~nan].view(np.uint32), want[~nan].view(np.uint32)
    assert np.array_equal(got, want), what


def host(t):
    return t.detach().cpu().numpy().copy()


def snapshot(rb):
    return {k: host(v) for k, v in rb.arrays().items()}


def assert_buffer(rb, ref, what, keys=STORED + GAE):
    a = snapshot(rb)
    for k in keys:
        assert_same(a[k], ref.a[k], f"{what} {k}")
    for k in KEYS:
        assert_same(a["last_" + k], ref.last[k], f"{what} carry {k}")
    assert_same(a["last_episode_start"], ref.last_start, f"{what} carry episode_start")
    rec = a["records"]
    assert not rec[:, :, rb.obs_dim + 6 + rb.action_dim:].any(), f"{what}: record padding is not zero"


# ------------------------------------------------------------------ array level
def make_trace(N, T, od, A, seed, poison=False):
    """Reset observation and T steps of synthetic policy / step outputs.  An env is done with probability
    0.2 per step; a done env is terminated, truncated or both, and every step carries terminal values,
    so timeouts (truncated & ~terminated) are bootstrapped.  ``poison``: env N // 2 gets a NaN value in
    the middle step and an inf reward in the first."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    obs = lambda: {"observation": f(N, od), "achieved_goal": f(N, 3), "desired_goal": f(N, 3)}  # noqa: E731
    steps = []
    for t in range(T):
        done = rng.random(N) < 0.2
        te = done & (rng.random(N) < 0.5)
        tr = done & (~te | (rng.random(N) < 0.3))
        steps.append(dict(action=f(N, A), reward=f(N), value=f(N), log_prob=f(N), obs=obs(),
                          terminated=te.astype(np.uint8), truncated=tr.astype(np.uint8), terminal_value=f(N)))
    if poison:
        steps[T // 2]["value"][N // 2] = np.nan
        steps[0]["reward"][N // 2] = np.inf
    return obs(), steps, f(N), (rng.random(N) < 0.2).astype(F32)


def fill(rb, ref, first, steps):
    rb.set_last(first)
    ref.set_last(first)
    for s in steps:
        rb.add_tensors(**s)
        ref.add(**s)


def make_pair(N, T, od, A, seed=0):
    rb = pg.RolloutBuffer(T, n_envs=N, obs_dim=od, action_dim=A, gamma=GAMMA, gae_lambda=LAMBDA, seed=seed)
    return rb, RefRollout(T, N, od, A, GAMMA, LAMBDA)


SHAPES = [(96, 5, 7, 3), (1, 1, 6, 3), (130, 33, 56, 7)]   # one and a half waves and an odd row; one; > CH steps


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("explicit_dones", [False, True])
def test_arrays_equal_the_restatement(shape, explicit_dones):
    N, T, od, A = shape
    rb, ref = make_pair(N, T, od, A)
    first, steps, last_values, dones = make_trace(N, T, od, A, seed=N + T)
    fill(rb, ref, first, steps)
    assert rb.pos == T and rb.full and rb.size() == T
    assert_buffer(rb, ref, "after the adds", STORED)
    boot = sum(int(((s["truncated"] != 0) & (s["terminated"] == 0)).sum()) for s in steps)
    starts = int(ref.a["episode_start"][1:].sum())
    print(f"{shape}: {boot} bootstrapped timeouts, {starts} episode starts inside the window")
    if N > 1:
        assert boot > 0 and starts > 0   # the trace exercises both
    d = dones if explicit_dones else None
    rb.compute_returns_and_advantage(last_values, d)
    ref.compute_returns_and_advantage(last_values, d)
    assert_buffer(rb, ref, "after GAE")
    rb.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nonfinite_stays_in_its_env(shape):
    N, T, od, A = shape
    rb, ref = make_pair(N, T, od, A)
    first, steps, last_values, _ = make_trace(N, T, od, A, seed=3, poison=True)
    fill(rb, ref, first, steps)
    rb.compute_returns_and_advantage(last_values)
    ref.compute_returns_and_advantage(last_values)
    assert_buffer(rb, ref, "poisoned")
    a = snapshot(rb)
    bad = N // 2
    others = np.arange(N) != bad
    for k in ("reward", "value", "advantage", "return"):
        assert np.isfinite(a[k][:, others]).all(), k
    assert not np.isfinite(a["advantage"][:, bad]).all() and not np.isfinite(a["return"][:, bad]).all()
    rb.close()


# ------------------------------------------------------------------ gather / permutation / get
@pytest.fixture(scope="module")
def filled():
    """(130, 33, 56, 7) and (96, 5, 7, 3), filled and with GAE done, shared by the read-only tests."""
    out = {}
    for shape in ((130, 33, 56, 7), (96, 5, 7, 3)):
        N, T, od, A = shape
        rb, ref = make_pair(N, T, od, A, seed=7)
        first, steps, last_values, _ = make_trace(N, T, od, A, seed=11)
        fill(rb, ref, first, steps)
        rb.compute_returns_and_advantage(last_values)
        ref.compute_returns_and_advantage(last_values)
        out[shape] = (rb, ref)
    yield out
    for rb, _ in out.values():
        rb.close()


def assert_samples(s, ref, idx, what):
    idx = np.asarray(idx)
    for k in KEYS:
        assert_same(host(s.observations[k]), ref.flat(k)[idx], f"{what} {k}")
    for got, k in ((s.actions, "action"), (s.old_values, "value"), (s.old_log_prob, "log_prob"),
                   (s.advantages, "advantage"), (s.returns, "return")):
        assert_same(host(got), ref.flat(k)[idx], f"{what} {k}")


@pytest.mark.parametrize("shape", [(130, 33, 56, 7), (96, 5, 7, 3)], ids=lambda s: "x".join(map(str, s)))
def test_gather_explicit_indices(filled, shape):
    rb, ref = filled[shape]
    M = rb.total
    rng = np.random.default_rng(0)
    cases = {"reversed": np.arange(M)[::-1].copy(), "repeated": np.concatenate([rng.integers(0, M, 77), [5, 5, 5]]),
             "last": np.array([M - 1])}
    for name, idx in cases.items():
        assert_samples(rb.gather(idx), ref, idx, name)
    # p = env * T + step: the row of p is the stored data at (step, env) = (p % T, p // T)
    p = 3 * rb.buffer_size + 2
    s = rb.gather([p])
    assert_same(host(s.observations["observation"])[0], ref.a["observation"][2, 3], "swap_and_flatten order")
    # the row's padding is zero and the views are the documented offsets
    out = rb.alloc_batch(5)
    rb.gather_into(out, torch.arange(5, dtype=torch.int32, device="cuda:0"))
    rows = host(out["rows"])
    assert rows.shape == (5, rb.row_stride) and not rows[:, rb.row_dim:].any()
    assert_same(rows[:, rb.row_dim - 1], ref.flat("return")[:5], "return column")
    rb.raise_device_errors()   # nothing flagged


@pytest.mark.parametrize("N,T", [(1, 1), (2, 1), (1, 5), (96, 5), (241, 17)], ids=lambda x: str(x))
def test_permutation_equals_the_restatement(N, T):
    rb = pg.RolloutBuffer(T, n_envs=N, obs_dim=6, action_dim=3, seed=7 + 2 ** 40)
    M = N * T
    for epoch in EPOCHS:
        got = host(rb.permutation(epoch))
        assert got.dtype == np.int32
        assert np.array_equal(got, ref_permutation(7 + 2 ** 40, epoch, M)), (M, epoch)
        assert np.array_equal(np.sort(got), np.arange(M))
    assert rb.epoch == 0   # an explicit epoch does not count
    rb.close()


def test_get_minibatches(filled):
    rb, ref = filled[(96, 5, 7, 3)]
    M = rb.total
    assert M == 480
    seen = []
    inner = rb.gather_into

    def spy(out, idx):
        seen.append(host(idx))
        return inner(out, idx)

    rb.gather_into = spy
    try:
        for epoch in (rb.epoch, rb.epoch + 1):
            del seen[:]
            batches = list(rb.get(128))
            perm = ref_permutation(7, epoch, M)
            assert [len(b.advantages) for b in batches] == [128, 128, 128, 96]
            assert np.array_equal(np.concatenate(seen), perm), epoch
            for i, b in enumerate(batches):
                assert_samples(b, ref, perm[128 * i:128 * (i + 1)], f"epoch {epoch} batch {i}")
            assert rb.epoch == epoch + 1
        del seen[:]
        whole = list(rb.get())   # batch_size None: the whole buffer
        assert len(whole) == 1 and len(seen) == 1 and np.array_equal(seen[0], ref_permutation(7, rb.epoch - 1, M))
        assert_samples(whole[0], ref, seen[0], "whole buffer")
    finally:
        del rb.gather_into


# ------------------------------------------------------------------ misuse
def test_add_past_full_stores_nothing():
    N, T, od, A = 96, 5, 7, 3
    rb, ref = make_pair(N, T, od, A)
    first, steps, _, _ = make_trace(N, T + 1, od, A, seed=2)
    fill(rb, ref, first, steps[:T])
    before = snapshot(rb)
    rb.add_tensors(**steps[T])
    ref.add(**steps[T])
    after = snapshot(rb)
    for k in before:   # every stored byte, the records' padding and the carry included
        assert np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)), k
    assert rb.pos == T and ref.errors == ERR_OVERFLOW
    with pytest.raises(pg.PgxError, match="PGX_ROLLOUT_ERR_OVERFLOW"):
        rb.raise_device_errors()
    rb.raise_device_errors()   # cleared
    assert_buffer(rb, ref, "after the overflowing add", STORED)
    # reset keeps the carry and the next rollout starts from it
    rb.reset()
    ref.reset()
    assert rb.pos == 0 and not rb.full
    rb.add_tensors(**steps[0])
    ref.add(**steps[0])
    a = snapshot(rb)
    assert_same(a["observation"][0], ref.a["observation"][0], "first slot after reset")
    assert_same(a["episode_start"][0], ref.a["episode_start"][0], "first slot after reset")
    rb.close()


def test_get_and_gae_before_full():
    N, T, od, A = 96, 5, 7, 3
    rb, ref = make_pair(N, T, od, A)
    first, steps, last_values, _ = make_trace(N, T, od, A, seed=2)
    fill(rb, ref, first, steps[:2])
    assert rb.pos == 2 and not rb.full
    with pytest.raises(AssertionError):
        next(rb.get(128))
    before = snapshot(rb)
    with pytest.raises(pg.PgxError, match="PGX_ROLLOUT_ERR_NOT_FULL"):
        rb.compute_returns_and_advantage(last_values)
    after = snapshot(rb)
    for k in GAE:
        assert np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)), k
    ref.compute_returns_and_advantage(last_values)
    assert ref.errors == ERR_NOT_FULL
    rb.close()


def test_index_out_of_range_gives_a_zero_row(filled):
    rb, ref = filled[(96, 5, 7, 3)]
    M = rb.total
    idx = np.array([0, M, -1, 3, 2 ** 31 - 1])
    out = rb.alloc_batch(len(idx))
    out["rows"].fill_(7.0)
    rb.gather_into(out, torch.as_tensor(idx, dtype=torch.int32, device="cuda:0"))
    rows = host(out["rows"])
    assert not rows[[1, 2, 4]].any()
    assert_same(rows[[0, 3], :rb.obs_dim], ref.flat("observation")[[0, 3]], "valid rows beside the bad ones")
    assert_same(rows[[0, 3], rb.row_dim - 2], ref.flat("advantage")[[0, 3]], "valid rows beside the bad ones")
    with pytest.raises(pg.PgxError, match="PGX_ROLLOUT_ERR_INDEX"):
        rb.raise_device_errors()
    rb.raise_device_errors()
    assert abi.ROLLOUT_ERR_INDEX == ERR_INDEX


# ------------------------------------------------------------------ with the env
def value_of(obs):
    """The "critic": a fixed function of the observation (its column sum); log_prob another."""
    v = obs["observation"].sum(dim=1)
    return v, -0.5 * v


def collect(venv, rb, T, ref=None, reset=True, raw_rewards=None):
    """T eager steps with the random policy; ``ref`` is fed host copies of the same step outputs."""
    base = venv.venv if isinstance(venv, pg.VecNormalize) else venv
    if reset:
        obs = venv.reset_tensors(episode_phase="staggered")
        rb.set_last(obs)
        if ref is not None:
            ref.set_last({k: host(obs[k]) for k in KEYS})
    for i in range(T):
        obs = {k: rb.arrays()["last_" + k] for k in KEYS}   # the carry is the observation the policy sees
        value, log_prob = value_of(obs)
        action = base.sample_actions(base._step_index).clone()
        new_obs, reward, te, tr, _ = venv.step_tensors(action)
        tv = value_of(terminal_observation(venv))[0]
        rb.add_from_vec_env(venv, action, value, log_prob, tv)
        if raw_rewards is not None:
            raw_rewards.append(host(base.reward))
        if ref is not None:
            ref.add(host(action), host(reward), host(value), host(log_prob), {k: host(new_obs[k]) for k in KEYS},
                    host(te), host(tr), terminal_value=host(tv))
    last_values = value_of({k: rb.arrays()["last_" + k] for k in KEYS})[0]
    rb.compute_returns_and_advantage(last_values)
    if ref is not None:
        ref.compute_returns_and_advantage(host(last_values))


@pytest.mark.parametrize("env_id,T,normalize", [("PandaReach-v3", 8, False), ("PandaReach-v3", 8, True),
                                                ("PandaReachAO-v3", 4, False)])
def test_rollout_over_the_env(env_id, T, normalize):
    n = 64
    base = pg.PandaVecEnv(env_id, num_envs=n, device="cuda:0", seed=5)
    venv = pg.VecNormalize(base) if normalize else base
    rb = pg.RolloutBuffer(T, env=venv, gamma=GAMMA, gae_lambda=LAMBDA)
    assert (rb.n_envs, rb.obs_dim, rb.action_dim) == (n, base.obs_dim, base.action_dim)
    ref = RefRollout(T, n, base.obs_dim, base.action_dim, GAMMA, LAMBDA)
    raw = []
    collect(venv, rb, T, ref, raw_rewards=raw)
    assert_buffer(rb, ref, env_id)
    a = snapshot(rb)
    assert a["episode_start"][0].all() and a["episode_start"][1:].any(), "time limits fall inside the window"
    assert not a["episode_start"][1:].all()
    if normalize:   # the stored reward is the normalised one
        assert not np.array_equal(a["reward"], np.stack(raw))
        assert np.abs(a["observation"]).max() <= 10.0
    s = next(rb.get(None))
    perm = ref_permutation(0, 0, n * T)
    assert_samples(s, ref, perm, "get over the env")
    venv.close()
    rb.close()


def test_through_monitor_and_normalize():
    """VecMonitor(VecNormalize(env)): the buffer stores what the stack presents (normalised), eagerly and
    behind the monitor's launches in the monitor's captured loop."""
    n, T = 64, 4
    venv = pg.VecMonitor(pg.VecNormalize(pg.PandaVecEnv("PandaReach-v3", num_envs=n, device="cuda:0", seed=5)))
    rb = pg.RolloutBuffer(T, env=venv, gamma=GAMMA, gae_lambda=LAMBDA)
    ref = RefRollout(T, n, venv.obs_dim, venv.action_dim, GAMMA, LAMBDA)
    raw = []
    collect(venv, rb, T, ref, raw_rewards=raw)
    assert_buffer(rb, ref, "monitor over normalize")
    assert not np.array_equal(snapshot(rb)["reward"], np.stack(raw))
    assert venv.totals()["steps"] == T
    g = torch.Generator(device="cuda:0").manual_seed(1)
    actions = torch.rand(T, n, venv.action_dim, device="cuda:0", generator=g) * 2 - 1
    values, log_probs = torch.randn(T, n, device="cuda:0", generator=g), torch.randn(T, n, device="cuda:0", generator=g)
    rb.reset()
    graph = venv.capture_steps(T, actions, after_step=rb.after_step(venv, actions, values, log_probs))
    graph.replay()
    assert rb.pos == T and venv.totals()["steps"] == 2 * T
    a = snapshot(rb)
    assert_same(a["action"], host(actions), "captured actions")
    assert_same(a["value"], host(values), "captured values")
    assert_same(a["last_observation"], host(venv.venv._n["observation"]), "the carry is the normalised observation")
    rb.raise_device_errors()
    venv.close()
    rb.close()


def test_graph_capture_and_replay():
    n, T = 64, 4
    rng = np.random.default_rng(4)
    mk = lambda: pg.PandaVecEnv("PandaReach-v3", num_envs=n, device="cuda:0", seed=9)  # noqa: E731
    dev = lambda x: torch.as_tensor(x, device="cuda:0")  # noqa: E731
    envs = [mk(), mk()]
    A = envs[0].action_dim
    actions = dev(rng.uniform(-1, 1, (T, n, A)).astype(F32))
    values, log_probs, tvs = (dev(rng.standard_normal((T, n)).astype(F32)) for _ in range(3))
    fills = [[], []]
    # eager
    env, rb = envs[0], pg.RolloutBuffer(T, env=envs[0])
    rb.set_last(env.reset_tensors(episode_phase="staggered"))
    for rep in range(2):
        for i in range(T):
            env.step_tensors(actions[i])
            rb.add_from_vec_env(env, actions[i], values[i], log_probs[i], tvs[i])
        assert rb.pos == T
        fills[0].append(snapshot(rb))
        rb.reset()
    rb.close()
    # captured: the same launches in one graph, replayed twice around a reset
    env, rb = envs[1], pg.RolloutBuffer(T, env=envs[1])
    rb.set_last(env.reset_tensors(episode_phase="staggered"))
    g = env.capture_steps(T, actions, after_step=rb.after_step(env, actions, values, log_probs, tvs))
    assert rb.pos == 0   # capture runs nothing
    for rep in range(2):
        g.replay()
        assert rb.pos == T
        fills[1].append(snapshot(rb))
        rb.reset()
    rb.raise_device_errors()
    for rep in range(2):
        for k in fills[0][rep]:
            assert_same(fills[1][rep][k], fills[0][rep][k], f"fill {rep} {k}")
    assert not np.array_equal(fills[0][0]["observation"], fills[0][1]["observation"])   # the env moved on
    rb.close()
    for e in envs:
        e.close()


def test_buffer_has_no_side_effect_on_the_env():
    n, T = 64, 8
    mk = lambda: pg.PandaVecEnv("PandaReach-v3", num_envs=n, device="cuda:0", seed=13)  # noqa: E731
    plain, watched = mk(), mk()
    rb = pg.RolloutBuffer(T, env=watched)
    plain.reset_tensors(episode_phase="staggered")
    rb.set_last(watched.reset_tensors(episode_phase="staggered"))
    for i in range(T):
        action = plain.sample_actions(i).clone()
        outs = []
        for env in (plain, watched):
            o, r, te, tr, su = env.step_tensors(action)
            if env is watched:
                v, lp = value_of(o)
                rb.add_from_vec_env(env, action, v, lp, v)
            outs.append([host(o[k]) for k in KEYS] + [host(r), host(te), host(tr), host(su), host(env.terminal_obs)])
        for x, y in zip(*outs):
            assert_same(y, x, f"step {i}")
    assert rb.pos == T
    rb.close()
    plain.close()
    watched.close()
