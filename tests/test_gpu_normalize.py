"""GPU tests of the device VecNormalize (pgx_norm.hip, panda_gym_amd/normalize.py) against a numpy
fp64 restatement of SB3's VecNormalize / RunningMeanStd written here from the rules of include/pgx.h.

Bars.  Statistics (mean, var, count, returns) against the restatement's own: rtol 1e-9 (var: plus
atol 1e-9 * var_ref) -- fp64 summation in another order differs by about T * N * 2^-53 ~ 3e-12 of a
column's scale at these shapes, two orders inside the bar, while a sum-of-squares variance misses
it by orders on the offset column; count exact; returns bit-exact.  Outputs (normalised
observations, terminal rows of done envs, rewards): bit-exact against the restatement evaluated
with the device's own statistics, and within 1 f32 ulp of the restatement run on its own.
Measured on an MI355X over every test here: statistics within 6.4e-13 (mean) and 5.2e-15 (var)
relative of the restatement's.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import panda_gym_amd.normalize as NZ  # noqa: E402
from panda_gym_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("observation", "achieved_goal", "desired_goal")
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------ restatement
class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean, self.var, self.count = np.zeros(shape, F64), np.ones(shape, F64), 1e-4

    def update(self, batch):
        x = np.asarray(batch).astype(np.float64)
        batch_mean, batch_var, n = np.mean(x, axis=0), np.var(x, axis=0), x.shape[0]
        delta = batch_mean - self.mean
        tot = self.count + n
        new_mean = self.mean + delta * n / tot
        m2 = self.var * self.count + batch_var * n + np.square(delta) * self.count * n / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


class RefNorm:
    """VecNormalize in numpy.  `stats` (mean, var [obs_dim + 7], the returns column last) replaces the
    restatement's own statistics in the output expressions where given."""

    def __init__(self, n, od, keys=KEYS, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, eps=1e-8):
        self.n, self.od, self.keys, self.norm_reward = n, od, tuple(keys), norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.eps = clip_obs, clip_reward, gamma, eps
        self.width = {"observation": od, "achieved_goal": 3, "desired_goal": 3}
        self.base = {"observation": 0, "achieved_goal": od, "desired_goal": od + 3}
        self.rms = {k: RunningMeanStd((self.width[k],)) for k in KEYS}
        self.ret = RunningMeanStd(())
        self.returns = np.zeros(n, F64)
        self.training = True

    def stats(self):
        mean = np.concatenate([self.rms[k].mean for k in KEYS] + [[self.ret.mean]])
        var = np.concatenate([self.rms[k].var for k in KEYS] + [[self.ret.var]])
        count = np.concatenate([np.full(self.width[k], self.rms[k].count) for k in KEYS] + [[self.ret.count]])
        return mean, var, count

    def _mv(self, stats):
        m, v, _ = self.stats()
        return (m, v) if stats is None else (np.asarray(stats[0]), np.asarray(stats[1]))

    def norm_obs(self, key, x, stats=None):
        if key not in self.keys:
            return np.array(x, dtype=F32, copy=True)
        m, v = self._mv(stats)
        s = slice(self.base[key], self.base[key] + self.width[key])
        return np.clip((x.astype(F64) - m[s]) / np.sqrt(v[s] + self.eps), -self.clip_obs, self.clip_obs).astype(F32)

    def norm_reward_(self, r, stats=None):
        if not self.norm_reward:
            return np.array(r, dtype=F32, copy=True)
        _, v = self._mv(stats)
        return np.clip(r.astype(F64) / np.sqrt(v[-1] + self.eps), -self.clip_reward, self.clip_reward).astype(F32)

    def reset(self, obs):
        self.returns = np.zeros(self.n, F64)
        if self.training:
            for k in self.keys:
                self.rms[k].update(obs[k])

    def step(self, obs, reward, done):
        if self.training:
            for k in self.keys:
                self.rms[k].update(obs[k])
        self.returns = self.returns * self.gamma + reward.astype(F64)
        if self.training:
            self.ret.update(self.returns)
        self.returns[done] = 0.0

    def outputs(self, obs, reward, terminal, stats=None):
        out = {k: self.norm_obs(k, obs[k], stats) for k in KEYS}
        if reward is not None:
            out["reward"] = self.norm_reward_(reward, stats)
        if terminal is not None:
            for k, t in zip(KEYS, ("terminal_obs", "terminal_ag", "terminal_dg")):
                out[t] = self.norm_obs(k, terminal[k], stats)
        return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    assert np.array_equal(bits(got), bits(want)), what


def assert_one_ulp(got, want, what):
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    tol = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(F32))
    assert (np.abs(got.astype(F64) - want.astype(F64)) <= tol.astype(F64)).all(), what


def assert_stats(dev, ref, what):
    """dev: (mean, var, count, returns) of pgx_norm_get_stats; ref: the RefNorm."""
    mean, var, count, ret = dev
    rm, rv, rc = ref.stats()
    for a in (mean, var, count, ret, rm, rv, rc, ref.returns):
        assert np.isfinite(a).all(), what
    print(f"{what}: max rel mean {np.max(np.abs(mean - rm) / np.maximum(np.abs(rm), 1e-300)):.3e} "
          f"max rel var {np.max(np.abs(var - rv) / rv):.3e}")
    np.testing.assert_allclose(mean, rm, rtol=1e-9, atol=0, err_msg=what)
    assert (np.abs(var - rv) <= 1e-9 * rv + 1e-9 * np.abs(rv)).all(), what
    assert np.array_equal(count, rc), what
    assert_bits(ret, ref.returns, what + " returns")


def compare_outputs(out, ref, obs, reward, terminal, done, dev_stats, what):
    """out: dict of numpy outputs of the device; bit-exact with the device's statistics, 1 ulp with
    the restatement's own; terminal rows only where done."""
    for stats, check in ((dev_stats[:2], assert_bits), (None, assert_one_ulp)):
        want = ref.outputs(obs, reward, terminal, stats)
        for k, w in want.items():
            g = out[k]
            if k.startswith("terminal"):
                g, w = g[done], w[done]
            check(g, w, f"{what} {k}")


def synth(rng, n, od):
    """One step of synthetic data: standard normal f32, observation column 1 offset to mean 1e3 with
    standard deviation 1e-3, column 2 constant, rewards from {-1, 0, -101}, done with probability 0.1."""
    f = lambda *s: rng.standard_normal((n,) + s).astype(F32)  # noqa: E731
    obs = {"observation": f(od), "achieved_goal": f(3), "desired_goal": f(3)}
    term = {"observation": f(od), "achieved_goal": f(3), "desired_goal": f(3)}
    for d in (obs, term):
        d["observation"][:, 1] = (1e3 + 1e-3 * rng.standard_normal(n)).astype(F32)
        d["observation"][:, 2] = F32(0.7)
    reward = rng.choice(np.array([-1.0, 0.0, -101.0], dtype=F32), size=n)
    done = rng.random(n) < 0.1
    terminated = (done & (rng.random(n) < 0.5)).astype(np.uint8)
    truncated = (done & (terminated == 0)).astype(np.uint8)
    return obs, term, reward, done, terminated, truncated


def dev_step(nz, obs, term, reward, terminated, truncated, out=None):
    o = nz.step_arrays(obs["observation"], obs["achieved_goal"], obs["desired_goal"], reward, terminated, truncated,
                       term["observation"], term["achieved_goal"], term["desired_goal"], out=out)
    return {k: v.cpu().numpy() for k, v in o.items()}


# ------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("od", [6, 19, 56])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_statistics_and_outputs_vs_restatement(n, od):
    """30 updates (a reset, then 29 steps) of synthetic data: one lane, a ragged wave, and more than
    one 256-env slab with a ragged tail; the 12-, 25- and 62-column layouts."""
    rng = np.random.default_rng(1000 * n + od)
    nz = NZ.Normalizer(n, od, device="cuda:0")
    ref = RefNorm(n, od)
    obs = synth(rng, n, od)[0]
    o = nz.reset_arrays(obs["observation"], obs["achieved_goal"], obs["desired_goal"])
    ref.reset(obs)
    st = nz.get_stats()
    assert_stats(st, ref, f"reset n={n} od={od}")
    compare_outputs({k: v.cpu().numpy() for k, v in o.items() if k in KEYS}, ref, obs, None, None, None, st, "reset")
    out = nz.alloc_outputs()
    for t in range(29):
        obs, term, reward, done, terminated, truncated = synth(rng, n, od)
        got = dev_step(nz, obs, term, reward, terminated, truncated, out)
        ref.step(obs, reward, done)
        st = nz.get_stats()
        assert_stats(st, ref, f"step {t} n={n} od={od}")
        compare_outputs(got, ref, obs, reward, term, done, st, f"step {t} n={n} od={od}")
    assert ref.ret.count == pytest.approx(1e-4 + 29 * n) and st[2][0] == pytest.approx(1e-4 + 30 * n)
    nz.close()


def _run_sequence(n, od, steps, seed, **kw):
    rng = np.random.default_rng(seed)
    nz = NZ.Normalizer(n, od, device="cuda:0", **kw)
    outs = []
    for t in range(steps):
        obs, term, reward, done, terminated, truncated = synth(rng, n, od)
        outs.append(dev_step(nz, obs, term, reward, terminated, truncated))
    st = nz.get_stats()
    nz.close()
    return st, outs


def test_same_sequence_twice_gives_identical_bits():
    a, oa = _run_sequence(1000, 19, 10, 5)
    b, ob = _run_sequence(1000, 19, 10, 5)
    for x, y, name in zip(a, b, ("mean", "var", "count", "returns")):
        assert_bits(x, y, name)
    for x, y in zip(oa, ob):
        for k in x:
            assert np.array_equal(bits(x[k]), bits(y[k])), k


def test_training_off_freezes_statistics():
    n, od = 257, 6
    rng = np.random.default_rng(2)
    nz = NZ.Normalizer(n, od, device="cuda:0")
    ref = RefNorm(n, od)
    for t in range(3):
        obs, term, reward, done, terminated, truncated = synth(rng, n, od)
        dev_step(nz, obs, term, reward, terminated, truncated)
        ref.step(obs, reward, done)
    before = nz.get_stats()
    nz.set_training(False)
    ref.training = False
    for t in range(5):
        obs, term, reward, done, terminated, truncated = synth(rng, n, od)
        got = dev_step(nz, obs, term, reward, terminated, truncated)
        ref.step(obs, reward, done)
        st = nz.get_stats()
        for x, y, name in zip(before[:3], st[:3], ("mean", "var", "count")):
            assert_bits(y, x, f"frozen {name}")
        assert_bits(st[3], ref.returns, "returns go on")
        compare_outputs(got, ref, obs, reward, term, done, st, f"frozen step {t}")
    nz.set_training(True)
    ref.training = True
    obs, term, reward, done, terminated, truncated = synth(rng, n, od)
    dev_step(nz, obs, term, reward, terminated, truncated)
    ref.step(obs, reward, done)
    assert_stats(nz.get_stats(), ref, "training on again")
    nz.close()


@pytest.mark.parametrize("case", ["no_reward", "observation_only", "no_obs", "tight_clips"])
def test_settings(case):
    n, od = 63, 19
    kw = {"no_reward": dict(norm_reward=False), "observation_only": dict(keys=abi.NORM_KEY_BITS["observation"]),
          "no_obs": dict(keys=0), "tight_clips": dict(clip_obs=0.5, clip_reward=0.25)}[case]
    rkw = {"no_reward": dict(norm_reward=False), "observation_only": dict(keys=("observation",)),
           "no_obs": dict(keys=()), "tight_clips": dict(clip_obs=0.5, clip_reward=0.25)}[case]
    rng = np.random.default_rng(11)
    nz = NZ.Normalizer(n, od, device="cuda:0", **kw)
    ref = RefNorm(n, od, **rkw)
    for t in range(4):
        obs, term, reward, done, terminated, truncated = synth(rng, n, od)
        got = dev_step(nz, obs, term, reward, terminated, truncated)
        ref.step(obs, reward, done)
        st = nz.get_stats()
        assert_stats(st, ref, f"{case} step {t}")
        compare_outputs(got, ref, obs, reward, term, done, st, f"{case} step {t}")
        if case == "no_reward":
            assert_bits(got["reward"], reward, "raw reward")
        if case in ("observation_only", "no_obs"):   # goals raw, their statistics untouched
            assert_bits(got["achieved_goal"], obs["achieved_goal"], "raw achieved_goal")
            assert_bits(got["desired_goal"], obs["desired_goal"], "raw desired_goal")
            assert_bits(got["terminal_dg"][done], term["desired_goal"][done], "raw terminal desired_goal")
            assert (st[2][od:od + 6] == 1e-4).all() and (st[0][od:od + 6] == 0).all()
        if case == "no_obs":
            assert_bits(got["observation"], obs["observation"], "raw observation")
        if case == "tight_clips":
            assert np.abs(got["observation"]).max() == F32(0.5) and np.abs(got["reward"]).max() == F32(0.25)
    nz.close()


def test_set_stats_get_stats_round_trip_and_apply():
    n, od = 63, 6
    rng = np.random.default_rng(4)
    nz = NZ.Normalizer(n, od, device="cuda:0")
    S = od + 7
    mean, var, count = rng.standard_normal(S), rng.random(S) + 0.1, np.full(S, 1234.5)
    ret = rng.standard_normal(n)
    nz.set_stats(mean, var, count, ret)
    got = nz.get_stats()
    for x, y, name in zip(got, (mean, var, count, ret), ("mean", "var", "count", "returns")):
        assert_bits(x, y, name)
    ref = RefNorm(n, od)
    x = rng.standard_normal((5, 7, od)).astype(F32) * 3
    y = nz.apply(0, torch.as_tensor(x)).cpu().numpy()
    assert_bits(y.reshape(-1, od), ref.norm_obs("observation", x.reshape(-1, od), (mean, var)), "apply observation")
    g = rng.standard_normal((9, 3)).astype(F32)
    assert_bits(nz.apply(2, torch.as_tensor(g)).cpu().numpy(), ref.norm_obs("desired_goal", g, (mean, var)), "apply dg")
    inv = nz.apply(1, torch.as_tensor(g), inverse=True).cpu().numpy()
    assert_bits(inv, (g.astype(F64) * np.sqrt(var[od:od + 3] + 1e-8) + mean[od:od + 3]).astype(F32), "inverse ag")
    r = np.array([-1.0, -0.0, 0.0, -101.0, 2.5], dtype=F32)
    assert_bits(nz.apply(3, torch.as_tensor(r)).cpu().numpy(), ref.norm_reward_(r, (mean, var)), "apply reward")
    assert_bits(nz.apply(3, torch.as_tensor(r), inverse=True).cpu().numpy(),
                (r.astype(F64) * np.sqrt(var[-1] + 1e-8)).astype(F32), "inverse reward")
    with pytest.raises(Exception):
        nz.set_stats(mean, -var, count)
    nz.close()


# ------------------------------------------------------------------ integration
@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    return pg


def _raw(env):
    torch.cuda.synchronize()
    obs = {k: v.cpu().numpy().copy() for k, v in env._obs_dict().items()}
    term = {"observation": env.terminal_obs.cpu().numpy().copy(), "achieved_goal": env.terminal_ag.cpu().numpy().copy(),
            "desired_goal": env.terminal_dg.cpu().numpy().copy()}
    return obs, term, env.reward.cpu().numpy().copy(), env.terminated.cpu().numpy() != 0, \
        env.truncated.cpu().numpy() != 0, env.success.cpu().numpy() != 0


def _tensor_path(pg, env_id, n, steps, **wkw):
    """The wrapped env's tensor path against the restatement fed the raw outputs of a bare env with
    the same seed and actions; the raw trajectory itself bit for bit the bare env's."""
    kw = dict(num_envs=n, device="cuda:0", seed=3)
    bare, inner = pg.PandaVecEnv(env_id, **kw), pg.PandaVecEnv(env_id, **kw)
    w = pg.VecNormalize(inner, **wkw)
    ref = RefNorm(n, bare.obs_dim)
    assert w.num_envs == n and w.obs_dim == bare.obs_dim and w.action_dim == bare.action_dim   # forwarded
    bare.reset_tensors()
    o = w.reset_tensors()
    obs = _raw(bare)[0]
    ref.reset(obs)
    st = w.get_stats()
    assert_stats(st, ref, f"{env_id} reset")
    compare_outputs({k: v.cpu().numpy() for k, v in o.items()}, ref, obs, None, None, None, st, f"{env_id} reset")
    dones = 0
    for t in range(steps):
        a = bare.sample_actions(t).clone()
        bare.step_tensors(a)
        o, r, te, tr, su = w.step_tensors(a)
        obs, term, reward, terminated, truncated, success = _raw(bare)
        for k in KEYS:   # the raw trajectory is unchanged by the wrapper
            assert_bits(w.get_original_obs()[k], obs[k], f"raw {k} step {t}")
            assert torch.equal(w.get_original_obs(tensors=True)[k], inner._obs_dict()[k])
        assert_bits(w.get_original_reward(), reward, "raw reward")
        assert np.array_equal(te.cpu().numpy() != 0, terminated) and np.array_equal(tr.cpu().numpy() != 0, truncated)
        assert np.array_equal(su.cpu().numpy() != 0, success)
        done = terminated | truncated
        dones += int(done.sum())
        ref.step(obs, reward, done)
        st = w.get_stats()
        assert_stats(st, ref, f"{env_id} step {t}")
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["reward"] = r.cpu().numpy()
        got.update({k: w._n[k].cpu().numpy() for k in ("terminal_obs", "terminal_ag", "terminal_dg")})
        compare_outputs(got, ref, obs, reward, term, done, st, f"{env_id} step {t}")
    assert_bits(w.returns, ref.returns, "returns")
    rms = w.obs_rms
    assert set(rms) == set(KEYS) and rms["observation"].mean.shape == (bare.obs_dim,)
    assert rms["desired_goal"].count == ref.rms["desired_goal"].count and w.ret_rms.count == ref.ret.count
    bare.close()
    return w, dones


def test_reach_tensor_path(pg):
    w, dones = _tensor_path(pg, "PandaReach-v3", 64, 60)
    assert dones >= 64   # the 50-step limit fired: terminal rows were compared
    with pytest.raises(ValueError, match="mask"):
        w.reset_tensors(mask=torch.ones(64, dtype=torch.uint8, device="cuda:0"))
    lo = w.observation_space["observation"]
    assert lo.shape == (6,) and float(lo.high[0]) == 10.0 and float(lo.low[0]) == -10.0
    w.close()


@pytest.mark.parametrize("env_id,od", [("PandaPickAndPlace-v3", 19), ("PandaReachAO-v3", 56)])
def test_other_tasks_tensor_path(pg, env_id, od):
    w, _ = _tensor_path(pg, env_id, 32, 5)
    assert w.obs_dim == od
    w.close()


def test_reach_sb3_path(pg):
    """step_wait: normalised numpy observations / rewards, normalised terminal_observation, the
    other info fields passed through -- against the restatement fed a bare env's step_wait."""
    n = 64
    kw = dict(num_envs=n, device="cuda:0", seed=5)
    bare, inner = pg.PandaVecEnv("PandaReach-v3", **kw), pg.PandaVecEnv("PandaReach-v3", **kw)
    w = pg.VecNormalize(inner)
    ref = RefNorm(n, 6)
    bare.seed(5)
    w.seed(5)
    obs = bare.reset()
    o = w.reset()
    ref.reset(obs)
    st = w.get_stats()
    compare_outputs(o, ref, obs, None, None, None, st, "sb3 reset")
    rng = np.random.default_rng(0)
    n_term = 0
    for t in range(60):
        a = rng.uniform(-1, 1, (n, 3)).astype(F32)
        obs, reward, done, infos = bare.step(a)
        o, r, d, winfos = w.step(a)
        assert np.array_equal(d, done)
        ref.step(obs, reward, done)
        st = w.get_stats()
        assert_stats(st, ref, f"sb3 step {t}")
        compare_outputs(dict(o, reward=r), ref, obs, reward, None, done, st, f"sb3 step {t}")
        for k in KEYS:
            assert_bits(w.get_original_obs()[k], obs[k], f"sb3 raw {k}")
        assert_bits(w.get_original_reward(), reward, "sb3 raw reward")
        for i in range(n):
            a_i, b_i = dict(infos[i]), dict(winfos[i])
            ta, tb = a_i.pop("terminal_observation", None), b_i.pop("terminal_observation", None)
            assert a_i == b_i, (t, i)
            assert (ta is None) == (tb is None) == (not done[i])
            if ta is not None:
                n_term += 1
                for k in KEYS:
                    assert_bits(tb[k], ref.norm_obs(k, ta[k][None], st[:2])[0], f"terminal {k}")
    assert n_term >= n
    # normalize_obs / unnormalize_obs / rewards: numpy in, numpy out; tensors in, tensors out
    no = w.normalize_obs(obs)
    for k in KEYS:
        assert isinstance(no[k], np.ndarray)
        assert_bits(no[k], ref.norm_obs(k, obs[k], st[:2]), f"normalize_obs {k}")
    assert_bits(w.normalize_reward(reward), ref.norm_reward_(reward, st[:2]), "normalize_reward")
    back = w.unnormalize_obs({k: torch.as_tensor(v, device="cuda:0") for k, v in no.items()})
    assert torch.is_tensor(back["observation"])
    unclipped = np.abs(no["observation"]) < 10
    assert np.allclose(back["observation"].cpu().numpy()[unclipped], obs["observation"][unclipped], rtol=1e-5, atol=1e-6)
    ur = w.unnormalize_reward(w.normalize_reward(reward))
    assert np.allclose(ur[np.abs(w.normalize_reward(reward)) < 10], reward[np.abs(w.normalize_reward(reward)) < 10],
                       rtol=1e-5)
    bare.close()
    w.close()


def test_save_load_reproduces_next_step(pg, tmp_path):
    n = 64
    kw = dict(num_envs=n, device="cuda:0", seed=8)
    a_env, b_env = pg.PandaVecEnv("PandaReach-v3", **kw), pg.PandaVecEnv("PandaReach-v3", **kw)
    wa = pg.VecNormalize(a_env, clip_obs=5.0, gamma=0.95, norm_obs_keys=["observation", "desired_goal"])
    wa.reset_tensors(seed=8)
    b_env.reset_tensors(seed=8)
    for t in range(4):
        act = a_env.sample_actions(t).clone()
        wa.step_tensors(act)
        b_env.step_tensors(act)
    path = str(tmp_path / "vecnormalize.npz")
    wa.save(path)
    with np.load(path, allow_pickle=False) as z:   # a plain npz: loads without pickle
        assert {"mean", "var", "count", "returns", "gamma", "norm_obs_keys"} <= set(z.files)
    wb = pg.VecNormalize.load(path, b_env)
    assert wb.clip_obs == 5.0 and wb.gamma == 0.95 and wb.norm_obs_keys == ["observation", "desired_goal"]
    for x, y, name in zip(wa.get_stats(), wb.get_stats(), ("mean", "var", "count", "returns")):
        assert_bits(x, y, name)
    act = a_env.sample_actions(4).clone()
    oa, ra = wa.step_tensors(act)[:2]
    ob, rb = wb.step_tensors(act)[:2]
    torch.cuda.synchronize()
    for k in KEYS:
        assert_bits(oa[k].cpu().numpy(), ob[k].cpu().numpy(), k)
    assert_bits(ra.cpu().numpy(), rb.cpu().numpy(), "reward")
    assert_bits(oa["achieved_goal"].cpu().numpy(), a_env.achieved_goal.cpu().numpy(), "achieved_goal stays raw")
    for x, y, name in zip(wa.get_stats(), wb.get_stats(), ("mean", "var", "count", "returns")):
        assert_bits(x, y, name)
    # the assignable switches
    assert float(wa.observation_space["observation"].high[0]) == 5.0
    assert float(wa.observation_space["achieved_goal"].high[0]) == 10.0   # not normalised: the env's own bound
    wa.training = False
    before = wa.get_stats()
    wa.step_tensors(act)
    for x, y in zip(before[:3], wa.get_stats()[:3]):
        assert_bits(y, x, "training = False")
    wa.norm_reward = False
    _, r = wa.step_tensors(act)[:2]
    assert torch.equal(r, a_env.reward)
    wa.norm_obs = False
    o = wa.step_tensors(act)[0]
    assert torch.equal(o["observation"], a_env.obs) and float(wa.observation_space["observation"].high[0]) == 10.0
    wa.close()
    wb.close()


@pytest.mark.parametrize("k,replays", [(3, 2), (1, 4)])
def test_captured_steps_equal_eager_steps(pg, k, replays):
    """capture_steps(k) replayed `replays` times == k * replays eager steps with the same actions, bit
    for bit (statistics and outputs); k = 1 is the odd length a parity scheme could get wrong."""
    n = 64
    kw = dict(num_envs=n, device="cuda:0", seed=9, max_episode_steps=4)
    eager = pg.VecNormalize(pg.PandaVecEnv("PandaReach-v3", **kw))
    graphed = pg.VecNormalize(pg.PandaVecEnv("PandaReach-v3", **kw))
    eager.reset_tensors(seed=9)
    graphed.reset_tensors(seed=9)
    acts = torch.empty((k, n, 3), device="cuda:0")
    for i in range(k):
        acts[i].copy_(eager.sample_actions(i))
    g = graphed.capture_steps(k, acts)
    for rep in range(replays):
        for i in range(k):
            eager.step_tensors(acts[i])
        g.replay()
        torch.cuda.synchronize()
        for x, y, name in zip(eager.get_stats(), graphed.get_stats(), ("mean", "var", "count", "returns")):
            assert_bits(y, x, f"replay {rep} {name}")
        for name in ("observation", "achieved_goal", "desired_goal", "reward"):
            assert_bits(graphed._n[name].cpu().numpy(), eager._n[name].cpu().numpy(), f"replay {rep} {name}")
        done = (eager.truncated | eager.terminated).bool()
        assert torch.equal(done, (graphed.truncated | graphed.terminated).bool())
        assert torch.equal(graphed._n["terminal_obs"][done], eager._n["terminal_obs"][done])
    assert eager.ret_rms.count == pytest.approx(1e-4 + k * replays * n)
    eager.close()
    graphed.close()


# ------------------------------------------------------------------ HER
def _ring(od, ad, N=64, C=29, seed=5):
    from oracle import her as H
    from panda_gym_amd.her import STRATEGIES, HerReplayBuffer

    buf = HerReplayBuffer(C * N, device="cuda:0", n_envs=N, obs_dim=od, action_dim=ad, seed=seed)
    orc = H.HerOracle(N, C, od, ad, reward_type=0, strategy=STRATEGIES["future"], her_ratio=buf.her_ratio, seed=seed)
    rng = np.random.default_rng(od)
    left = rng.integers(2, 12, N)
    for t in range(40):
        left -= 1
        done = (left == 0).astype(np.uint8)
        left[done == 1] = rng.integers(2, 12, int(done.sum()))
        timeout = (done & (rng.random(N) < 0.5)).astype(np.uint8)
        f = lambda *s: rng.standard_normal((N,) + s).astype(F32)  # noqa: E731
        args = [f(od), f(3) * 0.05, f(3) * 0.05, f(ad), f(), f(od), f(3) * 0.05, f(3) * 0.05, done, timeout]
        orc.add(*args)
        buf.add_tensors(*args)
    return buf, orc


HER_FIELDS = ["obs", "achieved_goal", "desired_goal", "action", "reward", "next_obs", "next_achieved_goal",
              "next_desired_goal", "done", "slot", "env", "goal_slot"]


@pytest.mark.parametrize("od,ad", [(19, 4), (56, 7)])
def test_her_batch_normalised_in_place(od, ad):
    B = 1031
    buf, orc = _ring(od, ad)
    raw = {k: v.cpu().numpy().copy() for k, v in buf.sample_raw(B, draw=2).items()}
    want = orc.sample(B, 2)
    for k in HER_FIELDS:   # env=None: the batch as ever
        assert np.array_equal(bits(raw[k]) if raw[k].dtype == F32 else raw[k],
                              bits(want[k]) if want[k].dtype == F32 else want[k]), k
    rng = np.random.default_rng(1)
    S = od + 7
    nz = NZ.Normalizer(64, od, device="cuda:0")
    mean, var = rng.standard_normal(S) * 0.05, rng.random(S) * 0.5 + 0.01
    nz.set_stats(mean, var, np.full(S, 100.0))
    ref = RefNorm(64, od)
    got = {k: v.cpu().numpy() for k, v in buf.sample_raw(B, draw=2, env=nz).items()}
    stats = nz.get_stats()[:2]
    for k in ("slot", "env", "goal_slot"):
        assert np.array_equal(got[k], raw[k]), k
    assert_bits(got["action"], raw["action"], "action")
    assert_bits(got["done"], raw["done"], "done")
    for f, key in (("obs", "observation"), ("next_obs", "observation"), ("achieved_goal", "achieved_goal"),
                   ("next_achieved_goal", "achieved_goal"), ("desired_goal", "desired_goal"),
                   ("next_desired_goal", "desired_goal")):
        assert_bits(got[f], ref.norm_obs(key, raw[f], stats), f)
    assert_bits(got["reward"], ref.norm_reward_(raw["reward"], stats), "reward")
    assert not np.array_equal(bits(got["reward"]), bits(raw["reward"]))
    # only the enabled keys
    nz.set_keys(abi.NORM_KEY_BITS["desired_goal"], False)
    got = {k: v.cpu().numpy() for k, v in buf.sample_raw(B, draw=2, env=nz).items()}
    for f in ("obs", "next_obs", "achieved_goal", "next_achieved_goal", "reward", "action", "done"):
        assert_bits(got[f], raw[f], f)
    assert_bits(got["next_desired_goal"], ref.norm_obs("desired_goal", raw["next_desired_goal"], stats), "next dg")
    nz.close()
    buf.close()


def test_her_add_from_wrapped_env_stores_raw_values(pg):
    from panda_gym_amd.her import HerReplayBuffer

    n = 64
    kw = dict(num_envs=n, device="cuda:0", seed=1, max_episode_steps=5)
    bare = pg.PandaVecEnv("PandaReach-v3", **kw)
    w = pg.VecNormalize(pg.PandaVecEnv("PandaReach-v3", **kw))
    bufs = [HerReplayBuffer(100 * n, env=e, device="cuda:0", seed=2) for e in (bare, w)]
    bare.reset_tensors()
    w.reset_tensors()
    for t in range(12):
        a = bare.sample_actions(t).clone()
        o_b = {k: v.clone() for k, v in bare._obs_dict().items()}
        o_w = {k: v.clone() for k, v in w.get_original_obs(tensors=True).items()}
        bare.step_tensors(a)
        w.step_tensors(a)
        bufs[0].add_from_vec_env(bare, o_b, a)
        bufs[1].add_from_vec_env(w, o_w, a)
    x, y = bufs[0].sample_raw(2048, draw=0), bufs[1].sample_raw(2048, draw=0)
    for k in ("rows", "slot", "env", "goal_slot"):
        assert torch.equal(x[k], y[k]), k
    for a_, b_ in zip(bufs[0]._arrays(), bufs[1]._arrays()):
        assert torch.equal(a_, b_)
    s = bufs[1].sample(256, env=w)   # the SB3 call
    st = w.get_stats()[:2]
    ref = RefNorm(n, 6)
    r = bufs[1].sample_raw(256, draw=bufs[1]._draw - 1)
    assert_bits(s.observations["observation"].cpu().numpy(), ref.norm_obs("observation", r["obs"].cpu().numpy(), st),
                "sample(env=) observation")
    assert_bits(s.rewards.cpu().numpy()[:, 0], ref.norm_reward_(r["reward"].cpu().numpy(), st), "sample(env=) reward")
    for b in bufs:
        b.close()
    bare.close()
    w.close()
