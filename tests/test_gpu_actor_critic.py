"""GPU tests of the device actor-critic (pgx_actor_critic.hip): the forward kernel's mean and values against
the library's host model bit for bit (both trunks, K order, padding, tail masking, both env tiles), the values
entry and its need mask, the Gaussian epilogue against fp64 with a margin measured against torch's f32
evaluation of the same expression, the device noise stream (its own tag) against oracle.her's Philox, SB3's
collect_rollouts captured in one graph against the same steps through the public eager calls (bare env and
VecMonitor(VecNormalize), with the time-limit bootstrap proven to run), repeats and live weights under the
graph, pg.evaluate, and that the actor-critic writes nothing but its own buffers."""
import numpy as np
import pytest
import torch

import panda_gym_amd as pg
from oracle import her as H
from panda_gym_amd import abi
from panda_gym_amd.rollout import step_buffers, terminal_observation
from test_actor_abi import bits, random_obs, random_state_dict
from test_actor_critic_abi import random_ac_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def host(t):
    return t.detach().cpu().numpy()


def make_ac(rng, n, obs_dim, pi, vf, A, scale=1.0, **kw):
    ac = pg.ActorCritic(obs_dim=obs_dim, action_dim=A, n_envs=n, net_arch=dict(pi=pi, vf=vf), device=DEV, **kw)
    ac.load_state_dict(random_ac_state_dict(ac, rng, scale=scale))
    return ac


def tile_of(n):
    """Envs per workgroup: 32 from 4096 envs on (where the LDS regions fit, as in every case here), else 16."""
    return 32 if n >= 4096 else 16


# ------------------------------------------------------------------ 1. kernel == host model
# (N, in_dim, pi, vf, A): one env; unequal depth and widths that are no multiple of 16; the reference's; the LDS
# limit (three 512-wide layers); the 32-env tile with a 4-env tail
CASES = [(1, 12, (32,), (32,), 1), (33, 24, (33, 7), (96,), 7), (257, 62, (256, 256), (256, 256), 4),
         (65, 12, (400, 300), (512, 512, 512), 3), (4100, 12, (33, 7), (7, 33), 4)]


@pytest.mark.parametrize("n,in_dim,pi,vf,A", CASES)
def test_kernel_equals_host_model_bit_for_bit(n, in_dim, pi, vf, A):
    rng = np.random.default_rng(n + in_dim)
    ac = make_ac(rng, n, in_dim - 6, pi, vf, A)
    dbg = ac.enable_debug()
    obs = random_obs(rng, n, in_dim - 6)
    actions, values, log_probs = ac(obs, deterministic=True)
    mean, value = ac.forward_host(obs)
    got = host(dbg["mean"])
    assert np.isfinite(got).all() and got.any() and np.array_equal(bits(got), bits(mean))
    got = host(values)
    assert np.isfinite(got).all() and got.any() and np.array_equal(bits(got), bits(value))
    assert np.array_equal(bits(host(actions)), bits(mean))   # deterministic: the mode
    assert np.isfinite(host(log_probs)).all()
    # the values entry alone: the same bits
    assert np.array_equal(bits(host(ac.predict_values(obs))), bits(value))
    ac.close()


def test_kernel_equals_host_model_with_denormal_and_negative_zero_inputs():
    rng = np.random.default_rng(5)
    n, od = 31, 6
    ac = make_ac(rng, n, od, (96,), (33, 7), 4)
    dbg = ac.enable_debug()
    obs = random_obs(rng, n, od)
    obs["observation"][::3, 1] = F32(-0.0)
    obs["observation"][1::3, 2] = F32(1e-41)      # subnormal
    obs["achieved_goal"][::2, 0] = F32(-3e-39)    # subnormal
    obs["desired_goal"][:, 2] = F32(-0.0)
    # an env whose every input is tiny: the products and the first layers' sums stay subnormal where the bias is 0
    sd = {k: host(v) for k, v in ac.state_dict().items()}
    sd["mlp_extractor.policy_net.0.bias"][:48] = 0.0
    sd["mlp_extractor.value_net.0.bias"][:16] = 0.0
    ac.load_state_dict(sd)
    for k in obs:
        obs[k][7] = (rng.standard_normal(obs[k].shape[1]) * 1e-39).astype(F32)
    _, values, _ = ac(obs, deterministic=True)
    mean, value = ac.forward_host(obs)
    assert np.isfinite(mean).all() and np.isfinite(value).all()
    assert np.array_equal(bits(host(dbg["mean"])), bits(mean))
    assert np.array_equal(bits(host(values)), bits(value))
    ac.close()


# ------------------------------------------------------------------ 2. predict_values and its mask
@pytest.mark.parametrize("n", [33, 4100])
def test_predict_values_and_the_need_mask(n):
    rng = np.random.default_rng(n)
    ac = make_ac(rng, n, 6, (33, 7), (7, 33), 4)
    obs = {k: torch.as_tensor(v, device=DEV) for k, v in random_obs(rng, n, 6).items()}
    fwd = host(ac(obs)[1]).copy()
    full = host(ac.predict_values(obs)).copy()
    assert fwd.all() and np.array_equal(bits(full), bits(fwd))   # no value is zero: a skipped env shows
    T = tile_of(n)
    tiles = np.arange(n) // T
    masks = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "last": np.arange(n) == n - 1,
             "one inside": np.arange(n) == 5, "two tiles": np.isin(np.arange(n), (T - 1, n - 1))}
    out = torch.full((n,), 7.0, device=DEV)
    for name, need in masks.items():
        out.fill_(7.0)
        got = ac.predict_values(obs, need=torch.as_tensor(need, device=DEV), out=out)
        assert got is out
        got = host(got)
        live = np.isin(tiles, np.unique(tiles[need]))   # every env of a tile that holds a flag
        assert np.array_equal(bits(got[live]), bits(full[live])), name
        assert not bits(got[~live]).any(), name            # +0, bit pattern 0
        assert live[need].all() and (name != "last" or live.sum() == n - (n - 1) // T * T), name
    # a uint8 mask with values other than 1, as a flag buffer may hold
    need = torch.zeros(n, dtype=torch.uint8, device=DEV)
    need[n - 1] = 255
    got = host(ac.predict_values(obs, need=need))
    assert bits(got[n - 1]) == bits(full[n - 1]) and not bits(got[:(n - 1) // T * T]).any()
    ac.close()


# ------------------------------------------------------------------ 3. the epilogue
def fp64_actions(mean, log_std, eps):
    return mean.astype(np.float64) + np.exp(log_std.astype(np.float64)) * eps.astype(np.float64)


def fp64_log_prob(actions, mean, log_std):
    a, m, ls = actions.astype(np.float64), mean.astype(np.float64), log_std.astype(np.float64)
    return (-((a - m) ** 2) / (2.0 * np.exp(ls) ** 2) - ls - HALF_LOG_2PI).sum(axis=1)


def check_against_fp64(what, got, want, torch_f32):
    """Margin: twice the largest error of torch's f32 evaluation of the same expression on the same device
    tensors, plus one ulp of the result's magnitude."""
    torch_err = float(np.abs(host(torch_f32).astype(np.float64) - want).max())
    kernel_err = float(np.abs(got.astype(np.float64) - want).max())
    ulp = float(np.spacing(F32(np.abs(want).max())))
    print(f"{what}: kernel max error {kernel_err:.3e}, torch f32 max error {torch_err:.3e}, one ulp {ulp:.3e}")
    assert np.isfinite(got).all()
    assert kernel_err <= 2.0 * torch_err + ulp, what


def test_gaussian_epilogue_against_fp64():
    rng = np.random.default_rng(11)
    n, A = 257, 7
    ac = make_ac(rng, n, 6, (32, 32), (32,), A, scale=2.0)   # log_std from -3 to 0.5; scale 2: some actions leave the box
    dbg = ac.enable_debug()
    log_std = host(ac.state_dict()["log_std"])
    assert log_std.min() == F32(-3.0) and log_std.max() == F32(0.5)
    ls_t = torch.as_tensor(np.tile(log_std, (n, 1)), device=DEV)
    obs = random_obs(rng, n, 6)
    eps = torch.as_tensor(rng.standard_normal((n, A)).astype(F32), device=DEV)
    actions, values, log_probs = ac(obs, eps=eps)
    act, lp, clipped = host(actions).copy(), host(log_probs).copy(), host(ac.clipped_actions).copy()
    mean_t = dbg["mean"].clone()
    mean = host(mean_t)
    assert np.array_equal(bits(host(dbg["eps"])), bits(host(eps)))
    # the clip: bit for bit, with actions on both sides of the box's faces
    assert (act > 1).any() and (act < -1).any() and (np.abs(act) < 1).any()
    assert np.array_equal(bits(clipped), bits(np.clip(act, F32(-1.0), F32(1.0))))
    check_against_fp64("actions", act, fp64_actions(mean, np.tile(log_std, (n, 1)), host(eps)),
                       mean_t + torch.exp(ls_t) * eps)
    dist = torch.distributions.Normal(mean_t, torch.exp(ls_t))
    check_against_fp64("log_probs", lp, fp64_log_prob(act, mean, np.tile(log_std, (n, 1))),
                       dist.log_prob(actions).sum(1))
    # deterministic=True ignores eps bit for bit; its actions are the mean plane, its log_probs the mode's density
    d1 = [host(t).copy() for t in ac(obs, deterministic=True, eps=eps)] + [host(ac.clipped_actions).copy()]
    d2 = [host(t).copy() for t in ac(obs, deterministic=True)] + [host(ac.clipped_actions).copy()]
    for x, y in zip(d1, d2):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(bits(d1[0]), bits(mean)) and np.array_equal(bits(host(dbg["mean"])), bits(mean))
    assert not host(dbg["eps"]).any()
    assert np.array_equal(bits(d1[1]), bits(host(values)))
    check_against_fp64("log_probs of the mode", d1[2], fp64_log_prob(mean, mean, np.tile(log_std, (n, 1))),
                       dist.log_prob(mean_t).sum(1))
    ac.close()


# ------------------------------------------------------------------ 4. the device noise
def expected_words(tag, seed, step, n, pairs):
    e, p = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(pairs, dtype=np.uint64), indexing="ij")
    c0 = np.full(e.shape, step & 0xFFFFFFFF, np.uint64)
    c1 = np.full(e.shape, step >> 32, np.uint64)
    r = H.philox4x32_10(c0, c1, e, np.uint64(tag) ^ p, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(r, axis=-1)   # [n, pairs, 4] uint32


def test_device_noise_words_box_muller_and_step_word():
    rng = np.random.default_rng(13)
    n, A, seed, step0 = 257, 7, (5 << 32) | 17, (3 << 32) | 9
    ac = make_ac(rng, n, 6, (32,), (32,), A, seed=seed)
    dbg = ac.enable_debug()
    obs = random_obs(rng, n, 6)
    ac.noise_step = step0
    assert ac.noise_step == step0
    ac(obs)
    assert ac.noise_step == step0 + 1
    words = host(dbg["philox"]).view(np.uint32)
    want = expected_words(abi.AC_PHILOX_TAG, seed, step0, n, 4)
    assert np.array_equal(words, want)   # all four pairs of A = 7
    assert not np.array_equal(words, expected_words(abi.ACTOR_PHILOX_TAG, seed, step0, n, 4))
    u1 = ((want[..., 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (want[..., 1] >> 8).astype(np.float64) * 2.0 ** -24
    rad, ang = np.sqrt(-2.0 * np.log(u1)), float(F32(6.2831855)) * u2
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(n, 8)[:, :A]
    # the margin: torch's f32 evaluation of the same lines from the same words
    tu1, tu2 = torch.as_tensor(u1.astype(F32), device=DEV), torch.as_tensor(u2.astype(F32), device=DEV)
    trad, tang = torch.sqrt(-2.0 * torch.log(tu1)), 6.2831855 * tu2
    tz = torch.stack([trad * torch.cos(tang), trad * torch.sin(tang)], dim=-1).reshape(n, 8)[:, :A]
    eps_t = dbg["eps"].clone()
    eps = host(eps_t)
    check_against_fp64("Box-Muller", eps, z, tz)
    # the action is the mean moved by that plane
    log_std = np.tile(host(ac.state_dict()["log_std"]), (n, 1))
    ls_t = torch.as_tensor(log_std, device=DEV)
    check_against_fp64("actions from the device noise", host(ac.actions), fp64_actions(host(dbg["mean"]), log_std, eps),
                       dbg["mean"] + torch.exp(ls_t) * eps_t)
    # the word moves by one per drawing forward, and only then; setting it back reproduces the plane
    ac(obs)
    assert not np.array_equal(bits(host(dbg["eps"])), bits(eps))
    ac(obs, deterministic=True)
    ac(obs, eps=torch.zeros((n, A), device=DEV))
    ac.predict(obs)
    ac.predict_values(obs)
    assert ac.noise_step == step0 + 2
    ac.noise_step = step0
    ac(obs)
    assert np.array_equal(bits(host(dbg["eps"])), bits(eps))
    # an Actor of the same seed at the same step draws other words
    actor = pg.Actor(obs_dim=6, action_dim=A, n_envs=n, net_arch=(32,), kind="gaussian", seed=seed, device=DEV)
    actor.load_state_dict(random_state_dict(actor, rng))
    adbg = actor.enable_debug()
    actor.noise_step = step0
    actor(obs)
    theirs = host(adbg["philox"]).view(np.uint32)
    assert np.array_equal(theirs, expected_words(abi.ACTOR_PHILOX_TAG, seed, step0, n, 4))
    assert not (theirs == words).all(axis=-1).any()   # no counter block in common
    assert not np.array_equal(bits(host(adbg["eps"])), bits(eps))
    actor.close()
    ac.close()


# ------------------------------------------------------------------ 5. collect_rollouts: graph == eager
GAMMA, LAMBDA = 0.99, 0.9


def rollout_side(wrapped, N, T, sd=None, seed=21):
    base = pg.PandaVecEnv("PandaReach-v3", num_envs=N, device=DEV, seed=7)
    venv = pg.VecMonitor(pg.VecNormalize(base)) if wrapped else base
    ac = pg.ActorCritic(env=venv, net_arch=dict(pi=[32, 32], vf=[33]), seed=seed)
    buf = pg.RolloutBuffer(T, env=venv, device=DEV, gamma=GAMMA, gae_lambda=LAMBDA)
    if sd is not None:
        ac.load_state_dict(sd)
    return base, venv, ac, buf


def snapshot(buf):
    torch.cuda.synchronize()
    return {k: host(v).copy() for k, v in buf.arrays().items()}


@pytest.mark.parametrize("wrapped", [False, True])
def test_captured_rollout_equals_eager(wrapped):
    N, T = 65, 4
    rng = np.random.default_rng(19)
    sides = [rollout_side(wrapped, N, T) for _ in range(2)]
    sd = random_ac_state_dict(sides[0][2], rng, log_std=(-1.0, 0.0))
    sd["value_net.bias"] = np.array([0.75], F32)   # V(terminal) cannot vanish: the bootstrap shows in the reward
    first = []
    for base, venv, ac, buf in sides:
        ac.load_state_dict(sd)
        ac.noise_step = 100
        first.append(venv.reset_tensors(seed=7, episode_phase="staggered"))
        buf.set_last(first[-1])
    (cb, cv, ca, cbuf), (eb, ev, ea, ebuf) = sides
    # the graph
    g = ca.capture_rollout(cv, cbuf)
    cbuf.reset()
    g.replay()
    # the public eager calls
    obs = first[1]
    raw_reward, term, trunc, tvals = [], [], [], []
    for _ in range(T):
        actions, values, log_probs = ea(obs)
        obs = ev.step_tensors(ea.clipped_actions)[0]
        tv = ea.predict_values(terminal_observation(ev))
        _, r, te, tr = step_buffers(ev)
        raw_reward.append(host(r).copy()), term.append(host(te).copy()), trunc.append(host(tr).copy())
        tvals.append(host(tv).copy())
        ebuf.add_from_vec_env(ev, actions, values, log_probs, terminal_value=tv)
    ebuf.compute_returns_and_advantage(ea.predict_values(obs))
    cbuf.raise_device_errors()
    assert ca.noise_step == ea.noise_step == 100 + T
    assert cbuf.pos == ebuf.pos == T
    a, b = snapshot(cbuf), snapshot(ebuf)
    assert set(a) == set(b) and {"advantage", "return", "value", "log_prob", "reward", "action"} <= set(a)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert np.array_equal(host(cb._outbuf), host(eb._outbuf))   # the envs ended in the same place
    assert np.isfinite(a["advantage"]).all() and a["advantage"].any() and a["value"].any()
    acts = a["action"]
    assert all(not np.array_equal(acts[i], acts[j]) for i in range(T) for j in range(i + 1, T))
    # the time limit: env g starts at phase g mod max_episode_steps, so who is cut off inside the window is known
    raw_reward, term, trunc, tvals = (np.stack(x) for x in (raw_reward, term, trunc, tvals))
    limit = int(eb.spec.max_episode_steps)
    phase = np.arange(N) % limit
    assert int(trunc.astype(bool).sum()) == int((phase >= limit - T).sum()) == 4
    cut = trunc.astype(bool) & ~term.astype(bool)
    assert cut.any()
    stored = a["reward"].astype(np.float64)
    boot = float(F32(GAMMA)) * tvals.astype(np.float64)
    assert (np.abs(boot[cut]) > 0.1).all()   # value_net.bias is 0.75
    want = raw_reward.astype(np.float64) + boot
    # f32: the product rounds once (half an ulp of it), the sum once more (half an ulp of the result), or both
    # at once as one fma; twice that is allowed
    tol = np.spacing(np.abs(boot[cut]).astype(F32)).astype(np.float64) + np.spacing(np.abs(want[cut]).astype(F32))
    assert (np.abs(stored[cut] - want[cut]) <= tol).all()
    assert (stored[cut] != raw_reward[cut]).all()
    assert np.array_equal(bits(a["reward"][~cut]), bits(raw_reward[~cut]))   # everyone else: the reward as it came
    for base, venv, ac, buf in sides:
        buf.close()
        ac.close()
        venv.close()


# ------------------------------------------------------------------ 6. repeats and live weights
def test_replays_draw_new_noise_and_use_the_weights_loaded_last():
    N, T = 33, 2
    rng = np.random.default_rng(23)
    base, venv, ac, buf = rollout_side(False, N, T)
    ac.load_state_dict(random_ac_state_dict(ac, rng, log_std=(-1.0, 0.0)))
    buf.set_last(venv.reset_tensors(seed=7))
    g = ac.capture_rollout(venv, buf)
    planes = []
    for i in range(2):
        buf.reset()
        g.replay()
        buf.raise_device_errors()
        assert buf.pos == T and ac.noise_step == (i + 1) * T
        planes.append(snapshot(buf))
    assert not np.array_equal(bits(planes[0]["action"]), bits(planes[1]["action"]))
    assert np.array_equal(bits(planes[1]["observation"][0]), bits(planes[0]["last_observation"]))   # the carry went on
    # deterministic, one step per replay: the stored action and value are the host model's on the observation
    # the replay read, under the weights loaded just before it
    dbg = ac.enable_debug()
    one = pg.RolloutBuffer(1, env=venv, device=DEV, gamma=GAMMA, gae_lambda=LAMBDA)
    one.set_last(step_buffers(venv)[0])
    g1 = ac.capture_rollout(venv, one, deterministic=True)
    means = []
    for _ in range(2):
        ac.load_state_dict(random_ac_state_dict(ac, rng))   # the next replay must see these
        before = {k: host(v).copy() for k, v in step_buffers(venv)[0].items()}
        one.reset()
        g1.replay()
        got = snapshot(one)
        mean, value = ac.forward_host(before)
        assert np.array_equal(bits(host(dbg["mean"])), bits(mean))
        assert np.array_equal(bits(got["action"][0]), bits(mean)) and np.array_equal(bits(got["value"][0]), bits(value))
        means.append(mean)
    assert not np.array_equal(means[0], means[1])
    assert ac.noise_step == 2 * T   # deterministic replays draw nothing
    one.close()
    buf.close()
    ac.close()
    venv.close()


# ------------------------------------------------------------------ 7. evaluate
def test_evaluate_takes_predict():
    venv = pg.PandaVecEnv("PandaReach-v3", num_envs=8, device=DEV, seed=7)
    ac = pg.ActorCritic(env=venv, net_arch=[32, 32])
    ac.load_state_dict(random_ac_state_dict(ac, np.random.default_rng(29), scale=3.0))
    res, eps = pg.evaluate(venv, ac.predict, 16, return_episodes=True)
    assert ac.noise_step == 0   # evaluation is deterministic: no draw
    assert set(res) == {"mean_reward", "std_reward", "success_rate", "collision_rate", "timeout_rate", "nonfinite_rate",
                        "num_episodes", "mean_ep_length", "mean_ep_length_success", "mean_num_sim_steps",
                        "mean_num_sim_steps_success", "mean_ee_speed"}   # as with the Actor
    assert res["num_episodes"] == 16 and len(eps["r"]) == 16
    # predict is clip(mean)
    dbg = ac.enable_debug()
    obs = venv.reset_tensors(seed=3)
    got = host(ac.predict(obs)).copy()
    mean = host(dbg["mean"])
    assert (np.abs(mean) > 1).any() and np.array_equal(bits(got), bits(np.clip(mean, F32(-1.0), F32(1.0))))
    assert np.array_equal(bits(mean), bits(ac.forward_host(obs)[0]))
    # a gSDE-trained policy: deterministic prediction and the critic work, exploration is refused
    sde = pg.ActorCritic(env=venv, net_arch=[32, 32], use_sde=True)
    sd = {k: host(v) for k, v in ac.state_dict().items()}
    sd["log_std"] = np.zeros((32, venv.action_dim), F32)
    sde.load_state_dict(sd)
    assert np.array_equal(bits(host(sde.predict(obs))), bits(got))
    assert np.array_equal(bits(host(sde.predict_values(obs))), bits(host(ac.predict_values(obs))))
    buf = pg.RolloutBuffer(2, env=venv, device=DEV)
    for call in (lambda: sde(obs), lambda: sde.predict(obs, deterministic=False), lambda: sde.collect_rollouts(venv, buf),
                 lambda: sde.capture_rollout(venv, buf)):
        with pytest.raises(pg.PgxError, match="gSDE exploration is not built"):
            call()
    buf.close()
    sde.close()
    ac.close()
    venv.close()


# ------------------------------------------------------------------ 8. isolation
def test_actor_critic_writes_only_its_own_buffers():
    """A forward and a values launch leave the env's observation and terminal buffers and the rollout's records
    bit-unchanged, and guard words around the outputs intact."""
    N, T = 65, 2
    rng = np.random.default_rng(31)
    base, venv, ac, buf = rollout_side(False, N, T)
    ac.load_state_dict(random_ac_state_dict(ac, rng))
    buf.set_last(venv.reset_tensors(seed=7))
    ac.collect_rollouts(venv, buf)   # fills the records, the outputs and the terminal buffers
    A, G = ac.action_dim, 64
    # the outputs as slices of one arena, guard words of a NaN pattern no kernel produces on every side
    sizes = {"actions": N * A, "clipped_actions": N * A, "values": N, "log_probs": N, "pv": N}
    arena = torch.full((G + sum(s + G for s in sizes.values()),), float("nan"), device=DEV)
    arena_bits = arena.view(torch.int32)
    arena_bits.fill_(0x7FC0BEEF)
    off, view = G, {}
    for k, s in sizes.items():
        view[k] = arena[off:off + s]
        off += s + G
    ac.actions, ac.clipped_actions = view["actions"].view(N, A), view["clipped_actions"].view(N, A)
    ac.values, ac.log_probs = view["values"], view["log_probs"]
    inside = torch.zeros(arena.shape, dtype=torch.bool, device=DEV)
    off = G
    for s in sizes.values():
        inside[off:off + s] = True
        off += s + G
    obs, tobs = step_buffers(venv)[0], terminal_observation(venv)
    before = {"out": base._outbuf.clone(), "records": buf.arrays()["records"].clone(),
              **{f"obs.{k}": v.clone() for k, v in obs.items()}, **{f"tobs.{k}": v.clone() for k, v in tobs.items()}}
    ac(obs)
    ac.predict_values(tobs, need=step_buffers(venv)[3], out=view["pv"])
    ac.predict_values(obs, out=view["pv"])
    torch.cuda.synchronize()
    after = {"out": base._outbuf, "records": buf.arrays()["records"], **{f"obs.{k}": v for k, v in obs.items()},
             **{f"tobs.{k}": v for k, v in tobs.items()}}
    for k in before:
        assert torch.equal(before[k].view(torch.uint8), after[k].contiguous().view(torch.uint8)), k
    got = host(arena_bits)
    inside = host(inside)
    assert (got[~inside] == 0x7FC0BEEF).all()
    assert (got[inside] != 0x7FC0BEEF).all() and np.isfinite(host(arena)[inside]).all()   # every output word written
    buf.close()
    ac.close()
    venv.close()
