"""The action log-probability entries on an MI355X (pgx_actor_action_log_prob, pgx_sde_actor_action_log_prob):
the Linear-chain planes against the library's host model bit for bit, `action` and `log_prob` against fp64 from
the kernel's own debug planes (margin: twice the largest error of torch's f32 evaluation of SB3's lines on the
same device tensors, plus one ulp of the result's magnitude), the noise streams, the gSDE batch entry against
the per-env forward, a HER batch read in place, the captured chain sample_into -> action_log_prob_rows ->
td_target_rows, and containment."""
import ctypes as C

import numpy as np
import pytest
import torch

import panda_gym_amd as pg
from oracle import her as H
from panda_gym_amd import abi
from test_action_log_prob_abi import (TANH_EPS, fp64_gaussian, fp64_sde_action, fp64_sde_log_prob, make_gaussian,
                                      make_sde)
from test_actor_abi import bits, random_obs
from test_quantile_critic_abi import make_qc
from test_sde_actor_abi import random_sde_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CANARY = 12345.0
PAD = 64
UNITS = ["gaussian", "sde"]


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def guarded(rows, width):
    """A contiguous [rows, width] f32 view ([rows] for width 0) with PAD canary floats in front of and behind it."""
    n = rows * max(width, 1)
    flat = torch.full((2 * PAD + n,), CANARY, dtype=torch.float32, device=DEV)
    body = flat[PAD:PAD + n]
    return flat, (body.view(rows, width) if width else body)


def canaries_intact(flat):
    f = host(flat)
    return bool((f[:PAD] == CANARY).all() and (f[-PAD:] == CANARY).all())


def strided(a, extra=5, lead=2):
    """The array as a device view whose row stride is larger than its width."""
    a = np.asarray(a, F32)
    wide = torch.full((a.shape[0], a.shape[1] + extra), 777.0, dtype=torch.float32, device=DEV)
    v = wide[:, lead:lead + a.shape[1]]
    v.copy_(dev(a))
    return v


def make(unit, od, A, arch, rng, n_envs=1, **kw):
    return (make_gaussian if unit == "gaussian" else make_sde)(od, A, arch, rng, device=DEV, n_envs=n_envs, **kw)[0]


class Run:
    """One guarded action_log_prob call: outputs and every debug plane between canaries, B + 3 output rows."""

    def __init__(self, actor, obs, B, eps=None):
        self.flats, self.B = [], B
        fa, self.act = guarded(B + 3, actor.action_dim)
        fl, self.lp = guarded(B + 3, 0)
        self.flats += [fa, fl]
        planes = {}
        for k, w in actor._lp_planes().items():
            f, planes[k] = guarded(B, w)
            self.flats.append(f)
        if actor._LP_PHILOX:
            planes["philox"] = torch.zeros((B, 4, 4), dtype=torch.int32, device=DEV)
        actor._lp_debug = planes
        kw = {} if eps is None else {"eps": eps}
        out = actor.action_log_prob(obs, out=(self.act, self.lp), **kw)
        assert out[0] is self.act and out[1] is self.lp
        torch.cuda.synchronize()
        self.t = planes
        self.p = {k: host(v).copy() for k, v in planes.items()}
        self.action, self.log_prob = host(self.act)[:B].copy(), host(self.lp)[:B].copy()

    def contained(self):
        return all(canaries_intact(f) for f in self.flats) and bool((host(self.act)[self.B:] == CANARY).all()) \
            and bool((host(self.lp)[self.B:] == CANARY).all())


def margin(what, got, want, torch_f32):
    torch_err = float(np.abs(host(torch_f32).astype(np.float64) - want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    ulp = float(np.spacing(F32(np.abs(want).max())))
    print(f"{what}: kernel max error {err:.3e}, torch f32 max error {torch_err:.3e}, one ulp {ulp:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= 2.0 * torch_err + ulp, what


def check_gaussian_epilogue(what, run):
    """action, gaussian_action and log_prob of every row against fp64 from the kernel's own planes."""
    m, ls, e = run.t["mean"], run.t["log_std"], run.t["eps"]
    std = torch.exp(ls)
    g = m + std * e
    a = torch.tanh(g)
    lp = torch.distributions.Normal(m, std).log_prob(g).sum(1) - torch.log(1 - a ** 2 + 1e-6).sum(1)
    want_a, want_lp = fp64_gaussian(run.p["mean"], run.p["log_std"], run.p["eps"], run.action)
    margin(f"{what} action", run.action, want_a, a)
    margin(f"{what} gaussian_action", run.p["gaussian_action"],
           np.exp(run.p["log_std"].astype(np.float64)) * run.p["eps"] + run.p["mean"], g)
    margin(f"{what} log_prob", run.log_prob, want_lp, lp)


def check_sde_epilogue(what, run):
    m, z, v = run.t["mean"], run.t["noise"], run.t["variance"]
    a = torch.tanh(m + z)
    x = dev(run.action).clamp(-1 + TANH_EPS, 1 - TANH_EPS)   # SB3 inverts the squashed action it was given
    g = 0.5 * (x.log1p() - (-x).log1p())
    scale = torch.sqrt(v + 1e-6)
    lp = torch.distributions.Normal(m, scale).log_prob(g).sum(1) - torch.log(1 - torch.tanh(g) ** 2 + 1e-6).sum(1)
    margin(f"{what} action", run.action, fp64_sde_action(run.p["mean"], run.p["noise"]), a)
    want_lp, want_g = fp64_sde_log_prob(run.action, run.p["mean"], run.p["variance"])
    margin(f"{what} gaussian_action", run.p["gaussian_action"], want_g, g)
    margin(f"{what} log_prob", run.log_prob, want_lp, lp)


def check_against_host(unit, actor, run, obs_np, eps=None, Eb=None):
    """The chain planes equal the host model's bit for bit; the epilogue holds the fp64 margin, no row exempt."""
    if unit == "gaussian":
        want = actor.log_prob_host(obs_np, eps)
        for k in ("mean", "log_std", "eps"):
            assert np.array_equal(bits(run.p[k]), bits(want[k])), k
        check_gaussian_epilogue(unit, run)
    else:
        want = actor.log_prob_host(obs_np, Eb)   # std: the handle's
        for k in ("mean", "latent", "noise", "variance"):
            assert np.array_equal(bits(run.p[k]), bits(want[k])), k
        check_sde_epilogue(unit, run)
    assert run.contained()   # (the host model's own epilogue goes through another libm: checked against fp64 on a CPU)


def random_Eb(actor, rng):
    Eb = (rng.standard_normal((actor.latent_dim, actor.action_dim)) * 0.05).astype(F32)
    actor.exploration_mat = Eb
    assert np.array_equal(bits(host(actor.exploration_mat)), bits(Eb))
    return Eb


# ------------------------------------------------------------------ 1. kernel == host model, epilogue vs fp64
# B (1, 15, 16: the 16-row tile; from 17 on the 32-row tile, tails of 17, 1 and 1 rows), obs_dim, net_arch, A,
# inputs with row strides above their widths
CASES = [(1, 6, (16,), 1, False), (15, 19, (20, 300), 3, True), (16, 6, (256, 256), 7, False), (17, 19, (16,), 3, True),
         (33, 6, (20, 300), 7, True), (257, 19, (256, 256), 3, False)]


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("B,od,arch,A,wide", CASES, ids=[f"B{c[0]}-od{c[1]}-{'x'.join(map(str, c[2]))}-A{c[3]}"
                                                         f"{'-strided' if c[4] else ''}" for c in CASES])
def test_planes_equal_host_model_and_epilogue_holds_fp64(unit, B, od, arch, A, wide):
    rng = np.random.default_rng(B + od + A)
    actor = make(unit, od, A, arch, rng, n_envs=3)   # n_envs has no say in a batch launch
    obs_np = random_obs(rng, B, od)
    obs = {k: strided(v) for k, v in obs_np.items()} if wide else {k: dev(v) for k, v in obs_np.items()}
    if wide:
        assert all(v.stride(0) > v.shape[1] for v in obs.values())
    if unit == "gaussian":
        eps = rng.standard_normal((B, A)).astype(F32)
        run = Run(actor, obs, B, eps=dev(eps))
        check_against_host(unit, actor, run, obs_np, eps=eps)
    else:
        Eb = random_Eb(actor, rng)
        run = Run(actor, obs, B)
        assert (run.p["noise"] != 0).any() and (run.p["variance"] > 0).all()
        check_against_host(unit, actor, run, obs_np, Eb=Eb)
    if wide:
        assert all(bool((v._base == 777.0).sum() == v.shape[0] * 5) for v in obs.values())   # read only
    actor.close()


@pytest.mark.parametrize("unit", UNITS)
@pytest.mark.parametrize("tile", ["16", "32"])
def test_both_row_tiles_with_a_tail(monkeypatch, unit, tile):
    """PGX_ACTOR_LP_TILE / PGX_SDE_LP_TILE (read at every launch) force the 16- or the 32-row tile; the library
    takes 32 from 17 rows on.  33 rows: three tiles of 16 with a one-row tail, or one of 32 and a single row."""
    rng = np.random.default_rng(3)
    B, od, A = 33, 19, 4
    actor = make(unit, od, A, (96, 40), rng)
    obs_np = random_obs(rng, B, od)
    obs = {k: dev(v) for k, v in obs_np.items()}
    eps = rng.standard_normal((B, A)).astype(F32)
    kw = {"eps": dev(eps)} if unit == "gaussian" else {}
    Eb = None if unit == "gaussian" else random_Eb(actor, rng)
    default = Run(actor, obs, B, **kw)
    monkeypatch.setenv("PGX_ACTOR_LP_TILE" if unit == "gaussian" else "PGX_SDE_LP_TILE", tile)
    run = Run(actor, obs, B, **kw)
    assert np.array_equal(bits(run.action), bits(default.action)) and np.array_equal(bits(run.log_prob), bits(default.log_prob))
    for k in default.p:
        assert np.array_equal(run.p[k].view(np.uint32), default.p[k].view(np.uint32)), k
    check_against_host(unit, actor, run, obs_np, eps=eps, Eb=Eb)
    actor.close()


@pytest.mark.parametrize("unit", UNITS)
def test_subnormal_and_negative_zero_inputs(unit):
    rng = np.random.default_rng(5)
    B, od, A, arch = 33, 6, 4, (96, 30)
    actor = make(unit, od, A, arch, rng)
    sd = {k: host(v) for k, v in actor.state_dict().items()}
    sd["latent_pi.0.bias"][:] = 0.0   # sums of tiny products stay subnormal where the bias is 0
    sd["latent_pi.2.bias"][:] = 0.0
    actor.load_state_dict(sd)
    obs_np = random_obs(rng, B, od)
    obs_np["observation"][::3, 1] = F32(-0.0)
    obs_np["observation"][1::3, 2] = F32(1e-41)
    obs_np["achieved_goal"][::2, 0] = F32(-3e-39)
    obs_np["desired_goal"][:, 2] = F32(-0.0)
    for k in obs_np:
        obs_np[k][7] = (rng.standard_normal(obs_np[k].shape[1]) * 1e-39).astype(F32)
    obs = {k: strided(v) for k, v in obs_np.items()}
    if unit == "gaussian":
        eps = rng.standard_normal((B, A)).astype(F32)
        eps[::4, 0] = F32(-0.0)
        eps[1::4, 1] = F32(2e-42)
        run = Run(actor, obs, B, eps=dev(eps))
        check_against_host(unit, actor, run, obs_np, eps=eps)
    else:
        Eb = (rng.standard_normal((arch[-1], A)) * 0.05).astype(F32)
        Eb[::5, 0] = F32(-0.0)
        Eb[1::5, 1] = F32(2e-40)
        Eb[:, 2] = F32(-0.0)          # a column of -0: the padded chain from +0 ends at +0
        Eb[:, 3] *= F32(1e-38)        # products that underflow
        actor.exploration_mat = Eb
        run = Run(actor, obs, B)
        lat7 = run.p["latent"][7][run.p["latent"][7] != 0]
        assert lat7.size and (np.abs(lat7) < np.finfo(F32).tiny).all()
        assert not bits(run.p["noise"][:, 2]).any()
        check_against_host(unit, actor, run, obs_np, Eb=Eb)
    actor.close()


# ------------------------------------------------------------------ 2. the guards: saturation, zero variance
@pytest.mark.parametrize("unit", UNITS)
def test_saturated_rows_and_a_zero_latent_stay_finite(unit):
    """clip_mean = 0 and a large mu bias: tanhf returns exactly +-1 and the 1e-6 / 1 - EPS guards carry the
    result.  gSDE: a row whose latent is all zero (var = 0, scale = 1e-3).  No row is exempt."""
    rng = np.random.default_rng(7)
    B, od, A = 257, 6, 3   # (the margin compares two maxima over the rows: enough rows for both to settle)
    actor = make(unit, od, A, (32,), rng, clip_mean=0.0)
    sd = {k: host(v) for k, v in actor.state_dict().items()}
    sd["mu.bias"] = np.array([40.0, -40.0, 0.1], F32)
    sd["latent_pi.0.bias"][:] = 0.0
    actor.load_state_dict(sd)
    obs_np = random_obs(rng, B, od)
    for k in obs_np:
        obs_np[k][4] = 0.0   # zero features, zero bias: the latent of row 4 is +0
    obs = {k: dev(v) for k, v in obs_np.items()}
    if unit == "gaussian":
        eps = rng.standard_normal((B, A)).astype(F32)
        run = Run(actor, obs, B, eps=dev(eps))
        check_against_host(unit, actor, run, obs_np, eps=eps)
    else:
        Eb = random_Eb(actor, rng)
        run = Run(actor, obs, B)
        check_against_host(unit, actor, run, obs_np, Eb=Eb)
        assert not bits(run.p["latent"][4]).any() and not bits(run.p["variance"][4]).any()
        # atanh(1 - EPS) = 8.3178 from two f32 log1p of magnitude 0.69 and 15.9: a few ulp of 16, 1e-6 relative
        assert np.allclose(np.abs(run.p["gaussian_action"][:, :2]), np.arctanh(1.0 - TANH_EPS), rtol=1e-5)
    assert (run.action[:, 0] == 1).all() and (run.action[:, 1] == -1).all() and (np.abs(run.action[:, 2]) < 1).all()
    assert np.isfinite(run.log_prob).all()
    actor.close()


# ------------------------------------------------------------------ 3. the noise
def expected_words(tag, seed, word, rows, blocks, per_row=True):
    e, q = np.meshgrid(np.arange(rows, dtype=np.uint64) if per_row else np.zeros(1, np.uint64),
                       np.arange(blocks, dtype=np.uint64), indexing="ij")
    c0 = np.full(e.shape, word & 0xFFFFFFFF, np.uint64)
    c1 = np.full(e.shape, word >> 32, np.uint64)
    return np.stack(H.philox4x32_10(c0, c1, e, np.uint64(tag) ^ q, seed & 0xFFFFFFFF, seed >> 32), axis=-1)


def box_muller(words, pairs, torch_f32=False):
    """eps in fp64 (or torch's f32 on the device) from words [..., 4]: (r0, r1), and with pairs = 2 (r2, r3)."""
    out = []
    for c in range(0, 2 * pairs, 2):
        u1 = ((words[..., c] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (words[..., c + 1] >> 8).astype(np.float64) * 2.0 ** -24
        if torch_f32:
            tu1, tu2 = dev(u1.astype(F32)), dev(u2.astype(F32))
            rad, ang = torch.sqrt(-2.0 * torch.log(tu1)), 6.2831855 * tu2
            out += [host(rad * torch.cos(ang)), host(rad * torch.sin(ang))]
        else:
            rad, ang = np.sqrt(-2.0 * np.log(u1)), float(F32(6.2831855)) * u2
            out += [rad * np.cos(ang), rad * np.sin(ang)]
    return np.stack(out, axis=-1).reshape(words.shape[0], -1)


def test_gaussian_noise_stream_and_its_word():
    rng = np.random.default_rng(13)
    B, N, A, seed, word0 = 257, 16, 7, (5 << 32) | 17, (3 << 32) | 9
    a = make("gaussian", 6, A, (32,), rng, n_envs=N, seed=seed)
    dbg = a.enable_debug()
    obs = {k: dev(v) for k, v in random_obs(rng, B, 6).items()}
    env_obs = {k: v[:N].contiguous() for k, v in obs.items()}
    # the rollout forward's draws, before anything else
    a.noise_step = 11
    a(env_obs)
    fwd_eps, fwd_act = host(dbg["eps"]).copy(), host(a.actions).copy()
    a.log_prob_noise_step = word0
    assert a.log_prob_noise_step == word0
    run = Run(a, obs, B)
    assert a.log_prob_noise_step == word0 + 1 and a.noise_step == 12
    want = expected_words(abi.ACTOR_LP_PHILOX_TAG, seed, word0, B, 4)
    assert np.array_equal(run.p["philox"].view(np.uint32), want)
    z = box_muller(want, 1)[:, :A]
    torch_err = float(np.abs(box_muller(want, 1, torch_f32=True)[:, :A].astype(np.float64) - z).max())
    err = float(np.abs(run.p["eps"].astype(np.float64) - z).max())
    print(f"log-prob stream Box-Muller: kernel max error {err:.3e}, torch f32 max error {torch_err:.3e}")
    assert err <= 2.0 * torch_err + float(np.spacing(F32(1.0)))
    check_gaussian_epilogue("device stream", run)
    # with io.eps the plane is the input bit for bit and the word stays
    eps = rng.standard_normal((B, A)).astype(F32)
    given = Run(a, obs, B, eps=dev(eps))
    assert np.array_equal(bits(given.p["eps"]), bits(eps)) and a.log_prob_noise_step == word0 + 1
    # every drawing launch moves the word on by one and draws anew; setting it back reproduces the draw
    second = Run(a, obs, B)
    assert a.log_prob_noise_step == word0 + 2 and not np.array_equal(bits(second.p["eps"]), bits(run.p["eps"]))
    a.log_prob_noise_step = word0
    again = Run(a, obs, B)
    assert np.array_equal(bits(again.p["eps"]), bits(run.p["eps"])) and np.array_equal(bits(again.log_prob), bits(run.log_prob))
    # the rollout forward's step word and draws are what they are without any of these calls
    assert a.noise_step == 12
    a.noise_step = 11
    a(env_obs)
    assert np.array_equal(bits(host(dbg["eps"])), bits(fwd_eps)) and np.array_equal(bits(host(a.actions)), bits(fwd_act))
    assert not np.array_equal(bits(fwd_eps), bits(run.p["eps"][:N]))   # another tag: another stream
    a.close()


def test_sde_batch_matrix_draw_and_the_untouched_per_env_side():
    rng = np.random.default_rng(17)
    N, Hd, A, seed, gen0 = 16, 30, 7, (5 << 32) | 17, (1 << 32) + 1   # H A = 210: 53 blocks, the last half used
    a = make("sde", 6, A, (32, Hd), rng, n_envs=N, seed=seed)
    dbg = a.enable_debug()
    obs = {k: dev(v) for k, v in random_obs(rng, N, 6).items()}
    a.noise_generation = 5
    a.reset_noise()
    E_env = host(a.exploration_matrices).copy()
    a(obs)
    fwd = {k: host(dbg[k]).copy() for k in ("mean", "latent", "noise")}
    fwd_act = host(a.actions).copy()
    std = host(a.std)
    a.batch_noise_generation = gen0
    assert a.batch_noise_generation == gen0
    blocks = (Hd * A + 3) // 4
    mats = []
    for g in (gen0, gen0 + 1):   # two generations
        eps_t = torch.zeros((Hd, A), dtype=torch.float32, device=DEV)
        a.reset_batch_noise(eps_out=eps_t)
        assert a.batch_noise_generation == g + 1
        want = expected_words(abi.SDE_BATCH_PHILOX_TAG, seed, g, 1, blocks, per_row=False)
        z = box_muller(want, 2)[:, :Hd * A]
        torch_err = float(np.abs(box_muller(want, 2, torch_f32=True)[:, :Hd * A].astype(np.float64) - z).max())
        eps = host(eps_t).reshape(1, Hd * A)
        err = float(np.abs(eps.astype(np.float64) - z).max())
        print(f"batch matrix draw Box-Muller: kernel max error {err:.3e}, torch f32 max error {torch_err:.3e}")
        assert err <= 2.0 * torch_err + float(np.spacing(F32(1.0)))
        Eb = host(a.exploration_mat)
        assert np.array_equal(bits(Eb), bits(eps.reshape(Hd, A) * std))   # one f32 multiply
        mats.append(Eb.copy())
    assert not np.array_equal(bits(mats[0]), bits(mats[1]))
    a.batch_noise_generation = gen0
    a.reset_batch_noise()
    assert np.array_equal(bits(host(a.exploration_mat)), bits(mats[0]))
    # the kernel reads that matrix: the noise plane is the host model's on it
    run = Run(a, obs, N)
    check_against_host("sde", a, run, {k: host(v) for k, v in obs.items()}, Eb=mats[0])
    # the per-env side: matrices, generation word and a following forward, bit for bit what they were
    assert a.noise_generation == 6 and np.array_equal(bits(host(a.exploration_matrices)), bits(E_env))
    a(obs)
    for k, v in fwd.items():
        assert np.array_equal(bits(host(dbg[k])), bits(v)), k
    assert np.array_equal(bits(host(a.actions)), bits(fwd_act))
    a.reset_noise()   # and the per-env resample leaves the shared matrix alone
    assert a.noise_generation == 7 and np.array_equal(bits(host(a.exploration_mat)), bits(mats[0]))
    a.close()


# ------------------------------------------------------------------ 4. the batch entry against the per-env forward
@pytest.mark.parametrize("arch", [(256, 256), (20, 300)], ids=["H256", "H300"])
def test_sde_batch_entry_against_the_per_env_forward(arch):
    """One SdeActor, 16 envs, every env's matrix equal to Eb, the same 16 observations: the mean planes are
    equal bit for bit; the noise planes too where H is a multiple of 16, and elsewhere but for a -0 sum, which
    the batch chain's +0 padding turns into +0 (include/pgx.h)."""
    rng = np.random.default_rng(19)
    N, od, A = 16, 19, 7
    a = make("sde", od, A, arch, rng, n_envs=N)
    dbg = a.enable_debug()
    Eb = random_Eb(a, rng)
    a.exploration_matrices = np.tile(Eb, (N, 1, 1))
    obs = {k: dev(v) for k, v in random_obs(rng, N, od).items()}
    act_env = host(a(obs)).copy()
    run = Run(a, obs, N)
    assert np.array_equal(bits(run.p["mean"]), bits(host(dbg["mean"])))
    assert np.array_equal(bits(run.p["latent"]), bits(host(dbg["latent"])))
    env_noise = host(dbg["noise"])
    if arch[-1] % 16 == 0:
        assert np.array_equal(bits(run.p["noise"]), bits(env_noise))
        assert np.array_equal(bits(run.action), bits(act_env))
    else:
        assert np.array_equal(bits(run.p["noise"]), bits(env_noise + F32(0.0)))   # -0 + +0 = +0, all else as it is
    assert (env_noise != 0).all()
    a.close()


# ------------------------------------------------------------------ 5. a HER batch in place, and the captured chain
def fill_ring(buf, rng, N, od, A, steps):
    for t in range(steps):
        done = (np.arange(N) % 4 == t % 4).astype(np.uint8)
        f = lambda *s: (rng.standard_normal((N,) + s) * 0.5).astype(F32)  # noqa: E731
        buf.add_tensors(f(od), f(3), f(3), f(A), f(), f(od), f(3), f(3), done)


@pytest.mark.parametrize("unit", UNITS)
def test_a_her_batch_read_in_place_equals_dense_copies(unit):
    rng = np.random.default_rng(11)
    N, od, A, B = 16, 6, 3, 64
    buf = pg.HerReplayBuffer(N * 8, device=DEV, n_envs=N, obs_dim=od, action_dim=A, seed=3)
    fill_ring(buf, rng, N, od, A, 26)
    b = buf.alloc_batch(B)
    buf.sample_into(b, draw=0)
    assert b["rows"].stride(0) == buf.row_stride > od and not b["next_obs"].is_contiguous()
    actor = make(unit, od, A, (96, 40), rng)
    eps = rng.standard_normal((B, A)).astype(F32)
    Eb = None if unit == "gaussian" else random_Eb(actor, rng)
    rows_before = b["rows"].clone()
    for nxt in (True, False):
        p = "next_" if nxt else ""
        views = {"observation": b[p + "obs"], "achieved_goal": b[p + "achieved_goal"], "desired_goal": b[p + "desired_goal"]}
        dense = {k: v.contiguous() for k, v in views.items()}
        if unit == "gaussian":   # (the rows entry draws from the stream: the same word for both calls)
            actor.log_prob_noise_step = 4
            act_r, lp_r = [host(t).copy() for t in actor.action_log_prob_rows(b, next=nxt)]
            actor.log_prob_noise_step = 4
            act_d, lp_d = [host(t).copy() for t in actor.action_log_prob(dense)]
            run = Run(actor, views, B, eps=dev(eps))
        else:
            act_r, lp_r = [host(t).copy() for t in actor.action_log_prob_rows(b, next=nxt)]
            act_d, lp_d = [host(t).copy() for t in actor.action_log_prob(dense)]
            run = Run(actor, views, B)
            assert np.array_equal(bits(run.action), bits(act_r)) and np.array_equal(bits(run.log_prob), bits(lp_r))
        assert np.isfinite(lp_r).all() and np.array_equal(bits(act_r), bits(act_d)) and np.array_equal(bits(lp_r), bits(lp_d))
        check_against_host(unit, actor, run, {k: host(v) for k, v in dense.items()}, eps=eps, Eb=Eb)
    assert torch.equal(b["rows"], rows_before)   # read only
    assert not torch.equal(b["obs"], b["next_obs"])
    actor.close()
    buf.close()


@pytest.mark.parametrize("unit", UNITS)
def test_captured_chain_equals_eager_and_the_host_target(unit):
    """sample_into -> action_log_prob_rows(out=) -> td_target_rows in one graph, replayed after the ring, the
    actor weights, Eb and ent_coef changed: every replay equals the eager chain, and the target is
    td_target_host on the kernel's own action / log_prob bit for bit."""
    rng = np.random.default_rng(23)
    N, od, A, B = 16, 6, 3, 64
    buf = pg.HerReplayBuffer(N * 8, device=DEV, n_envs=N, obs_dim=od, action_dim=A, seed=3)
    fill_ring(buf, rng, N, od, A, 13)
    actor = make(unit, od, A, (96, 40), rng)
    qc, _ = make_qc(od, A, (96, 40), 2, 25, drop=2, device=DEV, seed=23)
    if unit == "sde":
        actor.reset_batch_noise()
    b = buf.alloc_batch(B)
    act = torch.zeros((B, A), dtype=torch.float32, device=DEV)
    lp = torch.zeros((B,), dtype=torch.float32, device=DEV)
    ent = dev(np.array([0.2], F32))
    flat, target = guarded(B, qc.n_target)

    def chain():
        buf.sample_into(b, draw=0)
        actor.action_log_prob_rows(b, out=(act, lp))
        qc.td_target_rows(b, act, lp, ent, out=target)

    def snapshot():
        torch.cuda.synchronize()
        return [host(t).copy() for t in (b["rows"], act, lp, target)]

    chain()
    first = snapshot()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    fill_ring(buf, rng, N, od, A, 9)   # another batch behind the same draw
    sd = random_sde_state_dict(actor, rng) if unit == "sde" else \
        {k: (host(v) * F32(0.7)).astype(F32) for k, v in actor.state_dict().items()}
    actor.load_state_dict(sd)
    if unit == "sde":
        actor.reset_batch_noise()
    ent.fill_(0.55)
    word = actor.log_prob_noise_step if unit == "gaussian" else None
    g.replay()
    replayed = snapshot()
    assert not np.array_equal(replayed[0], first[0]) and not np.array_equal(replayed[3], first[3])
    if unit == "gaussian":
        assert actor.log_prob_noise_step == word + 1
        actor.log_prob_noise_step = word   # the eager chain draws what the replay drew
    chain()
    eager = snapshot()
    for x, y in zip(replayed, eager):
        assert np.array_equal(bits(x), bits(y))
    nxt = {"observation": host(b["next_obs"]), "achieved_goal": host(b["next_achieved_goal"]),
           "desired_goal": host(b["next_desired_goal"])}
    want = qc.td_target_host(nxt, replayed[1], replayed[2], host(b["reward"]), host(b["done"]), host(ent))
    assert np.isfinite(replayed[2]).all() and np.array_equal(bits(replayed[3]), bits(want)) and canaries_intact(flat)
    if unit == "gaussian":   # two replays draw different eps
        g.replay()
        again = snapshot()
        assert np.array_equal(bits(again[0]), bits(replayed[0])) and not np.array_equal(bits(again[1]), bits(replayed[1]))
        assert actor.log_prob_noise_step == word + 2
    for x in (actor, qc, buf):
        x.close()


# ------------------------------------------------------------------ 6. containment
@pytest.mark.parametrize("unit", UNITS)
def test_a_nan_row_disturbs_no_other_row(unit):
    rng = np.random.default_rng(29)
    B, od, A = 33, 6, 3
    actor = make(unit, od, A, (96, 40), rng)
    obs_np = random_obs(rng, B, od)
    eps = rng.standard_normal((B, A)).astype(F32)
    kw = (lambda: {"eps": dev(eps)}) if unit == "gaussian" else (lambda: {})
    if unit == "sde":
        random_Eb(actor, rng)
    clean = Run(actor, {k: dev(v) for k, v in obs_np.items()}, B, **kw())
    obs_np["achieved_goal"][10, 1] = np.nan
    eps[5, 0] = np.nan
    run = Run(actor, {k: dev(v) for k, v in obs_np.items()}, B, **kw())
    others = np.ones(B, bool)
    others[[5, 10] if unit == "gaussian" else [10]] = False
    assert np.array_equal(bits(run.action[others]), bits(clean.action[others]))
    assert np.array_equal(bits(run.log_prob[others]), bits(clean.log_prob[others]))
    for k in clean.p:
        assert np.array_equal(run.p[k][others].view(np.uint32), clean.p[k][others].view(np.uint32)), k
    assert run.contained() and not (run.action == CANARY).any() and not (run.log_prob == CANARY).any()
    if unit == "gaussian":
        assert np.isnan(run.log_prob[5])
    actor.close()


def test_device_entries_refuse_bad_launches_and_launch_nothing():
    rng = np.random.default_rng(31)
    B, od, A = 4, 6, 3
    g, s = make("gaussian", od, A, (16,), rng), make("sde", od, A, (16,), rng)
    d = pg.Actor(obs_dim=od, action_dim=A, n_envs=1, net_arch=(16,), kind="deterministic", device=DEV)
    t = {k: torch.zeros(shape, dtype=torch.float32, device=DEV) for k, shape in
         {"obs": (B, od), "achieved_goal": (B, 3), "desired_goal": (B, 3)}.items()}
    fa, act = guarded(B, A)
    fl, lp = guarded(B, 0)

    def io(cls, **over):
        x = cls()
        for k, v in t.items():
            setattr(x, k, v.data_ptr())
        x.action, x.log_prob = act.data_ptr(), lp.data_ptr()
        x.obs_stride, x.achieved_goal_stride, x.desired_goal_stride = od, 3, 3
        for k, v in over.items():
            setattr(x, k, v)
        return x

    bad = [({"obs_stride": od - 1}, B, b"obs_stride"), ({}, 0, b"B must be > 0"), ({"log_prob": None}, B, b"null log_prob"),
           ({"desired_goal": None}, B, b"null desired_goal"), ({"achieved_goal_stride": 2}, B, b"achieved_goal_stride")]
    for actor, cls, fn, name in ((g, abi.PgxActorLpIo, g.lib.pgx_actor_action_log_prob, b"pgx_actor_action_log_prob"),
                                 (s, abi.PgxSdeActorLpIo, s.lib.pgx_sde_actor_action_log_prob, b"pgx_sde_actor_action_log_prob")):
        for over, n, word in bad:
            assert fn(actor._h, C.byref(io(cls, **over)), n, actor._stream()) == abi.PGX_E_INVALID
            assert name in actor.lib.pgx_last_error() and word in actor.lib.pgx_last_error()
    assert g.lib.pgx_actor_action_log_prob(d._h, C.byref(io(abi.PgxActorLpIo)), B, d._stream()) == abi.PGX_E_INVALID
    assert b"kind" in g.lib.pgx_last_error() and b"DETERMINISTIC" in g.lib.pgx_last_error()
    with pytest.raises(pg.PgxError, match="kind"):
        d.action_log_prob({"observation": t["obs"], "achieved_goal": t["achieved_goal"], "desired_goal": t["desired_goal"]})
    word = g.log_prob_noise_step
    torch.cuda.synchronize()
    assert (host(fa) == CANARY).all() and (host(fl) == CANARY).all()   # nothing was launched
    assert g.log_prob_noise_step == word
    assert g.lib.pgx_actor_action_log_prob(g._h, C.byref(io(abi.PgxActorLpIo)), B, g._stream()) == abi.PGX_OK
    torch.cuda.synchronize()
    assert canaries_intact(fa) and canaries_intact(fl) and np.isfinite(host(lp)).all() and g.log_prob_noise_step == word + 1
    with pytest.raises(ValueError, match="out must be"):
        g.action_log_prob({"observation": t["obs"], "achieved_goal": t["achieved_goal"], "desired_goal": t["desired_goal"]},
                          out=(act[:, :2], lp))
    # the planes enable_log_prob_debug allocates are what the next launch of that many rows fills
    obs = {"observation": t["obs"], "achieved_goal": t["achieved_goal"], "desired_goal": t["desired_goal"]}
    for actor, keys in ((g, ["mean", "log_std", "eps", "gaussian_action", "philox"]),
                        (s, ["mean", "latent", "noise", "variance", "gaussian_action"])):
        planes = actor.enable_log_prob_debug(B)
        assert list(planes) == keys and all(p.shape[0] == B for p in planes.values())
        a_out, lp_out = actor.action_log_prob(obs)
        want = actor.log_prob_host({k: host(v) for k, v in obs.items()},
                                   host(planes["eps"]) if actor is g else host(actor.exploration_mat))
        assert np.array_equal(bits(host(planes["mean"])), bits(want["mean"])) and np.isfinite(host(lp_out)).all()
        with pytest.raises(ValueError, match="debug planes"):
            actor.action_log_prob({k: torch.cat([v, v]) for k, v in obs.items()})
        assert actor.enable_log_prob_debug(None) == {}
        assert tuple(actor.action_log_prob({k: torch.cat([v, v]) for k, v in obs.items()})[0].shape) == (2 * B, A)
    for x in (g, s, d):
        x.close()
