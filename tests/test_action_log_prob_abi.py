"""The action log-probability entries of the Actor and the SdeActor (include/pgx.h, pgx_actor_action_log_prob /
pgx_sde_actor_action_log_prob) without a GPU: the ctypes mirrors of the two IO structs against the header's
layout through gcc, the exported entry points, every refusal of the launch checks (one function per unit,
shared by the device entry and its host model, reached here through the host models; each names its field),
the host models' Linear-chain planes against a numpy + libm-fmaf restatement bit for bit, their transcendental
epilogue against an fp64 evaluation of the same expression from the host model's own f32 planes, and the
Python surface."""
import ctypes as C
import inspect

import numpy as np
import pytest

import panda_gym_amd as pg
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi
from test_actor_abi import bits, chain, random_obs, random_state_dict
from test_actor_abi import restated_forward as restated_gaussian
from test_sde_actor_abi import random_sde_state_dict
from test_sde_actor_abi import restated_forward as restated_sde

F32 = np.float32
LP_EXPORTS = ["pgx_actor_action_log_prob", "pgx_actor_lp_state", "pgx_actor_lp_set_state", "pgx_actor_log_prob_host",
              "pgx_sde_actor_action_log_prob", "pgx_sde_actor_reset_batch_noise", "pgx_sde_actor_get_batch_matrix",
              "pgx_sde_actor_set_batch_matrix", "pgx_sde_actor_batch_state", "pgx_sde_actor_batch_set_state",
              "pgx_sde_actor_log_prob_host"]
HALF_LOG_2PI = float(F32(0.9189385))
TANH_EPS = float(F32(1.1920929e-7))


# ---------------------------------------------------------------- helpers shared with the GPU tests
def fp64_gaussian(mean, log_std, eps, action=None):
    """(action [n, A], log_prob [n]) in fp64 by the header's lines from f32 planes; with the f32 ``action``
    plane the correction term is taken from it (SB3: log(1 - actions**2 + epsilon) reads the actions)."""
    m, ls, e = (np.asarray(x, F32).astype(np.float64) for x in (mean, log_std, eps))
    std = np.exp(ls)
    g = std * e + m
    a = np.tanh(g)
    z = g - m
    lp = -(z * z) / (2.0 * std * std) - ls - HALF_LOG_2PI
    t = a if action is None else np.asarray(action, F32).astype(np.float64)
    c = np.log((1.0 - t * t) + float(F32(1e-6)))
    return a, lp.sum(1) - c.sum(1)


def fp64_sde_action(mean, noise):
    return np.tanh(np.asarray(mean, F32).astype(np.float64) + np.asarray(noise, F32).astype(np.float64))


def fp64_sde_log_prob(action, mean, variance):
    """log_prob [n] in fp64 by the header's lines from the f32 action (what SB3's gSDE path inverts), mean and
    variance planes; also g' [n, A]."""
    a, m, v = (np.asarray(x, F32).astype(np.float64) for x in (action, mean, variance))
    scale = np.sqrt(v + float(F32(1e-6)))
    lim = 1.0 - TANH_EPS
    x = np.clip(a, -lim, lim)
    g = 0.5 * (np.log1p(x) - np.log1p(-x))
    z = g - m
    lp = -(z * z) / (2.0 * scale * scale) - np.log(scale) - HALF_LOG_2PI
    t = np.tanh(g)
    c = np.log((1.0 - t * t) + float(F32(1e-6)))
    return lp.sum(1) - c.sum(1), g


def f32_gaussian(mean, log_std, eps):
    """The same lines evaluated in numpy f32, as SB3 writes them: the margin's yardstick on a CPU."""
    m, ls, e = (np.asarray(x, F32) for x in (mean, log_std, eps))
    std = np.exp(ls)
    g = m + std * e
    a = np.tanh(g)
    lp = -((g - m) ** 2) / (2 * std * std) - ls - F32(0.9189385)
    return a, lp.sum(1, dtype=F32) - np.log(F32(1.0) - a * a + F32(1e-6)).sum(1, dtype=F32)


def f32_sde_log_prob(action, mean, variance):
    a, m, v = (np.asarray(x, F32) for x in (action, mean, variance))
    scale = np.sqrt(v + F32(1e-6))
    lim = F32(1.0) - F32(1.1920929e-7)
    x = np.clip(a, -lim, lim)
    g = F32(0.5) * (np.log1p(x) - np.log1p(-x))
    lp = -((g - m) ** 2) / (2 * scale * scale) - np.log(scale) - F32(0.9189385)
    t = np.tanh(g)
    return lp.sum(1, dtype=F32) - np.log(F32(1.0) - t * t + F32(1e-6)).sum(1, dtype=F32)


def within_margin(what, got, want, yardstick):
    """The project's margin (check_against_fp64 of test_gpu_actor_critic.py): twice the largest error of an f32
    evaluation of the same lines, plus one ulp of the result's magnitude."""
    ref_err = float(np.abs(np.asarray(yardstick).astype(np.float64) - want).max())
    err = float(np.abs(np.asarray(got).astype(np.float64) - want).max())
    ulp = float(np.spacing(F32(np.abs(want).max())))
    print(f"{what}: max error {err:.3e}, f32 restatement max error {ref_err:.3e}, one ulp {ulp:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= 2.0 * ref_err + ulp, what


def padded_chain(x, col):
    """The Linear chain with bias +0 over x against one column, K rounded up to 16."""
    return chain(x, col, 0.0)


def restated_noise_and_variance(latent, Eb, std):
    """noise, variance [n, A] f32 by the header's contract, one libm fmaf at a time."""
    latent, Eb, std = np.asarray(latent, F32), np.asarray(Eb, F32), np.asarray(std, F32)
    std2 = (std * std).astype(F32)
    sq = (latent * latent).astype(F32)
    n, A = latent.shape[0], Eb.shape[1]
    noise, var = np.zeros((n, A), F32), np.zeros((n, A), F32)
    for b in range(n):
        for a in range(A):
            noise[b, a] = padded_chain(latent[b], Eb[:, a])
            var[b, a] = padded_chain(sq[b], std2[:, a])
    return noise, var


def make_gaussian(od, A, arch, rng, device="cpu", n_envs=1, **kw):
    a = pg.Actor(obs_dim=od, action_dim=A, n_envs=n_envs, net_arch=arch, kind="gaussian", device=device, **kw)
    sd = random_state_dict(a, rng)
    a.load_state_dict(sd)
    return a, sd


def make_sde(od, A, arch, rng, device="cpu", n_envs=1, **kw):
    a = pg.SdeActor(obs_dim=od, action_dim=A, n_envs=n_envs, net_arch=arch, device=device, **kw)
    sd = random_sde_state_dict(a, rng)
    a.load_state_dict(sd)
    return a, sd


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    structs = {"pgx_actor_lp_io": abi.PgxActorLpIo, "pgx_sde_actor_lp_io": abi.PgxSdeActorLpIo}
    out = header_layout(structs, ['printf("tags %u %u %u\\n", PGX_ACTOR_LP_PHILOX_TAG, PGX_SDE_BATCH_PHILOX_TAG, '
                                  'PGX_SDE_PHILOX_TAG);'])
    assert out["tags"] == f"{abi.ACTOR_LP_PHILOX_TAG} {abi.SDE_BATCH_PHILOX_TAG} {abi.SDE_PHILOX_TAG}"
    # the counter tags of the five streams are disjoint over every block they are xored with
    spans = [{abi.ACTOR_PHILOX_TAG ^ p for p in range(4)}, {abi.ACTOR_LP_PHILOX_TAG ^ p for p in range(4)},
             {abi.AC_PHILOX_TAG ^ p for p in range(4)}, {abi.SDE_PHILOX_TAG ^ q for q in range(1024)},
             {abi.SDE_BATCH_PHILOX_TAG ^ q for q in range(1024)}]
    assert len(set().union(*spans)) == sum(len(s) for s in spans)


def test_library_exports_the_entry_points():
    assert_exported(LP_EXPORTS)


def _gaussian_call(n=3, kind=abi.ACTOR_GAUSSIAN):
    cfg = abi.PgxActorConfig()
    cfg.n_envs, cfg.obs_dim, cfg.action_dim, cfg.n_layers, cfg.kind = 1, 6, 3, 1, kind
    cfg.hidden[0] = 16
    rng = np.random.default_rng(0)
    w, keep = abi.PgxActorWeights(), []
    for i, shape in enumerate([(16, 12), (3, 16), (3, 16)]):
        W, b = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape[0]).astype(F32)
        w.weight[i], w.bias[i] = W.ctypes.data, b.ctypes.data
        keep += [W, b]
    io = abi.PgxActorLpIo()
    for k, shape in {"obs": (n, 6), "achieved_goal": (n, 3), "desired_goal": (n, 3), "eps": (n, 3), "action": (n, 3),
                     "log_prob": (n,)}.items():
        a = np.zeros(shape, F32)
        setattr(io, k, a.ctypes.data)
        keep.append(a)
    io.obs_stride, io.achieved_goal_stride, io.desired_goal_stride = 6, 3, 3
    lib = _native.load()
    return (lambda n_=n: lib.pgx_actor_log_prob_host(C.byref(cfg), C.byref(w), C.byref(io), n_)), io, keep


def _sde_call(n=3):
    cfg = abi.PgxSdeActorConfig()
    cfg.n_envs, cfg.obs_dim, cfg.action_dim, cfg.n_layers, cfg.clip_mean = 1, 6, 3, 1, 2.0
    cfg.hidden[0] = 16
    rng = np.random.default_rng(0)
    w, keep = abi.PgxSdeActorWeights(), []
    for i, shape in enumerate([(16, 12), (3, 16)]):
        W, b = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape[0]).astype(F32)
        w.weight[i], w.bias[i] = W.ctypes.data, b.ctypes.data
        keep += [W, b]
    ls, Eb = np.full((16, 3), -3.0, F32), np.zeros((16, 3), F32)
    w.log_std = ls.ctypes.data
    io = abi.PgxSdeActorLpIo()
    for k, shape in {"obs": (n, 6), "achieved_goal": (n, 3), "desired_goal": (n, 3), "action": (n, 3),
                     "log_prob": (n,)}.items():
        a = np.zeros(shape, F32)
        setattr(io, k, a.ctypes.data)
        keep.append(a)
    io.obs_stride, io.achieved_goal_stride, io.desired_goal_stride = 6, 3, 3
    lib = _native.load()
    call = lambda n_=n, mat=Eb: lib.pgx_sde_actor_log_prob_host(  # noqa: E731
        C.byref(cfg), C.byref(w), None, None if mat is None else mat.ctypes.data, C.byref(io), n_)
    return call, io, keep + [ls, Eb]


BAD_LAUNCH = [("obs", None, b"null obs"), ("achieved_goal", None, b"null achieved_goal"),
              ("desired_goal", None, b"null desired_goal"), ("action", None, b"null action"),
              ("log_prob", None, b"null log_prob"), ("B", 0, b"B must be > 0"), ("B", -2, b"B must be > 0"),
              ("obs_stride", 5, b"obs_stride"), ("achieved_goal_stride", 2, b"achieved_goal_stride"),
              ("desired_goal_stride", 0, b"desired_goal_stride")]


@pytest.mark.parametrize("unit", ["gaussian", "sde"])
@pytest.mark.parametrize("field,value,words", BAD_LAUNCH, ids=[f"{b[0]}={b[1]}" for b in BAD_LAUNCH])
def test_launch_checks_refuse_without_a_device(unit, field, value, words):
    """pgx_actor_lp_check_launch / pgx_sde_actor_lp_check_launch, the one function per unit that the device
    entry and the host model call in front of anything else: every refusal names its field; the valid call
    passes."""
    lib = _native.load()
    call, io, keep = _gaussian_call() if unit == "gaussian" else _sde_call()
    assert call() == abi.PGX_OK, lib.pgx_last_error()
    if field == "B":
        rc = call(value)
    else:
        setattr(io, field, value)
        rc = call()
    assert rc == abi.PGX_E_INVALID
    msg = lib.pgx_last_error()
    entry = b"pgx_actor_log_prob_host" if unit == "gaussian" else b"pgx_sde_actor_log_prob_host"
    assert entry in msg and words in msg, msg


def test_deterministic_kind_null_io_and_host_only_refusals():
    lib = _native.load()
    call, io, keep = _gaussian_call(kind=abi.ACTOR_DETERMINISTIC)
    assert call() == abi.PGX_E_INVALID
    msg = lib.pgx_last_error()
    assert b"pgx_actor_log_prob_host" in msg and b"kind" in msg and b"DETERMINISTIC" in msg, msg
    call, io, keep = _gaussian_call()
    io.eps = None   # the host model has no stream
    assert call() == abi.PGX_E_INVALID and b"null eps" in lib.pgx_last_error()
    call, io, keep = _sde_call()
    assert call(mat=None) == abi.PGX_E_INVALID and b"null exploration_mat" in lib.pgx_last_error()
    # null handles and io, at the device entries, before any device call
    gio, sio = abi.PgxActorLpIo(), abi.PgxSdeActorLpIo()
    word = C.c_uint64(0)
    for rc in (lib.pgx_actor_action_log_prob(None, C.byref(gio), 4, None), lib.pgx_actor_lp_state(None, C.byref(word), None),
               lib.pgx_actor_lp_set_state(None, 0, None), lib.pgx_sde_actor_action_log_prob(None, C.byref(sio), 4, None),
               lib.pgx_sde_actor_reset_batch_noise(None, None, None), lib.pgx_sde_actor_get_batch_matrix(None, None, None),
               lib.pgx_sde_actor_set_batch_matrix(None, None, None),
               lib.pgx_sde_actor_batch_state(None, C.byref(word), None), lib.pgx_sde_actor_batch_set_state(None, 0, None)):
        assert rc == abi.PGX_E_INVALID
        assert b"null" in lib.pgx_last_error()


# ---------------------------------------------------------------- the chain planes, bit for bit
# obs_dim (K = obs_dim + 6: 15, 16, 29), net_arch (H = 16, 20, 256, 300), A, rows
SHAPES = [(9, (16,), 1, 1), (10, (300, 20), 3, 17), (23, (256, 256), 7, 1), (9, (20, 300), 4, 17), (10, (16,), 7, 17)]
IDS = [f"K{s[0] + 6}-{'x'.join(map(str, s[1]))}-A{s[2]}-n{s[3]}" for s in SHAPES]


@pytest.mark.parametrize("od,arch,A,n", SHAPES, ids=IDS)
def test_gaussian_host_model_equals_the_restatement_and_fp64(od, arch, A, n):
    rng = np.random.default_rng(od * 100 + A)
    a, sd = make_gaussian(od, A, arch, rng, clip_mean=1.5)
    obs, eps = random_obs(rng, n, od), rng.standard_normal((n, A)).astype(F32)
    got = a.log_prob_host(obs, eps)
    mean, log_std = restated_gaussian(a, sd, obs)
    assert np.array_equal(bits(got["mean"]), bits(mean)) and np.array_equal(bits(got["log_std"]), bits(log_std))
    assert np.array_equal(bits(got["eps"]), bits(eps))
    m2, ls2 = a.forward_host(obs)   # the forward's planes, word for word
    assert np.array_equal(bits(got["mean"]), bits(m2)) and np.array_equal(bits(got["log_std"]), bits(ls2))
    want_a, want_lp = fp64_gaussian(got["mean"], got["log_std"], eps, got["action"])
    ref_a, ref_lp = f32_gaussian(got["mean"], got["log_std"], eps)
    within_margin("gaussian action", got["action"], want_a, ref_a)
    within_margin("gaussian log_prob", got["log_prob"], want_lp, ref_lp)
    g64 = np.exp(got["log_std"].astype(np.float64)) * eps + got["mean"]
    within_margin("gaussian_action", got["gaussian_action"], g64, got["mean"] + np.exp(got["log_std"]) * eps)
    assert got["action"].shape == (n, A) and got["log_prob"].shape == (n,)


@pytest.mark.parametrize("od,arch,A,n", SHAPES, ids=IDS)
def test_sde_host_model_equals_the_restatement_and_fp64(od, arch, A, n):
    rng = np.random.default_rng(od * 100 + A + 1)
    a, sd = make_sde(od, A, arch, rng, log_std_init=-1.0)
    H = arch[-1]
    obs = random_obs(rng, n, od)
    std = np.exp(sd["log_std"]).astype(F32)
    Eb = (rng.standard_normal((H, A)).astype(F32) * std).astype(F32)
    got = a.log_prob_host(obs, Eb, std=std)
    mean, latent, _ = restated_sde(a, sd, obs, np.zeros((n, H, A), F32))
    noise, var = restated_noise_and_variance(latent, Eb, std)
    for k, want in (("mean", mean), ("latent", latent), ("noise", noise), ("variance", var)):
        assert np.array_equal(bits(got[k]), bits(want)), k
    assert (got["variance"] > 0).all() and (got["noise"] != 0).any()
    within_margin("gSDE action", got["action"], fp64_sde_action(got["mean"], got["noise"]), np.tanh(got["mean"] + got["noise"]))
    want_lp, want_g = fp64_sde_log_prob(got["action"], got["mean"], got["variance"])
    within_margin("gSDE log_prob", got["log_prob"], want_lp, f32_sde_log_prob(got["action"], got["mean"], got["variance"]))
    x = np.clip(got["action"], F32(-1) + F32(TANH_EPS), F32(1) - F32(TANH_EPS))
    within_margin("gSDE gaussian_action", got["gaussian_action"], want_g, F32(0.5) * (np.log1p(x) - np.log1p(-x)))
    # std = None on a CPU actor: the host libm's exp(log_std) (within an ulp or two of numpy's: std2 within 1e-6
    # relative, every term of the chain positive, so the sum within 1e-5 relative with room)
    got2 = a.log_prob_host(obs, Eb)
    assert np.array_equal(bits(got2["noise"]), bits(noise)) and np.allclose(got2["variance"], var, rtol=1e-5)


def test_sde_noise_and_variance_with_negative_zero_subnormals_and_a_zero_column():
    rng = np.random.default_rng(9)
    od, A, arch, n = 9, 4, (20,), 17
    a, sd = make_sde(od, A, arch, rng)
    H = arch[-1]
    sd["latent_pi.0.bias"][:] = 0.0
    a.load_state_dict(sd)
    obs = random_obs(rng, n, od)
    for k in obs:
        obs[k][5] = (rng.standard_normal(obs[k].shape[1]) * 1e-39).astype(F32)   # a subnormal latent
        obs[k][6] = 0.0                                                           # an all-zero latent
    log_std = (-3.0 + 0.5 * rng.standard_normal((H, A))).astype(F32)
    log_std[::4, 0] = F32(-0.0)     # std = 1
    log_std[1::4, 1] = F32(1e-40)   # subnormal: std = 1
    log_std[:, 2] = F32(-200.0)     # a zero column of std
    log_std[2::4, 3] = F32(-50.0)   # std2 = exp(-100): subnormal
    std = np.exp(log_std).astype(F32)
    assert not std[:, 2].any() and (std[::4, 0] == 1).all()
    Eb = (rng.standard_normal((H, A)) * 0.05).astype(F32)
    Eb[::3, 0] = F32(-0.0)
    Eb[1::3, 1] = F32(2e-40)
    Eb[:, 2] = F32(0.0)
    Eb[:, 3] = F32(-0.0)            # a whole column of -0: the padded chain from +0 ends at +0
    got = a.log_prob_host(obs, Eb, std=std)
    _, latent, _ = restated_sde(a, sd, obs, np.zeros((n, H, A), F32))
    noise, var = restated_noise_and_variance(latent, Eb, std)
    assert np.array_equal(bits(got["latent"]), bits(latent))
    assert np.array_equal(bits(got["noise"]), bits(noise)) and np.array_equal(bits(got["variance"]), bits(var))
    lat5 = latent[5][latent[5] != 0]
    assert lat5.size and (np.abs(lat5) < np.finfo(F32).tiny).all() and not latent[6].any()
    assert not bits(got["noise"][:, 2:]).any() and not bits(got["variance"][:, 2]).any()   # +0
    assert not bits(got["variance"][6]).any() and np.isfinite(got["log_prob"]).all()
    # var = 0: scale = sqrt(1e-6)
    want_lp, _ = fp64_sde_log_prob(got["action"], got["mean"], got["variance"])
    within_margin("gSDE log_prob (zero variance)", got["log_prob"], want_lp,
                  f32_sde_log_prob(got["action"], got["mean"], got["variance"]))


def test_saturated_rows_stay_finite():
    """A mean far outside the box: tanhf gives exactly +-1 and the 1e-6 / 1 - EPS guards carry the result."""
    rng = np.random.default_rng(3)
    n, A = 5, 3
    a, sd = make_gaussian(9, A, (16,), rng)
    sd["mu.bias"] = np.array([40.0, -40.0, 0.1], F32)
    a.load_state_dict(sd)
    obs, eps = random_obs(rng, n, 9), rng.standard_normal((n, A)).astype(F32)
    got = a.log_prob_host(obs, eps)
    assert (got["action"][:, 0] == 1).all() and (got["action"][:, 1] == -1).all() and np.isfinite(got["log_prob"]).all()
    want_a, want_lp = fp64_gaussian(got["mean"], got["log_std"], eps, got["action"])
    within_margin("saturated gaussian log_prob", got["log_prob"], want_lp, f32_gaussian(got["mean"], got["log_std"], eps)[1])
    s, ssd = make_sde(9, A, (16,), rng, clip_mean=0.0)
    ssd["mu.bias"] = np.array([40.0, -40.0, 0.1], F32)
    s.load_state_dict(ssd)
    got = s.log_prob_host(obs, np.zeros((16, A), F32))
    assert (got["action"][:, 0] == 1).all() and (got["action"][:, 1] == -1).all() and np.isfinite(got["log_prob"]).all()
    want_lp, want_g = fp64_sde_log_prob(got["action"], got["mean"], got["variance"])
    within_margin("saturated gSDE log_prob", got["log_prob"], want_lp,
                  f32_sde_log_prob(got["action"], got["mean"], got["variance"]))
    # atanh(1 - EPS) = 8.3178 from two f32 log1p of magnitude 0.69 and 15.9: a few ulp of 16, 1e-6 relative
    assert np.allclose(np.abs(got["gaussian_action"][:, :2]), np.arctanh(1.0 - TANH_EPS), rtol=1e-5)


# ---------------------------------------------------------------- the Python surface
def test_python_surface_and_unchanged_state_dicts():
    rng = np.random.default_rng(4)
    a, sd = make_gaussian(6, 3, (16, 8), rng)
    assert list(a.state_dict()) == [f"{n}.{p}" for n in ("latent_pi.0", "latent_pi.2", "mu", "log_std")
                                    for p in ("weight", "bias")]
    for k, v in a.state_dict().items():
        assert np.array_equal(bits(v.numpy()), bits(sd[k])), k
    s, ssd = make_sde(6, 3, (16, 8), rng)
    assert list(s.state_dict()) == ["latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias",
                                    "mu.0.weight", "mu.0.bias", "log_std"]
    for k, v in s.state_dict().items():
        assert np.array_equal(bits(v.numpy()), bits(ssd[k])), k
    assert list(inspect.signature(pg.Actor.action_log_prob).parameters)[1:] == ["obs", "eps", "out"]
    assert list(inspect.signature(pg.Actor.action_log_prob_rows).parameters)[1:] == ["batch", "next", "out"]
    assert list(inspect.signature(pg.SdeActor.action_log_prob).parameters)[1:] == ["obs", "out"]
    assert list(inspect.signature(pg.SdeActor.action_log_prob_rows).parameters)[1:] == ["batch", "next", "out"]
    assert inspect.signature(pg.Actor.action_log_prob_rows).parameters["next"].default is True
    for name in ("log_prob_noise_step", "log_prob_host"):
        assert hasattr(pg.Actor, name), name
    for name in ("reset_batch_noise", "exploration_mat", "batch_noise_generation", "log_prob_host"):
        assert hasattr(pg.SdeActor, name), name
    obs = random_obs(rng, 4, 6)
    # device only: no CPU fallback, the shared matrix has no host slot
    for call in (lambda: a.action_log_prob(obs), lambda: a.log_prob_noise_step, lambda: s.action_log_prob(obs),
                 s.reset_batch_noise, lambda: s.exploration_mat, lambda: s.batch_noise_generation,
                 lambda: setattr(s, "exploration_mat", np.zeros((8, 3), F32))):
        with pytest.raises(pg.PgxError, match="no CPU fallback"):
            call()
    d = pg.Actor(obs_dim=6, action_dim=3, n_envs=1, net_arch=(16,), kind="deterministic", device="cpu")
    with pytest.raises(pg.PgxError, match="kind"):
        d.log_prob_host(obs, np.zeros((4, 3), F32))
    with pytest.raises(ValueError, match="eps"):
        a.log_prob_host(obs, np.zeros((4, 2), F32))
    with pytest.raises(ValueError, match="exploration_mat"):
        s.log_prob_host(obs, np.zeros((3, 8), F32))
