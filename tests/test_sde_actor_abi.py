"""The SdeActor C-ABI (include/pgx.h, pgx_sde_actor_*) without a GPU: the ctypes mirrors against the
header's layout through gcc, the exported entry points, the argument checks (made before any device call),
the Python surface, SB3's gSDE state-dict key names, and the arithmetic contract: the library's host model
(pgx_sde_actor_forward_host) against an independent restatement written from the header's rules -- libm's
fmaf through ctypes; the trunk and mu as the Actor's chain (bias first, k ascending, K rounded up to 16);
the noise as ONE chain from +0 over exactly H terms, h ascending -- bit for bit."""
import ctypes as C
import inspect

import numpy as np
import pytest

import panda_gym_amd as pg
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi
from test_actor_abi import bits, chain, features, fmaf, random_obs

F32 = np.float32
SDE_EXPORTS = ["pgx_sde_actor_create", "pgx_sde_actor_destroy", "pgx_sde_actor_set_weights", "pgx_sde_actor_reset_noise",
               "pgx_sde_actor_forward", "pgx_sde_actor_state", "pgx_sde_actor_set_state", "pgx_sde_actor_get_matrices",
               "pgx_sde_actor_set_matrices", "pgx_sde_actor_get_std", "pgx_sde_actor_forward_host"]


# ---------------------------------------------------------------- helpers shared with the GPU tests
def random_sde_state_dict(actor, rng, scale=1.0):
    """standard_normal / sqrt(fan_in) weights (biases / 2) under the actor's own key names; log_std around
    log_std_init."""
    sd = {}
    for k, v in actor.state_dict().items():
        shape = tuple(v.shape)
        if k == "log_std":
            sd[k] = (actor.log_std_init + 0.5 * rng.standard_normal(shape)).astype(F32)
        else:
            s = scale / np.sqrt(shape[1]) if len(shape) == 2 else 0.5 * scale
            sd[k] = (rng.standard_normal(shape) * s).astype(F32)
    return sd


def mu_name(actor):
    return "mu.0" if actor.clip_mean > 0 else "mu"


def restated_forward(actor, sd, obs, matrices):
    """mean [n, A], latent [n, H], noise [n, A] f32 by the header's contract, one libm fmaf at a time."""
    nl = len(actor.net_arch)
    names = [f"latent_pi.{2 * i}" for i in range(nl)]
    trunk = [(np.asarray(sd[f"{n}.weight"], F32), np.asarray(sd[f"{n}.bias"], F32)) for n in names]
    Wm, bm = np.asarray(sd[f"{mu_name(actor)}.weight"], F32), np.asarray(sd[f"{mu_name(actor)}.bias"], F32)
    x = features(obs)
    n, A, H = x.shape[0], actor.action_dim, actor.net_arch[-1]
    mean, latent, noise = np.zeros((n, A), F32), np.zeros((n, H), F32), np.zeros((n, A), F32)
    E = np.asarray(matrices, F32)
    for e in range(n):
        h = x[e]
        for W, b in trunk:
            y = np.array([chain(h, W[o], b[o]) for o in range(W.shape[0])], F32)
            h = np.where(y > 0, y, F32(0.0)).astype(F32)
        latent[e] = h
        mean[e] = [chain(h, Wm[o], bm[o]) for o in range(A)]
        for a in range(A):
            acc = 0.0   # +0; exactly H terms, no padding
            for k in range(H):
                acc = fmaf(float(h[k]), float(E[e, k, a]), acc)
            noise[e, a] = acc
    if actor.clip_mean > 0:
        c = F32(actor.clip_mean)
        mean = np.where(mean < -c, -c, np.where(mean > c, c, mean)).astype(F32)
    return mean, latent, noise


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    structs = {"pgx_sde_actor_config": abi.PgxSdeActorConfig, "pgx_sde_actor_weights": abi.PgxSdeActorWeights,
               "pgx_sde_actor_io": abi.PgxSdeActorIo}
    out = header_layout(structs, ['printf("tag %u\\n", PGX_SDE_PHILOX_TAG);'])
    assert int(out["tag"]) == abi.SDE_PHILOX_TAG == 0x53444500
    # blocks q < 1024: disjoint from the Actor's and the ActorCritic's counter words
    for other in (abi.ACTOR_PHILOX_TAG, abi.AC_PHILOX_TAG):
        assert (abi.SDE_PHILOX_TAG ^ other) >= 1024


def test_library_exports_the_entry_points():
    assert_exported(SDE_EXPORTS)


def good_config():
    c = abi.PgxSdeActorConfig()
    c.n_envs, c.obs_dim, c.action_dim, c.n_layers = 64, 6, 3, 2
    c.hidden[0], c.hidden[1] = 256, 256
    c.clip_mean, c.seed = 2.0, 0
    return c


BAD = [("n_envs", 0, b"n_envs"), ("n_envs", -5, b"n_envs"), ("obs_dim", 0, b"obs_dim"), ("obs_dim", -1, b"obs_dim"),
       ("obs_dim", 4097, b"obs_dim"), ("action_dim", 0, b"action_dim"), ("action_dim", 8, b"action_dim"),
       ("n_layers", 0, b"n_layers"), ("n_layers", 4, b"n_layers"), ("hidden0", 0, b"hidden"), ("hidden1", 513, b"hidden"),
       ("hidden1", -2, b"hidden"), ("clip_mean", -1.0, b"clip_mean"), ("clip_mean", float("nan"), b"clip_mean"),
       ("clip_mean", float("inf"), b"clip_mean")]


@pytest.mark.parametrize("field,value,word", BAD)
def test_create_rejects_bad_config_without_a_device(field, value, word):
    """PGX_E_INVALID comes from the argument check, before any HIP call: this runs without a GPU (a HIP
    failure would be PGX_E_HIP), and the message names the field."""
    lib = _native.load()
    cfg = good_config()
    if field.startswith("hidden"):
        cfg.hidden[int(field[-1])] = value
    else:
        setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.pgx_sde_actor_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_sde_actor_create" in msg and word in msg, msg


def test_null_handles_are_rejected():
    lib = _native.load()
    h = C.c_void_p()
    assert lib.pgx_sde_actor_create(None, 0, C.byref(h)) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_create(C.byref(good_config()), 0, None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    assert lib.pgx_sde_actor_set_weights(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_reset_noise(None, None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_forward(None, None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_state(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_set_state(None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_get_matrices(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_set_matrices(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_get_std(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_forward_host(None, None, None, None, None, None, 0, None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_sde_actor_forward_host(C.byref(good_config()), None, None, None, None, None, 0, None, None,
                                          None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    lib.pgx_sde_actor_destroy(None)   # a no-op


def test_python_surface_is_exported():
    sig = inspect.signature(pg.SdeActor.__init__).parameters
    assert list(sig)[1:] == ["env", "obs_dim", "action_dim", "net_arch", "log_std_init", "clip_mean", "full_std",
                             "use_expln", "seed", "device", "n_envs"]
    want = {"env": None, "obs_dim": None, "action_dim": None, "net_arch": (256, 256), "log_std_init": -3.0,
            "clip_mean": 2.0, "full_std": True, "use_expln": False, "seed": 0, "device": None, "n_envs": None}
    for k, v in want.items():
        assert sig[k].default == v, k
    for name in ("load_state_dict", "state_dict", "reset_noise", "capture_rollout", "collect", "close", "forward_host",
                 "enable_debug", "forward"):
        assert hasattr(pg.SdeActor, name), name
    call = inspect.signature(pg.SdeActor.__call__).parameters
    assert list(call)[1:] == ["obs", "deterministic"] and call["deterministic"].default is False
    for fn in (pg.SdeActor.capture_rollout, pg.SdeActor.collect):
        cap = inspect.signature(fn).parameters
        assert list(cap)[1:] == ["venv", "k", "deterministic", "after_step", "sde_sample_freq"]
        assert cap["deterministic"].default is False and cap["after_step"].default is None
        assert cap["sde_sample_freq"].default == -1
    for prop in ("noise_generation", "exploration_matrices"):
        p = getattr(pg.SdeActor, prop)
        assert isinstance(p, property) and p.fset is not None, prop
    assert "SdeActor" in pg.__all__
    with pytest.raises(ValueError, match="full_std"):
        pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, full_std=False, device="cpu")
    with pytest.raises(ValueError, match="use_expln"):
        pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, use_expln=True, device="cpu")
    with pytest.raises(pg.PgxError, match="n_layers"):
        pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(8, 8, 8, 8), device="cpu")
    a = pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(8,), device="cpu")
    with pytest.raises(pg.PgxError, match="no CPU fallback"):
        a(random_obs(np.random.default_rng(0), 4, 6))
    with pytest.raises(pg.PgxError, match="no CPU fallback"):
        a.reset_noise()
    with pytest.raises(pg.PgxError, match="no CPU fallback"):
        a.noise_generation


# ---------------------------------------------------------------- state dicts
def test_state_dict_keys_and_round_trip():
    rng = np.random.default_rng(1)
    g = pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(16, 8, 4), device="cpu")
    assert list(g.state_dict()) == ["latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias",
                                    "latent_pi.4.weight", "latent_pi.4.bias", "mu.0.weight", "mu.0.bias", "log_std"]
    assert [tuple(v.shape) for v in g.state_dict().values()] == [(16, 12), (16,), (8, 16), (8,), (4, 8), (4,), (3, 4), (3,),
                                                                 (4, 3)]
    assert np.array_equal(bits(g.state_dict()["log_std"].numpy()), bits(np.full((4, 3), -3.0, F32)))
    d = pg.SdeActor(obs_dim=56, action_dim=7, n_envs=4, net_arch=(400, 300), clip_mean=0.0, log_std_init=-2.0, device="cpu")
    assert list(d.state_dict()) == ["latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias",
                                    "mu.weight", "mu.bias", "log_std"]
    assert [tuple(v.shape) for v in d.state_dict().values()] == [(400, 62), (400,), (300, 400), (300,), (7, 300), (7,),
                                                                 (300, 7)]
    assert np.array_equal(bits(d.state_dict()["log_std"].numpy()), bits(np.full((300, 7), -2.0, F32)))
    for actor in (g, d):
        sd = random_sde_state_dict(actor, rng)
        actor.load_state_dict(sd)
        back = actor.state_dict()
        assert list(back) == list(sd)
        for k in sd:
            assert np.array_equal(bits(back[k].numpy()), bits(sd[k])), k
        # a policy's state dict: the actor's keys under "actor.", everything else ignored
        policy = {f"actor.{k}": v for k, v in random_sde_state_dict(actor, rng).items()}
        policy["critic.qf0.0.weight"] = np.zeros((3, 3), F32)
        policy["log_std"] = np.zeros((1, 1), F32)   # not the actor's: no "actor." prefix in a prefixed dict
        actor.load_state_dict(policy)
        for k, v in actor.state_dict().items():
            assert np.array_equal(bits(v.numpy()), bits(policy[f"actor.{k}"])), k


def test_load_state_dict_names_the_offending_key():
    rng = np.random.default_rng(2)
    a = pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(16, 8), device="cpu")
    sd = random_sde_state_dict(a, rng)
    a.load_state_dict(sd)
    before = a.state_dict()
    wrong = dict(sd)
    wrong["latent_pi.2.weight"] = np.zeros((8, 15), F32)
    with pytest.raises(ValueError, match=r"latent_pi\.2\.weight"):
        a.load_state_dict(wrong)
    wrong = {f"actor.{k}": v for k, v in sd.items()}
    wrong["actor.log_std"] = np.zeros((3, 8), F32)   # [A, H]: transposed
    with pytest.raises(ValueError, match=r"log_std"):
        a.load_state_dict(wrong)
    missing = {k: v for k, v in sd.items() if k != "mu.0.bias"}
    with pytest.raises(KeyError, match=r"mu\.0\.bias"):
        a.load_state_dict(missing)
    plain_mu = {k.replace("mu.0.", "mu."): v for k, v in sd.items()}   # the clip_mean == 0 names
    with pytest.raises(KeyError, match=r"mu\.0\.weight"):
        a.load_state_dict(plain_mu)
    missing = {k: v for k, v in sd.items() if k != "log_std"}
    with pytest.raises(KeyError, match=r"log_std"):
        a.load_state_dict(missing)
    for k, v in a.state_dict().items():   # a failed load changes nothing
        assert np.array_equal(bits(v.numpy()), bits(before[k].numpy())), k


# ---------------------------------------------------------------- the arithmetic contract
SHAPES = [(12, (32,), 1), (24, (33, 7), 7), (12, (400, 300), 3)]


@pytest.mark.parametrize("in_dim,arch,A", SHAPES)
def test_host_model_equals_the_restatement_bit_for_bit(in_dim, arch, A):
    rng = np.random.default_rng(in_dim * 1000 + len(arch) * 100 + A)
    n = 5
    actor = pg.SdeActor(obs_dim=in_dim - 6, action_dim=A, n_envs=n, net_arch=arch, device="cpu")
    sd = random_sde_state_dict(actor, rng)
    actor.load_state_dict(sd)
    obs = random_obs(rng, n, in_dim - 6)
    E = (rng.standard_normal((n, arch[-1], A)) * 0.05).astype(F32)
    mean, latent, noise = actor.forward_host(obs, E)
    want_mean, want_latent, want_noise = restated_forward(actor, sd, obs, E)
    assert np.isfinite(mean).all() and np.array_equal(bits(mean), bits(want_mean))
    assert np.isfinite(latent).all() and np.array_equal(bits(latent), bits(want_latent))
    assert np.isfinite(noise).all() and np.array_equal(bits(noise), bits(want_noise))
    assert (latent > 0).any() and (noise != 0).any()


def test_noise_is_positive_zero_where_the_latent_is_zero():
    """Large negative last-layer biases: relu gives a latent of +0 everywhere, and the chain from +0 over
    products of +0 with finite entries of either sign stays +0 (never -0)."""
    rng = np.random.default_rng(4)
    n, A, arch = 5, 3, (16, 10)
    actor = pg.SdeActor(obs_dim=6, action_dim=A, n_envs=n, net_arch=arch, device="cpu")
    sd = random_sde_state_dict(actor, rng)
    sd["latent_pi.2.bias"] = np.full(10, -1e6, F32)
    actor.load_state_dict(sd)
    obs = random_obs(rng, n, 6)
    E = rng.standard_normal((n, 10, A)).astype(F32)
    E[0] = -np.abs(E[0])   # +0 * negative = -0 products: +0 + -0 = +0
    mean, latent, noise = actor.forward_host(obs, E)
    assert np.array_equal(bits(latent), np.zeros((n, 10), np.uint32))
    assert np.array_equal(bits(noise), np.zeros((n, A), np.uint32))
    r_mean, r_latent, r_noise = restated_forward(actor, sd, obs, E)
    assert np.array_equal(bits(noise), bits(r_noise)) and np.array_equal(bits(mean), bits(r_mean))
    # the mean is then mu's bias through the Hardtanh
    want = np.clip(sd["mu.0.bias"], -2.0, 2.0).astype(F32)
    assert np.array_equal(mean, np.tile(want, (n, 1)))


def test_hardtanh_edges():
    """Zero weights, so mu is its bias: beyond +-2 it meets clip_mean = 2, inside it passes untouched; with
    clip_mean = 0 the mean is left alone."""
    obs = random_obs(np.random.default_rng(3), 5, 6)
    mu_b = np.array([3.0, -3.0, 0.5, 2.0, -2.0000002], F32)
    E = np.zeros((5, 8, 5), F32)
    for clip in (2.0, 0.0):
        a = pg.SdeActor(obs_dim=6, action_dim=5, n_envs=5, net_arch=(8,), clip_mean=clip, device="cpu")
        sd = {k: np.zeros(tuple(v.shape), F32) for k, v in a.state_dict().items()}
        sd[f"{mu_name(a)}.bias"] = mu_b
        a.load_state_dict(sd)
        mean, latent, noise = a.forward_host(obs, E)
        want_mean = np.array([2.0, -2.0, 0.5, 2.0, -2.0], F32) if clip else mu_b
        assert np.array_equal(bits(mean), bits(np.tile(want_mean, (5, 1))))
        r_mean, _, _ = restated_forward(a, sd, obs, E)
        assert np.array_equal(bits(mean), bits(r_mean))
    with pytest.raises(ValueError, match="matrices"):
        a.forward_host(obs, np.zeros((5, 5, 8), F32))
