"""The Actor C-ABI (include/pgx.h, pgx_actor_*) without a GPU: the ctypes mirrors against the header's
layout through gcc, the exported entry points, the argument checks (made before any device call), the
Python surface, SB3's state-dict key names, and the arithmetic contract: the library's host model
(pgx_actor_forward_host) against an independent restatement written from the header's rules -- libm's
fmaf through ctypes, ascending k, the accumulator starting at the bias, K rounded up to 16 -- bit for
bit, and against an fp64 numpy forward within the f32-chain envelope of 1.5e-7 * sum|a b| per layer,
propagated through the layers here."""
import ctypes as C
import ctypes.util
import inspect
import itertools

import numpy as np
import pytest

import panda_gym_amd as pg
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi

F32 = np.float32
ACTOR_EXPORTS = ["pgx_actor_create", "pgx_actor_destroy", "pgx_actor_set_weights", "pgx_actor_forward",
                 "pgx_actor_state", "pgx_actor_set_state", "pgx_actor_forward_host"]

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
_libm.fmaf.restype = C.c_float
fmaf = _libm.fmaf


# ---------------------------------------------------------------- helpers shared with the GPU tests
def random_state_dict(actor, rng, scale=1.0):
    """standard_normal / sqrt(fan_in) weights (biases / 2) under the actor's own key names."""
    sd = {}
    for k, v in actor.state_dict().items():
        shape = tuple(v.shape)
        s = scale / np.sqrt(shape[1]) if len(shape) == 2 else 0.5 * scale
        sd[k] = (rng.standard_normal(shape) * s).astype(F32)
    return sd


def random_obs(rng, n, obs_dim):
    return {"observation": rng.standard_normal((n, obs_dim)).astype(F32),
            "achieved_goal": rng.standard_normal((n, 3)).astype(F32),
            "desired_goal": rng.standard_normal((n, 3)).astype(F32)}


def features(obs, dtype=F32):
    """SB3 CombinedExtractor: the Dict space's keys in sorted order."""
    return np.concatenate([obs["achieved_goal"], obs["desired_goal"], obs["observation"]], axis=1).astype(dtype)


def layer_params(actor, sd):
    """[(W, b)] of the trunk, then the heads' [(W, b)] (mu, and log_std for the Gaussian kind)."""
    nl = len(actor.net_arch)
    if actor.kind == "gaussian":
        names = [f"latent_pi.{2 * i}" for i in range(nl)] + ["mu", "log_std"]
    else:
        names = [f"mu.{2 * i}" for i in range(nl + 1)]
    p = [(np.asarray(sd[f"{n}.weight"], F32), np.asarray(sd[f"{n}.bias"], F32)) for n in names]
    return p[:nl], p[nl:]


def chain(x, w, b):
    """One output of a Linear by the header's rule: acc = bias, then fmaf over k ascending, K up to a multiple of 16."""
    acc = float(b)
    K = len(x)
    for k in range(K):
        acc = fmaf(float(x[k]), float(w[k]), acc)
    for _ in range(K, (K + 15) // 16 * 16):
        acc = fmaf(0.0, 0.0, acc)
    return acc


def restated_forward(actor, sd, obs):
    """mean, log_std [n, A] f32 by the header's contract, one libm fmaf at a time."""
    trunk, heads = layer_params(actor, sd)
    x = features(obs)
    n, A = x.shape[0], actor.action_dim
    out = [np.zeros((n, A), F32) for _ in heads]
    for e in range(n):
        h = x[e]
        for W, b in trunk:
            y = np.array([chain(h, W[o], b[o]) for o in range(W.shape[0])], F32)
            h = np.where(y > 0, y, F32(0.0)).astype(F32)
        for i, (W, b) in enumerate(heads):
            out[i][e] = [chain(h, W[o], b[o]) for o in range(A)]
    mean = out[0]
    if actor.clip_mean > 0:
        c = F32(actor.clip_mean)
        mean = np.where(mean < -c, -c, np.where(mean > c, c, mean)).astype(F32)
    log_std = None
    if len(out) == 2:
        v = out[1]
        log_std = np.where(v < F32(-20.0), F32(-20.0), np.where(v > F32(2.0), F32(2.0), v)).astype(F32)
    return mean, log_std


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    structs = {"pgx_actor_config": abi.PgxActorConfig, "pgx_actor_weights": abi.PgxActorWeights,
               "pgx_actor_io": abi.PgxActorIo}
    out = header_layout(structs, ['printf("kinds %d %d\\n", PGX_ACTOR_GAUSSIAN, PGX_ACTOR_DETERMINISTIC);'])
    assert out["kinds"] == f"{abi.ACTOR_GAUSSIAN} {abi.ACTOR_DETERMINISTIC}"
    assert abi.ACTOR_KINDS == {"gaussian": 0, "deterministic": 1}


def test_library_exports_the_entry_points():
    assert_exported(ACTOR_EXPORTS)


def good_config():
    c = abi.PgxActorConfig()
    c.n_envs, c.obs_dim, c.action_dim, c.n_layers = 64, 6, 3, 2
    c.hidden[0], c.hidden[1] = 256, 256
    c.kind, c.clip_mean, c.noise_mu, c.noise_sigma, c.seed = abi.ACTOR_GAUSSIAN, 0.0, 0.0, 0.1, 0
    return c


BAD = [("n_envs", 0, b"n_envs"), ("n_envs", -5, b"n_envs"), ("obs_dim", 0, b"obs_dim"), ("obs_dim", -1, b"obs_dim"),
       ("action_dim", 0, b"action_dim"), ("action_dim", 8, b"action_dim"), ("n_layers", 0, b"n_layers"),
       ("n_layers", 4, b"n_layers"), ("hidden0", 0, b"hidden"), ("hidden1", 513, b"hidden"), ("hidden1", -2, b"hidden"),
       ("kind", 2, b"kind"), ("kind", -1, b"kind"), ("noise_sigma", -0.1, b"noise_sigma"),
       ("noise_sigma", float("nan"), b"noise_sigma"), ("clip_mean", -1.0, b"clip_mean"),
       ("clip_mean", float("nan"), b"clip_mean")]


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
    assert lib.pgx_actor_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_actor_create" in msg and word in msg, msg


def test_null_handles_are_rejected():
    lib = _native.load()
    h = C.c_void_p()
    assert lib.pgx_actor_create(None, 0, C.byref(h)) == abi.PGX_E_INVALID
    assert lib.pgx_actor_create(C.byref(good_config()), 0, None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    assert lib.pgx_actor_set_weights(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_actor_forward(None, None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_actor_state(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_actor_set_state(None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_actor_forward_host(None, None, None, None, None, 0, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_actor_forward_host(C.byref(good_config()), None, None, None, None, 0, None, None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    lib.pgx_actor_destroy(None)   # a no-op


def test_python_surface_is_exported():
    sig = inspect.signature(pg.Actor.__init__).parameters
    assert list(sig)[1:] == ["env", "obs_dim", "action_dim", "net_arch", "kind", "clip_mean", "action_noise", "seed",
                             "device", "n_envs"]
    want = {"env": None, "obs_dim": None, "action_dim": None, "net_arch": (256, 256), "kind": "gaussian",
            "clip_mean": 0.0, "action_noise": None, "seed": 0, "device": None, "n_envs": None}
    for k, v in want.items():
        assert sig[k].default == v, k
    for name in ("load_state_dict", "state_dict", "capture_rollout", "close", "noise_step", "forward_host",
                 "enable_debug", "forward"):
        assert hasattr(pg.Actor, name), name
    call = inspect.signature(pg.Actor.__call__).parameters
    assert list(call)[1:] == ["obs", "deterministic", "eps"]
    assert call["deterministic"].default is False and call["eps"].default is None
    cap = inspect.signature(pg.Actor.capture_rollout).parameters
    assert list(cap)[1:] == ["venv", "k", "deterministic", "after_step"]
    assert cap["deterministic"].default is False and cap["after_step"].default is None
    assert isinstance(pg.Actor.noise_step, property) and pg.Actor.noise_step.fset is not None
    assert "Actor" in pg.__all__ and hasattr(pg.VecMonitor, "_enqueue_step")
    with pytest.raises(ValueError):
        pg.Actor(obs_dim=6, action_dim=3, n_envs=4, kind="beta", device="cpu")
    with pytest.raises(pg.PgxError, match="n_layers"):
        pg.Actor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(8, 8, 8, 8), device="cpu")
    a = pg.Actor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(8,), device="cpu")
    with pytest.raises(pg.PgxError, match="no CPU fallback"):
        a(random_obs(np.random.default_rng(0), 4, 6))


# ---------------------------------------------------------------- state dicts
def test_state_dict_keys_and_round_trip():
    rng = np.random.default_rng(1)
    g = pg.Actor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(16, 8, 4), kind="gaussian", device="cpu")
    assert list(g.state_dict()) == ["latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias",
                                    "latent_pi.4.weight", "latent_pi.4.bias", "mu.weight", "mu.bias", "log_std.weight",
                                    "log_std.bias"]
    assert [tuple(v.shape) for v in g.state_dict().values()] == [(16, 12), (16,), (8, 16), (8,), (4, 8), (4,), (3, 4), (3,),
                                                                 (3, 4), (3,)]
    d = pg.Actor(obs_dim=56, action_dim=7, n_envs=4, net_arch=(400, 300), kind="deterministic", device="cpu")
    assert list(d.state_dict()) == ["mu.0.weight", "mu.0.bias", "mu.2.weight", "mu.2.bias", "mu.4.weight", "mu.4.bias"]
    assert [tuple(v.shape) for v in d.state_dict().values()] == [(400, 62), (400,), (300, 400), (300,), (7, 300), (7,)]
    for actor in (g, d):
        sd = random_state_dict(actor, rng)
        actor.load_state_dict(sd)
        back = actor.state_dict()
        assert list(back) == list(sd)
        for k in sd:
            assert np.array_equal(bits(back[k].numpy()), bits(sd[k])), k
        # a policy's state dict: the actor's keys under "actor.", everything else ignored
        policy = {f"actor.{k}": v for k, v in random_state_dict(actor, rng).items()}
        policy["critic.qf0.0.weight"] = np.zeros((3, 3), F32)
        policy["mu.weight"] = np.zeros((1, 1), F32)   # not the actor's: no "actor." prefix in a prefixed dict
        actor.load_state_dict(policy)
        for k, v in actor.state_dict().items():
            assert np.array_equal(bits(v.numpy()), bits(policy[f"actor.{k}"])), k


def test_load_state_dict_names_the_offending_key():
    rng = np.random.default_rng(2)
    a = pg.Actor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(16, 8), device="cpu")
    sd = random_state_dict(a, rng)
    before = a.state_dict()
    wrong = dict(sd)
    wrong["latent_pi.2.weight"] = np.zeros((8, 15), F32)
    with pytest.raises(ValueError, match=r"latent_pi\.2\.weight"):
        a.load_state_dict(wrong)
    wrong = {f"actor.{k}": v for k, v in sd.items()}
    wrong["actor.log_std.bias"] = np.zeros(4, F32)
    with pytest.raises(ValueError, match=r"log_std\.bias"):
        a.load_state_dict(wrong)
    missing = {k: v for k, v in sd.items() if k != "mu.bias"}
    with pytest.raises(KeyError, match=r"mu\.bias"):
        a.load_state_dict(missing)
    for k, v in a.state_dict().items():   # a failed load changes nothing
        assert np.array_equal(bits(v.numpy()), bits(before[k].numpy())), k


# ---------------------------------------------------------------- the arithmetic contract
SHAPES = list(itertools.product((12, 62), ((32,), (96, 32), (33, 7, 20)), (3, 7), ("gaussian", "deterministic")))


@pytest.mark.parametrize("in_dim,arch,A,kind", SHAPES)
def test_host_model_equals_the_restatement_bit_for_bit(in_dim, arch, A, kind):
    rng = np.random.default_rng(in_dim * 1000 + len(arch) * 100 + A * 10 + len(kind))
    n = 5
    actor = pg.Actor(obs_dim=in_dim - 6, action_dim=A, n_envs=n, net_arch=arch, kind=kind, device="cpu")
    sd = random_state_dict(actor, rng)
    actor.load_state_dict(sd)
    obs = random_obs(rng, n, in_dim - 6)
    mean, log_std = actor.forward_host(obs)
    want_mean, want_log_std = restated_forward(actor, sd, obs)
    assert np.isfinite(mean).all() and np.array_equal(bits(mean), bits(want_mean))
    if kind == "gaussian":
        assert np.isfinite(log_std).all() and np.array_equal(bits(log_std), bits(want_log_std))
    else:
        assert log_std is None and want_log_std is None


def test_negative_zero_accumulator_follows_the_padded_chain():
    """The one place the padding shows (include/pgx.h): a -0 bias with only -0 products ends as +0 where K
    is no multiple of 16 and stays -0 where it is."""
    for width, negative in ((16, True), (12, False)):   # the head's K: no padded term, four of them
        a = pg.Actor(obs_dim=6, action_dim=1, n_envs=1, net_arch=(width,), kind="deterministic", device="cpu")
        sd = {k: np.zeros(tuple(v.shape), F32) for k, v in a.state_dict().items()}
        sd["mu.2.bias"] = np.array([-0.0], F32)   # the head: relu(0) = +0 inputs times -0 weights = -0 products
        sd["mu.2.weight"] = np.full((1, width), -0.0, F32)
        a.load_state_dict(sd)
        obs = {"observation": np.zeros((1, 6), F32), "achieved_goal": np.zeros((1, 3), F32),
               "desired_goal": np.zeros((1, 3), F32)}
        mean, _ = a.forward_host(obs)
        assert mean[0, 0] == 0.0 and bool(np.signbit(mean[0, 0])) == negative
        want, _ = restated_forward(a, sd, obs)
        assert np.array_equal(bits(mean), bits(want))


@pytest.mark.parametrize("in_dim,arch,A,kind", [(12, (96, 32), 3, "gaussian"), (62, (33, 7, 20), 7, "deterministic"),
                                                (62, (256, 256), 7, "gaussian")])
def test_host_model_within_the_f32_chain_envelope_of_fp64(in_dim, arch, A, kind):
    """Per Linear, the f32 chain is within 1.5e-7 * (|b| + sum|x w|) of the exact sum on the same inputs (the
    f32-input MFMA's stated envelope); an input error e_in adds at most sum|w| e_in, ReLU does not grow it.
    The bound for the heads is propagated layer by layer from that, on the fp64 forward's own activations
    plus the bound so far -- nothing here comes from the host model's output."""
    rng = np.random.default_rng(7)
    n = 16
    actor = pg.Actor(obs_dim=in_dim - 6, action_dim=A, n_envs=n, net_arch=arch, kind=kind, device="cpu")
    sd = random_state_dict(actor, rng)
    actor.load_state_dict(sd)
    obs = random_obs(rng, n, in_dim - 6)
    mean, log_std = actor.forward_host(obs)
    trunk, heads = layer_params(actor, sd)
    x = features(obs, np.float64)
    err = np.zeros_like(x)
    for W, b in trunk:
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        mag = np.abs(b64) + (np.abs(x) + err) @ np.abs(W64).T
        err = 1.5e-7 * mag + err @ np.abs(W64).T
        x = np.maximum(x @ W64.T + b64, 0.0)
    got = [mean, log_std]
    worst = 0.0
    for i, (W, b) in enumerate(heads):
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        bound = 1.5e-7 * (np.abs(b64) + (np.abs(x) + err) @ np.abs(W64).T) + err @ np.abs(W64).T
        want = x @ W64.T + b64
        if i == 1:
            want = np.clip(want, -20.0, 2.0)   # 1-Lipschitz: the bound holds through it
        diff = np.abs(got[i].astype(np.float64) - want)
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all(), (i, float(diff.max()), float(bound.min()))
    print(f"host model vs fp64, {arch}: largest error / bound = {worst:.3f}")


def test_clip_mean_and_log_std_clamp_edges():
    """Zero weights, so the heads are their biases: mu beyond +-2 meets clip_mean = 2, log_std beyond -20 and
    2 meets the clamp; the values inside pass untouched.  Without clip_mean the mean is left alone."""
    obs = random_obs(np.random.default_rng(3), 5, 6)
    mu_b = np.array([3.0, -3.0, 0.5, 2.0, -2.0000002], F32)
    ls_b = np.array([-25.0, 5.0, 0.25, -20.0, 2.0000002], F32)
    for clip in (2.0, 0.0):
        a = pg.Actor(obs_dim=6, action_dim=5, n_envs=5, net_arch=(8,), clip_mean=clip, device="cpu")
        sd = {k: np.zeros(tuple(v.shape), F32) for k, v in a.state_dict().items()}
        sd["mu.bias"], sd["log_std.bias"] = mu_b, ls_b
        a.load_state_dict(sd)
        mean, log_std = a.forward_host(obs)
        want_mean = np.array([2.0, -2.0, 0.5, 2.0, -2.0], F32) if clip else mu_b
        assert np.array_equal(bits(mean), bits(np.tile(want_mean, (5, 1))))
        assert np.array_equal(bits(log_std), bits(np.tile(np.array([-20.0, 2.0, 0.25, -20.0, 2.0], F32), (5, 1))))
        r_mean, r_log_std = restated_forward(a, sd, obs)
        assert np.array_equal(bits(mean), bits(r_mean)) and np.array_equal(bits(log_std), bits(r_log_std))
    d = pg.Actor(obs_dim=6, action_dim=5, n_envs=5, net_arch=(8,), kind="deterministic", device="cpu")
    sd = {k: np.zeros(tuple(v.shape), F32) for k, v in d.state_dict().items()}
    sd["mu.2.bias"] = mu_b
    d.load_state_dict(sd)
    assert np.array_equal(bits(d.forward_host(obs)[0]), bits(np.tile(mu_b, (5, 1))))
