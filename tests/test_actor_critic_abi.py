"""The ActorCritic C-ABI (include/pgx.h, pgx_ac_*) without a GPU: the ctypes mirrors against the header's
layout through gcc, the exported entry points, the argument checks (made before any device call), the
Python surface, SB3's ActorCriticPolicy state-dict key names, use_sde's shape rule and refusals, and the
arithmetic contract: the library's host model (pgx_ac_forward_host) against the restatement of
test_actor_abi.py (libm's fmaf through ctypes, ascending k, the accumulator starting at the bias, K rounded
up to 16), bit for bit, for unequal trunk depths."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import panda_gym_amd as pg
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi
from test_actor_abi import bits, chain, features, random_obs

F32 = np.float32
AC_EXPORTS = ["pgx_ac_create", "pgx_ac_destroy", "pgx_ac_set_weights", "pgx_ac_forward", "pgx_ac_values",
              "pgx_ac_state", "pgx_ac_set_state", "pgx_ac_forward_host"]


# ---------------------------------------------------------------- helpers shared with the GPU tests
def random_ac_state_dict(ac, rng, scale=1.0, log_std=(-3.0, 0.5)):
    """standard_normal / sqrt(fan_in) weights (biases / 2) under the policy's own key names; log_std spread
    evenly over ``log_std`` so small and large variances both occur."""
    sd = {}
    for k, v in ac.state_dict().items():
        shape = tuple(v.shape)
        if k == "log_std":
            sd[k] = np.linspace(log_std[0], log_std[1], int(np.prod(shape))).reshape(shape).astype(F32)
        else:
            s = scale / np.sqrt(shape[1]) if len(shape) == 2 else 0.5 * scale
            sd[k] = (rng.standard_normal(shape) * s).astype(F32)
    return sd


def restated_forward(ac, sd, obs):
    """mean [n, A], value [n] f32 by the header's contract, one libm fmaf at a time."""
    x = features(obs)
    n, A = x.shape[0], ac.action_dim
    mean, value = np.zeros((n, A), F32), np.zeros((n,), F32)
    for e in range(n):
        for net, depth, head, out in (("policy_net", len(ac.pi_arch), "action_net", mean),
                                      ("value_net", len(ac.vf_arch), "value_net", value)):
            h = x[e]
            for i in range(depth):
                W, b = sd[f"mlp_extractor.{net}.{2 * i}.weight"], sd[f"mlp_extractor.{net}.{2 * i}.bias"]
                y = np.array([chain(h, W[o], b[o]) for o in range(W.shape[0])], F32)
                h = np.where(y > 0, y, F32(0.0)).astype(F32)
            W, b = sd[f"{head}.weight"], sd[f"{head}.bias"]
            y = [chain(h, W[o], b[o]) for o in range(W.shape[0])]
            out[e] = y if head == "action_net" else y[0]
    return mean, value


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    structs = {"pgx_ac_config": abi.PgxAcConfig, "pgx_ac_weights": abi.PgxAcWeights, "pgx_ac_io": abi.PgxAcIo}
    out = header_layout(structs, ['printf("tag %u\\n", PGX_AC_PHILOX_TAG);'])
    assert int(out["tag"]) == abi.AC_PHILOX_TAG
    assert abi.AC_PHILOX_TAG != abi.ACTOR_PHILOX_TAG
    # no dimension pair of one stream meets one of the other
    assert not {abi.AC_PHILOX_TAG ^ p for p in range(4)} & {abi.ACTOR_PHILOX_TAG ^ p for p in range(4)}


def test_library_exports_the_entry_points():
    assert_exported(AC_EXPORTS)


def good_config():
    c = abi.PgxAcConfig()
    c.n_envs, c.obs_dim, c.action_dim, c.n_pi_layers, c.n_vf_layers = 64, 6, 3, 2, 2
    c.pi_hidden[0], c.pi_hidden[1], c.vf_hidden[0], c.vf_hidden[1] = 256, 256, 256, 256
    return c


BAD = [("n_envs", 0, b"n_envs"), ("n_envs", -5, b"n_envs"), ("obs_dim", 0, b"obs_dim"), ("obs_dim", -1, b"obs_dim"),
       ("obs_dim", 4097, b"obs_dim"), ("action_dim", 0, b"action_dim"), ("action_dim", 8, b"action_dim"),
       ("n_pi_layers", 0, b"n_pi_layers"), ("n_pi_layers", 4, b"n_pi_layers"), ("n_vf_layers", 0, b"n_vf_layers"),
       ("n_vf_layers", 4, b"n_vf_layers"), ("pi_hidden0", 0, b"pi_hidden"), ("pi_hidden1", 513, b"pi_hidden"),
       ("vf_hidden0", -2, b"vf_hidden"), ("vf_hidden1", 513, b"vf_hidden")]


@pytest.mark.parametrize("field,value,word", BAD)
def test_create_rejects_bad_config_without_a_device(field, value, word):
    """PGX_E_INVALID comes from the argument check, before any HIP call: this runs without a GPU (a HIP
    failure would be PGX_E_HIP), and the message names the field."""
    lib = _native.load()
    cfg = good_config()
    if "hidden" in field:
        getattr(cfg, field[:-1])[int(field[-1])] = value
    else:
        setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.pgx_ac_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_ac_create" in msg and word in msg, msg


def test_null_pointers_are_rejected():
    lib = _native.load()
    h = C.c_void_p()
    assert lib.pgx_ac_create(None, 0, C.byref(h)) == abi.PGX_E_INVALID
    assert lib.pgx_ac_create(C.byref(good_config()), 0, None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    assert lib.pgx_ac_set_weights(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_ac_forward(None, None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_ac_values(None, None, None, None, None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_ac_state(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_ac_set_state(None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_ac_forward_host(None, None, None, None, None, 0, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_ac_forward_host(C.byref(good_config()), None, None, None, None, 0, None, None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    lib.pgx_ac_destroy(None)   # a no-op


def test_python_surface_is_exported():
    sig = inspect.signature(pg.ActorCritic.__init__).parameters
    assert list(sig)[1:] == ["env", "obs_dim", "action_dim", "n_envs", "net_arch", "log_std_init", "activation_fn",
                             "use_sde", "seed", "device"]
    assert sig["log_std_init"].default == 0.0 and sig["activation_fn"].default == "relu"
    assert sig["use_sde"].default is False and sig["seed"].default == 0 and sig["device"].default is None
    for name in ("load_state_dict", "state_dict", "capture_rollout", "collect_rollouts", "close", "noise_step",
                 "forward_host", "enable_debug", "forward", "predict", "predict_values"):
        assert hasattr(pg.ActorCritic, name), name
    call = inspect.signature(pg.ActorCritic.__call__).parameters
    assert list(call)[1:] == ["obs", "deterministic", "eps"]
    assert call["deterministic"].default is False and call["eps"].default is None
    assert inspect.signature(pg.ActorCritic.predict).parameters["deterministic"].default is True
    assert list(inspect.signature(pg.ActorCritic.predict_values).parameters)[1:] == ["obs", "need", "out"]
    for fn in (pg.ActorCritic.capture_rollout, pg.ActorCritic.collect_rollouts):
        cap = inspect.signature(fn).parameters
        assert list(cap)[1:] == ["venv", "buf", "deterministic"] and cap["deterministic"].default is False
    assert isinstance(pg.ActorCritic.noise_step, property) and pg.ActorCritic.noise_step.fset is not None
    assert "ActorCritic" in pg.__all__
    # the default is the reference's PPO net_arch; a list means both trunks
    a = pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, device="cpu")
    assert a.pi_arch == (256, 256) and a.vf_arch == (256, 256)
    a = pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=[64, 32], device="cpu")
    assert a.pi_arch == (64, 32) and a.vf_arch == (64, 32)
    with pytest.raises(pg.PgxError, match="n_pi_layers"):
        pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[8, 8, 8, 8], vf=[8]), device="cpu")
    with pytest.raises(pg.PgxError, match="vf_hidden"):
        pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[8], vf=[8, 600]), device="cpu")
    with pytest.raises(ValueError, match="pi"):
        pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[8]), device="cpu")
    a = pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=(8,), device="cpu")
    obs = random_obs(np.random.default_rng(0), 4, 6)
    for call in (lambda: a(obs), lambda: a.predict(obs), lambda: a.predict_values(obs)):
        with pytest.raises(pg.PgxError, match="no CPU fallback"):
            call()


def test_only_relu_is_built():
    kw = dict(obs_dim=6, action_dim=3, n_envs=4, net_arch=(8,), device="cpu")
    for ok in ("relu", "ReLU", torch.nn.ReLU, torch.nn.ReLU()):
        pg.ActorCritic(activation_fn=ok, **kw)
    for bad in ("tanh", torch.nn.Tanh, torch.nn.ELU, None):
        with pytest.raises(ValueError, match="Tanh"):
            pg.ActorCritic(activation_fn=bad, **kw)


# ---------------------------------------------------------------- state dicts
def test_state_dict_keys_and_round_trip_from_a_whole_policy_dict():
    rng = np.random.default_rng(1)
    a = pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[16, 8, 4], vf=[5]), log_std_init=-0.5,
                       device="cpu")
    sd0 = a.state_dict()
    assert list(sd0) == ["log_std", "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
                         "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
                         "mlp_extractor.policy_net.4.weight", "mlp_extractor.policy_net.4.bias",
                         "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "action_net.weight",
                         "action_net.bias", "value_net.weight", "value_net.bias"]
    assert [tuple(v.shape) for v in sd0.values()] == [(3,), (16, 12), (16,), (8, 16), (8,), (4, 8), (4,), (5, 12), (5,),
                                                      (3, 4), (3,), (1, 5), (1,)]
    # before a load: zero parameters, log_std = log_std_init
    assert np.array_equal(sd0["log_std"].numpy(), np.full(3, -0.5, F32))
    assert all(not v.numpy().any() for k, v in sd0.items() if k != "log_std")
    mean, value = a.forward_host(random_obs(rng, 5, 6))
    assert not mean.any() and not value.any()
    sd = random_ac_state_dict(a, rng)
    policy = dict(sd)   # a whole policy's state dict: the extractor's own keys are ignored
    policy["features_extractor.extractors.observation.0.weight"] = np.zeros((2, 2), F32)
    policy["pi_features_extractor.flatten"] = np.zeros((1,), F32)
    a.load_state_dict(policy)
    back = a.state_dict()
    assert list(back) == list(sd0)
    for k in sd:
        assert np.array_equal(bits(back[k].numpy()), bits(sd[k])), k
    a.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})   # tensors as well
    for k in sd:
        assert np.array_equal(bits(a.state_dict()[k].numpy()), bits(sd[k])), k


def test_load_state_dict_names_the_offending_key():
    rng = np.random.default_rng(2)
    a = pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[16, 8], vf=[8, 16]), device="cpu")
    sd = random_ac_state_dict(a, rng)
    a.load_state_dict(sd)
    before = a.state_dict()
    other = random_ac_state_dict(a, rng)
    for key, shape in (("mlp_extractor.value_net.2.weight", (16, 9)), ("action_net.bias", (4,)), ("log_std", (3, 1)),
                       ("value_net.weight", (2, 16))):
        wrong = dict(other)
        wrong[key] = np.zeros(shape, F32)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            a.load_state_dict(wrong)
    for key in ("value_net.bias", "log_std", "mlp_extractor.policy_net.2.bias"):
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            a.load_state_dict({k: v for k, v in other.items() if k != key})
    for k, v in a.state_dict().items():   # a failed load changes nothing
        assert np.array_equal(bits(v.numpy()), bits(before[k].numpy())), k


def test_use_sde_shape_rule_and_refusals():
    """use_sde=True: log_std is SB3's gSDE matrix [last pi width, A], kept for state_dict; the plain [A] vector
    is a shape error there, and the matrix is one without the flag.  forward_host works on such a policy."""
    rng = np.random.default_rng(3)
    kw = dict(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[16, 8], vf=[5]), device="cpu")
    s = pg.ActorCritic(use_sde=True, log_std_init=-2.0, **kw)
    assert tuple(s.state_dict()["log_std"].shape) == (8, 3)
    assert np.array_equal(s.state_dict()["log_std"].numpy(), np.full((8, 3), -2.0, F32))
    sd = random_ac_state_dict(s, rng)
    s.load_state_dict(sd)
    assert np.array_equal(bits(s.state_dict()["log_std"].numpy()), bits(sd["log_std"]))
    with pytest.raises(ValueError, match="log_std.*use_sde"):
        s.load_state_dict({**sd, "log_std": np.zeros(3, F32)})
    p = pg.ActorCritic(**kw)
    with pytest.raises(ValueError, match="log_std"):
        p.load_state_dict(sd)
    plain = {**sd, "log_std": np.zeros(3, F32)}
    p.load_state_dict(plain)
    obs = random_obs(rng, 5, 6)
    for got, want in zip(s.forward_host(obs), p.forward_host(obs)):   # the trunks do not read log_std
        assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- the arithmetic contract
SHAPES = [(12, (32,), (33, 7, 20), 3), (12, (96, 32), (16,), 7), (62, (33, 7, 20), (96, 32), 1), (24, (7,), (7,), 4)]


@pytest.mark.parametrize("in_dim,pi,vf,A", SHAPES)
def test_host_model_equals_the_restatement_bit_for_bit(in_dim, pi, vf, A):
    rng = np.random.default_rng(in_dim * 1000 + len(pi) * 100 + len(vf) * 10 + A)
    n = 5
    ac = pg.ActorCritic(obs_dim=in_dim - 6, action_dim=A, n_envs=n, net_arch=dict(pi=pi, vf=vf), device="cpu")
    sd = random_ac_state_dict(ac, rng)
    ac.load_state_dict(sd)
    obs = random_obs(rng, n, in_dim - 6)
    mean, value = ac.forward_host(obs)
    want_mean, want_value = restated_forward(ac, sd, obs)
    assert mean.shape == (n, A) and value.shape == (n,)
    assert np.isfinite(mean).all() and np.array_equal(bits(mean), bits(want_mean))
    assert np.isfinite(value).all() and np.array_equal(bits(value), bits(want_value))
    assert mean.any() and value.any()

