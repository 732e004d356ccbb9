"""What the three policy units (Actor, ActorCritic, SdeActor) share, pinned without a GPU: the widest
observation whose activations still fit a workgroup's LDS (the limit and the tile fallback are one helper
for the three), ``OBS_KEYS``'s old home, and ``load_state_dict``'s validate-all-then-copy for every class."""
import ctypes as C

import numpy as np
import pytest

import panda_gym_amd as pg
from panda_gym_amd import _native, abi
from test_actor_abi import bits


def _actor_cfg(obs_dim, n_envs):
    c = abi.PgxActorConfig()
    c.n_envs, c.obs_dim, c.action_dim, c.n_layers, c.kind = n_envs, obs_dim, 3, 1, abi.ACTOR_KINDS["gaussian"]
    c.hidden[0] = 16
    return c


def _sde_cfg(obs_dim, n_envs):
    c = abi.PgxSdeActorConfig()
    c.n_envs, c.obs_dim, c.action_dim, c.n_layers, c.clip_mean = n_envs, obs_dim, 3, 1, 2.0
    c.hidden[0] = 16
    return c


def _ac_cfg(obs_dim, n_envs):
    c = abi.PgxAcConfig()
    c.n_envs, c.obs_dim, c.action_dim, c.n_pi_layers, c.n_vf_layers = n_envs, obs_dim, 3, 1, 1
    c.pi_hidden[0], c.vf_hidden[0] = 16, 16
    return c


# entry prefix, config, the widest obs_dim that fits, the words of the refusal
UNITS = [("pgx_actor", _actor_cfg, 1258, b"pgx_actor_create: obs_dim too wide for the activations in LDS"),
         ("pgx_sde_actor", _sde_cfg, 1258, b"pgx_sde_actor_create: obs_dim too wide for the activations in LDS"),
         ("pgx_ac", _ac_cfg, 2490, b"pgx_ac_create: obs_dim too wide for the features in LDS")]
FITS = [(u, 1) for u in UNITS] + [(u, 4096) for u in UNITS[:2]]   # at 4096 envs the 32-env tile falls back to 16


@pytest.mark.parametrize("unit,n_envs", FITS, ids=[f"{u[0]}-{n}" for u, n in FITS])
def test_widest_observation_is_accepted(unit, n_envs):
    """One hidden layer of 16: S = 16 j + 4 with j = ceil((obs_dim + 6) / 16), and the Actor / SdeActor need
    2048 j + 512 bytes per 16 envs, so j = 79 (obs_dim 1258) is the last that fits 160 KiB less the static
    words; the ActorCritic's feature region of its own moves that to obs_dim 2490.  Not PGX_E_UNSUPPORTED:
    PGX_E_HIP without a device, PGX_OK with one."""
    prefix, make, widest, _ = unit
    lib = _native.load()
    cfg, h = make(widest, n_envs), C.c_void_p()
    rc = getattr(lib, f"{prefix}_create")(C.byref(cfg), 0, C.byref(h))
    assert rc in (abi.PGX_OK, abi.PGX_E_HIP), (rc, lib.pgx_last_error())
    if rc == abi.PGX_OK:
        getattr(lib, f"{prefix}_destroy")(h)


@pytest.mark.parametrize("unit", UNITS, ids=[u[0] for u in UNITS])
def test_one_more_observation_column_is_refused(unit):
    prefix, make, widest, words = unit
    lib = _native.load()
    cfg, h = make(widest + 1, 1), C.c_void_p()
    assert getattr(lib, f"{prefix}_create")(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_UNSUPPORTED
    assert not h.value
    assert lib.pgx_last_error() == words


def test_obs_keys_stay_importable_from_actor():
    from panda_gym_amd.actor import OBS_KEYS

    assert OBS_KEYS == ("observation", "achieved_goal", "desired_goal")


POLICIES = [lambda: pg.Actor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(16, 8), device="cpu"),
            lambda: pg.ActorCritic(obs_dim=6, action_dim=3, n_envs=4, net_arch=dict(pi=[16, 8], vf=[8]), device="cpu"),
            lambda: pg.SdeActor(obs_dim=6, action_dim=3, n_envs=4, net_arch=(16, 8), device="cpu")]


@pytest.mark.parametrize("make", POLICIES, ids=["Actor", "ActorCritic", "SdeActor"])
@pytest.mark.parametrize("fault", ["shape", "missing"])
def test_a_load_that_fails_on_its_last_key_changes_nothing(make, fault):
    """Every key is validated before the first parameter is copied: the shared loop keeps that for all three."""
    policy = make()
    rng = np.random.default_rng(5)
    first = {k: rng.standard_normal(tuple(v.shape)).astype(np.float32) for k, v in policy.state_dict().items()}
    policy.load_state_dict(first)
    before = {k: v.numpy().copy() for k, v in policy.state_dict().items()}
    assert all(np.array_equal(bits(before[k]), bits(first[k])) for k in first)
    sd = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in first.items()}
    last = [k for k, _ in policy._slots()][-1]
    if fault == "shape":
        sd[last] = np.zeros(tuple(d + 1 for d in sd[last].shape), np.float32)
    else:
        del sd[last]
    with pytest.raises(ValueError if fault == "shape" else KeyError, match=last.replace(".", r"\.")):
        policy.load_state_dict(sd)
    after = policy.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert np.array_equal(bits(after[k].numpy()), bits(before[k])), k
