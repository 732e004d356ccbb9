"""The QuantileCritic C-ABI (include/pgx.h, pgx_qc_*) without a GPU: the ctypes mirrors against the header's
layout through gcc, the exported entry points, every refusal (made before any device call, naming its
field; the launch checks are one function for the device entries and the host models, and are reached here
through the host models), the widest observation, the Python surface, sb3_contrib's key names, and the
arithmetic: pgx_qc_forward_host against an independent restatement that drives libm's fmaf (the Actor's
chain: bias first, k ascending, K rounded up to 16), and pgx_qc_target_host against a numpy f32 restatement
that sorts by the header's integer key with ties by flat index, truncates and applies the four unfused
operations -- both bit for bit.  The Polyak rule has no host path: it is pinned on the GPU only
(test_gpu_quantile_critic.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import panda_gym_amd as pg
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi
from test_actor_abi import bits, chain, random_obs

F32 = np.float32
QC_EXPORTS = ["pgx_qc_create", "pgx_qc_destroy", "pgx_qc_set_weights", "pgx_qc_get_weights", "pgx_qc_forward",
              "pgx_qc_target", "pgx_qc_polyak", "pgx_qc_sync_target", "pgx_qc_forward_host", "pgx_qc_target_host"]


# ---------------------------------------------------------------- helpers shared with the GPU tests
def random_qc_state_dict(qc, rng, which="both", scale=1.0):
    """standard_normal / sqrt(fan_in) weights (biases / 2) under the critic's own key names."""
    sd = {}
    for k, v in qc.state_dict(which).items():
        shape = tuple(v.shape)
        s = scale / np.sqrt(shape[1]) if len(shape) == 2 else 0.5 * scale
        sd[k] = (rng.standard_normal(shape) * s).astype(F32)
    return sd


def qc_features(obs, actions):
    """CombinedExtractor's sorted keys, then th.cat([obs, action], dim=1)."""
    return np.concatenate([obs["achieved_goal"], obs["desired_goal"], obs["observation"], actions], axis=1).astype(F32)


def restated_forward(qc, sd, obs, actions, prefix=""):
    """quantiles [n, n_critics, n_quantiles] f32 by the header's contract, one libm fmaf at a time."""
    x = qc_features(obs, actions)
    nl = len(qc.net_arch)
    out = np.zeros((x.shape[0], qc.n_critics, qc.n_quantiles), F32)
    for c in range(qc.n_critics):
        layers = [(np.asarray(sd[f"{prefix}qf{c}.{2 * l}.weight"], F32), np.asarray(sd[f"{prefix}qf{c}.{2 * l}.bias"], F32))
                  for l in range(nl + 1)]
        for e in range(x.shape[0]):
            h = x[e]
            for W, b in layers[:-1]:
                y = np.array([chain(h, W[o], b[o]) for o in range(W.shape[0])], F32)
                h = np.where(y > 0, y, F32(0.0)).astype(F32)
            W, b = layers[-1]
            out[e, c] = [chain(h, W[o], b[o]) for o in range(qc.n_quantiles)]
    return out


def order_keys(z):
    """The header's key of every f32's bits: u & 0x80000000 ? ~u : u | 0x80000000."""
    u = bits(z).astype(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def restated_target(pool, n_target, ent_coef, next_log_prob, rewards, dones, gamma):
    """[n, n_target] f32: sort each row of the pool by (key, flat index), keep the lowest n_target, then
    t1 = ent * lp; t2 = z - t1; m = (1 - done) * gamma; out = reward + m * t2, one f32 rounding each."""
    pool = np.asarray(pool, F32)
    n, T = pool.shape
    keys = order_keys(pool)
    order = np.stack([np.lexsort((np.arange(T), keys[b])) for b in range(n)])   # last key first: (key, index)
    z = np.take_along_axis(pool, order, axis=1)[:, :n_target]
    with np.errstate(all="ignore"):
        t1 = (F32(ent_coef) * np.asarray(next_log_prob, F32)).astype(F32)[:, None]
        t2 = (z - t1).astype(F32)
        m = ((F32(1.0) - np.asarray(dones, F32)).astype(F32) * F32(gamma)).astype(F32)[:, None]
        return (np.asarray(rewards, F32)[:, None] + (m * t2).astype(F32)).astype(F32)


def make_qc(od, A, arch, nc, nq, drop=0, gamma=0.98, device="cpu", seed=0, scale=1.0):
    """A QuantileCritic with two different random parameter sets loaded; returns it and the prefixed dict."""
    qc = pg.QuantileCritic(obs_dim=od, action_dim=A, net_arch=arch, n_critics=nc, n_quantiles=nq,
                           top_quantiles_to_drop_per_net=drop, gamma=gamma, device=device)
    sd = random_qc_state_dict(qc, np.random.default_rng(seed), scale=scale)
    qc.load_state_dict(sd)
    return qc, sd


def crafted_bias_dict(qc, rng):
    """Random hidden layers, zero last-layer weights and crafted last-layer biases in the target set, so the
    pooled quantiles ARE the biases: duplicates, -0 beside +0, a descending run, subnormals, infinities.  The
    zero weights are -0 and the last hidden width is 16 (no padding term): every product is -0 (the ReLU
    gives +0 or more), and b + -0 = b for every b, -0 included, where +0 products would turn a -0 bias into +0."""
    assert qc.net_arch[-1] == 16
    sd = random_qc_state_dict(qc, rng)
    nl, nq = len(qc.net_arch), qc.n_quantiles
    special = np.array([1.5, -0.0, 0.0, 1.5, 0.0, -0.0, -2.0, 1e-45, -1e-45, np.inf, -np.inf, 1.5], F32)
    pool = np.concatenate([special, np.arange(qc.n_pool - special.size, 0, -1).astype(F32) * F32(0.25) + F32(0.125)])[:qc.n_pool]
    for c in range(qc.n_critics):
        sd[f"critic_target.qf{c}.{2 * nl}.weight"] = np.full((nq, qc.net_arch[-1]), -0.0, F32)
        sd[f"critic_target.qf{c}.{2 * nl}.bias"] = pool[c * nq:(c + 1) * nq].copy()
    return sd, pool


def target_inputs(rng, n):
    return {"next_log_prob": rng.standard_normal(n).astype(F32), "rewards": rng.standard_normal(n).astype(F32),
            "dones": (np.arange(n) % 2).astype(F32)}


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    structs = {"pgx_qc_config": abi.PgxQcConfig, "pgx_qc_weights": abi.PgxQcWeights, "pgx_qc_io": abi.PgxQcIo}
    out = header_layout(structs, ['printf("consts %d %d %d %d %d\\n", PGX_QC_ONLINE, PGX_QC_TARGET, PGX_QC_MAX_CRITICS, '
                 'PGX_QC_MAX_QUANTILES, PGX_QC_MAX_POOL);'])
    assert out["consts"] == f"{abi.QC_ONLINE} {abi.QC_TARGET} {abi.QC_MAX_CRITICS} {abi.QC_MAX_QUANTILES} {abi.QC_MAX_POOL}"
    assert abi.QC_SETS == {"online": 0, "target": 1}
    # weight[c][l]: critic-major, four Linears each
    w = abi.PgxQcWeights()
    w.weight[2][3] = 0x1234
    assert C.cast(C.byref(w), C.POINTER(C.c_void_p))[2 * 4 + 3] == 0x1234


def test_library_exports_the_entry_points():
    assert_exported(QC_EXPORTS)


def good_config(obs_dim=6, hidden0=16, n_critics=2, n_quantiles=5):
    c = abi.PgxQcConfig()
    c.obs_dim, c.action_dim, c.n_layers, c.n_critics, c.n_quantiles, c.gamma = obs_dim, 3, 1, n_critics, n_quantiles, 0.98
    c.hidden[0] = hidden0
    return c


BAD = [("obs_dim", 0, b"obs_dim"), ("obs_dim", -1, b"obs_dim"), ("obs_dim", 4097, b"obs_dim"),
       ("action_dim", 0, b"action_dim"), ("action_dim", 8, b"action_dim"), ("n_layers", 0, b"n_layers"),
       ("n_layers", 4, b"n_layers"), ("hidden0", 0, b"hidden"), ("hidden0", 513, b"hidden"), ("n_critics", 0, b"n_critics"),
       ("n_critics", 6, b"n_critics"), ("n_quantiles", 0, b"n_quantiles"), ("n_quantiles", 33, b"n_quantiles"),
       ("product", None, b"n_critics * n_quantiles"), ("gamma", float("nan"), b"gamma"), ("gamma", float("inf"), b"gamma")]


@pytest.mark.parametrize("field,value,word", BAD)
def test_create_rejects_bad_config_without_a_device(field, value, word):
    """PGX_E_INVALID comes from the argument check, before any HIP call: this runs without a GPU (a HIP
    failure would be PGX_E_HIP), and the message names the field."""
    lib = _native.load()
    cfg = good_config()
    if field == "hidden0":
        cfg.hidden[0] = value
    elif field == "product":
        cfg.n_critics, cfg.n_quantiles = 5, 26   # each in range, 130 > 128
    else:
        setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.pgx_qc_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_qc_create" in msg and word in msg, msg
    if field == "product":
        cfg.n_critics, cfg.n_quantiles = 4, 32   # 128 is accepted
        assert lib.pgx_qc_create(C.byref(cfg), 0, C.byref(h)) in (abi.PGX_OK, abi.PGX_E_HIP)
        if h.value:
            lib.pgx_qc_destroy(h)


def _host_call(n=3, n_target=4):
    """Everything a host-model call takes, valid: (cfg, weights, io, n, n_target, keep-alive)."""
    cfg = good_config()
    rng = np.random.default_rng(0)
    w, keep = abi.PgxQcWeights(), []
    for c in range(2):
        for l, shape in enumerate([(16, 12), (5, 16)]):
            W, b = rng.standard_normal(shape).astype(F32), rng.standard_normal(shape[0]).astype(F32)
            w.weight[c][l], w.bias[c][l] = W.ctypes.data, b.ctypes.data
            keep += [W, b]
    arrays = {"obs": (n, 6), "achieved_goal": (n, 3), "desired_goal": (n, 3), "action": (n, 3), "reward": (n,),
              "done": (n,), "next_log_prob": (n,), "ent_coef": (1,), "out": (n, 10), "quantiles_out": (n, 10)}
    io = abi.PgxQcIo()
    for k, shape in arrays.items():
        a = np.zeros(shape, F32)
        setattr(io, k, a.ctypes.data)
        keep.append(a)
    io.obs_stride, io.achieved_goal_stride, io.desired_goal_stride, io.action_stride = 6, 3, 3, 3
    io.reward_stride = io.done_stride = 1
    return cfg, w, io, n, n_target, keep


# (field, value, the words of the message, also refused by the forward)
BAD_LAUNCH = [("obs", None, b"null obs", True), ("achieved_goal", None, b"null achieved_goal", True),
              ("desired_goal", None, b"null desired_goal", True), ("action", None, b"null action", True),
              ("out", None, b"null out", True), ("reward", None, b"null reward", False), ("done", None, b"null done", False),
              ("next_log_prob", None, b"null next_log_prob", False), ("ent_coef", None, b"null ent_coef", False),
              ("B", 0, b"B must be > 0", True), ("B", -3, b"B must be > 0", True),
              ("n_target", 0, b"n_target", False), ("n_target", 11, b"n_target", False), ("n_target", -1, b"n_target", False),
              ("obs_stride", 5, b"obs_stride", True), ("achieved_goal_stride", 2, b"achieved_goal_stride", True),
              ("desired_goal_stride", 0, b"desired_goal_stride", True), ("action_stride", 2, b"action_stride", True),
              ("reward_stride", 0, b"reward_stride", False), ("done_stride", -1, b"done_stride", False)]


@pytest.mark.parametrize("field,value,words,forward_too", BAD_LAUNCH, ids=[f"{b[0]}={b[1]}" for b in BAD_LAUNCH])
def test_launch_checks_refuse_without_a_device(field, value, words, forward_too):
    """pgx_qc_check_launch, the one function pgx_qc_forward / pgx_qc_target and the host models call in front
    of anything else: every refusal names its field; the valid call passes."""
    lib = _native.load()
    cfg, w, io, n, n_target, keep = _host_call()
    assert lib.pgx_qc_target_host(C.byref(cfg), C.byref(w), C.byref(io), n, n_target) == abi.PGX_OK
    assert lib.pgx_qc_forward_host(C.byref(cfg), C.byref(w), C.byref(io), n) == abi.PGX_OK
    if field == "B":
        n = value
    elif field == "n_target":
        n_target = value
    else:
        setattr(io, field, value)
    assert lib.pgx_qc_target_host(C.byref(cfg), C.byref(w), C.byref(io), n, n_target) == abi.PGX_E_INVALID
    msg = lib.pgx_last_error()
    assert b"pgx_qc_target_host" in msg and words in msg, msg
    rc = lib.pgx_qc_forward_host(C.byref(cfg), C.byref(w), C.byref(io), n)
    assert rc == (abi.PGX_E_INVALID if forward_too else abi.PGX_OK)
    if forward_too:
        msg = lib.pgx_last_error()
        assert b"pgx_qc_forward_host" in msg and words in msg, msg


@pytest.mark.parametrize("tau", [-0.01, 1.0000001, float("nan"), float("inf")])
def test_polyak_refuses_tau_without_a_device(tau):
    lib = _native.load()
    assert lib.pgx_qc_polyak(None, tau, None) == abi.PGX_E_INVALID
    msg = lib.pgx_last_error()
    assert b"pgx_qc_polyak" in msg and b"tau" in msg, msg
    assert lib.pgx_qc_polyak(None, 0.5, None) == abi.PGX_E_INVALID   # then the handle
    assert b"null handle" in lib.pgx_last_error()


def test_null_handles_and_pointers_are_rejected():
    lib = _native.load()
    h = C.c_void_p()
    cfg, w, io, n, n_target, keep = _host_call()
    assert lib.pgx_qc_create(None, 0, C.byref(h)) == abi.PGX_E_INVALID
    assert lib.pgx_qc_create(C.byref(cfg), 0, None) == abi.PGX_E_INVALID
    assert b"null" in lib.pgx_last_error()
    for rc in (lib.pgx_qc_set_weights(None, 0, C.byref(w), None), lib.pgx_qc_get_weights(None, 0, C.byref(w), None),
               lib.pgx_qc_forward(None, 0, C.byref(io), n, None), lib.pgx_qc_target(None, C.byref(io), n, n_target, None),
               lib.pgx_qc_sync_target(None, None), lib.pgx_qc_forward_host(None, C.byref(w), C.byref(io), n),
               lib.pgx_qc_forward_host(C.byref(cfg), None, C.byref(io), n),
               lib.pgx_qc_forward_host(C.byref(cfg), C.byref(w), None, n),
               lib.pgx_qc_target_host(C.byref(cfg), C.byref(w), None, n, n_target)):
        assert rc == abi.PGX_E_INVALID
        assert b"null" in lib.pgx_last_error()
    w.bias[1][1] = None
    assert lib.pgx_qc_forward_host(C.byref(cfg), C.byref(w), C.byref(io), n) == abi.PGX_E_INVALID
    assert b"null weight or bias" in lib.pgx_last_error()
    lib.pgx_qc_destroy(None)   # a no-op


def test_widest_observation_is_accepted_and_one_more_column_refused():
    """One hidden layer of 16, one critic, one quantile, action_dim 3: a workgroup of 16 rows needs
    64 (K16 + 4 + 2 * 20 + 20) bytes, so K16 = 2480 (obs_dim 2471) is the last that fits 160 KiB less the
    static words.  Accepted is PGX_E_HIP without a device, PGX_OK with one."""
    lib = _native.load()
    cfg, h = good_config(obs_dim=2471, n_critics=1, n_quantiles=1), C.c_void_p()
    rc = lib.pgx_qc_create(C.byref(cfg), 0, C.byref(h))
    assert rc in (abi.PGX_OK, abi.PGX_E_HIP), (rc, lib.pgx_last_error())
    if rc == abi.PGX_OK:
        lib.pgx_qc_destroy(h)
    cfg, h = good_config(obs_dim=2472, n_critics=1, n_quantiles=1), C.c_void_p()
    assert lib.pgx_qc_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_UNSUPPORTED
    assert not h.value
    assert lib.pgx_last_error() == b"pgx_qc_create: obs_dim too wide for the features in LDS"


def test_python_surface_is_exported():
    sig = inspect.signature(pg.QuantileCritic.__init__).parameters
    assert list(sig)[1:] == ["env", "obs_dim", "action_dim", "net_arch", "n_critics", "n_quantiles",
                             "top_quantiles_to_drop_per_net", "gamma", "device"]
    want = {"env": None, "obs_dim": None, "action_dim": None, "net_arch": (256, 256), "n_critics": 2, "n_quantiles": 25,
            "top_quantiles_to_drop_per_net": 2, "gamma": 0.99, "device": None}
    for k, v in want.items():
        assert sig[k].default == v, k
    for name in ("critic", "td_target", "td_target_rows", "polyak_update", "sync_target", "state_dict", "load_state_dict",
                 "forward_host", "td_target_host", "close"):
        assert hasattr(pg.QuantileCritic, name), name
    assert list(inspect.signature(pg.QuantileCritic.critic).parameters)[1:4] == ["obs", "actions", "target"]
    assert list(inspect.signature(pg.QuantileCritic.td_target).parameters)[1:8] == [
        "next_obs", "next_actions", "next_log_prob", "rewards", "dones", "ent_coef", "out"]
    assert list(inspect.signature(pg.QuantileCritic.td_target_rows).parameters)[1:6] == [
        "batch", "next_actions", "next_log_prob", "ent_coef", "out"]
    assert "QuantileCritic" in pg.__all__
    q = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8,), device="cpu")
    assert (q.n_pool, q.n_target) == (50, 46)   # T - top_quantiles_to_drop_per_net * n_critics
    assert pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8,), n_critics=5, n_quantiles=25,
                             top_quantiles_to_drop_per_net=5, device="cpu").n_target == 100   # the reference's TQC_v2
    with pytest.raises(ValueError, match="top_quantiles_to_drop_per_net"):
        pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8,), n_quantiles=5, top_quantiles_to_drop_per_net=5,
                          device="cpu")
    with pytest.raises(pg.PgxError, match="n_layers"):
        pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8, 8, 8, 8), device="cpu")
    with pytest.raises(pg.PgxError, match="n_critics"):
        pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8,), n_critics=6, n_quantiles=2,
                          top_quantiles_to_drop_per_net=0, device="cpu")
    rng = np.random.default_rng(0)
    obs, a = random_obs(rng, 4, 6), np.zeros((4, 3), F32)
    for call in (lambda: q.critic(obs, a), lambda: q.td_target(obs, a, np.zeros(4), np.zeros(4), np.zeros(4), 0.1),
                 lambda: q.polyak_update(0.02), q.sync_target):
        with pytest.raises(pg.PgxError, match="no CPU fallback"):
            call()


# ---------------------------------------------------------------- state dicts
def test_state_dict_keys_prefixes_and_round_trip():
    rng = np.random.default_rng(1)
    q = pg.QuantileCritic(obs_dim=19, action_dim=4, net_arch=(16, 8), n_critics=2, n_quantiles=5, device="cpu")
    keys = [f"qf{c}.{l}.{p}" for c in range(2) for l in (0, 2, 4) for p in ("weight", "bias")]
    assert list(q.state_dict()) == keys and list(q.state_dict("target")) == keys
    assert list(q.state_dict("both")) == [f"critic.{k}" for k in keys] + [f"critic_target.{k}" for k in keys]
    assert [tuple(v.shape) for v in q.state_dict().values()] == [(16, 29), (16,), (8, 16), (8,), (5, 8), (5,)] * 2
    # a whole policy's dict: both sets, everything else ignored
    policy = random_qc_state_dict(q, rng)
    policy["actor.mu.weight"] = np.zeros((4, 8), F32)
    policy["qf0.0.weight"] = np.zeros((1, 1), F32)   # not a critic's: no prefix in a prefixed dict
    q.load_state_dict(policy)
    for which, p in (("online", "critic."), ("target", "critic_target.")):
        for k, v in q.state_dict(which).items():
            assert np.array_equal(bits(v.numpy()), bits(policy[p + k])), (which, k)
    # a critic's own dict: the online set by default, the target with which=
    own = random_qc_state_dict(q, rng, which="online")
    q.load_state_dict(own)
    for k, v in q.state_dict().items():
        assert np.array_equal(bits(v.numpy()), bits(own[k])), k
    for k, v in q.state_dict("target").items():
        assert np.array_equal(bits(v.numpy()), bits(policy["critic_target." + k])), k   # untouched
    q.load_state_dict(own, which="target")
    for k, v in q.state_dict("target").items():
        assert np.array_equal(bits(v.numpy()), bits(own[k])), k
    # a policy's dict with which=: that set alone
    policy2 = random_qc_state_dict(q, rng)
    q.load_state_dict(policy2, which="online")
    for k, v in q.state_dict("target").items():
        assert np.array_equal(bits(v.numpy()), bits(own[k])), k
    for k, v in q.state_dict().items():
        assert np.array_equal(bits(v.numpy()), bits(policy2["critic." + k])), k
    with pytest.raises(ValueError, match="which"):
        q.load_state_dict(own, which="both")


@pytest.mark.parametrize("fault", ["shape", "missing"])
def test_a_failed_load_changes_nothing(fault):
    """Every key of both sets is validated before the first parameter is copied (Policy._load_slots)."""
    rng = np.random.default_rng(2)
    q = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(16, 8), n_critics=2, n_quantiles=5, device="cpu")
    first = random_qc_state_dict(q, rng)
    q.load_state_dict(first)
    sd = random_qc_state_dict(q, rng)
    last = "critic_target.qf1.4.bias"
    assert list(sd)[-1] == last
    if fault == "shape":
        sd[last] = np.zeros(6, F32)
    else:
        del sd[last]
    with pytest.raises(ValueError if fault == "shape" else KeyError, match=r"critic_target\.qf1\.4\.bias"):
        q.load_state_dict(sd)
    for k, v in q.state_dict("both").items():
        assert np.array_equal(bits(v.numpy()), bits(first[k])), k


# ---------------------------------------------------------------- the arithmetic contract: forward
# obs_dim, action_dim (K = obs_dim + 6 + action_dim: Reach 15, 16, PickAndPlace 29), net_arch, n_critics,
# n_quantiles, rows
FORWARD = [(6, 3, (16,), 1, 1, 5), (7, 3, (16,), 5, 17, 5), (7, 3, (16,), 2, 16, 5), (19, 4, (256, 256), 2, 25, 3),
           (6, 3, (400, 300), 2, 32, 2), (19, 4, (16,), 5, 25, 3)]


@pytest.mark.parametrize("od,A,arch,nc,nq,n", FORWARD, ids=[f"K{c[0] + 6 + c[1]}-{'x'.join(map(str, c[2]))}-{c[3]}x{c[4]}"
                                                            for c in FORWARD])
def test_forward_host_model_equals_the_restatement_bit_for_bit(od, A, arch, nc, nq, n):
    rng = np.random.default_rng(od * 1000 + nc * 100 + nq)
    qc, sd = make_qc(od, A, arch, nc, nq, seed=od + nq)
    obs, act = random_obs(rng, n, od), rng.uniform(-1, 1, (n, A)).astype(F32)
    for target, prefix in ((False, "critic."), (True, "critic_target.")):
        got = qc.forward_host(obs, act, target=target)
        want = restated_forward(qc, sd, obs, act, prefix)
        assert got.shape == (n, nc, nq) and np.isfinite(got).all()
        assert np.array_equal(bits(got), bits(want)), (target, np.abs(got - want).max())
    assert not np.array_equal(qc.forward_host(obs, act), qc.forward_host(obs, act, target=True))   # two sets


# ---------------------------------------------------------------- the arithmetic contract: target
# n_critics, n_quantiles: T = 1, 50, 64, 65, 128
POOLS = [(1, 1), (2, 25), (2, 32), (5, 13), (4, 32)]


def n_targets(nc, nq):
    return sorted({k for k in (1, nc * nq - 2 * nc, nc * nq) if k >= 1})


@pytest.mark.parametrize("nc,nq", POOLS, ids=[f"T{c * q}" for c, q in POOLS])
def test_target_host_model_equals_the_numpy_restatement_bit_for_bit(nc, nq):
    rng = np.random.default_rng(nc * 100 + nq)
    n, gamma = 6, 0.98
    qc, sd = make_qc(6, 3, (16,), nc, nq, gamma=gamma, seed=nq)
    obs, act = random_obs(rng, n, 6), rng.uniform(-1, 1, (n, 3)).astype(F32)
    x = target_inputs(rng, n)   # dones 0, 1, 0, 1, ...
    ent = F32(0.37)
    for k in n_targets(nc, nq):
        got, pool = qc.td_target_host(obs, act, x["next_log_prob"], x["rewards"], x["dones"], ent, n_target=k,
                                      return_quantiles=True)
        assert np.array_equal(bits(pool), bits(qc.forward_host(obs, act, target=True).reshape(n, -1)))
        want = restated_target(pool, k, ent, x["next_log_prob"], x["rewards"], x["dones"], gamma)
        assert got.shape == (n, k) and np.array_equal(bits(got), bits(want)), k
        done = x["dones"] == 1   # reward + 0 * t2: the reward itself (finite t2)
        assert np.array_equal(got[done], np.repeat(x["rewards"][done, None], k, axis=1))
        assert (np.diff(got[~done], axis=1) >= 0).all()


@pytest.mark.parametrize("nc,nq", [(2, 25), (5, 13), (4, 32)], ids=["T50", "T65", "T128"])
def test_the_order_rule_on_crafted_biases(nc, nq):
    """Zero (-0) last-layer weights: the pool is the biases, whatever the matmul does.  With reward -0, done 0,
    gamma 1, ent_coef 0 and a positive log-probability the backup returns z itself (-0 + 1 * (z - +0) = z, -0 included), so the output
    is the sorted pool: -inf, the negatives, -0 -0 +0 +0 (equal bits in flat-index order, which the values
    cannot show but the restatement's keys fix), the subnormal, the positives with 1.5 three times, +inf."""
    rng = np.random.default_rng(7)
    n, T = 3, nc * nq
    qc = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(16,), n_critics=nc, n_quantiles=nq, gamma=1.0, device="cpu")
    sd, pool = crafted_bias_dict(qc, rng)
    qc.load_state_dict(sd)
    obs, act = random_obs(rng, n, 6), rng.uniform(-1, 1, (n, 3)).astype(F32)
    lp, r, d = np.abs(rng.standard_normal(n)).astype(F32), np.full(n, -0.0, F32), np.zeros(n, F32)   # t1 = +0
    got, z = qc.td_target_host(obs, act, lp, r, d, 0.0, n_target=T, return_quantiles=True)
    assert np.array_equal(bits(z), bits(np.tile(pool, (n, 1))))
    want = restated_target(z, T, 0.0, lp, r, d, 1.0)
    assert np.array_equal(bits(got), bits(want))
    row = got[0]
    assert row[0] == -np.inf and row[-1] == np.inf
    zeros = np.flatnonzero(row == 0)
    assert list(bits(row[zeros])) == [0x80000000, 0x80000000, 0, 0] and row[zeros[0] - 1] < 0 < row[zeros[-1] + 1]
    assert bits(row[zeros[0] - 1:zeros[0]])[0] == 0x80000001 and bits(row[zeros[-1] + 1:zeros[-1] + 2])[0] == 1
    assert (row == F32(1.5)).sum() == 3 and (np.diff(row[1:-1]) >= 0).all()
    # a truncated target is the head of the same order
    part = qc.td_target_host(obs, act, lp, r, d, 0.0, n_target=T - 2 * nc)
    assert np.array_equal(bits(part), bits(got[:, :T - 2 * nc]))


def test_order_keys_are_a_total_order_on_special_values():
    """The restatement's own key: monotone over the f32 line, -0 in front of +0, NaNs at the ends."""
    v = np.array([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 3.0, np.inf], F32)
    k = order_keys(v).astype(np.int64)
    assert (np.diff(k) > 0).all()
    nan_pos, nan_neg = np.array([0x7FC00000], np.uint32).view(F32), np.array([0xFFC00000], np.uint32).view(F32)
    assert order_keys(nan_pos)[0] > k[-1] and order_keys(nan_neg)[0] < k[0]
