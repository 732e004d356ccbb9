"""The RolloutBuffer C-ABI (include/pgx.h, pgx_rollout_*) without a GPU: the ctypes mirrors against the
header's layout through gcc, the exported entry points, pgx_rollout_create's argument checks (made
before any device call), the Python surface, and the two restatements the GPU tests compare against,
written from the rules of include/pgx.h: RefRollout (numpy, SB3's RolloutBuffer: f32 arrays, the
time-limit bootstrap, the GAE loop in SB3's operation order), pinned on a trace small enough to follow
by hand, and the keyed Feistel permutation (ref_permutation), checked to be a bijection, to depend on
both halves of the epoch and to be uniform in its first element."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
M32 = 0xFFFFFFFF

ROLLOUT_EXPORTS = ["pgx_rollout_row_dim", "pgx_rollout_row_stride", "pgx_rollout_create", "pgx_rollout_destroy",
                   "pgx_rollout_add", "pgx_rollout_compute_returns_and_advantage", "pgx_rollout_permutation",
                   "pgx_rollout_gather", "pgx_rollout_reset", "pgx_rollout_set_last", "pgx_rollout_state",
                   "pgx_rollout_arrays"]
ERR_OVERFLOW, ERR_NOT_FULL, ERR_INDEX = 1, 2, 4
EPOCHS = (0, 1, 2 ** 32 + 1)
PLANES = ("observation", "achieved_goal", "desired_goal", "action", "reward", "episode_start", "value", "log_prob")


# ---------------------------------------------------------------- the restatements
class RefRollout:
    """SB3's (Dict)RolloutBuffer in numpy, from include/pgx.h's rules: arrays [T, N, ...] f32, the carry
    (``_last_obs`` / ``_last_episode_starts``, ones at first), ``add`` with collect_rollouts' bootstrap
    ``reward + (float)gamma * terminal_value`` where truncated & ~terminated, the GAE loop with every
    f32 operation rounded on its own, and the sticky error bits."""

    def __init__(self, n_steps, n_envs, obs_dim, action_dim, gamma=0.99, gae_lambda=1.0):
        T, N = n_steps, n_envs
        self.T, self.N, self.gamma, self.gae_lambda = T, N, float(gamma), float(gae_lambda)
        z = lambda *s: np.zeros((T, N) + s, F32)  # noqa: E731
        self.a = {"observation": z(obs_dim), "achieved_goal": z(3), "desired_goal": z(3), "action": z(action_dim),
                  "reward": z(), "episode_start": z(), "value": z(), "log_prob": z(), "advantage": z(), "return": z()}
        self.last = {"observation": np.zeros((N, obs_dim), F32), "achieved_goal": np.zeros((N, 3), F32),
                     "desired_goal": np.zeros((N, 3), F32)}
        self.last_start = np.ones(N, F32)
        self.pos, self.errors = 0, 0

    def reset(self):
        self.pos = 0

    def set_last(self, obs, episode_start=None):
        self.last = {k: np.array(obs[k], F32) for k in self.last}
        self.last_start = np.ones(self.N, F32) if episode_start is None else np.array(episode_start, F32)

    def add(self, action, reward, value, log_prob, obs=None, terminated=None, truncated=None, terminal_value=None):
        if self.pos == self.T:
            self.errors |= ERR_OVERFLOW
            return
        t, a = self.pos, self.a
        for k in self.last:
            a[k][t] = self.last[k]
        a["episode_start"][t] = self.last_start
        a["action"][t], a["value"][t], a["log_prob"][t] = action, value, log_prob
        r = np.array(reward, F32)
        te = np.zeros(self.N, bool) if terminated is None else np.asarray(terminated) != 0
        tr = np.zeros(self.N, bool) if truncated is None else np.asarray(truncated) != 0
        if terminal_value is not None:
            m = tr & ~te
            with np.errstate(invalid="ignore", over="ignore"):
                boot = F32(self.gamma) * np.asarray(terminal_value, F32)[m]   # one f32 multiply
                r[m] = r[m] + boot                                            # one f32 add
        a["reward"][t] = r
        if obs is not None:
            self.last = {k: np.array(obs[k], F32) for k in self.last}
            self.last_start = (te | tr).astype(F32)
        self.pos += 1

    def compute_returns_and_advantage(self, last_values, dones=None):
        if self.pos != self.T:
            self.errors |= ERR_NOT_FULL
            return
        a = self.a
        g, gl = F32(self.gamma), F32(self.gamma * self.gae_lambda)   # the double product rounded once
        last = np.zeros(self.N, F32)
        dones = self.last_start if dones is None else np.asarray(dones, F32)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in reversed(range(self.T)):
                if t == self.T - 1:
                    nnt, nv = F32(1.0) - dones, np.asarray(last_values, F32)
                else:
                    nnt, nv = F32(1.0) - a["episode_start"][t + 1], a["value"][t + 1]
                delta = (a["reward"][t] + (g * nv) * nnt) - a["value"][t]
                last = delta + (gl * nnt) * last
                assert last.dtype == F32 and delta.dtype == F32
                a["advantage"][t] = last
                a["return"][t] = last + a["value"][t]

    def flat(self, key):
        """SB3 swap_and_flatten: flat index p = env * T + step."""
        x = self.a[key].swapaxes(0, 1)
        return x.reshape((self.T * self.N,) + x.shape[2:])


def fmix(h):
    """murmur3's 32-bit finaliser on a Python int or a uint64 array holding 32-bit values."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def perm_keys(seed, epoch, M):
    s = fmix((seed & M32) ^ 0x9E3779B9)
    s = fmix(s ^ ((seed >> 32) & M32))
    s = fmix(s ^ (epoch & M32))
    s = fmix(s ^ ((epoch >> 32) & M32))
    keys = []
    for r in range(6):
        s = fmix((s + 0x9E3779B9 * (r + 1)) & M32)
        keys.append(s)
    k = max(1, (max(M - 1, 1).bit_length() + 1) // 2)
    return keys, k


def _rounds(x, keys, k):
    mask = (1 << k) - 1
    L, R = x >> k, x & mask
    for r in range(6):
        L, R = R, L ^ (fmix((R * 0x9E3779B1 + keys[r]) & M32) & mask)
    return (L << k) | R


def ref_perm_at(seed, epoch, M, i):
    """perm(i) in Python ints."""
    keys, k = perm_keys(seed, epoch, M)
    x = _rounds(i, keys, k)
    while x >= M:
        x = _rounds(x, keys, k)
    return x


def ref_permutation(seed, epoch, M):
    """[perm(0), ..., perm(M - 1)] int32, the walk vectorised over the elements still outside [0, M)."""
    keys, k = perm_keys(seed, epoch, M)
    x = np.arange(M, dtype=np.uint64)
    pending = np.arange(M)
    while len(pending):
        xs = _rounds(x[pending], keys, k)
        x[pending] = xs
        pending = pending[xs >= M]
    return x.astype(np.int32)


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    """ctypes mirrors of pgx_rollout_config / _io / _batch / _views == the header's sizeof / offsetof (gcc, as C)."""
    structs = {"pgx_rollout_config": abi.PgxRolloutConfig, "pgx_rollout_io": abi.PgxRolloutIo,
               "pgx_rollout_batch": abi.PgxRolloutBatch, "pgx_rollout_views": abi.PgxRolloutViews}
    header_layout(structs)
    hdr = open(os.path.join(ROOT, "include", "pgx.h")).read()
    for name, code in (("OVERFLOW", ERR_OVERFLOW), ("NOT_FULL", ERR_NOT_FULL), ("INDEX", ERR_INDEX)):
        assert f"#define PGX_ROLLOUT_ERR_{name} {code}" in hdr and getattr(abi, f"ROLLOUT_ERR_{name}") == code
        assert code in abi.ROLLOUT_ERRORS


def test_library_exports_the_entry_points():
    assert_exported(ROLLOUT_EXPORTS)


def good_config():
    return abi.PgxRolloutConfig(64, 8, 6, 3, 0.99, 0.95, 0)


@pytest.mark.parametrize("field,value", [("n_envs", 0), ("n_envs", -3), ("n_steps", 0), ("n_steps", -1), ("obs_dim", 0),
                                         ("action_dim", 0), ("action_dim", -2), ("gamma", 1.5), ("gamma", -0.1),
                                         ("gamma", float("nan")), ("gae_lambda", 1.0001), ("gae_lambda", -1.0),
                                         ("gae_lambda", float("nan"))])
def test_create_rejects_bad_config_without_a_device(field, value):
    """PGX_E_INVALID comes from the argument check, before any HIP call: this runs without a GPU (a HIP
    failure would be PGX_E_HIP), and the message names the field."""
    lib = _native.load()
    cfg = good_config()
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.pgx_rollout_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_rollout_create" in msg and field.encode() in msg, msg


def test_create_rejects_2_31_transitions_and_null_handles():
    lib = _native.load()
    h = C.c_void_p()
    cfg = good_config()
    cfg.n_envs, cfg.n_steps = 65536, 32768   # 2^31 exactly
    assert lib.pgx_rollout_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID and not h.value
    assert b"2^31" in lib.pgx_last_error() and b"n_steps" in lib.pgx_last_error()
    assert lib.pgx_rollout_create(None, 0, C.byref(h)) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_create(C.byref(good_config()), 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_add(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_compute_returns_and_advantage(None, None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_permutation(None, 0, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_gather(None, None, 1, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_reset(None, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_set_last(None, None, None, None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_state(None, None, None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_arrays(None, None) == abi.PGX_E_INVALID
    lib.pgx_rollout_destroy(None)   # a no-op


def test_row_layout():
    lib = _native.load()
    for od, ad in ((6, 3), (7, 3), (56, 7), (19, 4), (1, 1)):
        cfg = abi.PgxRolloutConfig(4, 4, od, ad, 0.99, 0.95, 0)
        fields, dim = abi.rollout_row_fields(od, ad)
        assert dim == od + 6 + ad + 4 == lib.pgx_rollout_row_dim(C.byref(cfg))
        stride = lib.pgx_rollout_row_stride(C.byref(cfg))
        assert stride % 4 == 0 and dim <= stride < dim + 4
        assert [f[0] for f in fields] == ["observation", "achieved_goal", "desired_goal", "action", "old_value",
                                          "old_log_prob", "advantage", "return"]
        assert [f[1] for f in fields] == [0, od, od + 3, od + 6, od + 6 + ad, od + 7 + ad, od + 8 + ad, od + 9 + ad]
    bad = abi.PgxRolloutConfig(4, 4, 0, 3, 0.99, 0.95, 0)
    assert lib.pgx_rollout_row_dim(C.byref(bad)) == abi.PGX_E_INVALID
    assert lib.pgx_rollout_row_stride(C.byref(bad)) == abi.PGX_E_INVALID


def test_python_surface_is_exported():
    import panda_gym_amd as pg

    sig = inspect.signature(pg.RolloutBuffer.__init__).parameters
    assert list(sig)[1:] == ["buffer_size", "observation_space", "action_space", "device", "gae_lambda", "gamma",
                             "n_envs", "env", "seed", "obs_dim", "action_dim"]
    want = {"observation_space": None, "action_space": None, "device": "cuda:0", "gae_lambda": 1.0, "gamma": 0.99,
            "n_envs": 1, "env": None, "seed": 0, "obs_dim": None, "action_dim": None}
    for k, v in want.items():
        assert sig[k].default == v, k
    for name in ("reset", "set_last", "add_from_vec_env", "add", "compute_returns_and_advantage", "get", "gather",
                 "arrays", "after_step", "raise_device_errors", "pos", "full", "size", "close", "permutation"):
        assert hasattr(pg.RolloutBuffer, name), name
    assert list(inspect.signature(pg.RolloutBuffer.add).parameters)[1:] == ["obs", "action", "reward", "episode_start",
                                                                           "value", "log_prob"]
    assert list(inspect.signature(pg.RolloutBuffer.add_from_vec_env).parameters)[1:] == [
        "venv", "action", "value", "log_prob", "terminal_value"]
    assert list(inspect.signature(pg.RolloutBuffer.after_step).parameters)[1:] == [
        "venv", "actions", "values", "log_probs", "terminal_values"]
    assert inspect.isgeneratorfunction(pg.RolloutBuffer.get)
    assert pg.RolloutBufferSamples._fields == ("observations", "actions", "old_values", "old_log_prob", "advantages",
                                               "returns")
    # the monitor's capture loop takes the buffer's hook behind its own
    assert "after_step" in inspect.signature(pg.VecMonitor.capture_steps).parameters


# ---------------------------------------------------------------- RefRollout, by hand
def test_restatement_on_a_trace_followed_by_hand():
    """2 envs x 3 steps, gamma = gae_lambda = 0.5 (g = 0.5, gl = 0.25: every product below is exact in
    f32).  Env 1 times out at step 0 with terminal value 8 (reward 2 + 0.5 * 8 = 6), so its
    episode_start at step 1 is 1; env 0 terminates at step 2 (the carry's episode_start = dones = [1, 0])."""
    ref = RefRollout(3, 2, 2, 1, gamma=0.5, gae_lambda=0.5)
    o = lambda x: {"observation": np.full((2, 2), x, F32), "achieved_goal": np.full((2, 3), x + 0.25, F32),  # noqa: E731
                   "desired_goal": np.full((2, 3), x + 0.5, F32)}
    f = lambda *x: np.array(x, F32)  # noqa: E731
    u8 = lambda *x: np.array(x, np.uint8)  # noqa: E731
    ref.set_last(o(0.0))
    ref.add(f([1], [1]), f(1, 2), f(0.5, 1), f(-1, -1), o(1.0), u8(0, 0), u8(0, 1), terminal_value=f(4, 8))
    assert ref.a["reward"][0].tolist() == [1.0, 6.0] and ref.last_start.tolist() == [0.0, 1.0]
    ref.add(f([2], [2]), f(1, -1), f(2, 0.5), f(-2, -2), o(2.0), u8(0, 0), u8(0, 0), terminal_value=f(4, 8))
    # terminated wins over truncated: no bootstrap for env 0 at step 2
    ref.add(f([3], [3]), f(0, 3), f(1, 2), f(-3, -3), o(3.0), u8(1, 0), u8(1, 0), terminal_value=f(16, 16))
    assert ref.pos == 3 and ref.errors == 0
    assert ref.a["episode_start"].tolist() == [[1, 1], [0, 1], [0, 0]]
    assert ref.a["reward"].tolist() == [[1, 6], [1, -1], [0, 3]]
    assert ref.a["observation"][:, 0, 0].tolist() == [0.0, 1.0, 2.0]   # the carry of the step before
    assert ref.a["desired_goal"][2, 1].tolist() == [2.5, 2.5, 2.5]
    assert ref.last["observation"][0].tolist() == [3.0, 3.0] and ref.last_start.tolist() == [1.0, 0.0]
    ref.compute_returns_and_advantage(f(4, 2))   # dones: the carry
    # env 0: t2 nnt 0: delta 0 + 0 - 1 = -1, last -1 | t1: delta 1 + .5*1 - 2 = -.5, last -.5 + .25*-1 = -.75
    #        t0: delta 1 + .5*2 - .5 = 1.5, last 1.5 + .25*-.75 = 1.3125
    # env 1: t2 nnt 1: delta 3 + .5*2 - 2 = 2, last 2 | t1: delta -1 + .5*2 - .5 = -.5, last -.5 + .25*2 = 0
    #        t0: nnt 0 (episode_start[1] = 1): delta 6 + 0 - 1 = 5, last 5
    assert ref.a["advantage"].tolist() == [[1.3125, 5.0], [-0.75, 0.0], [-1.0, 2.0]]
    assert ref.a["return"].tolist() == [[1.8125, 6.0], [1.25, 0.5], [0.0, 4.0]]
    assert ref.flat("advantage").tolist() == [1.3125, -0.75, -1.0, 5.0, 0.0, 2.0]   # p = env * T + step
    # explicit dones override the carry
    ref.compute_returns_and_advantage(f(4, 2), dones=u8(0, 0))
    assert ref.a["advantage"][2].tolist() == [0 + 0.5 * 4 - 1, 2.0]
    # one add past full stores nothing and sets the bit; reset keeps the carry
    before = {k: v.copy() for k, v in ref.a.items()}
    ref.add(f([9], [9]), f(9, 9), f(9, 9), f(9, 9), o(9.0), u8(0, 0), u8(0, 0))
    assert ref.errors == ERR_OVERFLOW and all(np.array_equal(before[k], ref.a[k]) for k in before)
    assert ref.last["observation"][0].tolist() == [3.0, 3.0]
    ref.reset()
    assert ref.pos == 0 and ref.last_start.tolist() == [1.0, 0.0]
    ref.compute_returns_and_advantage(f(4, 2))
    assert ref.errors == ERR_OVERFLOW | ERR_NOT_FULL


def test_restatement_is_sb3s_expression():
    """The explicit casts of RefRollout against SB3's own lines (f32 arrays, Python-float gamma), bit for bit."""
    rng = np.random.default_rng(5)
    T, N, gamma, lam = 7, 33, 0.99, 0.95
    ref = RefRollout(T, N, 2, 1, gamma, lam)
    ref.a["reward"][:] = rng.standard_normal((T, N)).astype(F32)
    ref.a["value"][:] = rng.standard_normal((T, N)).astype(F32)
    ref.a["episode_start"][:] = (rng.random((T, N)) < 0.2).astype(F32)
    ref.pos = T
    last_values, dones = rng.standard_normal(N).astype(F32), rng.random(N) < 0.2
    ref.compute_returns_and_advantage(last_values, dones)
    rewards, values, starts = ref.a["reward"], ref.a["value"], ref.a["episode_start"]
    adv = np.zeros((T, N), F32)
    last_gae_lam = 0
    for step in reversed(range(T)):   # stable_baselines3/common/buffers.py RolloutBuffer.compute_returns_and_advantage
        if step == T - 1:
            next_non_terminal = 1.0 - dones.astype(np.float32)
            next_values = last_values
        else:
            next_non_terminal = 1.0 - starts[step + 1]
            next_values = values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * lam * next_non_terminal * last_gae_lam
        adv[step] = last_gae_lam
    assert delta.dtype == F32
    assert np.array_equal(adv.view(np.uint32), ref.a["advantage"].view(np.uint32))
    assert np.array_equal((adv + values).view(np.uint32), ref.a["return"].view(np.uint32))


# ---------------------------------------------------------------- the permutation
@pytest.mark.parametrize("M", [1, 2, 3, 5, 64, 96, 480, 4097])
def test_permutation_is_a_bijection(M):
    for epoch in EPOCHS:
        p = ref_permutation(7, epoch, M)
        assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(M)), (M, epoch)
        for i in {0, M // 2, M - 1}:
            assert ref_perm_at(7, epoch, M, i) == p[i]   # the scalar walk agrees with the vectorised one


def test_permutation_depends_on_both_halves_of_epoch_and_on_the_seed():
    M = 480
    p = [ref_permutation(7, e, M) for e in EPOCHS]
    assert not np.array_equal(p[0], p[1]) and not np.array_equal(p[1], p[2]) and not np.array_equal(p[0], p[2])
    assert not np.array_equal(p[0], ref_permutation(8, 0, M))
    assert not np.array_equal(p[0], ref_permutation(7 + 2 ** 32, 0, M))
    assert np.array_equal(p[1], ref_permutation(7, 1, M))   # a pure function


def test_permutation_first_element_is_uniform():
    """chi^2 of perm[0] over 2000 epochs at M = 96 (95 degrees of freedom) below 160: p ~ 3e-5."""
    M, E = 96, 2000
    counts = np.bincount([ref_perm_at(0, e, M, 0) for e in range(E)], minlength=M)
    chi2 = float(((counts - E / M) ** 2 / (E / M)).sum())
    print(f"chi^2 of perm[0] over {E} epochs at M = {M}: {chi2:.1f}")
    assert chi2 < 160.0
