"""Device-resident VecNormalize: stable-baselines3's observation / reward normalisation over a
``PandaVecEnv``, the wrapper the reference's training settings switch on
(classes/hyperparameters.py:42 ``normalize = True``; :116 for TQC on PandaReach).

Mirrors ``stable_baselines3.common.vec_env.VecNormalize``: running mean / variance per
observation column (``RunningMeanStd(epsilon=1e-4)``), reward scaling by the running variance of
the discounted returns, clipping, ``training`` / ``norm_obs`` / ``norm_reward`` switches,
``normalize_obs`` / ``unnormalize_obs`` / ``normalize_reward`` / ``unnormalize_reward``,
``get_original_obs`` / ``get_original_reward``, ``save`` / ``load`` -- with the statistics and the
arithmetic on the device (libpgx.so, pgx_norm.hip; C-ABI in include/pgx.h).  A normalised step is
the env's step launch plus two more on the same stream, so it captures into a HIP graph
(``capture_steps``) and never leaves HBM (``step_tensors``); ``HerReplayBuffer.sample(batch_size,
env=vec_normalize)`` normalises a sampled batch through the same statistics.  No CPU fallback.

``Normalizer`` is the low-level binding (one handle, raw device tensors in and out);
``VecNormalize`` wraps an env with it.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import abi
from ._handle import Handle, torch
from ._native import check, load

KEYS = abi.NORM_KEYS


def key_mask(keys: Optional[Sequence[str]]) -> int:
    """PGX_NORM_KEY_* bits of ``norm_obs_keys`` (None: all three keys)."""
    if keys is None:
        return abi.NORM_KEY_ALL
    m = 0
    for k in keys:
        if k not in abi.NORM_KEY_BITS:
            raise ValueError(f"norm_obs_keys: unknown key {k!r}; the observation keys are {list(KEYS)}")
        m |= abi.NORM_KEY_BITS[k]
    return m


class RunningMeanStd:
    """``mean``, ``var`` (fp64 numpy) and ``count`` of one key as read from the device
    (stable_baselines3.common.running_mean_std.RunningMeanStd's attributes)."""

    def __init__(self, mean: np.ndarray, var: np.ndarray, count: float):
        self.mean, self.var, self.count = mean, var, float(count)

    def __repr__(self) -> str:
        return f"RunningMeanStd(mean={self.mean!r}, var={self.var!r}, count={self.count!r})"


class Normalizer(Handle):
    """One pgx_norm handle: statistics of ``obs_dim + 6`` observation columns (observation,
    achieved_goal, desired_goal) and of the returns, on ``device``."""

    _PREFIX = "pgx_norm"

    def __init__(self, n_envs: int, obs_dim: int, device: Any = "cuda:0", keys: int = abi.NORM_KEY_ALL,
                 norm_reward: bool = True, clip_obs: float = 10.0, clip_reward: float = 10.0, gamma: float = 0.99,
                 epsilon: float = 1e-8, training: bool = True, lib=None):
        self._need_torch()
        self.lib = lib or load()
        self._on_device(device)
        self.n_envs, self.obs_dim = int(n_envs), int(obs_dim)
        self.columns = self.obs_dim + 6
        cfg = abi.PgxNormConfig(self.n_envs, self.obs_dim, int(keys), 1 if norm_reward else 0, float(clip_obs),
                                float(clip_reward), float(gamma), float(epsilon))
        self._cfg = cfg
        self.keys, self.norm_reward = int(keys), bool(norm_reward)
        self._create(cfg)
        self.training = True
        if not training:
            self.set_training(False)

    # ------------------------------------------------------------ launches
    def step(self, io: abi.PgxNormIo) -> None:
        """pgx_norm_step over the device buffers ``io`` names (two launches, no allocation)."""
        check(self.lib.pgx_norm_step(self._h, C.byref(io), self._stream()), "pgx_norm_step", self.lib)

    def reset(self, io: abi.PgxNormIo) -> None:
        self._call("reset", self._h, C.byref(io), self._stream())

    def rows(self, rows: "torch.Tensor", action_dim: int) -> None:
        """Normalise a HER batch ``rows`` [B, row_stride] (include/pgx.h layout) in place."""
        if rows.dtype != torch.float32 or rows.device != self.device or not rows.is_contiguous() or rows.dim() != 2:
            raise ValueError(f"rows must be a contiguous f32 [B, row_stride] tensor on {self.device}")
        self._call("rows", self._h, C.c_void_p(rows.data_ptr()), C.c_int64(rows.shape[0]), int(action_dim),
                   int(rows.shape[1]), self._stream())

    normalize_rows = rows   # what HerReplayBuffer.sample_into(..., env=) calls

    def apply(self, key: int, x: "torch.Tensor", inverse: bool = False) -> "torch.Tensor":
        """Stateless (un)normalisation of ``x`` [..., width] by one key's statistics (key 3: rewards,
        any shape), whatever the key mask says; returns a new f32 tensor of ``x``'s shape."""
        w = (self.obs_dim, 3, 3, 1)[key]
        a = x.to(device=self.device, dtype=torch.float32).contiguous()
        if key != abi.NORM_REWARD and (a.dim() == 0 or a.shape[-1] != w):
            raise ValueError(f"{KEYS[key]} arrays must end in {w} columns, got shape {tuple(a.shape)}")
        out = torch.empty_like(a)
        self._call("apply", self._h, int(key), 1 if inverse else 0, C.c_void_p(a.data_ptr()), C.c_void_p(out.data_ptr()),
                   C.c_int64(a.numel() // w), self._stream())
        self._keep = a   # read by the queued launch
        return out

    def set_training(self, training: bool) -> None:
        self._call("set_training", self._h, 1 if training else 0, self._stream())
        self.training = bool(training)

    def set_keys(self, keys: int, norm_reward: bool) -> None:
        self._call("set_keys", self._h, int(keys), 1 if norm_reward else 0)
        self.keys, self.norm_reward = int(keys), bool(norm_reward)

    # ---------------------------------------------------------- statistics
    def get_stats(self):
        """(mean, var, count) [obs_dim + 7] fp64 -- the returns column last -- and returns [n_envs]."""
        S = self.columns + 1
        mean, var, count = np.empty(S), np.empty(S), np.empty(S)
        ret = np.empty(self.n_envs)
        self._call("get_stats", self._h, abi.ptr(mean), abi.ptr(var), abi.ptr(count), abi.ptr(ret), self._stream())
        return mean, var, count, ret

    def set_stats(self, mean, var, count, returns=None) -> None:
        S = self.columns + 1
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (mean, var, count)]
        for a in arrs:
            if a.shape != (S,):
                raise ValueError(f"statistics arrays must have shape ({S},), got {a.shape}")
        ret = None
        if returns is not None:
            ret = np.ascontiguousarray(returns, dtype=np.float64)
            if ret.shape != (self.n_envs,):
                raise ValueError(f"returns must have shape ({self.n_envs},), got {ret.shape}")
        self._call("set_stats", self._h, abi.ptr(arrs[0]), abi.ptr(arrs[1]), abi.ptr(arrs[2]), abi.ptr(ret),
                   self._stream())

    # ------------------------------------------- array-level step (tests, tools)
    def alloc_outputs(self) -> Dict[str, "torch.Tensor"]:
        n, od, kw = self.n_envs, self.obs_dim, dict(dtype=torch.float32, device=self.device)
        return {"observation": torch.zeros((n, od), **kw), "achieved_goal": torch.zeros((n, 3), **kw),
                "desired_goal": torch.zeros((n, 3), **kw), "reward": torch.zeros((n,), **kw),
                "terminal_obs": torch.zeros((n, od), **kw), "terminal_ag": torch.zeros((n, 3), **kw),
                "terminal_dg": torch.zeros((n, 3), **kw)}

    def step_arrays(self, obs, achieved_goal, desired_goal, reward, terminated, truncated, terminal_obs=None,
                    terminal_ag=None, terminal_dg=None, out: Optional[Dict[str, "torch.Tensor"]] = None):
        """One pgx_norm_step over host or device arrays (copied to fresh device buffers): returns the
        output tensors of ``alloc_outputs`` (``out`` to reuse them)."""
        n, od, f, u8 = self.n_envs, self.obs_dim, torch.float32, torch.uint8
        out = out or self.alloc_outputs()
        t = [self._dev(obs, (n, od), f), self._dev(achieved_goal, (n, 3), f), self._dev(desired_goal, (n, 3), f),
             self._dev(reward, (n,), f), self._dev(terminated, (n,), u8), self._dev(truncated, (n,), u8)]
        term = [None if x is None else self._dev(x, s, f)
                for x, s in ((terminal_obs, (n, od)), (terminal_ag, (n, 3)), (terminal_dg, (n, 3)))]
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        io = abi.PgxNormIo(*[p(x) for x in t], *[p(x) for x in term], None,
                           *[out[k].data_ptr() for k in ("observation", "achieved_goal", "desired_goal", "reward",
                                                         "terminal_obs", "terminal_ag", "terminal_dg")], None, 0, 0)
        self.step(io)
        self._keep = t + term
        return out

    def reset_arrays(self, obs, achieved_goal, desired_goal, out: Optional[Dict[str, "torch.Tensor"]] = None):
        n, od, f = self.n_envs, self.obs_dim, torch.float32
        out = out or self.alloc_outputs()
        t = [self._dev(obs, (n, od), f), self._dev(achieved_goal, (n, 3), f), self._dev(desired_goal, (n, 3), f)]
        io = abi.PgxNormIo()
        io.obs, io.achieved_goal, io.desired_goal = (x.data_ptr() for x in t)
        io.out_obs, io.out_achieved_goal, io.out_desired_goal = (out[k].data_ptr() for k in KEYS)
        self.reset(io)
        self._keep = t
        return out


class VecNormalize:
    """SB3 ``VecNormalize`` over a ``PandaVecEnv``, on the device.

    ``step_tensors`` / ``reset_tensors`` / ``capture_steps`` are the device path (normalised
    observations and reward in this wrapper's own persistent buffers; the env's raw buffers are
    never written); ``reset`` / ``step_async`` / ``step_wait`` / ``step`` the SB3 path (numpy, one
    pinned D2H copy per step).  Every other attribute forwards to the wrapped env (``num_envs``,
    ``obs_dim``, ``compute_reward``, ``env_method``, ``state``, the raw output tensors ``obs``,
    ``reward``, ``terminal_obs`` ...).  ``training = False`` freezes every statistic."""

    def __init__(self, venv, training: bool = True, norm_obs: bool = True, norm_reward: bool = True,
                 clip_obs: float = 10.0, clip_reward: float = 10.0, gamma: float = 0.99, epsilon: float = 1e-8,
                 norm_obs_keys: Optional[List[str]] = None):
        self.venv = venv
        self.norm_obs_keys = list(KEYS) if norm_obs_keys is None else list(norm_obs_keys)
        self._key_bits = key_mask(norm_obs_keys)
        self._norm_obs, self._norm_reward = bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), \
            float(epsilon)
        self._norm = Normalizer(venv.num_envs, venv.obs_dim, device=venv.device,
                                keys=self._key_bits if norm_obs else 0, norm_reward=norm_reward, clip_obs=clip_obs,
                                clip_reward=clip_reward, gamma=gamma, epsilon=epsilon, training=training, lib=venv.lib)
        n, od = venv.num_envs, venv.obs_dim
        # the env's own output layout (f32 arrays, then the u8 flags the step carries along), so the
        # SB3 path brings a normalised step back with a single D2H copy
        f32 = [("observation", (n, od)), ("achieved_goal", (n, 3)), ("desired_goal", (n, 3)), ("reward", (n,)),
               ("terminal_obs", (n, od)), ("terminal_ag", (n, 3)), ("terminal_dg", (n, 3))]
        nf = sum(int(np.prod(s)) for _, s in f32)
        rows = int(venv._out_u8.shape[0])
        self._outbuf = torch.zeros(4 * nf + rows * n, dtype=torch.uint8, device=venv.device)
        self._out_f32 = self._outbuf[:4 * nf].view(torch.float32)
        self._flags = self._outbuf[4 * nf:].view(rows, n)
        self._n: Dict[str, "torch.Tensor"] = {}
        o = 0
        for name, shape in f32:
            k = int(np.prod(shape))
            self._n[name] = self._out_f32[o:o + k].view(shape)
            o += k
        p = lambda t: t.data_ptr()  # noqa: E731
        self._io = abi.PgxNormIo(
            p(venv.obs), p(venv.achieved_goal), p(venv.desired_goal), p(venv.reward), p(venv.terminated),
            p(venv.truncated), p(venv.terminal_obs), p(venv.terminal_ag), p(venv.terminal_dg), p(venv._out_u8),
            p(self._n["observation"]), p(self._n["achieved_goal"]), p(self._n["desired_goal"]), p(self._n["reward"]),
            p(self._n["terminal_obs"]), p(self._n["terminal_ag"]), p(self._n["terminal_dg"]), p(self._flags), rows, 0)
        self._hs = None
        self.observation_space = self._make_space()

    # ------------------------------------------------------------ plumbing
    def __getattr__(self, name: str):
        if name in ("venv", "_norm"):   # (not set yet: no recursion)
            raise AttributeError(name)
        return getattr(self.venv, name)

    def _make_space(self):
        from .envs import Box, DictSpace, _gym_spaces

        src = self.venv.observation_space
        out = {}
        for k in KEYS:
            if self._norm_obs and k in self.norm_obs_keys:
                n = self.venv.obs_dim if k == "observation" else 3
                out[k] = (_gym_spaces.Box(-self.clip_obs, self.clip_obs, shape=(n,), dtype=np.float32)
                          if _gym_spaces is not None else Box(-self.clip_obs, self.clip_obs, (n,)))
            else:
                out[k] = src[k]
        return _gym_spaces.Dict(out) if _gym_spaces is not None else DictSpace(**out)

    def close(self) -> None:
        if getattr(self, "_norm", None) is not None:
            self._norm.close()
        self.venv.close()

    def _push_keys(self) -> None:
        self._norm.set_keys(self._key_bits if self._norm_obs else 0, self._norm_reward)
        self.observation_space = self._make_space()

    @property
    def training(self) -> bool:
        return self._norm.training

    @training.setter
    def training(self, value: bool) -> None:
        self._norm.set_training(bool(value))

    @property
    def norm_obs(self) -> bool:
        return self._norm_obs

    @norm_obs.setter
    def norm_obs(self, value: bool) -> None:
        self._norm_obs = bool(value)
        self._push_keys()

    @property
    def norm_reward(self) -> bool:
        return self._norm_reward

    @norm_reward.setter
    def norm_reward(self, value: bool) -> None:
        self._norm_reward = bool(value)
        self._push_keys()

    def _obs_out(self) -> Dict[str, "torch.Tensor"]:
        return {k: self._n[k] for k in KEYS}

    # ---------------------------------------------------------- device path
    def reset_tensors(self, seed: Optional[int] = None, **kwargs) -> Dict[str, "torch.Tensor"]:
        """``PandaVecEnv.reset_tensors`` plus VecNormalize.reset: returns zeroed, statistics updated
        from the reset observations (training), which come back normalised.  ``mask`` is rejected:
        a partial reset has no VecNormalize meaning."""
        if kwargs.get("mask") is not None:
            raise ValueError("VecNormalize.reset_tensors takes no mask: VecNormalize.reset resets every env")
        self.venv.reset_tensors(seed=seed, **kwargs)
        self._norm.reset(self._io)
        return self._obs_out()

    def step_tensors(self, actions: "torch.Tensor"):
        """Device-resident step -> (obs dict, reward, terminated, truncated, success): observations and
        reward normalised, in this wrapper's persistent buffers (overwritten by the next step)."""
        _, _, term, trunc, succ = self.venv.step_tensors(actions)
        self._norm.step(self._io)
        return self._obs_out(), self._n["reward"], term, trunc, succ

    def _enqueue_step(self, a: "torch.Tensor", what: str = "pgx_step") -> None:
        """The env step's launch and the normalisation's two, on the current stream."""
        self.venv._enqueue_step(a, what)
        self._norm.step(self._io)

    def capture_steps(self, k: int, actions: Optional["torch.Tensor"] = None, after_step=None):
        """``PandaVecEnv.capture_steps`` with the normalisation behind every env step: one HIP graph
        of ``k`` x (env step, moments, apply).  Statistics move on replay, by the value ``training``
        has then.  ``after_step``: as in ``PandaVecEnv.capture_steps``."""
        v = self.venv
        if actions is not None:
            if tuple(actions.shape) != (k, v.num_envs, v.action_dim) or actions.dtype != torch.float32 \
                    or actions.device != v.device or not actions.is_contiguous():
                raise ValueError(f"actions must be a contiguous f32 [{k}, {v.num_envs}, {v.action_dim}] "
                                 f"tensor on {v.device}")
        torch.cuda.synchronize(v.device)
        g = torch.cuda.CUDAGraph()
        base = v._step_index
        with torch.cuda.graph(g):
            for i in range(k):
                a = actions[i] if actions is not None else v.sample_actions(base + i)
                self._enqueue_step(a, "pgx_step (capture)")
                if after_step is not None:
                    after_step()
        g._pgx_keep = actions   # the graph reads the buffer at replay
        return g

    # ------------------------------------------------------------- SB3 path
    def _host_stage(self):
        if self._hs is None:
            v = self.venv
            n, od = v.num_envs, v.obs_dim
            hs = {"packed": torch.empty(self._outbuf.numel(), dtype=torch.uint8, pin_memory=True),
                  "errors": torch.zeros(1, dtype=torch.int32, pin_memory=True), "errors_dev": v.state()["errors"]}
            nf = self._out_f32.numel()
            hf = hs["packed"][:4 * nf].view(torch.float32)
            o = 0
            for name, shape in (("observation", (n, od)), ("achieved_goal", (n, 3)), ("desired_goal", (n, 3)),
                                ("reward", (n,)), ("t_observation", (n, od)), ("t_achieved_goal", (n, 3)),
                                ("t_desired_goal", (n, 3))):
                k = int(np.prod(shape))
                hs[name] = hf[o:o + k].view(shape)
                o += k
            hs["flags"] = hs["packed"][4 * nf:].view(self._flags.shape[0], n)
            self._hs = hs
        return self._hs

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        """SB3 VecNormalize.reset: normalised numpy observations."""
        v = self.venv
        if seed is None:
            seed = v._pending_seed
        v._pending_seed = None
        self.reset_tensors(seed=seed)
        v.raise_device_errors()
        return {k: t.cpu().numpy().copy() for k, t in self._obs_out().items()}

    def seed(self, seed: Optional[int] = None):
        return self.venv.seed(seed)

    def step_async(self, actions) -> None:
        self.venv.step_async(actions)

    def step_wait(self):
        """SB3 VecNormalize.step_wait: (normalised obs dict, normalised rewards, dones, infos) as
        numpy; ``infos[i]["terminal_observation"]`` normalised, the other info fields as the env
        reports them."""
        from .envs import _INFO_TEMPLATES

        v = self.venv
        self.step_tensors(v._pending)
        v._pending = None
        hs = self._host_stage()
        stream = torch.cuda.current_stream(v.device)
        hs["packed"].copy_(self._outbuf, non_blocking=True)   # every output and the flags, one DMA
        hs["errors"].copy_(hs["errors_dev"], non_blocking=True)
        infos: List[Dict[str, Any]] = list(map(dict.copy, [_INFO_TEMPLATES[0]] * v.num_envs))
        if v._pre_sync is not None:   # a wrapper's launches and copies, ahead of the one sync
            v._pre_sync()
        stream.synchronize()
        guard = v.nonfinite_mode != "off"
        if hs["errors"].item():
            v.raise_device_errors(int(hs["errors"].item()),
                                  caught=np.flatnonzero(hs["flags"].numpy()[4]) if guard else None)
        o = {k: hs[k].numpy().copy() for k in KEYS}
        r = hs["reward"].numpy().copy()
        fl = hs["flags"].numpy() != 0
        sc, te, tr, col = fl[0], fl[1].copy(), fl[2].copy(), fl[3]
        d = te | tr
        code = sc.view(np.uint8) + 2 * col.view(np.uint8)
        for i in np.flatnonzero(code).tolist():
            infos[i] = _INFO_TEMPLATES[int(code[i])].copy()
        idx = np.nonzero(d)[0]
        if len(idx):
            tobs, tag, tdg = hs["t_observation"].numpy(), hs["t_achieved_goal"].numpy(), hs["t_desired_goal"].numpy()
            for i in idx.tolist():
                infos[i]["terminal_observation"] = {"observation": tobs[i].copy(), "achieved_goal": tag[i].copy(),
                                                    "desired_goal": tdg[i].copy()}
                infos[i]["TimeLimit.truncated"] = bool(tr[i] and not te[i])
        if guard:
            for i in np.flatnonzero(fl[4]).tolist():
                infos[i]["nonfinite"] = True
                if not v.auto_reset:
                    infos[i].pop("terminal_observation", None)
        return o, r, d, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # ------------------------------------------------- SB3's remaining surface
    def get_original_obs(self, tensors: bool = False):
        """The last raw observations: numpy copies (SB3), or with ``tensors`` the env's device buffers."""
        return self.venv._obs_dict() if tensors else self.venv._numpy_obs()

    def get_original_reward(self, tensors: bool = False):
        return self.venv.reward if tensors else self.venv.reward.cpu().numpy().copy()

    def _apply(self, key: int, x, inverse: bool):
        is_np = not torch.is_tensor(x)
        t = torch.as_tensor(np.asarray(x, dtype=np.float32)) if is_np else x
        out = self._norm.apply(key, t, inverse)
        return out.cpu().numpy() if is_np else out

    def _copy(self, x):
        return x.clone() if torch.is_tensor(x) else np.array(x, copy=True)

    def _obs_map(self, obs, inverse: bool, key: Optional[str]):
        if isinstance(obs, dict):
            return {k: self._obs_map(x, inverse, k) for k, x in obs.items()}
        key = key or "observation"
        if key not in KEYS:
            raise ValueError(f"unknown observation key {key!r}")
        if not (self._norm_obs and key in self.norm_obs_keys):
            return self._copy(obs)
        return self._apply(KEYS.index(key), obs, inverse)

    def normalize_obs(self, obs, key: Optional[str] = None):
        """VecNormalize.normalize_obs with the current statistics (no update): a dict by key, or one
        array of key ``key`` (default "observation"); numpy in, numpy out; device tensor in, tensor out."""
        return self._obs_map(obs, False, key)

    def unnormalize_obs(self, obs, key: Optional[str] = None):
        return self._obs_map(obs, True, key)

    def normalize_reward(self, reward):
        return self._apply(abi.NORM_REWARD, reward, False) if self._norm_reward else self._copy(reward)

    def unnormalize_reward(self, reward):
        return self._apply(abi.NORM_REWARD, reward, True) if self._norm_reward else self._copy(reward)

    def normalize_rows(self, rows: "torch.Tensor", action_dim: int) -> None:
        """A HER batch (``HerReplayBuffer.alloc_batch()["rows"]``) in place, one launch."""
        self._norm.rows(rows, action_dim)

    def get_stats(self):
        return self._norm.get_stats()

    def set_stats(self, mean, var, count, returns=None) -> None:
        self._norm.set_stats(mean, var, count, returns)

    @property
    def obs_rms(self) -> Dict[str, RunningMeanStd]:
        mean, var, count, _ = self._norm.get_stats()
        od = self.venv.obs_dim
        out, o = {}, 0
        for k, w in zip(KEYS, (od, 3, 3)):
            if k in self.norm_obs_keys:
                out[k] = RunningMeanStd(mean[o:o + w].copy(), var[o:o + w].copy(), count[o])
            o += w
        return out

    @property
    def ret_rms(self) -> RunningMeanStd:
        mean, var, count, _ = self._norm.get_stats()
        return RunningMeanStd(mean[-1:].reshape(()).copy(), var[-1:].reshape(()).copy(), count[-1])

    @property
    def returns(self) -> np.ndarray:
        return self._norm.get_stats()[3]

    def save(self, path: str) -> None:
        """Statistics and settings as a plain ``.npz`` (no pickle)."""
        mean, var, count, ret = self._norm.get_stats()
        with open(path, "wb") as f:
            np.savez(f, mean=mean, var=var, count=count, returns=ret, obs_dim=np.int64(self.venv.obs_dim),
                     training=np.bool_(self.training), norm_obs=np.bool_(self._norm_obs),
                     norm_reward=np.bool_(self._norm_reward), clip_obs=np.float64(self.clip_obs),
                     clip_reward=np.float64(self.clip_reward), gamma=np.float64(self.gamma),
                     epsilon=np.float64(self.epsilon), norm_obs_keys=np.array(self.norm_obs_keys, dtype="U32"))

    @classmethod
    def load(cls, path: str, venv) -> "VecNormalize":
        """A wrapper of ``venv`` with the statistics and settings ``save`` wrote (the per-env returns
        too where ``venv`` has as many envs)."""
        with np.load(path, allow_pickle=False) as z:
            if int(z["obs_dim"]) != venv.obs_dim:
                raise ValueError(f"{path} holds statistics of obs_dim {int(z['obs_dim'])}, the env has {venv.obs_dim}")
            w = cls(venv, training=bool(z["training"]), norm_obs=bool(z["norm_obs"]),
                    norm_reward=bool(z["norm_reward"]), clip_obs=float(z["clip_obs"]),
                    clip_reward=float(z["clip_reward"]), gamma=float(z["gamma"]), epsilon=float(z["epsilon"]),
                    norm_obs_keys=[str(k) for k in z["norm_obs_keys"]])
            ret = z["returns"]
            w.set_stats(z["mean"], z["var"], z["count"], ret if ret.shape == (venv.num_envs,) else None)
        return w
