"""Device-resident RolloutBuffer: stable-baselines3's on-policy buffer over a ``PandaVecEnv``.

SB3's ``OnPolicyAlgorithm.collect_rollouts`` fills a ``DictRolloutBuffer`` step by step, adds
``gamma * V(terminal observation)`` to the reward of an env the TimeLimit cut off, runs the GAE(lambda)
pass ``compute_returns_and_advantage`` and ``PPO.train`` reads shuffled minibatches from ``get``.
Here the ``n_steps`` x ``n_envs`` transitions, the carry (SB3's ``_last_obs`` /
``_last_episode_starts``), the GAE pass, the permutation and the minibatch gather live on the device
(libpgx.so, pgx_rollout.hip; C-ABI in include/pgx.h, section "RolloutBuffer"): every operation is one
kernel launch on the current stream, so an ``add`` captures into the step graph behind the env step
(``after_step``) and a rollout never leaves HBM.  No CPU fallback.

The minibatch order is a pure function of (seed, epoch, n_steps * n_envs) -- a keyed Feistel
permutation, include/pgx.h -- in place of numpy's global stream, as the HER buffer's draws are.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Dict, Iterator, List, NamedTuple, Optional

import numpy as np

from . import abi
from ._handle import OBS_KEYS, Handle, _view, resolve_dims, torch
from ._native import PgxError, check, load
from .monitor import VecMonitor
from .normalize import VecNormalize


class RolloutBufferSamples(NamedTuple):
    """stable_baselines3.common.type_aliases.DictRolloutBufferSamples (torch tensors on device)."""

    observations: Dict[str, "torch.Tensor"]
    actions: "torch.Tensor"
    old_values: "torch.Tensor"
    old_log_prob: "torch.Tensor"
    advantages: "torch.Tensor"
    returns: "torch.Tensor"


def step_buffers(venv):
    """What ``venv.step_tensors`` returned last, as ``venv`` presents it: (obs dict, reward,
    terminated, truncated).  A ``VecMonitor`` returns what it wraps; a ``VecNormalize`` the
    normalised observations and reward (on-policy SB3 stores those); flags are the env's."""
    v = venv
    while isinstance(v, VecMonitor):
        v = v.venv
    if isinstance(v, VecNormalize):
        return v._obs_out(), v._n["reward"], v.venv.terminated, v.venv.truncated
    return v._obs_dict(), v.reward, v.terminated, v.truncated


def terminal_observation(venv) -> Dict[str, "torch.Tensor"]:
    """The last step's terminal observation dict as ``venv`` presents it (through a ``VecNormalize``
    the normalised one), valid for the envs with ``terminated | truncated``: what the critic
    evaluates for ``add_from_vec_env``'s ``terminal_value``."""
    v = venv
    while isinstance(v, VecMonitor):
        v = v.venv
    src = v._n if isinstance(v, VecNormalize) else None
    pick = (lambda k: src[k]) if src is not None else (lambda k: getattr(v, k))  # noqa: E731
    return {"observation": pick("terminal_obs"), "achieved_goal": pick("terminal_ag"),
            "desired_goal": pick("terminal_dg")}


class RolloutBuffer(Handle):
    """SB3 ``DictRolloutBuffer`` of ``buffer_size`` steps x ``n_envs`` envs on the device.

    ``env`` may be a ``PandaVecEnv`` or a wrapper of one (``n_envs`` and the dims are read from it).
    Collect with ``add_from_vec_env`` after every ``step_tensors`` (or ``after_step`` inside
    ``capture_steps``), then ``compute_returns_and_advantage`` and ``get``; ``reset`` starts the
    next rollout and keeps the carry, as SB3's ``rollout_buffer.reset()`` keeps ``_last_obs``."""

    _PREFIX = "pgx_rollout"

    def __init__(self, buffer_size: int, observation_space: Any = None, action_space: Any = None,
                 device: Any = "cuda:0", gae_lambda: float = 1.0, gamma: float = 0.99, n_envs: int = 1, env: Any = None,
                 seed: int = 0, obs_dim: Optional[int] = None, action_dim: Optional[int] = None):
        self._need_torch()
        self.lib = load()
        self._on_device(device)
        self.n_envs, self.obs_dim, self.action_dim = resolve_dims(env, observation_space, action_space, n_envs, obs_dim,
                                                                  action_dim)
        self.buffer_size = int(buffer_size)   # SB3 RolloutBuffer: buffer_size = n_steps
        self.gamma, self.gae_lambda, self.seed = float(gamma), float(gae_lambda), int(seed)
        self.env = env
        cfg = abi.PgxRolloutConfig(self.n_envs, self.buffer_size, self.obs_dim, self.action_dim, self.gamma,
                                   self.gae_lambda, self.seed & 0xFFFFFFFFFFFFFFFF)
        self._cfg = cfg
        self._fields, self.row_dim = abi.rollout_row_fields(self.obs_dim, self.action_dim)
        self._create(cfg)
        self.row_stride = self.lib.pgx_rollout_row_stride(C.byref(cfg))
        if self.lib.pgx_rollout_row_dim(C.byref(cfg)) != self.row_dim:
            raise PgxError("libpgx batch row layout differs from abi.rollout_row_fields")
        self.total = self.buffer_size * self.n_envs
        self.epoch = 0                      # permutations drawn so far: get() uses it and adds one
        self._perm = torch.empty(self.total, dtype=torch.int32, device=self.device)
        self._keep: List[Any] = []

    # ------------------------------------------------------------ plumbing
    def _flag(self, x) -> Optional["torch.Tensor"]:
        return None if x is None else self._dev(x, (self.n_envs,), torch.uint8)

    def _state(self, clear: bool = False):
        pos, err = C.c_int32(0), C.c_uint32(0)
        self._call("state", self._h, C.byref(pos), C.byref(err), 1 if clear else 0, self._stream())
        return int(pos.value), int(err.value)

    # ---------------------------------------------------------------- state
    @property
    def pos(self) -> int:
        """Steps stored so far (a device word: this synchronises)."""
        return self._state()[0]

    @property
    def full(self) -> bool:
        return self.pos == self.buffer_size

    def size(self) -> int:
        """SB3 BaseBuffer.size: steps stored per env."""
        return self.pos

    def raise_device_errors(self) -> None:
        """Raise what the kernels flagged in the sticky device word and clear it (one sync)."""
        self._raise(self._state(clear=True)[1])

    def _raise(self, err: int) -> None:
        self._raise_flags(err, abi.ROLLOUT_ERRORS, "rollout")

    def arrays(self) -> Dict[str, "torch.Tensor"]:
        """Device views of every stored plane: ``observation`` [T, N, obs_dim], ``achieved_goal`` /
        ``desired_goal`` [T, N, 3], ``action`` [T, N, A] (strided views into the records), ``reward``,
        ``episode_start``, ``value``, ``log_prob``, ``advantage``, ``return`` [T, N], and the carry
        ``last_observation`` [N, obs_dim], ``last_achieved_goal`` / ``last_desired_goal`` [N, 3],
        ``last_episode_start`` [N]."""
        v = abi.PgxRolloutViews()
        self._call("arrays", self._h, C.byref(v))
        T, N, od, ad, R, f = self.buffer_size, self.n_envs, self.obs_dim, self.action_dim, int(v.record_stride), \
            torch.float32
        rec = _view(v.records, (T, N, R), f, self.device)
        out = {"observation": rec[:, :, :od], "achieved_goal": rec[:, :, od:od + 3],
               "desired_goal": rec[:, :, od + 3:od + 6], "action": rec[:, :, od + 6:od + 6 + ad], "records": rec}
        for name, key in (("reward", "reward"), ("episode_start", "episode_start"), ("value", "value"),
                          ("log_prob", "log_prob"), ("advantage", "advantage"), ("returns", "return")):
            out[key] = _view(getattr(v, name), (T, N), f, self.device)
        out["last_observation"] = _view(v.last_obs, (N, od), f, self.device)
        out["last_achieved_goal"] = _view(v.last_achieved_goal, (N, 3), f, self.device)
        out["last_desired_goal"] = _view(v.last_desired_goal, (N, 3), f, self.device)
        out["last_episode_start"] = _view(v.last_episode_start, (N,), f, self.device)
        return out

    # -------------------------------------------------------------- collect
    def reset(self) -> None:
        """SB3 ``RolloutBuffer.reset``: ``pos = 0`` (one launch); the carry stays."""
        self._call("reset", self._h, self._stream())

    def set_last(self, obs: Dict[str, Any], episode_starts: Any = None) -> None:
        """The carry, SB3's ``_last_obs`` / ``_last_episode_starts``: the observation dict of
        ``env.reset()`` (``episode_starts`` None: ones, as SB3 starts)."""
        N = self.n_envs
        t = [self._dev(obs["observation"], (N, self.obs_dim)), self._dev(obs["achieved_goal"], (N, 3)),
             self._dev(obs["desired_goal"], (N, 3)), None if episode_starts is None else self._dev(episode_starts, (N,))]
        self._call("set_last", self._h, *[None if x is None else C.c_void_p(x.data_ptr()) for x in t], self._stream())
        self._keep_last = t   # read by the queued launch

    def _launch_add(self, action, reward, value, log_prob, terminal_value, obs, terminated, truncated) -> None:
        p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        io = abi.PgxRolloutIo(p(action), p(reward), p(value), p(log_prob), p(terminal_value),
                              *([None] * 3 if obs is None else [p(obs[k]) for k in OBS_KEYS]), p(terminated), p(truncated))
        check(self.lib.pgx_rollout_add(self._h, C.byref(io), self._stream()), "pgx_rollout_add", self.lib)

    def add_tensors(self, action, reward, value, log_prob, obs: Dict[str, Any], terminated, truncated,
                    terminal_value=None) -> None:
        """One add from device (or host) arrays: the step's ``action`` [N, A], ``reward``, ``value``,
        ``log_prob`` [N], the post-step observation dict, the step's flags [N], and optionally
        ``terminal_value`` [N].  Device f32 / u8 contiguous tensors are read in place."""
        N = self.n_envs
        t = [self._dev(action, (N, self.action_dim)), self._dev(reward, (N,)), self._dev(value, (N,)),
             self._dev(log_prob, (N,)), None if terminal_value is None else self._dev(terminal_value, (N,)),
             {k: self._dev(obs[k], (N, self.obs_dim if k == "observation" else 3)) for k in OBS_KEYS},
             self._flag(terminated), self._flag(truncated)]
        self._launch_add(*t)
        self._keep = t   # alive until the stream has consumed them

    def add_from_vec_env(self, venv, action, value, log_prob, terminal_value=None) -> None:
        """Store the step ``venv.step_tensors(action)`` has just taken (one launch): the carry's
        observation and episode_start with ``action``, ``value`` and ``log_prob`` [N] (the policy's
        outputs for the carry's observation) and the step's reward; the carry becomes the post-step
        observation and ``terminated | truncated``.  Reward, flags and observation are those of
        ``venv`` as given: through a ``VecNormalize`` the normalised ones (on-policy SB3 stores what
        the policy saw).  ``terminal_value`` [N]: V(terminal observation); envs with ``truncated &
        ~terminated`` get ``reward + gamma * terminal_value`` (SB3's time-limit bootstrap)."""
        obs, reward, terminated, truncated = step_buffers(venv)
        self.add_tensors(action, reward, value, log_prob, obs, terminated, truncated, terminal_value)

    def add(self, obs: Dict[str, Any], action, reward, episode_start, value, log_prob) -> None:
        """SB3's ``DictRolloutBuffer.add``: ``set_last(obs, episode_start)``, then the add (no
        post-step observation: the carry is left for the next ``add`` to set)."""
        N = self.n_envs
        self.set_last(obs, episode_start)
        t = [self._dev(action, (N, self.action_dim)), self._dev(reward, (N,)), self._dev(value, (N,)),
             self._dev(log_prob, (N,)), None, None, None, None]
        self._launch_add(*t)
        self._keep = t

    def after_step(self, venv, actions, values, log_probs, terminal_values=None) -> Callable[[], None]:
        """The callable for ``venv.capture_steps(k, actions, after_step=...)``: its i-th call
        enqueues the add of step i, reading ``actions[i]`` [N, A], ``values[i]`` and ``log_probs[i]``
        [N] (and ``terminal_values[i]``) -- static contiguous f32 device buffers [k, ...] the graph
        reads at replay -- and the step outputs of ``venv`` as given.  ``actions`` may also be one
        [N, A] buffer every step reads (``Actor.actions`` under ``Actor.capture_rollout``); ``k`` is then
        ``values.shape[0]``."""
        same = torch.is_tensor(actions) and actions.dim() == 2
        k, N = int(values.shape[0] if same else actions.shape[0]), self.n_envs
        want = {"actions": (actions, (N, self.action_dim) if same else (k, N, self.action_dim)), "values": (values, (k, N)),
                "log_probs": (log_probs, (k, N))}
        if terminal_values is not None:
            want["terminal_values"] = (terminal_values, (k, N))
        for name, (t, shape) in want.items():
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32 \
                    or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous f32 {list(shape)} tensor on {self.device}")
        obs, reward, terminated, truncated = step_buffers(venv)
        count = [0]

        def enqueue() -> None:
            i = count[0]
            if i >= k:
                raise IndexError(f"after_step: more than the {k} steps its buffers hold")
            self._launch_add(actions if same else actions[i], reward, values[i], log_probs[i],
                             None if terminal_values is None else terminal_values[i], obs, terminated, truncated)
            count[0] = i + 1

        self._keep_graph = (actions, values, log_probs, terminal_values)
        return enqueue

    # ---------------------------------------------------------------- learn
    def compute_returns_and_advantage(self, last_values, dones=None) -> None:
        """SB3's GAE(lambda) pass in f32, one launch: ``last_values`` [N] = V(carry observation),
        ``dones`` [N] (None: the carry's episode_start, which is what SB3 passes).  Raises if the
        buffer is not full (one sync: ``raise_device_errors``)."""
        self.enqueue_returns_and_advantage(last_values, dones)
        self.raise_device_errors()

    def enqueue_returns_and_advantage(self, last_values, dones=None) -> None:
        """The GAE launch alone: no sync, no look at the error word (a captured or timed loop)."""
        lv = self._dev(last_values, (self.n_envs,))
        dn = None if dones is None else self._dev(dones, (self.n_envs,))
        self._call("compute_returns_and_advantage", self._h, C.c_void_p(lv.data_ptr()),
                   None if dn is None else C.c_void_p(dn.data_ptr()), self._stream())
        self._keep_gae = (lv, dn)

    def permutation(self, epoch: Optional[int] = None) -> "torch.Tensor":
        """The minibatch order of ``epoch`` (None: the next one, counted on): int32 [n_steps * n_envs]
        flat indices ``env * n_steps + step`` in the buffer's own tensor, one launch."""
        if epoch is None:
            epoch, self.epoch = self.epoch, self.epoch + 1
        self._call("permutation", self._h, C.c_uint64(int(epoch) & 0xFFFFFFFFFFFFFFFF),
                   C.c_void_p(self._perm.data_ptr()), self._stream())
        return self._perm

    def alloc_batch(self, batch_size: int) -> Dict[str, "torch.Tensor"]:
        """Batch tensors: ``rows`` [B, row_stride] plus per-field views into it (include/pgx.h layout)."""
        rows = torch.empty((int(batch_size), self.row_stride), dtype=torch.float32, device=self.device)
        od, ad = self.obs_dim, self.action_dim
        # two view calls rather than one per field: a minibatch loop is bound by the host
        o, ag, dg, act, tail = rows.split([od, 3, 3, ad, self.row_stride - od - 6 - ad], dim=1)
        value, log_prob, adv, ret = tail.unbind(dim=1)[:4]
        return {"rows": rows, "observation": o, "achieved_goal": ag, "desired_goal": dg, "action": act,
                "old_value": value, "old_log_prob": log_prob, "advantage": adv, "return": ret}

    def gather_into(self, out: Dict[str, "torch.Tensor"], indices: "torch.Tensor") -> None:
        """Fill a batch from ``alloc_batch`` with the transitions ``indices`` (int32 device tensor
        [B], flat ``env * n_steps + step``) names: one launch, no allocation."""
        rows = out["rows"]
        if indices.dtype != torch.int32 or indices.device != self.device or not indices.is_contiguous() \
                or tuple(indices.shape) != (rows.shape[0],):
            raise ValueError(f"indices must be a contiguous int32 [{rows.shape[0]}] tensor on {self.device}")
        b = abi.PgxRolloutBatch(rows.data_ptr())
        check(self.lib.pgx_rollout_gather(self._h, C.c_void_p(indices.data_ptr()), C.c_int64(rows.shape[0]), C.byref(b),
                                          self._stream()), "pgx_rollout_gather", self.lib)

    def gather(self, indices) -> RolloutBufferSamples:
        """The transitions with flat indices ``indices`` (``env * n_steps + step``, SB3's
        ``swap_and_flatten`` order) as ``RolloutBufferSamples``.  An index out of range gives a zero
        row and sets the device error word (``raise_device_errors``)."""
        idx = indices
        if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.device != self.device or idx.dim() != 1 \
                or not idx.is_contiguous():
            idx = idx if torch.is_tensor(idx) else torch.as_tensor(np.asarray(idx))
            idx = idx.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        r = self.alloc_batch(idx.shape[0])
        self.gather_into(r, idx)
        return RolloutBufferSamples(observations={k: r[k] for k in OBS_KEYS}, actions=r["action"],
                                    old_values=r["old_value"], old_log_prob=r["old_log_prob"],
                                    advantages=r["advantage"], returns=r["return"])

    def get(self, batch_size: Optional[int] = None) -> Iterator[RolloutBufferSamples]:
        """SB3's ``RolloutBuffer.get``: one permutation launch (the next epoch), then one gather per
        minibatch of ``batch_size`` (the last one short; None: the whole buffer in one).  Raises
        ``AssertionError`` if the buffer is not full, as SB3 asserts; one sync per call."""
        pos, err = self._state(clear=True)
        self._raise(err)
        if pos != self.buffer_size:
            raise AssertionError(f"RolloutBuffer.get: the buffer is not full ({pos} of {self.buffer_size} steps)")
        bs = self.total if batch_size is None else int(batch_size)
        if bs <= 0:
            raise ValueError("batch_size must be positive")
        perm = self.permutation()
        for start in range(0, self.total, bs):
            yield self.gather(perm[start:start + bs])
