"""Device HER replay buffer: the goal-relabelling buffer the reference trains with, on MI355X.

Mirrors stable-baselines3's ``HerReplayBuffer`` as the reference configures it
(training/utils/setup_training.py:14,176-179; classes/train_config.py:2,15:
``replay_buffer_class=HerReplayBuffer``, ``n_sampled_goal=4``,
``goal_selection_strategy="future"``) with the same public surface --
``add(obs, next_obs, action, reward, done, infos)``, ``sample(batch_size)``
returning ``DictReplayBufferSamples``-shaped tensors (real rows first, then the
relabelled ones), ``size()``, ``full``, ``pos``, ``ep_start``/``ep_length``
views -- plus a device-resident path (``add_tensors``, ``add_from_vec_env``)
that never leaves HBM.  Storage, episode bookkeeping, relabelling and reward
recomputation run in libpgx.so (pgx_her.hip); there is no CPU fallback.

Collection on the device: ``set_last(obs)`` keeps SB3's ``_last_original_obs`` as a
device carry, ``collect_from_vec_env(venv, action)`` builds the transition from it and
the env's own output buffers in one launch, the ring position is a device word (``pos``,
``full`` and ``size()`` read it: one sync), so ``after_step(venv, actions)`` puts the
collect into ``capture_steps``' graph, and ``truncate_last_trajectory()`` closes the open
episodes after a forced reset (include/pgx.h, "Collection on the device").

Draws: the device Philox stream (key = buffer seed, counter = (sample, call))
replaces numpy's global RNG, so a sample is a pure function of (seed, call
index, buffer contents) -- the oracle (oracle/her.py) reproduces it exactly.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import abi
from ._handle import Handle, _view, resolve_dims, torch
from ._native import PgxError, check, load

STRATEGIES = {"future": abi.HER_FUTURE, "final": abi.HER_FINAL, "episode": abi.HER_EPISODE}


class DictReplayBufferSamples(NamedTuple):
    """stable_baselines3.common.type_aliases.DictReplayBufferSamples (torch tensors on device)."""

    observations: Dict[str, "torch.Tensor"]
    actions: "torch.Tensor"
    next_observations: Dict[str, "torch.Tensor"]
    dones: "torch.Tensor"
    rewards: "torch.Tensor"


class HerReplayBuffer(Handle):
    """SB3 HerReplayBuffer over a device ring of ``buffer_size // n_envs`` slots x ``n_envs``.

    ``env`` may be a ``PandaVecEnv`` (reward type, threshold and dims are read
    from it, as SB3 reads them through ``env.env_method("compute_reward")``).
    """

    _PREFIX = "pgx_replay"

    def __init__(self, buffer_size: int, observation_space: Any = None, action_space: Any = None, env: Any = None,
                 device: Any = "cuda:0", n_envs: int = 1, n_sampled_goal: int = 4,
                 goal_selection_strategy: str = "future", copy_info_dict: bool = False,
                 handle_timeout_termination: bool = True, seed: int = 0, obs_dim: Optional[int] = None,
                 action_dim: Optional[int] = None, reward_type: Optional[str] = None,
                 distance_threshold: Optional[float] = None):
        self._need_torch()
        if goal_selection_strategy not in STRATEGIES:
            raise ValueError(f"Invalid goal selection strategy, please use one of {list(STRATEGIES)}")
        if copy_info_dict:
            raise NotImplementedError("copy_info_dict: infos are not needed by Task.compute_reward")
        self.lib = load()
        self._on_device(device)
        if env is not None:
            reward_type = env.reward_type if reward_type is None else reward_type
            distance_threshold = env.distance_threshold if distance_threshold is None else distance_threshold
        self.n_envs, self.obs_dim, self.action_dim = resolve_dims(env, observation_space, action_space, n_envs, obs_dim,
                                                                  action_dim)
        self.buffer_size = max(int(buffer_size) // self.n_envs, 1)   # SB3 BaseBuffer: per-env slots
        self.reward_type = reward_type or "sparse"
        self.distance_threshold = 0.05 if distance_threshold is None else float(distance_threshold)
        self.n_sampled_goal = n_sampled_goal
        self.her_ratio = 1 - (1.0 / (n_sampled_goal + 1))            # SB3 HerReplayBuffer.__init__
        self.goal_selection_strategy = goal_selection_strategy
        self.handle_timeout_termination = handle_timeout_termination
        self.env = env
        cfg = abi.PgxReplayConfig()
        cfg.n_envs, cfg.capacity = self.n_envs, self.buffer_size
        cfg.obs_dim, cfg.action_dim = self.obs_dim, self.action_dim
        cfg.reward_type = abi.REWARD_CODES[self.reward_type]
        cfg.strategy = STRATEGIES[goal_selection_strategy]
        cfg.distance_threshold, cfg.her_ratio, cfg.seed = self.distance_threshold, self.her_ratio, int(seed)
        self._cfg = cfg
        self._fields, self.row_dim = abi.replay_row_fields(self.obs_dim, self.action_dim)
        self.row_stride = self.lib.pgx_replay_row_stride(C.byref(cfg))
        if self.lib.pgx_replay_row_dim(C.byref(cfg)) != self.row_dim:
            raise PgxError("libpgx batch row layout differs from abi.replay_row_fields")
        self._create(cfg)
        self._draw = 0
        self._seen_valid = False
        self._keep: List[Any] = []

    # ------------------------------------------------------------ plumbing
    def _arrays(self):
        s, l, nv = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._call("episode_arrays", self._h, C.byref(s), C.byref(l), C.byref(nv))
        shp = (self.buffer_size, self.n_envs)
        return _view(s.value, shp, torch.int32, self.device), _view(l.value, shp, torch.int32, self.device), \
            _view(nv.value, (1,), torch.int32, self.device)

    # ---------------------------------------------------------------- state
    @property
    def ep_start(self) -> "torch.Tensor":
        return self._arrays()[0]

    @property
    def ep_length(self) -> "torch.Tensor":
        return self._arrays()[1]

    def _state(self, clear: bool = False):
        """(added, n_valid, errors) from the device words: one sync; refreshes libpgx's host mirror."""
        added, nv, err = C.c_int64(0), C.c_int32(0), C.c_uint32(0)
        self._call("state", self._h, C.byref(added), C.byref(nv), C.byref(err), 1 if clear else 0, self._stream())
        return int(added.value), int(nv.value), int(err.value)

    @property
    def pos(self) -> int:
        """The slot the next add or collect writes (a device word: this synchronises)."""
        return self._state()[0] % self.buffer_size

    @property
    def full(self) -> bool:
        return self._state()[0] >= self.buffer_size

    def size(self) -> int:
        """SB3 BaseBuffer.size: transitions stored per env."""
        return min(self._state()[0], self.buffer_size)

    def raise_device_errors(self) -> None:
        """Raise what the kernels flagged in the sticky device word and clear it (one sync)."""
        self._raise_flags(self._state(clear=True)[2], abi.REPLAY_ERRORS, "replay")

    def arrays(self) -> Dict[str, "torch.Tensor"]:
        """Device views of everything stored: ``records`` [C, N, record_stride] and the fields as
        strided views into it (``obs`` ... ``done`` as in a batch row, then ``rec_ep_start`` /
        ``rec_ep_length``, the records' int32 copies), the carry ``last_observation`` [N, obs_dim],
        ``last_achieved_goal`` / ``last_desired_goal`` [N, 3] (views into ``carry`` [N,
        carry_stride]), ``ep_start`` / ``ep_length`` [C, N], ``cur_ep_start`` [N] and the words
        ``n_valid``, ``added`` (int64), ``errors``, ``carry_set`` [1]."""
        v = abi.PgxReplayViews()
        self._call("arrays", self._h, C.byref(v))
        Cn, N, od, R, W, dev = self.buffer_size, self.n_envs, self.obs_dim, int(v.record_stride), \
            int(v.carry_stride), self.device
        rec = _view(v.records, (Cn, N, R), torch.float32, dev)
        out = {"records": rec}
        for name, off, w in self._fields:
            out[name] = rec[:, :, off] if name in ("reward", "done") else rec[:, :, off:off + w]
        irec = _view(v.records, (Cn, N, R), torch.int32, dev)
        out["rec_ep_start"], out["rec_ep_length"] = irec[:, :, self.row_dim], irec[:, :, self.row_dim + 1]
        carry = _view(v.carry, (N, W), torch.float32, dev)
        out.update(carry=carry, last_observation=carry[:, :od], last_achieved_goal=carry[:, od:od + 3],
                   last_desired_goal=carry[:, od + 3:od + 6],
                   ep_start=_view(v.ep_start, (Cn, N), torch.int32, dev),
                   ep_length=_view(v.ep_length, (Cn, N), torch.int32, dev),
                   cur_ep_start=_view(v.cur_ep_start, (N,), torch.int32, dev),
                   n_valid=_view(v.n_valid, (1,), torch.int32, dev), added=_view(v.added, (1,), torch.int64, dev),
                   errors=_view(v.errors, (1,), torch.int32, dev), carry_set=_view(v.carry_set, (1,), torch.int32, dev))
        return out

    # ------------------------------------------------------------------ add
    def add_tensors(self, obs, achieved_goal, desired_goal, action, reward, next_obs, next_achieved_goal,
                    next_desired_goal, done, timeout=None) -> None:
        """Store one transition per env from device (or host) arrays, SB3 HerReplayBuffer.add order."""
        N, od, ad = self.n_envs, self.obs_dim, self.action_dim
        f, u8 = torch.float32, torch.uint8
        t = [self._dev(obs, (N, od), f), self._dev(achieved_goal, (N, 3), f), self._dev(desired_goal, (N, 3), f),
             self._dev(action, (N, ad), f), self._dev(reward, (N,), f), self._dev(next_obs, (N, od), f),
             self._dev(next_achieved_goal, (N, 3), f), self._dev(next_desired_goal, (N, 3), f),
             self._dev(done, (N,), u8)]
        to = None
        if timeout is not None and self.handle_timeout_termination:
            to = self._dev(timeout, (N,), u8)
        tr = abi.PgxTransition(*[x.data_ptr() for x in t], None if to is None else to.data_ptr())
        self._call("add", self._h, C.byref(tr), self._stream())
        self._keep = t + [to]  # alive until the stream has consumed them (same-stream allocator reuse is safe)

    def add(self, obs: Dict[str, Any], next_obs: Dict[str, Any], action, reward, done,
            infos: Sequence[Dict[str, Any]]) -> None:
        """SB3 signature: obs/next_obs dicts of [n_envs, ...] arrays; timeouts from infos."""
        timeout = np.array([bool(i.get("TimeLimit.truncated", False)) for i in infos], dtype=np.uint8)
        self.add_tensors(obs["observation"], obs["achieved_goal"], obs["desired_goal"], action, reward,
                         next_obs["observation"], next_obs["achieved_goal"], next_obs["desired_goal"],
                         np.asarray(done).astype(np.uint8) if not torch.is_tensor(done) else done, timeout)

    def add_from_vec_env(self, venv, obs: Dict[str, "torch.Tensor"], action: "torch.Tensor") -> None:
        """Store the step just taken by ``venv.step_tensors(action)`` from ``obs``, on device.

        ``obs`` is a copy of the observation the action was taken from.  next_obs is
        the terminal observation for every env that was auto-reset, terminated or truncated
        (SB3 off_policy_algorithm _store_transition reads infos["terminal_observation"] of
        any done env), dones = terminated | truncated, timeouts = truncated & ~terminated.

        Given a ``VecNormalize`` wrapper, the raw values are stored (SB3 stores
        ``get_original_obs()`` / ``get_original_reward()``): ``obs`` is the raw observation
        (``get_original_obs(tensors=True)`` before the step) and the rest is read from the wrapped env."""
        venv = getattr(venv, "venv", venv)
        tr = venv.truncated.bool()
        te = venv.terminated.bool()
        done = (tr | te).to(torch.uint8)
        m = (tr | te).unsqueeze(1)   # every auto-reset env (time limit, collision, terminate_on_success)
        next_o = torch.where(m, venv.terminal_obs, venv.obs)
        next_ag = torch.where(m, venv.terminal_ag, venv.achieved_goal)
        next_dg = torch.where(m, venv.terminal_dg, venv.desired_goal)
        timeout = (tr & ~te).to(torch.uint8)
        self.add_tensors(obs["observation"], obs["achieved_goal"], obs["desired_goal"], action, venv.reward,
                         next_o, next_ag, next_dg, done, timeout)

    # -------------------------------------------------------------- collect
    def set_last(self, obs: Dict[str, Any]) -> None:
        """The carry, SB3's ``_last_original_obs``: the raw observation dict the next step's action
        is taken from (``env.reset()``'s; behind a ``VecNormalize``, ``get_original_obs``).  One
        launch.  Call it again after every forced reset, behind ``truncate_last_trajectory()``."""
        N = self.n_envs
        f = torch.float32
        t = [self._dev(obs["observation"], (N, self.obs_dim), f), self._dev(obs["achieved_goal"], (N, 3), f),
             self._dev(obs["desired_goal"], (N, 3), f)]
        self._call("set_last", self._h, *[C.c_void_p(x.data_ptr()) for x in t], self._stream())
        self._keep_last = t   # read by the queued launch

    def _launch_collect(self, action, reward, terminated, truncated, obs, ag, dg, tobs, tag, tdg) -> None:
        io = abi.PgxReplayStep(*[x.data_ptr() for x in (action, reward, terminated, truncated, obs, ag, dg, tobs, tag,
                                                        tdg)], 1 if self.handle_timeout_termination else 0, 0)
        check(self.lib.pgx_replay_collect(self._h, C.byref(io), self._stream()), "pgx_replay_collect", self.lib)

    def collect_tensors(self, action, reward, obs: Dict[str, Any], terminated, truncated,
                        terminal_obs: Dict[str, Any]) -> None:
        """Store the step from the carry to ``obs``: ``action`` [N, A], ``reward`` [N], the post-step
        observation dict, the step's flags [N] and the terminal observation dict (read for the envs
        with ``terminated | truncated``).  done = terminated | truncated, timeout = truncated &
        ~terminated (with ``handle_timeout_termination``), next_obs = the terminal observation of a
        done env; the carry becomes ``obs``.  Device f32 / u8 contiguous tensors are read in place."""
        N, od, f, u8 = self.n_envs, self.obs_dim, torch.float32, torch.uint8
        t = [self._dev(action, (N, self.action_dim), f), self._dev(reward, (N,), f), self._dev(terminated, (N,), u8),
             self._dev(truncated, (N,), u8)]
        for o in (obs, terminal_obs):
            t += [self._dev(o["observation"], (N, od), f), self._dev(o["achieved_goal"], (N, 3), f),
                  self._dev(o["desired_goal"], (N, 3), f)]
        self._launch_collect(*t)
        self._keep = t   # alive until the stream has consumed them

    @staticmethod
    def _base_env(venv):
        """The innermost ``PandaVecEnv`` behind ``VecMonitor`` / ``VecNormalize``: its buffers hold the
        raw step outputs, which SB3's off-policy path stores (``get_original_obs`` / ``_reward``)."""
        v = venv
        while hasattr(v, "venv"):
            v = v.venv
        return v

    def _step_buffers(self, venv):
        v = self._base_env(venv)
        return (v.reward, v.terminated, v.truncated, v.obs, v.achieved_goal, v.desired_goal, v.terminal_obs,
                v.terminal_ag, v.terminal_dg)

    def collect_from_vec_env(self, venv, action: "torch.Tensor") -> None:
        """Store the step ``venv.step_tensors(action)`` has just taken, from the carry: one collect
        launch that reads the env's own output buffers in place (no clone, no temporary), then the
        valid-list refresh.  ``venv`` may be the env, a ``VecNormalize`` or a ``VecMonitor``: the raw
        values of the env underneath are stored, as ``add_from_vec_env`` stores them."""
        a = action
        if a.dtype != torch.float32 or a.device != self.device or not a.is_contiguous() \
                or tuple(a.shape) != (self.n_envs, self.action_dim):
            a = self._dev(a, (self.n_envs, self.action_dim), torch.float32)
        self._launch_collect(a, *self._step_buffers(venv))
        self._keep = [a]

    def after_step(self, venv, actions: Optional["torch.Tensor"] = None):
        """The callable for ``venv.capture_steps(k, actions, after_step=...)`` of the env or either
        wrapper: its i-th call enqueues the collect of step i, reading ``actions[i]`` -- the static
        contiguous f32 [k, N, A] device buffer the captured steps read -- or, with ``actions=None``,
        the env's own action buffer, which the in-graph random policy fills before every step.  A
        contiguous f32 [N, A] buffer is read at every step: ``Actor.actions`` under
        ``Actor.capture_rollout``, which the in-graph actor fills before every step."""
        base = self._base_env(venv)
        bufs = self._step_buffers(venv)
        if torch.is_tensor(actions) and actions.dim() == 2:
            if tuple(actions.shape) != (self.n_envs, self.action_dim) or actions.dtype != torch.float32 \
                    or actions.device != self.device or not actions.is_contiguous():
                raise ValueError(f"actions must be a contiguous f32 [{self.n_envs}, {self.action_dim}] tensor on "
                                 f"{self.device}")

            def enqueue_same() -> None:
                self._launch_collect(actions, *bufs)

            self._keep_graph = actions
            return enqueue_same
        if actions is not None:
            if not torch.is_tensor(actions) or actions.dim() != 3 or \
                    tuple(actions.shape[1:]) != (self.n_envs, self.action_dim) or actions.dtype != torch.float32 \
                    or actions.device != self.device or not actions.is_contiguous():
                raise ValueError(f"actions must be a contiguous f32 [k, {self.n_envs}, {self.action_dim}] tensor on "
                                 f"{self.device}")
        count = [0]

        def enqueue() -> None:
            i = count[0]
            if actions is not None and i >= actions.shape[0]:
                raise IndexError(f"after_step: more than the {actions.shape[0]} steps its buffer holds")
            self._launch_collect(actions[i] if actions is not None else base._actions, *bufs)
            count[0] = i + 1

        self._keep_graph = actions
        return enqueue

    def truncate_last_trajectory(self) -> None:
        """SB3 ``HerReplayBuffer.truncate_last_trajectory``: close every open episode where it
        stands, so that its transitions become valid and no relabelled goal is drawn across it.
        Call it after a forced ``reset_tensors()``, an env switch or the end of a ``learn()``, then
        ``set_last(obs)``.  A no-op for envs at an episode start."""
        self._call("truncate_last_trajectory", self._h, 1 if self.handle_timeout_termination else 0, self._stream())

    # --------------------------------------------------------------- sample
    def alloc_batch(self, batch_size: int, with_indices: bool = True) -> Dict[str, "torch.Tensor"]:
        """Batch tensors: ``rows`` [B, row_stride] plus per-field views into it (include/pgx.h layout)."""
        B = int(batch_size)
        rows = torch.empty((B, self.row_stride), dtype=torch.float32, device=self.device)
        out = {"rows": rows}
        for name, off, w in self._fields:
            out[name] = rows[:, off] if name in ("reward", "done") else rows[:, off:off + w]
        for k in ("slot", "env", "goal_slot"):
            out[k] = torch.empty((B,), dtype=torch.int32, device=self.device) if with_indices else None
        return out

    def sample_raw(self, batch_size: int, draw: Optional[int] = None, env: Any = None) -> Dict[str, "torch.Tensor"]:
        """One relabelled batch: field views (obs, achieved_goal, ..., done) plus the drawn slot/env/goal_slot."""
        out = self.alloc_batch(batch_size)
        self.sample_into(out, draw, env=env)
        return out

    def sample_into(self, out: Dict[str, "torch.Tensor"], draw: Optional[int] = None, env: Any = None) -> None:
        """Fill a batch from alloc_batch() (no allocation; the benchmark's timed call).  ``env``: a
        ``VecNormalize`` whose current statistics normalise the batch in place (one more launch),
        after the relabelled rewards were computed on the raw goals (SB3 _get_virtual_samples)."""
        rows = out["rows"]
        d = self._draw if draw is None else int(draw)
        self._draw = d + 1
        ptr = lambda k: out[k].data_ptr() if out.get(k) is not None else None  # noqa: E731
        b = abi.PgxReplayBatch(rows.data_ptr(), ptr("slot"), ptr("env"), ptr("goal_slot"))
        check(self.lib.pgx_replay_sample(self._h, C.c_int64(rows.shape[0]), C.c_uint64(d), C.byref(b),
                                         self._stream()), "pgx_replay_sample", self.lib)
        if not self._seen_valid:
            # SB3 raises before the first episode has ended; check once (one sync) until it has
            if int(self._arrays()[2].item()) == 0:
                raise RuntimeError("Unable to sample before the end of the first episode. We recommend choosing "
                                   "a value for learning_starts that is greater than the maximum number of "
                                   "timesteps in the environment.")
            self._seen_valid = True
        if env is not None:
            env.normalize_rows(rows, self.action_dim)

    def sample(self, batch_size: int, env: Any = None) -> DictReplayBufferSamples:
        """SB3 HerReplayBuffer.sample: real rows first, then int(her_ratio * B) relabelled rows;
        ``env`` (a ``VecNormalize``) normalises observations, goals and rewards as SB3's
        ``sample(batch_size, env=vec_normalize)`` does."""
        r = self.sample_raw(batch_size, env=env)
        return DictReplayBufferSamples(
            observations={"observation": r["obs"], "achieved_goal": r["achieved_goal"],
                          "desired_goal": r["desired_goal"]},
            actions=r["action"],
            next_observations={"observation": r["next_obs"], "achieved_goal": r["next_achieved_goal"],
                               "desired_goal": r["next_desired_goal"]},
            dones=r["done"].reshape(-1, 1), rewards=r["reward"].reshape(-1, 1))
