"""Device-resident actor: stable-baselines3's off-policy actor forward as one HIP launch.

The reference trains SB3 off-policy algorithms with ``MultiInputPolicy`` and ``net_arch`` [256, 256] or
[400, 300] (setup_training.py, hyperparameters.py): TQC / SAC act through a squashed Gaussian, TD3 /
DDPG through a deterministic actor with ``NormalActionNoise``, every evaluation with
``deterministic=True``.  ``Actor`` is that forward pass -- CombinedExtractor's concatenation, the
Linear + ReLU trunk, the heads, the squash and the noise -- in libpgx.so (pgx_actor.hip; C-ABI and the
arithmetic contract in include/pgx.h, section "Actor").  It reads the persistent observation buffers
of an env or a wrapper and writes the action buffer the next step reads, so ``capture_rollout`` puts
``k`` closed-loop steps of observe, act, step, collect into one graph.  No CPU fallback: with
``device="cpu"`` an ``Actor`` only holds and maps parameters (``load_state_dict`` / ``state_dict`` /
``forward_host``, the host model of the kernel's arithmetic, which is a test oracle and not a way to step).

``action_log_prob`` is SB3's ``actor.action_log_prob(observations)`` for the Gaussian kind: actions and their
log-probability for a batch of any size in one launch, a HER batch's rows read in place
(``action_log_prob_rows``) -- the ``next_actions`` / ``next_log_prob`` of ``TQC.train``'s target.

PPO's actor-critic lives next door (actor_critic.py), the gSDE actor (``use_sde=True``, per-env exploration
matrices) in sde_actor.py, TQC's critics (forward, truncated TD target, Polyak step) in quantile_critic.py.
Optimisers are not here.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from ._native import check
from ._policy import OBS_KEYS, Policy, torch  # noqa: F401  (OBS_KEYS: importable from here as before)


class Actor(Policy):
    """SB3's SAC / TQC (``kind="gaussian"``) or TD3 / DDPG (``kind="deterministic"``) actor on the device.

    ``env``: a ``PandaVecEnv`` or a wrapper of one (``n_envs``, the dims and the device are read from
    it), or pass ``obs_dim``, ``action_dim`` and ``n_envs``.  ``net_arch``: 1 to 3 hidden widths of 1
    to 512.  ``clip_mean`` > 0: SB3's gSDE actor ``Hardtanh`` on the mean (what a ``use_sde=True``
    model needs for deterministic evaluation).  ``action_noise``: ``(mu, sigma)`` of SB3's
    ``NormalActionNoise`` for the deterministic kind (None: no noise, every call is deterministic).
    Parameters are zero until ``load_state_dict``."""

    def __init__(self, env: Any = None, obs_dim: Optional[int] = None, action_dim: Optional[int] = None,
                 net_arch: Sequence[int] = (256, 256), kind: str = "gaussian", clip_mean: float = 0.0,
                 action_noise: Optional[Tuple[float, float]] = None, seed: int = 0, device: Any = None,
                 n_envs: Optional[int] = None):
        self._need_torch()
        if kind not in abi.ACTOR_KINDS:
            raise ValueError(f"kind must be one of {list(abi.ACTOR_KINDS)}, got {kind!r}")
        self._resolve(env, obs_dim, action_dim, n_envs, device)
        self.net_arch = tuple(int(w) for w in net_arch)
        self.kind, self.clip_mean, self.seed = kind, float(clip_mean), int(seed)
        self.action_noise = None if action_noise is None else (float(action_noise[0]), float(action_noise[1]))
        if kind == "gaussian" and action_noise is not None:
            raise ValueError("action_noise belongs to the deterministic kind (SB3 NormalActionNoise)")
        cfg = abi.PgxActorConfig()
        cfg.n_envs, cfg.obs_dim, cfg.action_dim = self.n_envs, self.obs_dim, self.action_dim
        cfg.n_layers = len(self.net_arch)
        for i, w in enumerate(self.net_arch[:abi.ACTOR_MAX_LAYERS]):
            cfg.hidden[i] = w
        cfg.kind, cfg.clip_mean = abi.ACTOR_KINDS[kind], self.clip_mean
        cfg.noise_mu, cfg.noise_sigma = self.action_noise or (0.0, 0.0)
        cfg.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        self._cfg = cfg
        # the parameters as given (torch layout), on the actor's device: what set_weights reads
        dims = [self.obs_dim + 6] + list(self.net_arch)
        shapes = [(dims[i + 1], dims[i]) for i in range(len(self.net_arch))]
        shapes += [(self.action_dim, dims[-1])] * (2 if kind == "gaussian" else 1)
        self._names = self._key_names(kind, len(self.net_arch))
        self._w = [torch.zeros(s, dtype=torch.float32, device=self.device) for s in shapes]
        self._b = [torch.zeros(s[0], dtype=torch.float32, device=self.device) for s in shapes]
        self.actions = torch.zeros((self.n_envs, self.action_dim), dtype=torch.float32, device=self.device)
        self._open()

    # ------------------------------------------------------------ plumbing
    _PREFIX = "pgx_actor"
    _SD_PREFIX = "actor."

    @staticmethod
    def _key_names(kind: str, n_layers: int) -> List[str]:
        """SB3's module names per parameter slot: the hidden layers, mu, log_std."""
        if kind == "gaussian":   # sac/policies.py Actor: latent_pi = Sequential(Linear, ReLU, ...), mu, log_std
            return [f"latent_pi.{2 * i}" for i in range(n_layers)] + ["mu", "log_std"]
        # td3/policies.py Actor: mu = Sequential(Linear, ReLU, ..., Linear, Tanh)
        return [f"mu.{2 * i}" for i in range(n_layers + 1)]

    def _weights_struct(self, ws, bs) -> abi.PgxActorWeights:
        w = abi.PgxActorWeights()
        for i, (x, y) in enumerate(zip(ws[:5], bs[:5])):   # (more: the library rejects n_layers)
            w.weight[i], w.bias[i] = x, y
        return w

    def _push(self) -> None:
        w = self._weights_struct([t.data_ptr() for t in self._w], [t.data_ptr() for t in self._b])
        self._call("set_weights", self._h, C.byref(w), self._stream())

    # ----------------------------------------------------------- parameters
    _slots = Policy._pairs

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Load SB3 actor parameters: ``latent_pi.{0,2,4}`` / ``mu`` / ``log_std`` (SAC, TQC) or
        ``mu.{0,2,4,...}`` (TD3, DDPG), ``.weight`` [out, in] and ``.bias`` [out]; a policy's state
        dict works too (its ``actor.`` keys are read, the rest ignored).  The packed weights in the
        handle are replaced on the current stream: a captured graph uses them at its next replay."""
        self._load_slots(sd)   # validates every key, then copies

    # --------------------------------------------------------------- forward
    def enable_debug(self) -> Dict[str, "torch.Tensor"]:
        """Allocate the debug planes every later forward fills: ``mean`` (after ``clip_mean``),
        ``log_std`` (after the clamp), ``eps`` [N, A] f32 and ``philox`` [N, 4, 4] int32 (the words of
        the device noise stream).  Tests and tools only."""
        if self._debug is None:
            z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
            N, A = self.n_envs, self.action_dim
            self._debug = {"mean": z(N, A), "log_std": z(N, A), "eps": z(N, A), "philox": z(N, 4, 4, dt=torch.int32)}
        return self._debug

    def _launch(self, obs: Dict[str, "torch.Tensor"], deterministic: bool, eps: Optional["torch.Tensor"]) -> None:
        d = self._debug
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        io = abi.PgxActorIo(p(obs["observation"]), p(obs["achieved_goal"]), p(obs["desired_goal"]), p(self.actions),
                            p(eps), *([None] * 4 if d is None else [p(d[k]) for k in ("mean", "log_std", "eps", "philox")]))
        det = 1 if (deterministic or (self.kind == "deterministic" and self.action_noise is None)) else 0
        check(self.lib.pgx_actor_forward(self._h, C.byref(io), det, self._stream()), "pgx_actor_forward", self.lib)

    def __call__(self, obs: Dict[str, Any], deterministic: bool = False, eps: Any = None) -> "torch.Tensor":
        """Actions [N, A] for the observation dict ``obs`` (what ``step_tensors`` / ``reset_tensors`` of
        an env, a ``VecNormalize`` or a ``VecMonitor`` return; read in place): one launch.  ``eps``
        [N, A]: the Gaussian noise to use instead of the device stream.  Returns the actor's
        persistent action tensor (overwritten by the next call)."""
        self._need_device()
        o = self._obs(obs)
        e = None if eps is None else self._dev(eps, (self.n_envs, self.action_dim))
        self._launch(o, deterministic, e)
        self._keep = [o, e]   # alive until the stream has consumed them
        return self.actions

    forward = __call__

    def forward_host(self, obs: Dict[str, Any]):
        """``(mean, log_std)`` [n, A] numpy f32 from the library's host model of the kernel's arithmetic
        (``log_std`` None for the deterministic kind), for any number of rows.  A test oracle."""
        (o, n), (ws, bs) = self._host_obs(obs), self._host_params()
        w = self._weights_struct([x.ctypes.data for x in ws], [x.ctypes.data for x in bs])
        mean = np.zeros((n, self.action_dim), np.float32)
        log_std = np.zeros((n, self.action_dim), np.float32) if self.kind == "gaussian" else None
        self._call("forward_host", C.byref(self._cfg), C.byref(w), abi.ptr(o["observation"]),
                       abi.ptr(o["achieved_goal"]), abi.ptr(o["desired_goal"]), n, abi.ptr(mean), abi.ptr(log_std))
        return mean, log_std

    noise_step = property(Policy._get_word, Policy._set_word, doc="""The device word that counts the forwards that
        drew noise from the Philox stream (this synchronises).  Setting it back reproduces the draws.""")

    # ------------------------------------------------- action log-probability
    _LP_PHILOX = True

    def _lp_planes(self) -> Dict[str, int]:
        return {k: self.action_dim for k in ("mean", "log_std", "eps", "gaussian_action")}

    def action_log_prob(self, obs: Dict[str, Any], eps: Any = None, out=None):
        """SB3's ``actor.action_log_prob(obs)`` for the Gaussian kind: ``(actions [B, A], log_prob [B])`` of a
        batch of any size ``B``, one launch.  ``obs``: an observation dict of [B, .] tensors; device f32
        tensors with contiguous rows, views into a HER batch's rows included, are read in place.  ``eps``
        [B, A]: the Gaussian noise to use instead of the device stream (``log_prob_noise_step``, which a
        launch that draws moves on by one: a replayed graph draws new noise).  ``out``: a pair of
        contiguous f32 tensors [B, A] and [B] to fill (returned as they are)."""
        self._need_device()
        io = abi.PgxActorLpIo()
        B, act, lp, keep = self._lp_io(io, obs, out)
        e = None if eps is None else self._dev(eps, (B, self.action_dim))
        if e is not None:
            io.eps = e.data_ptr()
        self._lp_debug_into(io, B)
        check(self.lib.pgx_actor_action_log_prob(self._h, C.byref(io), B, self._stream()), "pgx_actor_action_log_prob",
              self.lib)
        self._keep = keep + [e, act, lp]   # alive until the stream has consumed them
        return act, lp

    def action_log_prob_rows(self, batch: Dict[str, "torch.Tensor"], next: bool = True, out=None):
        """``action_log_prob`` on a HER batch (``buf.alloc_batch`` / ``buf.sample_into``): ``next_obs``,
        ``next_achieved_goal`` and ``next_desired_goal`` (``next=False``: ``obs``, ``achieved_goal``,
        ``desired_goal``) are read from ``batch["rows"]`` in place."""
        return self.action_log_prob(self._batch_obs(batch, next), out=out)

    def _get_lp_word(self) -> int:
        self._need_device()
        v = C.c_uint64(0)
        self._call("lp_state", self._h, C.byref(v), self._stream())
        return int(v.value)

    def _set_lp_word(self, value: int) -> None:
        self._need_device()
        self._call("lp_set_state", self._h, C.c_uint64(int(value) & 0xFFFFFFFFFFFFFFFF), self._stream())

    log_prob_noise_step = property(_get_lp_word, _set_lp_word, doc="""The device word that counts the
        ``action_log_prob`` launches that drew noise from the Philox stream (this synchronises); ``noise_step``
        is another word.  Setting it back reproduces the draws.""")

    def log_prob_host(self, obs: Dict[str, Any], eps: Any) -> Dict[str, np.ndarray]:
        """The library's host model of ``action_log_prob`` for any number of rows and their ``eps`` [n, A]:
        ``action``, ``log_prob`` and the planes ``mean``, ``log_std``, ``eps``, ``gaussian_action`` as numpy
        f32.  ``mean`` and ``log_std`` are what the kernel gives bit for bit.  A test oracle."""
        ws, bs = self._host_params()
        w = self._weights_struct([x.ctypes.data for x in ws], [x.ctypes.data for x in bs])
        io = abi.PgxActorLpIo()
        n, res = self._host_lp_io(io, obs, self._lp_planes())
        e = np.ascontiguousarray(eps.cpu().numpy() if torch.is_tensor(eps) else eps, dtype=np.float32)
        if e.shape != (n, self.action_dim):
            raise ValueError(f"expected eps of shape {[n, self.action_dim]}, got {list(e.shape)}")
        io.eps = abi.ptr(e)
        self._call("log_prob_host", C.byref(self._cfg), C.byref(w), C.byref(io), n)
        del res["_keep"]
        return res

    # --------------------------------------------------------------- capture
    def capture_rollout(self, venv, k: int, deterministic: bool = False, after_step: Optional[Callable[[], None]] = None):
        """Capture ``k`` closed-loop steps into one HIP graph (``torch.cuda.CUDAGraph``): the forward
        on ``venv``'s persistent observation buffers (through a ``VecNormalize`` the normalised ones),
        ``venv._enqueue_step(self.actions)``, ``after_step()`` -- the loop of ``capture_steps`` with the
        policy inside.  ``venv``: the env, a ``VecNormalize`` or a ``VecMonitor``.  ``after_step``: e.g.
        ``buf.after_step(venv, actor.actions)`` of the HER ring.  Capture runs nothing; every replay
        draws new noise (the step word is on the device) and uses the weights loaded last."""
        from .rollout import step_buffers

        self._need_device()
        obs = step_buffers(venv)[0]
        self._check_venv_obs(obs)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(int(k)):
                self._launch(obs, deterministic, None)
                venv._enqueue_step(self.actions, "pgx_step (capture)")
                if after_step is not None:
                    after_step()
        g._pgx_keep = (self, obs)   # the graph reads these buffers at replay
        return g
