"""Device-resident gSDE actor: stable-baselines3's off-policy actor built with ``use_sde=True``.

The reference trains TQC by default (train_config.py) with ``use_sde=True``, ``log_std_init=-3`` and
``net_arch`` [256, 256] / [400, 300] (hyperparameters.py): every rollout it collects explores with
generalised state-dependent exploration.  Each env holds an exploration matrix ``E`` [H, A], drawn at
``reset_noise``; an action is ``tanh(mean + latent @ E)``, so between two resamples the noise is a fixed
function of the state.  ``SdeActor`` is that forward -- CombinedExtractor's concatenation, the Linear +
ReLU trunk, ``mu`` with its ``clip_mean`` Hardtanh, the per-env mat-vec and the squash -- and the
resampling, in libpgx.so (pgx_sde_actor.hip; C-ABI and the arithmetic contract in include/pgx.h, section
"SdeActor").  Both are kernel launches only and the draw's generation word lives on the device, so
``capture_rollout`` puts resample, observe, act, step, collect into one graph whose every replay draws
new matrices.  ``full_std=True``, ``use_expln=False`` and ``latent_sde = latent_pi`` (SB3's defaults) are
what is built.  No CPU fallback: with ``device="cpu"`` an ``SdeActor`` only holds and maps parameters
(``load_state_dict`` / ``state_dict`` / ``forward_host``, the host model of the kernel's arithmetic).

``action_log_prob`` is SB3's ``actor.action_log_prob(observations)`` as ``TQC.train`` reaches it: for a batch
of any size, with the noise of the ONE shared ``exploration_mat`` [H, A] (``reset_batch_noise``; SB3's
``get_noise`` takes it when the batch length differs from the number of per-env matrices), the
distribution's variance, the inverse of the squash and the log-probability with its correction, in one
launch that reads a HER batch's rows in place (``action_log_prob_rows``).

Gradients and optimisers are training-side and not here; the critics are in quantile_critic.py.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Callable, Dict, Optional, Sequence

import numpy as np

from . import abi
from ._native import check
from ._policy import Policy, torch


class SdeActor(Policy):
    """SB3's SAC / TQC actor with ``use_sde=True`` on the device.

    ``env``: a ``PandaVecEnv`` or a wrapper of one (``n_envs``, the dims and the device are read from it),
    or pass ``obs_dim``, ``action_dim`` and ``n_envs``.  ``net_arch``: 1 to 3 hidden widths of 1 to 512;
    the last one is the latent width H.  ``log_std_init``: the fill of the ``log_std`` parameter [H, A].
    ``clip_mean`` > 0: the Hardtanh on the mean.  The weights are zero and the exploration matrices are
    zero until ``load_state_dict`` and ``reset_noise``."""

    def __init__(self, env: Any = None, obs_dim: Optional[int] = None, action_dim: Optional[int] = None,
                 net_arch: Sequence[int] = (256, 256), log_std_init: float = -3.0, clip_mean: float = 2.0,
                 full_std: bool = True, use_expln: bool = False, seed: int = 0, device: Any = None,
                 n_envs: Optional[int] = None):
        self._need_torch()
        if not full_std:
            raise ValueError("full_std=False is not built")
        if use_expln:
            raise ValueError("use_expln=True is not built")
        self._resolve(env, obs_dim, action_dim, n_envs, device)
        self.net_arch = tuple(int(w) for w in net_arch)
        self.log_std_init, self.clip_mean, self.seed = float(log_std_init), float(clip_mean), int(seed)
        cfg = abi.PgxSdeActorConfig()
        cfg.n_envs, cfg.obs_dim, cfg.action_dim = self.n_envs, self.obs_dim, self.action_dim
        cfg.n_layers = len(self.net_arch)
        for i, w in enumerate(self.net_arch[:abi.ACTOR_MAX_LAYERS]):
            cfg.hidden[i] = w
        cfg.clip_mean = self.clip_mean
        cfg.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        self._cfg = cfg
        self.latent_dim = self.net_arch[min(len(self.net_arch), abi.ACTOR_MAX_LAYERS) - 1] if self.net_arch else 0
        # the parameters as given (torch layout), on the actor's device: what set_weights reads
        dims = [self.obs_dim + 6] + list(self.net_arch)
        shapes = [(dims[i + 1], dims[i]) for i in range(len(self.net_arch))] + [(self.action_dim, dims[-1])]
        # sac/policies.py Actor: latent_pi = Sequential(Linear, ReLU, ...); mu = Sequential(Linear, Hardtanh)
        # when clip_mean > 0, a bare Linear otherwise; log_std a bare parameter
        self._names = [f"latent_pi.{2 * i}" for i in range(len(self.net_arch))] + ["mu.0" if self.clip_mean > 0 else "mu"]
        self._w = [torch.zeros(s, dtype=torch.float32, device=self.device) for s in shapes]
        self._b = [torch.zeros(s[0], dtype=torch.float32, device=self.device) for s in shapes]
        self._log_std = torch.full((max(self.latent_dim, 0), self.action_dim), self.log_std_init, dtype=torch.float32,
                                   device=self.device)
        self.actions = torch.zeros((self.n_envs, self.action_dim), dtype=torch.float32, device=self.device)
        self._open(np.zeros((0, max(self.latent_dim, 0), self.action_dim), np.float32))

    # ------------------------------------------------------------ plumbing
    _PREFIX = "pgx_sde_actor"
    _SD_PREFIX = "actor."

    def _weights_struct(self, ws, bs, log_std) -> abi.PgxSdeActorWeights:
        w = abi.PgxSdeActorWeights()
        for i, (x, y) in enumerate(zip(ws[:4], bs[:4])):   # (more: the library rejects n_layers)
            w.weight[i], w.bias[i] = x, y
        w.log_std = log_std
        return w

    def _push(self) -> None:
        w = self._weights_struct([t.data_ptr() for t in self._w], [t.data_ptr() for t in self._b], self._log_std.data_ptr())
        self._call("set_weights", self._h, C.byref(w), self._stream())

    # ----------------------------------------------------------- parameters
    def _slots(self):
        """(key, tensor) of every parameter in SB3's order."""
        return self._pairs() + [("log_std", self._log_std)]

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Load SB3 gSDE actor parameters: ``latent_pi.{0,2,4}``, ``mu.0`` (``mu`` with ``clip_mean == 0``),
        ``.weight`` [out, in] and ``.bias`` [out], and ``log_std`` [H, A]; a policy's state dict works too
        (its ``actor.`` keys are read, the rest ignored).  The packed weights and ``std`` in the handle are
        replaced on the current stream: a captured graph uses them at its next replay."""
        self._load_slots(sd)   # validates every key, then copies

    @property
    def std(self) -> "torch.Tensor":
        """``exp(log_std)`` [H, A] as the handle holds it (a copy)."""
        self._need_device()
        out = torch.empty_like(self._log_std)
        self._call("get_std", self._h, C.c_void_p(out.data_ptr()), self._stream())
        return out

    # ----------------------------------------------------------------- noise
    def enable_debug(self) -> Dict[str, "torch.Tensor"]:
        """Allocate the debug planes every later call fills: of a forward ``mean`` [N, A] (after
        ``clip_mean``), ``latent`` [N, H] and ``noise`` [N, A]; of a ``reset_noise`` ``eps`` [N, H, A] f32
        and ``philox`` [N, 4, 4] int32 (the words of the blocks q < 4).  Tests and tools only."""
        if self._debug is None:
            z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
            N, A, H = self.n_envs, self.action_dim, self.latent_dim
            self._debug = {"mean": z(N, A), "latent": z(N, H), "noise": z(N, A), "eps": z(N, H, A),
                           "philox": z(N, 4, 4, dt=torch.int32)}
        return self._debug

    def reset_noise(self) -> None:
        """Resample every env's exploration matrix (SB3 ``reset_noise(n_envs)``): one launch, which moves
        ``noise_generation`` on by one."""
        self._need_device()
        d = self._debug
        e, p = (None, None) if d is None else (C.c_void_p(d["eps"].data_ptr()), C.c_void_p(d["philox"].data_ptr()))
        self._call("reset_noise", self._h, e, p, self._stream())

    noise_generation = property(Policy._get_word, Policy._set_word, doc="""The device word that keys the matrix draw
        and counts the resamples (this synchronises).  Setting it back reproduces the draws.""")

    @property
    def exploration_matrices(self) -> "torch.Tensor":
        """The matrices [N, H, A] in SB3's layout (a copy; the handle keeps a layout of its own)."""
        self._need_device()
        out = torch.empty((self.n_envs, self.latent_dim, self.action_dim), dtype=torch.float32, device=self.device)
        self._call("get_matrices", self._h, C.c_void_p(out.data_ptr()), self._stream())
        return out

    @exploration_matrices.setter
    def exploration_matrices(self, value: Any) -> None:
        self._need_device()
        t = self._dev(value, (self.n_envs, self.latent_dim, self.action_dim))
        self._call("set_matrices", self._h, C.c_void_p(t.data_ptr()), self._stream())
        self._keep_m = t   # alive until the stream has consumed it

    # --------------------------------------------------------------- forward
    def _launch(self, obs: Dict[str, "torch.Tensor"], deterministic: bool) -> None:
        d = self._debug
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        io = abi.PgxSdeActorIo(p(obs["observation"]), p(obs["achieved_goal"]), p(obs["desired_goal"]), p(self.actions),
                               *([None] * 3 if d is None else [p(d[k]) for k in ("mean", "latent", "noise")]))
        check(self.lib.pgx_sde_actor_forward(self._h, C.byref(io), 1 if deterministic else 0, self._stream()),
              "pgx_sde_actor_forward", self.lib)

    def __call__(self, obs: Dict[str, Any], deterministic: bool = False) -> "torch.Tensor":
        """Actions [N, A] for the observation dict ``obs`` (what ``step_tensors`` / ``reset_tensors`` of an
        env, a ``VecNormalize`` or a ``VecMonitor`` return; read in place): one launch.  ``deterministic``:
        ``tanh(mean)``, no matrix is read.  Returns the actor's persistent action tensor (overwritten by
        the next call)."""
        self._need_device()
        o = self._obs(obs)
        self._launch(o, deterministic)
        self._keep = [o]   # alive until the stream has consumed them
        return self.actions

    forward = __call__

    def forward_host(self, obs: Dict[str, Any], matrices: Any):
        """``(mean [n, A], latent [n, H], noise [n, A])`` numpy f32 from the library's host model of the
        kernel's arithmetic, for any number of rows and their ``matrices`` [n, H, A].  A test oracle."""
        (o, n), (ws, bs) = self._host_obs(obs), self._host_params()
        H, A = max(self.latent_dim, 0), self.action_dim
        m = np.ascontiguousarray(matrices.cpu().numpy() if torch.is_tensor(matrices) else matrices, dtype=np.float32)
        if m.shape != (n, H, A):
            raise ValueError(f"expected matrices of shape {[n, H, A]}, got {list(m.shape)}")
        ls = np.ascontiguousarray(self._log_std.cpu().numpy())
        w = self._weights_struct([x.ctypes.data for x in ws], [x.ctypes.data for x in bs], ls.ctypes.data)
        mean, latent, noise = np.zeros((n, A), np.float32), np.zeros((n, H), np.float32), np.zeros((n, A), np.float32)
        self._call("forward_host", C.byref(self._cfg), C.byref(w), abi.ptr(o["observation"]),
                       abi.ptr(o["achieved_goal"]), abi.ptr(o["desired_goal"]), abi.ptr(m), n, abi.ptr(mean),
                       abi.ptr(latent), abi.ptr(noise))
        return mean, latent, noise

    # ------------------------------------------------- action log-probability
    _LP_PHILOX = False

    def _lp_planes(self) -> Dict[str, int]:
        A, H = self.action_dim, max(self.latent_dim, 0)
        return {"mean": A, "latent": H, "noise": A, "variance": A, "gaussian_action": A}

    def reset_batch_noise(self, eps_out: Optional["torch.Tensor"] = None) -> None:
        """Resample the one exploration matrix the batch entry uses (SB3 ``actor.reset_noise()`` at the top of
        a gradient step): one launch, which moves ``batch_noise_generation`` on by one.  The per-env
        matrices and ``noise_generation`` are not touched.  ``eps_out`` (debug): a contiguous device f32 [H,
        A] tensor that receives the standard normal draw."""
        self._need_device()
        e = None
        if eps_out is not None:
            if eps_out.dtype != torch.float32 or eps_out.device != self.device or not eps_out.is_contiguous() \
                    or tuple(eps_out.shape) != (self.latent_dim, self.action_dim):
                raise ValueError(f"eps_out must be a contiguous f32 [{self.latent_dim}, {self.action_dim}] tensor on "
                                 f"{self.device}")
            e = C.c_void_p(eps_out.data_ptr())
        self._call("reset_batch_noise", self._h, e, self._stream())

    def _get_batch_word(self) -> int:
        self._need_device()
        v = C.c_uint64(0)
        self._call("batch_state", self._h, C.byref(v), self._stream())
        return int(v.value)

    def _set_batch_word(self, value: int) -> None:
        self._need_device()
        self._call("batch_set_state", self._h, C.c_uint64(int(value) & 0xFFFFFFFFFFFFFFFF), self._stream())

    batch_noise_generation = property(_get_batch_word, _set_batch_word, doc="""The device word that keys the draw
        of ``exploration_mat`` and counts ``reset_batch_noise`` (this synchronises); ``noise_generation`` is
        another word.  Setting it back reproduces the draws.""")

    @property
    def exploration_mat(self) -> "torch.Tensor":
        """The shared matrix [H, A] of the batch entry, SB3's ``exploration_mat`` (a copy).  Device only."""
        self._need_device()
        out = torch.empty((self.latent_dim, self.action_dim), dtype=torch.float32, device=self.device)
        self._call("get_batch_matrix", self._h, C.c_void_p(out.data_ptr()), self._stream())
        return out

    @exploration_mat.setter
    def exploration_mat(self, value: Any) -> None:
        self._need_device()
        t = self._dev(value, (self.latent_dim, self.action_dim))
        self._call("set_batch_matrix", self._h, C.c_void_p(t.data_ptr()), self._stream())
        self._keep_b = t   # alive until the stream has consumed it

    def action_log_prob(self, obs: Dict[str, Any], out=None):
        """SB3's ``actor.action_log_prob(obs)`` on the gSDE distribution as ``TQC.train`` reaches it: ``(actions
        [B, A], log_prob [B])`` of a batch of any size ``B`` with the noise of the one ``exploration_mat``, one
        launch.  ``obs``: an observation dict of [B, .] tensors; device f32 tensors with contiguous rows,
        views into a HER batch's rows included, are read in place.  ``out``: a pair of contiguous f32
        tensors [B, A] and [B] to fill (returned as they are)."""
        self._need_device()
        io = abi.PgxSdeActorLpIo()
        B, act, lp, keep = self._lp_io(io, obs, out)
        self._lp_debug_into(io, B)
        check(self.lib.pgx_sde_actor_action_log_prob(self._h, C.byref(io), B, self._stream()),
              "pgx_sde_actor_action_log_prob", self.lib)
        self._keep = keep + [act, lp]   # alive until the stream has consumed them
        return act, lp

    def action_log_prob_rows(self, batch: Dict[str, "torch.Tensor"], next: bool = True, out=None):
        """``action_log_prob`` on a HER batch (``buf.alloc_batch`` / ``buf.sample_into``): ``next_obs``,
        ``next_achieved_goal`` and ``next_desired_goal`` (``next=False``: ``obs``, ``achieved_goal``,
        ``desired_goal``) are read from ``batch["rows"]`` in place."""
        return self.action_log_prob(self._batch_obs(batch, next), out=out)

    def log_prob_host(self, obs: Dict[str, Any], exploration_mat: Any, std: Any = None) -> Dict[str, np.ndarray]:
        """The library's host model of ``action_log_prob`` for any number of rows: ``action``, ``log_prob`` and
        the planes ``mean``, ``latent``, ``noise``, ``variance``, ``gaussian_action`` as numpy f32.  ``std`` [H,
        A]: what the variance is built from -- by default the handle's (``self.std``), on a CPU actor the host
        libm's ``exp(log_std)``.  The planes but ``gaussian_action`` are what the kernel gives bit for bit.  A
        test oracle."""
        ws, bs = self._host_params()
        H, A = max(self.latent_dim, 0), self.action_dim
        f = lambda x: np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=np.float32)  # noqa: E731
        m = f(exploration_mat)
        if m.shape != (H, A):
            raise ValueError(f"expected exploration_mat of shape {[H, A]}, got {list(m.shape)}")
        if std is None and self._h is not None:
            std = self.std
        s = None if std is None else f(std)
        if s is not None and s.shape != (H, A):
            raise ValueError(f"expected std of shape {[H, A]}, got {list(s.shape)}")
        ls = np.ascontiguousarray(self._log_std.cpu().numpy())
        w = self._weights_struct([x.ctypes.data for x in ws], [x.ctypes.data for x in bs], ls.ctypes.data)
        io = abi.PgxSdeActorLpIo()
        n, res = self._host_lp_io(io, obs, self._lp_planes())
        self._call("log_prob_host", C.byref(self._cfg), C.byref(w), abi.ptr(s), abi.ptr(m), C.byref(io), n)
        del res["_keep"]
        return res

    # --------------------------------------------------------------- rollouts
    def _venv_obs(self, venv) -> Dict[str, "torch.Tensor"]:
        from .rollout import step_buffers

        self._need_device()
        obs = step_buffers(venv)[0]
        self._check_venv_obs(obs)
        return obs

    def _enqueue_rollout(self, venv, obs, k: int, deterministic: bool, after_step, sde_sample_freq: int, what: str) -> None:
        for j in range(int(k)):
            if j == 0 or (sde_sample_freq > 0 and j % sde_sample_freq == 0):
                self.reset_noise()
            self._launch(obs, deterministic)
            venv._enqueue_step(self.actions, what)
            if after_step is not None:
                after_step()

    def capture_rollout(self, venv, k: int, deterministic: bool = False, after_step: Optional[Callable[[], None]] = None,
                        sde_sample_freq: int = -1):
        """Capture ``k`` closed-loop steps into one HIP graph (``torch.cuda.CUDAGraph``): one
        ``reset_noise`` in front of step 0 and another before every step ``j > 0`` with ``sde_sample_freq
        > 0 and j % sde_sample_freq == 0``; per step the forward on ``venv``'s persistent observation
        buffers, ``venv._enqueue_step(self.actions)``, ``after_step()``.  With ``k = train_freq`` a replay
        is one SB3 off-policy ``collect_rollouts``.  (SB3 resamples twice before step 0 when
        ``sde_sample_freq > 0`` and throws the first draw away; here it is once.)  ``venv``: the env, a
        ``VecNormalize`` or a ``VecMonitor``.  ``after_step``: e.g. ``buf.after_step(venv, actor.actions)``
        of the HER ring.  Capture runs nothing; every replay draws new matrices (the generation word is
        on the device) and uses the weights loaded last."""
        obs = self._venv_obs(venv)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._enqueue_rollout(venv, obs, k, deterministic, after_step, int(sde_sample_freq), "pgx_step (capture)")
        g._pgx_keep = (self, obs)   # the graph reads these buffers at replay
        return g

    def collect(self, venv, k: int, deterministic: bool = False, after_step: Optional[Callable[[], None]] = None,
                sde_sample_freq: int = -1) -> None:
        """The launches of one ``capture_rollout`` replay, enqueued on the current stream without a graph."""
        obs = self._venv_obs(venv)
        self._enqueue_rollout(venv, obs, k, deterministic, after_step, int(sde_sample_freq), "pgx_step (collect)")
