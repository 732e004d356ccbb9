"""Device-resident actor-critic: stable-baselines3's on-policy ``ActorCriticPolicy`` forward in HIP.

The reference carries a PPO configuration beside its off-policy ones (setup_training.py,
hyperparameters.py: ``MultiInputPolicy``, ``net_arch=dict(pi=[256, 256], vf=[256, 256])``, ReLU).
``ActorCritic`` is that policy's forward pass -- CombinedExtractor's concatenation, MlpExtractor's two
trunks, ``action_net``, ``value_net`` and the diagonal Gaussian with its state-independent ``log_std``
-- in libpgx.so (pgx_actor_critic.hip; C-ABI and the arithmetic contract in include/pgx.h, section
"ActorCritic"): one launch gives what SB3's ``policy.forward`` returns (actions, values, log_probs) plus
the actions clipped to the Box, a second entry gives ``predict_values`` alone, for a mask of envs if
wanted.  With the ``RolloutBuffer`` they make SB3's ``OnPolicyAlgorithm.collect_rollouts`` -- forward,
clip, step, terminal-value bootstrap, add, last values, GAE -- one captured graph
(``capture_rollout``).  No CPU fallback: with ``device="cpu"`` an ``ActorCritic`` only holds and maps
parameters (``load_state_dict`` / ``state_dict`` / ``forward_host``, a test oracle).

``evaluate_actions`` and everything that needs gradients is not here: ``PPO.train`` stays torch on the
minibatches ``RolloutBuffer.get`` yields.  Tanh trunks and gSDE exploration are not built.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import abi
from ._native import PgxError, check
from ._policy import Policy, torch

DEFAULT_NET_ARCH = {"pi": (256, 256), "vf": (256, 256)}   # the reference's PPO setting


def _is_relu(fn: Any) -> bool:
    if isinstance(fn, str):
        return fn.lower() == "relu"
    return torch is not None and (fn is torch.nn.ReLU or isinstance(fn, torch.nn.ReLU))


class ActorCritic(Policy):
    """SB3's ``ActorCriticPolicy`` (``MultiInputPolicy``, PPO / A2C) forward on the device.

    ``env``: a ``PandaVecEnv`` or a wrapper of one (``n_envs``, the dims and the device are read from
    it), or pass ``obs_dim``, ``action_dim`` and ``n_envs``.  ``net_arch``: ``dict(pi=[...], vf=[...])``
    or one list for both trunks (SB3 >= 2.0: no shared layers), 1 to 3 widths of 1 to 512 each.
    ``activation_fn``: ReLU only.  ``use_sde=True`` (the reference's PPO setting): gSDE exploration is
    not built; the flag makes ``load_state_dict`` expect SB3's gSDE ``log_std`` [last pi width, A],
    kept for ``state_dict`` only, so such a policy can be evaluated (``predict``) and used as a critic
    (``predict_values``).  Parameters are zero and ``log_std = log_std_init`` until ``load_state_dict``."""

    def __init__(self, env: Any = None, obs_dim: Optional[int] = None, action_dim: Optional[int] = None,
                 n_envs: Optional[int] = None, net_arch: Union[None, Dict[str, Sequence[int]], Sequence[int]] = None,
                 log_std_init: float = 0.0, activation_fn: Any = "relu", use_sde: bool = False, seed: int = 0,
                 device: Any = None):
        self._need_torch()
        if not _is_relu(activation_fn):
            raise ValueError(f"activation_fn {activation_fn!r}: only ReLU is built; SB3's default Tanh is not (a device "
                             "tanhf in the trunk cannot meet the bit-exact host model)")
        self._resolve(env, obs_dim, action_dim, n_envs, device)
        arch = DEFAULT_NET_ARCH if net_arch is None else net_arch
        if isinstance(arch, dict):
            if set(arch) != {"pi", "vf"}:
                raise ValueError("net_arch as a dict needs exactly the keys 'pi' and 'vf'")
            pi, vf = arch["pi"], arch["vf"]
        else:
            pi = vf = arch
        self.pi_arch, self.vf_arch = tuple(int(w) for w in pi), tuple(int(w) for w in vf)
        self.net_arch = {"pi": self.pi_arch, "vf": self.vf_arch}
        self.log_std_init, self.use_sde, self.seed = float(log_std_init), bool(use_sde), int(seed)
        cfg = abi.PgxAcConfig()
        cfg.n_envs, cfg.obs_dim, cfg.action_dim = self.n_envs, self.obs_dim, self.action_dim
        cfg.n_pi_layers, cfg.n_vf_layers = len(self.pi_arch), len(self.vf_arch)
        for i, w in enumerate(self.pi_arch[:abi.ACTOR_MAX_LAYERS]):   # (more: the library rejects the count)
            cfg.pi_hidden[i] = w
        for i, w in enumerate(self.vf_arch[:abi.ACTOR_MAX_LAYERS]):
            cfg.vf_hidden[i] = w
        cfg.seed = self.seed & 0xFFFFFFFFFFFFFFFF
        self._cfg = cfg
        # the parameters as given (torch layout), on this device: what set_weights reads
        N, A, in_dim = self.n_envs, self.action_dim, self.obs_dim + 6
        self._names: List[str] = []
        shapes: List[Tuple[int, int]] = []
        for net, widths in (("policy_net", self.pi_arch), ("value_net", self.vf_arch)):
            dims = [in_dim] + list(widths)
            for i in range(len(widths)):
                self._names.append(f"mlp_extractor.{net}.{2 * i}")
                shapes.append((dims[i + 1], dims[i]))
        self._names += ["action_net", "value_net"]
        shapes += [(A, (self.pi_arch or (in_dim,))[-1]), (1, (self.vf_arch or (in_dim,))[-1])]
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
        self._w = [z(*s) for s in shapes]
        self._b = [z(s[0]) for s in shapes]
        # SB3: log_std [A]; with gSDE [latent_sde_dim, A] (kept, never handed to the library)
        ls_shape = (shapes[-2][1], A) if self.use_sde else (A,)
        self._log_std = torch.full(ls_shape, self.log_std_init, dtype=torch.float32, device=self.device)
        self._log_std_lib = z(A) if self.use_sde else self._log_std
        self.actions, self.clipped_actions = z(N, A), z(N, A)
        self.values, self.log_probs = z(N), z(N)
        self.terminal_values, self.last_values, self._pv = z(N), z(N), z(N)
        self._open()

    # ------------------------------------------------------------ plumbing
    _PREFIX = "pgx_ac"
    _WHO = "ActorCritic"

    def _weights_struct(self, ws, bs, log_std) -> abi.PgxAcWeights:
        w = abi.PgxAcWeights()
        npi, nvf = min(len(self.pi_arch), 3), min(len(self.vf_arch), 3)
        for i in range(npi):
            w.pi_weight[i], w.pi_bias[i] = ws[i], bs[i]
        off = len(self.pi_arch)
        for i in range(nvf):
            w.vf_weight[i], w.vf_bias[i] = ws[off + i], bs[off + i]
        w.action_net_weight, w.action_net_bias = ws[-2], bs[-2]
        w.value_net_weight, w.value_net_bias = ws[-1], bs[-1]
        w.log_std = log_std
        return w

    def _push(self) -> None:
        w = self._weights_struct([t.data_ptr() for t in self._w], [t.data_ptr() for t in self._b],
                                 self._log_std_lib.data_ptr())
        self._call("set_weights", self._h, C.byref(w), self._stream())

    # ----------------------------------------------------------- parameters
    def _slots(self):
        """(key, tensor) of every parameter: ``log_std`` first, then SB3's ``ActorCriticPolicy`` names."""
        return [("log_std", self._log_std)] + self._pairs()

    def _shape_hint(self, key: str) -> str:
        return " (use_sde=True expects SB3's gSDE log_std [last pi width, action_dim])" \
            if key == "log_std" and self.use_sde else ""

    def load_state_dict(self, sd: Dict[str, Any]) -> None:
        """Load an SB3 ``ActorCriticPolicy`` state dict: ``mlp_extractor.policy_net.{0,2,4}``,
        ``mlp_extractor.value_net.{0,2,4}``, ``action_net``, ``value_net`` (``.weight`` [out, in] and
        ``.bias`` [out]) and ``log_std`` ([A]; with ``use_sde`` [last pi width, A]).  Other keys
        (``features_extractor.*``, ...) are ignored.  A failed load changes nothing.  The packed
        weights in the handle are replaced on the current stream: a captured graph uses them at its
        next replay."""
        self._load_slots(sd)   # validates every key, then copies

    # --------------------------------------------------------------- forward
    def enable_debug(self) -> Dict[str, "torch.Tensor"]:
        """Allocate the debug planes every later forward fills: ``mean`` and ``eps`` [N, A] f32 and
        ``philox`` [N, 4, 4] int32 (the words of the device noise stream).  Tests and tools only."""
        if self._debug is None:
            z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
            N, A = self.n_envs, self.action_dim
            self._debug = {"mean": z(N, A), "eps": z(N, A), "philox": z(N, 4, 4, dt=torch.int32)}
        return self._debug

    def _launch(self, obs: Dict[str, "torch.Tensor"], deterministic: bool, eps: Optional["torch.Tensor"]) -> None:
        if self.use_sde and not deterministic:
            raise PgxError("gSDE exploration is not built: a use_sde=True ActorCritic only predicts deterministically")
        d = self._debug
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        io = abi.PgxAcIo(p(obs["observation"]), p(obs["achieved_goal"]), p(obs["desired_goal"]), p(self.actions),
                         p(self.clipped_actions), p(self.values), p(self.log_probs), p(eps),
                         *([None] * 3 if d is None else [p(d[k]) for k in ("mean", "eps", "philox")]))
        check(self.lib.pgx_ac_forward(self._h, C.byref(io), 1 if deterministic else 0, self._stream()), "pgx_ac_forward",
              self.lib)

    def _launch_values(self, obs: Dict[str, "torch.Tensor"], need: Optional["torch.Tensor"], out: "torch.Tensor") -> None:
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self._call("values", self._h, p(obs["observation"]), p(obs["achieved_goal"]), p(obs["desired_goal"]),
                       p(need), p(out), self._stream())

    def __call__(self, obs: Dict[str, Any], deterministic: bool = False, eps: Any = None):
        """SB3's ``policy.forward``: ``(actions [N, A], values [N], log_probs [N])`` for the observation
        dict ``obs`` (what ``step_tensors`` / ``reset_tensors`` of an env, a ``VecNormalize`` or a
        ``VecMonitor`` return; read in place), one launch.  ``actions`` are unclipped, as SB3 stores
        them; ``clipped_actions`` holds what the env takes.  ``eps`` [N, A]: the Gaussian noise to use
        instead of the device stream.  Returns persistent tensors (overwritten by the next call)."""
        self._need_device()
        o = self._obs(obs)
        e = None if eps is None else self._dev(eps, (self.n_envs, self.action_dim))
        self._launch(o, deterministic, e)
        self._keep = [o, e]   # alive until the stream has consumed them
        return self.actions, self.values, self.log_probs

    forward = __call__

    def predict(self, obs: Dict[str, Any], deterministic: bool = True) -> "torch.Tensor":
        """The actions clipped to the Box, [N, A] (SB3's ``policy.predict`` on tensors): fits
        ``pg.evaluate(venv, ac.predict, ...)``."""
        self.__call__(obs, deterministic=deterministic)
        return self.clipped_actions

    def predict_values(self, obs: Dict[str, Any], need: Any = None, out: Optional["torch.Tensor"] = None):
        """SB3's ``policy.predict_values``: V(obs) [N], the value trunk alone, one launch; bit for bit
        the forward's ``values``.  ``need`` [N] (bool / uint8): only workgroup tiles (16 or 32
        consecutive envs) that hold a flagged env are computed, every env of the others is +0.
        ``out``: the [N] f32 tensor to fill (default: a persistent one, overwritten by the next call)."""
        self._need_device()
        o = self._obs(obs)
        m = None
        if need is not None:
            m = need if torch.is_tensor(need) else torch.as_tensor(np.asarray(need))
            if tuple(m.shape) != (self.n_envs,):
                raise ValueError(f"need must be [{self.n_envs}], got {list(m.shape)}")
            m = m.to(device=self.device, dtype=torch.uint8).contiguous()
        dst = self._pv if out is None else out
        if tuple(dst.shape) != (self.n_envs,) or dst.dtype != torch.float32 or dst.device != self.device \
                or not dst.is_contiguous():
            raise ValueError(f"out must be a contiguous f32 [{self.n_envs}] tensor on {self.device}")
        self._launch_values(o, m, dst)
        self._keep_values = [o, m]
        return dst

    def forward_host(self, obs: Dict[str, Any]):
        """``(mean [n, A], value [n])`` numpy f32 from the library's host model of the kernel's
        arithmetic, for any number of rows.  A test oracle."""
        (o, n), (ws, bs) = self._host_obs(obs), self._host_params()
        ls = np.ascontiguousarray(self._log_std_lib.cpu().numpy())
        w = self._weights_struct([x.ctypes.data for x in ws], [x.ctypes.data for x in bs], ls.ctypes.data)
        mean = np.zeros((n, self.action_dim), np.float32)
        value = np.zeros((n,), np.float32)
        self._call("forward_host", C.byref(self._cfg), C.byref(w), abi.ptr(o["observation"]),
                       abi.ptr(o["achieved_goal"]), abi.ptr(o["desired_goal"]), n, abi.ptr(mean), abi.ptr(value))
        return mean, value

    noise_step = property(Policy._get_word, Policy._set_word, doc="""The device word that counts the forwards that
        drew noise from the Philox stream (this synchronises).  Setting it back reproduces the draws.""")

    # -------------------------------------------------------------- rollouts
    def _rollout_buffers(self, venv, buf):
        from .rollout import step_buffers, terminal_observation

        self._need_device()
        if self.use_sde:
            raise PgxError("gSDE exploration is not built: a use_sde=True ActorCritic collects no rollout")
        if buf.n_envs != self.n_envs or buf.obs_dim != self.obs_dim or buf.action_dim != self.action_dim \
                or buf.device != self.device:
            raise ValueError("the RolloutBuffer does not fit this ActorCritic")
        obs, reward, terminated, truncated = step_buffers(venv)
        tobs = terminal_observation(venv)
        self._check_venv_obs(obs)
        self._check_venv_obs(tobs)
        if truncated.dtype != torch.uint8 or tuple(truncated.shape) != (self.n_envs,) or not truncated.is_contiguous():
            raise ValueError("venv's truncated flags must be a contiguous uint8 [N] tensor")
        return obs, reward, terminated, truncated, tobs

    def _enqueue_rollout(self, venv, buf, deterministic: bool, bufs) -> None:
        obs, reward, terminated, truncated, tobs = bufs
        for _ in range(buf.buffer_size):
            self._launch(obs, deterministic, None)
            venv._enqueue_step(self.clipped_actions, "pgx_step (rollout)")
            # the time-limit bootstrap: V(terminal observation), computed only in tiles with a truncated env
            self._launch_values(tobs, truncated, self.terminal_values)
            buf._launch_add(self.actions, reward, self.values, self.log_probs, self.terminal_values, obs, terminated,
                            truncated)
        self._launch_values(obs, None, self.last_values)
        buf.enqueue_returns_and_advantage(self.last_values)

    def collect_rollouts(self, venv, buf, deterministic: bool = False) -> None:
        """SB3's ``OnPolicyAlgorithm.collect_rollouts`` for ``buf.buffer_size`` steps, enqueued on the
        current stream with no sync: per step the forward on ``venv``'s persistent observation buffers
        (through a ``VecNormalize`` the normalised ones), ``venv._enqueue_step(clipped_actions)``,
        V(terminal observation) for the tiles with a truncated env, the buffer's add with that
        ``terminal_value``; then V(last observation) and the GAE pass.  ``venv``: the env, a
        ``VecNormalize`` or a ``VecMonitor``.  The caller has done ``buf.set_last(venv.reset_tensors())``
        once and ``buf.reset()`` before each rollout; ``buf.raise_device_errors()`` looks afterwards."""
        self._enqueue_rollout(venv, buf, deterministic, self._rollout_buffers(venv, buf))

    def capture_rollout(self, venv, buf, deterministic: bool = False):
        """The enqueue sequence of ``collect_rollouts`` captured into one HIP graph
        (``torch.cuda.CUDAGraph``).  Capture runs nothing; every replay draws new noise (the step word
        is on the device) and uses the weights loaded last.  ``buf.reset()`` goes before each replay."""
        bufs = self._rollout_buffers(venv, buf)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._enqueue_rollout(venv, buf, deterministic, bufs)
        g._pgx_keep = (self, buf, bufs)   # the graph reads these buffers at replay
        return g
