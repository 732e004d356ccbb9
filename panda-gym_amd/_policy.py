"""What the device-resident policies (``Actor``, ``ActorCritic``, ``SdeActor``, ``QuantileCritic``) share on the
Python side:
resolving env, dims and device, the handle's life, the observation shaping in front of a launch, the
parameter slots behind ``state_dict`` / ``load_state_dict``, the numpy conversions in front of the host
model, the device noise word, and the check of a venv's persistent buffers in front of a capture.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ._handle import OBS_KEYS, Handle, torch  # noqa: F401  (OBS_KEYS, torch: importable from here as before)
from ._native import PgxError, load


class Policy(Handle):
    """Base of the four policies.  A subclass sets ``_PREFIX`` (its C entry points' prefix) and ``_WHO``
    (its name in a buffer-fit message), builds ``_cfg``, ``_names``, ``_w``, ``_b``, and defines ``_slots``,
    ``_push`` and ``forward_host``."""

    _NEEDS = "its buffers"
    _WHO = "actor"
    _SD_PREFIX: Optional[str] = None   # keys of a whole policy's state dict to read, when it has any

    def _resolve(self, env: Any, obs_dim: Optional[int], action_dim: Optional[int], n_envs: Optional[int],
                 device: Any) -> None:
        if env is not None:
            n_envs = env.num_envs
            obs_dim = env.obs_dim if obs_dim is None else obs_dim
            action_dim = env.action_dim if action_dim is None else action_dim
            device = env.device if device is None else device
        if obs_dim is None or action_dim is None or n_envs is None:
            raise ValueError("pass env, or obs_dim, action_dim and n_envs")
        if int(n_envs) <= 0:
            raise ValueError("n_envs must be > 0")
        self.lib = load()
        self.device = torch.device("cuda:0" if device is None else device)
        self.n_envs, self.obs_dim, self.action_dim = int(n_envs), int(obs_dim), int(action_dim)
        self._h = None
        self._debug: Optional[Dict[str, "torch.Tensor"]] = None
        self._keep: List[Any] = []

    def _open(self, *host_extra) -> None:
        """The device handle with the parameters pushed; on a CPU device the library's argument checks
        either way: the host model on no rows."""
        if self.device.type == "cuda":
            self._create(self._cfg)
            self._push()
        else:
            self.forward_host({"observation": np.zeros((0, self.obs_dim), np.float32),
                               "achieved_goal": np.zeros((0, 3), np.float32), "desired_goal": np.zeros((0, 3), np.float32)},
                              *host_extra)

    def _need_device(self):
        if self._h is None:
            raise PgxError(f"this {type(self).__name__} has no device handle (device='cpu' or closed): no CPU fallback")

    # ----------------------------------------------------------- parameters
    def _pairs(self) -> List[Tuple[str, "torch.Tensor"]]:
        """(key, tensor) of every Linear's weight and bias, in ``_names`` order."""
        out = []
        for name, w, b in zip(self._names, self._w, self._b):
            out += [(f"{name}.weight", w), (f"{name}.bias", b)]
        return out

    def state_dict(self) -> Dict[str, "torch.Tensor"]:
        """The parameters under SB3's key names (copies, on this policy's device)."""
        return {k: t.clone() for k, t in self._slots()}

    def _shape_hint(self, key: str) -> str:
        return ""

    def _load_slots(self, sd: Dict[str, Any]) -> None:
        """Every ``(key, tensor)`` of ``_slots()`` is validated before the first one is copied: a failed load
        changes nothing.  The copies are in place (the handle's copies read these same buffers)."""
        p = self._SD_PREFIX
        if p and any(k.startswith(p) for k in sd):
            sd = {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
        slots, new = self._slots(), []
        for key, cur in slots:
            if key not in sd:
                raise KeyError(f"load_state_dict: missing key {key!r}")
            v = sd[key]
            t = v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))
            if tuple(t.shape) != tuple(cur.shape):
                raise ValueError(f"load_state_dict: {key!r} has shape {tuple(t.shape)}, expected {tuple(cur.shape)}"
                                 f"{self._shape_hint(key)}")
            new.append(t.to(device=self.device, dtype=torch.float32).contiguous())
        for (_, cur), t in zip(slots, new):
            cur.copy_(t)
        if self._h is not None:
            self._push()

    def _host_params(self):
        """The Linears' weights and biases as contiguous numpy arrays, for the host model."""
        return ([np.ascontiguousarray(t.cpu().numpy()) for t in self._w],
                [np.ascontiguousarray(t.cpu().numpy()) for t in self._b])

    # --------------------------------------------------------- observations
    def _dev(self, x, shape) -> "torch.Tensor":
        """Unlike ``Handle._dev``, no reshape: an input of another shape is refused."""
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if tuple(t.shape) != shape:
            raise ValueError(f"expected shape {list(shape)}, got {list(t.shape)}")
        return t.to(device=self.device, dtype=torch.float32).contiguous()   # a no-op for the env's own buffers

    def _obs_shape(self, key: str) -> Tuple[int, int]:
        return (self.n_envs, self.obs_dim if key == "observation" else 3)

    def _obs(self, obs: Dict[str, Any]) -> Dict[str, "torch.Tensor"]:
        return {k: self._dev(obs[k], self._obs_shape(k)) for k in OBS_KEYS}

    @staticmethod
    def _host_obs(obs: Dict[str, Any]):
        """The observation dict as contiguous numpy f32, and its number of rows."""
        o = {k: np.ascontiguousarray(obs[k].cpu().numpy() if torch.is_tensor(obs[k]) else obs[k], dtype=np.float32)
             for k in OBS_KEYS}
        return o, o["observation"].shape[0]

    def _check_venv_obs(self, obs: Dict[str, "torch.Tensor"]) -> None:
        """A venv's persistent observation buffers must be what a launch can read in place."""
        for key in OBS_KEYS:
            t = obs[key]
            if tuple(t.shape) != self._obs_shape(key) or t.dtype != torch.float32 or t.device != self.device \
                    or not t.is_contiguous():
                raise ValueError(f"venv's {key} buffer does not fit this {self._WHO}")

    # ----------------------------------------------------------- noise word
    def _get_word(self) -> int:
        self._need_device()
        v = C.c_uint64(0)
        self._call("state", self._h, C.byref(v), self._stream())
        return int(v.value)

    def _set_word(self, value: int) -> None:
        self._need_device()
        self._call("set_state", self._h, C.c_uint64(int(value) & 0xFFFFFFFFFFFFFFFF), self._stream())
