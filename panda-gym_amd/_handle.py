"""What every Python object over a libpgx handle shares (``PandaVecEnv``, ``HerReplayBuffer``, ``Normalizer``,
``EpisodeMonitor``, ``RolloutBuffer`` and the policies): the one torch import, the refusals without torch or
off a HIP device, the handle's life (create, stream, close), the checked call of an entry point by its short
name, the conversion of an input to a device tensor, the sticky device error word, and the resolution of
env / spaces / dims in front of a buffer.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Optional, Tuple

import numpy as np

from ._native import PgxError, check

try:
    import torch
except ImportError:  # pragma: no cover - torch is part of the image
    torch = None

OBS_KEYS = ("observation", "achieved_goal", "desired_goal")


def _view(addr: int, shape, dtype, device):
    """Wrap a libpgx-owned device buffer as a torch tensor (no copy)."""
    typestr = {torch.float32: "<f4", torch.float64: "<f8", torch.int32: "<i4", torch.int64: "<i8"}[dtype]

    class _Iface:  # torch has no public from-pointer constructor; use __cuda_array_interface__
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(addr), False),
                                    "version": 2, "strides": None}

    return torch.as_tensor(_Iface(), device=device)


def resolve_dims(env: Any, observation_space: Any, action_space: Any, n_envs: int, obs_dim: Optional[int],
                 action_dim: Optional[int]) -> Tuple[int, int, int]:
    """(n_envs, obs_dim, action_dim) of a buffer: read from ``env`` where it is given, else from the
    spaces, else as passed."""
    if env is not None:
        n_envs = env.num_envs
        obs_dim = env.obs_dim if obs_dim is None else obs_dim
        action_dim = env.action_dim if action_dim is None else action_dim
    if observation_space is not None and obs_dim is None:
        obs_dim = int(np.prod(observation_space["observation"].shape))
    if action_space is not None and action_dim is None:
        action_dim = int(np.prod(action_space.shape))
    if obs_dim is None or action_dim is None:
        raise ValueError("obs_dim/action_dim: pass env, the spaces, or the dims")
    return int(n_envs), int(obs_dim), int(action_dim)


class Handle:
    """Base of the classes that own one libpgx handle ``_h`` of the library ``lib`` on ``device``.  A subclass
    sets ``_PREFIX``, its C entry points' prefix."""

    _PREFIX = ""
    _NEEDS = "device buffers"
    _LIVES = "lives on a HIP device only (no CPU fallback)"

    @classmethod
    def _need_torch(cls) -> None:
        if torch is None:
            raise PgxError(f"{cls.__name__} needs torch for {cls._NEEDS}")

    def _on_device(self, device: Any) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise PgxError(f"{type(self).__name__} {self._LIVES}")

    def _call(self, name: str, *args) -> None:
        """``<prefix>_<name>(*args)``, checked.  For the cold entry points: a per-step launch calls
        ``self.lib.<entry>`` itself."""
        entry = f"{self._PREFIX}_{name}"
        check(getattr(self.lib, entry)(*args), entry, self.lib)

    def _create(self, cfg) -> None:
        h = C.c_void_p()
        torch.cuda.set_device(self.device)
        self._call("create", C.byref(cfg), self.device.index or 0, C.byref(h))
        self._h = h

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self) -> None:
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            getattr(self.lib, f"{self._PREFIX}_destroy")(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, x, shape, dtype=None) -> "torch.Tensor":
        """``x`` (host or device) as a contiguous device tensor of ``shape`` (``dtype`` None: f32); a no-op
        for a tensor that is one already."""
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        return t.to(device=self.device, dtype=dtype or torch.float32).reshape(shape).contiguous()

    @staticmethod
    def _raise_flags(err: int, table: Dict[int, str], word: str) -> None:
        """Raise what the bits of a sticky device error word say (``table``: bit -> message)."""
        if err:
            names = [msg for bit, msg in table.items() if err & bit]
            raise PgxError("; ".join(names) if names else f"{word} device error flags 0x{err:x}")
