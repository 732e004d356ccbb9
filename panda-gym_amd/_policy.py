"""What the device-resident policies (``Actor``, ``ActorCritic``, ``SdeActor``, ``QuantileCritic``) share on the
Python side:
resolving env, dims and device, the handle's life, the observation shaping in front of a launch (per env, or
``_rows_into`` / ``_f32_out`` for the batch launches), the
parameter slots behind ``state_dict`` / ``load_state_dict``, the numpy conversions in front of the host
model, the device noise word, and the check of a venv's persistent buffers in front of a capture.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ._handle import OBS_KEYS, Handle, torch  # noqa: F401  (OBS_KEYS, torch: importable from here as before)
from ._native import PgxError, load
from .abi import ptr as abi_ptr


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

    def _field(self, x, width: int, B: Optional[int], name: str):
        """A row-indexed input as (tensor, row stride in floats): a device f32 tensor [B, width] (or [B] for
        width 1) whose rows are contiguous is read in place, whatever its row stride; anything else is
        copied to a dense one."""
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if t.dim() == 1 and width == 1:
            t = t.unsqueeze(1)
        if t.dim() != 2 or t.shape[1] != width or (B is not None and t.shape[0] != B):
            raise ValueError(f"{name}: expected shape [{'B' if B is None else B}, {width}], got {list(t.shape)}")
        ok = t.dtype == torch.float32 and t.device == self.device and (width == 1 or t.stride(1) == 1) \
            and (t.shape[0] == 1 or t.stride(0) >= width)
        if not ok:
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
        return t, (width if t.shape[0] == 1 else int(t.stride(0)))

    # ------------------------------------------------- action log-probability (Actor, SdeActor)
    _LP_PHILOX = False   # the unit draws its noise inside the launch and can record the words

    def _lp_planes(self) -> Dict[str, int]:
        """Name -> width of the debug planes of ``action_log_prob``."""
        raise PgxError(f"{type(self).__name__} has no action_log_prob")

    # ------------------------------------------------- batch launches (rows of any number, through row strides)
    def _rows_into(self, io, obs: Dict[str, Any], actions=None):
        """Fills any batch launch's ``io`` with the observation fields (and, given ``actions``, the action) and
        their row strides, read in place where they can be.  Returns (B, what the launch reads)."""
        o, io.obs_stride = self._field(obs["observation"], self.obs_dim, None, "observation")
        B = int(o.shape[0])
        ag, io.achieved_goal_stride = self._field(obs["achieved_goal"], 3, B, "achieved_goal")
        dg, io.desired_goal_stride = self._field(obs["desired_goal"], 3, B, "desired_goal")
        io.obs, io.achieved_goal, io.desired_goal = o.data_ptr(), ag.data_ptr(), dg.data_ptr()
        keep = [o, ag, dg]
        if actions is not None:
            a, io.action_stride = self._field(actions, self.action_dim, B, "actions")
            io.action = a.data_ptr()
            keep.append(a)
        return B, keep

    def _f32_out(self, t, B: int, tail: Tuple[Optional[int], ...], what: str) -> "torch.Tensor":
        """``t`` where it is a contiguous f32 [>= B, *tail] tensor on this device (``None`` in ``tail``: any
        width), for ``None`` a new one; anything else is refused with ``what``."""
        if t is None:
            return torch.empty((B,) + tuple(tail), dtype=torch.float32, device=self.device)
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous() \
                or t.dim() != 1 + len(tail) or t.shape[0] < B \
                or any(w is not None and n != w for n, w in zip(t.shape[1:], tail)):
            raise ValueError(what)
        return t

    def _lp_io(self, io, obs: Dict[str, Any], out):
        """Fills an ``action_log_prob`` launch's ``io`` (``PgxActorLpIo`` / ``PgxSdeActorLpIo``): the observation
        fields, and the outputs ``(actions [B, A], log_prob [B])``, ``out`` or new tensors.  Returns (B, actions,
        log_prob, what the launch reads)."""
        B, keep = self._rows_into(io, obs)
        what = f"out must be contiguous f32 tensors [>= {B}, {self.action_dim}] and [>= {B}] on {self.device} " \
               f"(rows past {B} are left alone)"
        act, lp = (None, None) if out is None else out
        if out is not None and (act is None or lp is None):
            raise ValueError(what)
        act, lp = self._f32_out(act, B, (self.action_dim,), what), self._f32_out(lp, B, (), what)
        io.action, io.log_prob = act.data_ptr(), lp.data_ptr()
        return B, act, lp, keep

    def enable_log_prob_debug(self, B: int) -> Dict[str, "torch.Tensor"]:
        """Allocate the debug planes every later ``action_log_prob`` of ``B`` rows fills: f32 [B, width] per
        name of ``_lp_planes()``, and ``philox`` [B, 4, 4] int32 where the unit draws its noise in that
        launch.  Tests and tools only; ``None`` turns them off."""
        self._need_device()
        if B is None:
            self._lp_debug = None
            return {}
        z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=self.device)  # noqa: E731
        d = {k: z(int(B), w) for k, w in self._lp_planes().items()}
        if self._LP_PHILOX:
            d["philox"] = z(int(B), 4, 4, dt=torch.int32)
        self._lp_debug = d
        return d

    def _lp_debug_into(self, io, B: int) -> None:
        d = getattr(self, "_lp_debug", None)
        if d is None:
            return
        if next(iter(d.values())).shape[0] != B:
            raise ValueError(f"the debug planes hold {next(iter(d.values())).shape[0]} rows, the batch {B}")
        for k, t in d.items():
            setattr(io, f"{k}_out", t.data_ptr())

    @staticmethod
    def _batch_obs(batch: Dict[str, "torch.Tensor"], next: bool) -> Dict[str, "torch.Tensor"]:
        """The observation dict of a HER batch (``buf.alloc_batch``): its ``next_*`` fields, or the current ones."""
        p = "next_" if next else ""
        return {"observation": batch[p + "obs"], "achieved_goal": batch[p + "achieved_goal"],
                "desired_goal": batch[p + "desired_goal"]}

    def _host_rows_into(self, io, obs: Dict[str, Any], actions=None):
        """``_rows_into`` for a host model: dense numpy inputs.  Returns (n, what the call reads)."""
        o, n = self._host_obs(obs)
        io.obs, io.achieved_goal, io.desired_goal = (abi_ptr(o["observation"]), abi_ptr(o["achieved_goal"]),
                                                     abi_ptr(o["desired_goal"]))
        io.obs_stride, io.achieved_goal_stride, io.desired_goal_stride = self.obs_dim, 3, 3
        if actions is None:
            return n, [o]
        a = np.ascontiguousarray(actions.cpu().numpy() if torch.is_tensor(actions) else actions, dtype=np.float32)
        if o["observation"].shape != (n, self.obs_dim) or a.shape != (n, self.action_dim):
            raise ValueError(f"expected observation [n, {self.obs_dim}] and actions [n, {self.action_dim}]")
        io.action, io.action_stride = abi_ptr(a), self.action_dim
        return n, [o, a]

    def _host_lp_io(self, io, obs: Dict[str, Any], planes: Dict[str, int]):
        """Fills ``io`` for a host model: dense numpy inputs, and every output and plane as a new array.
        Returns (n, {name: array})."""
        n, (o,) = self._host_rows_into(io, obs)
        res = {"action": np.zeros((n, self.action_dim), np.float32), "log_prob": np.zeros((n,), np.float32)}
        io.action, io.log_prob = abi_ptr(res["action"]), abi_ptr(res["log_prob"])
        for k, w in planes.items():
            res[k] = np.zeros((n, w), np.float32)
            setattr(io, f"{k}_out", abi_ptr(res[k]))
        res["_keep"] = o
        return n, res

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
