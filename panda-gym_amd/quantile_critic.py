"""Device-resident quantile critics: sb3_contrib TQC's ``critic`` / ``critic_target`` forward and the
truncated TD target of ``TQC.train`` as one HIP launch.

The reference trains TQC with HER (hyperparameters.py: batch 256, ``gradient_steps`` 8, ``net_arch`` [256,
256] or [400, 300], ``top_quantiles_to_drop_per_net`` 5 in ``TQC_v2``).  Every no-grad line of a gradient
step -- ``critic_target(next_obs, next_actions)``, the pooled sort, the truncation, the entropy term, the
Bellman backup, the Polyak step -- is inference on ``Linear + ReLU`` stacks, and ``QuantileCritic`` runs it
in libpgx.so (pgx_quantile_critic.hip; C-ABI, arithmetic contract and the sort's order rule in
include/pgx.h, section "QuantileCritic").  A launch reads dense tensors or, through row strides, the fields
of a HER batch's ``rows`` (``buf.alloc_batch`` / ``buf.sample_into``) where they lie.  (Through the C entry
point, ``n_quantiles = 1`` with ``n_target = 1`` is SAC's / TD3's ``min`` over the critics.)  No CPU
fallback: with ``device="cpu"`` a ``QuantileCritic`` only holds and maps parameters (``load_state_dict`` /
``state_dict`` / ``forward_host`` / ``td_target_host``, the host models of the kernels' arithmetic, which
are test oracles).

``next_actions`` and ``next_log_prob`` are the caller's buffers: ``Actor.action_log_prob_rows`` /
``SdeActor.action_log_prob_rows`` fill them from the same batch in one launch (actor.py, sde_actor.py).

The critic update runs there too (include/pgx.h, "QuantileCritic, the critic update"): ``critic_loss_backward``
is ``quantile_huber_loss(critic(obs, actions), target_quantiles)`` and its gradient for every online parameter
in two launches, ``adam_step`` is ``torch.optim.Adam``'s step on them with the learning rate read from the
device, and both capture behind ``td_target_rows`` in one graph.  ``critic_grad_host`` / ``adam_step_host`` are
the host models of that arithmetic (test oracles).

Not here: the actor loss's Q mean and dQ/d(action), the ``ent_coef`` loss, the actor's optimiser, gradient
clipping.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from ._native import PgxError, check
from ._policy import Policy, torch

SETS = ("online", "target")
SD_PREFIX = {"online": "critic.", "target": "critic_target."}


class QuantileCritic(Policy):
    """sb3_contrib's TQC critics (``tqc/policies.py`` ``Critic``) and their target copy on the device.

    ``env``: a ``PandaVecEnv`` or a wrapper of one (the dims and the device are read from it), or pass
    ``obs_dim`` and ``action_dim``.  ``net_arch``: 1 to 3 hidden widths of 1 to 512.  ``n_critics`` 1..5,
    ``n_quantiles`` 1..32, their product at most 128.  The target keeps the ``n_target = n_critics *
    (n_quantiles - top_quantiles_to_drop_per_net)`` lowest of the pooled quantiles.  The batch size is
    whatever a call is given.  Both parameter sets are zero until ``load_state_dict``."""

    _PREFIX = "pgx_qc"
    _WHO = "critic"

    def __init__(self, env: Any = None, obs_dim: Optional[int] = None, action_dim: Optional[int] = None,
                 net_arch: Sequence[int] = (256, 256), n_critics: int = 2, n_quantiles: int = 25,
                 top_quantiles_to_drop_per_net: int = 2, gamma: float = 0.99, device: Any = None):
        self._need_torch()
        self._resolve(env, obs_dim, action_dim, 1, device)   # (no per-env storage: the batch is a launch argument)
        self.net_arch = tuple(int(w) for w in net_arch)
        self.n_critics, self.n_quantiles = int(n_critics), int(n_quantiles)
        self.top_quantiles_to_drop_per_net, self.gamma = int(top_quantiles_to_drop_per_net), float(gamma)
        self.n_pool = self.n_critics * self.n_quantiles
        self.n_target = self.n_pool - self.top_quantiles_to_drop_per_net * self.n_critics
        if self.top_quantiles_to_drop_per_net < 0 or (self.n_pool > 0 and self.n_target < 1):
            raise ValueError(f"top_quantiles_to_drop_per_net must be in 0..n_quantiles - 1, got "
                             f"{top_quantiles_to_drop_per_net}")
        cfg = abi.PgxQcConfig()
        cfg.obs_dim, cfg.action_dim, cfg.n_layers = self.obs_dim, self.action_dim, len(self.net_arch)
        for i, w in enumerate(self.net_arch[:abi.ACTOR_MAX_LAYERS]):
            cfg.hidden[i] = w
        cfg.n_critics, cfg.n_quantiles, cfg.gamma = self.n_critics, self.n_quantiles, self.gamma
        self._cfg = cfg
        # the parameters as given (torch layout), per set and critic: what set_weights reads
        dims = [self.obs_dim + 6 + self.action_dim] + list(self.net_arch) + [self.n_quantiles]
        nc = min(max(self.n_critics, 0), abi.QC_MAX_CRITICS)   # (out of range: the library rejects it below)
        shapes = [(max(dims[i + 1], 0), dims[i]) for i in range(min(len(dims) - 1, 4))]
        self._names = [f"qf{c}.{2 * l}" for c in range(nc) for l in range(len(shapes))]
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)  # noqa: E731
        self._ws = {s: [z(*shp) for _ in range(nc) for shp in shapes] for s in SETS}
        self._bs = {s: [z(shp[0]) for _ in range(nc) for shp in shapes] for s in SETS}
        self._n_linear = len(shapes)
        self._loading: Tuple[str, ...] = SETS
        # The tensors here may lag the handle's copies: the target's once a Polyak step or a sync was enqueued,
        # the online set's once an Adam step was.  They stay set: a captured graph moves the handle's copies at
        # every replay, and nothing here sees a replay.
        self._stale = False
        self._stale_online = False
        self._opt: Optional[Tuple[float, float, float]] = None   # (beta1, beta2, eps) once init_optimizer ran
        self._open()

    # ------------------------------------------------------------ plumbing
    def _open(self) -> None:
        """The device handle with both sets pushed; on a CPU device the library's argument checks either
        way: the host model on one zero row."""
        if self.device.type == "cuda":
            super()._open()
        else:
            self.forward_host({"observation": np.zeros((1, self.obs_dim), np.float32),
                               "achieved_goal": np.zeros((1, 3), np.float32), "desired_goal": np.zeros((1, 3), np.float32)},
                              np.zeros((1, self.action_dim), np.float32))

    @staticmethod
    def _which(which: str) -> str:
        if which not in SETS:
            raise ValueError(f"which must be one of {list(SETS)}, got {which!r}")
        return which

    def _weights_struct(self, ws, bs) -> abi.PgxQcWeights:
        """``ws`` / ``bs``: every critic's Linears in ``_names`` order, tensors or numpy arrays."""
        p = lambda x: x.data_ptr() if torch.is_tensor(x) else x.ctypes.data  # noqa: E731
        w = abi.PgxQcWeights()
        for i, (x, y) in enumerate(zip(ws, bs)):
            c, l = divmod(i, self._n_linear)
            w.weight[c][l], w.bias[c][l] = p(x), p(y)
        return w

    def _set_struct(self, which: str) -> abi.PgxQcWeights:
        return self._weights_struct(self._ws[which], self._bs[which])

    def _push(self) -> None:
        for s in self._loading:
            w = self._set_struct(s)
            self._call("set_weights", self._h, abi.QC_SETS[s], C.byref(w), self._stream())

    def _pull_target(self) -> None:
        """The handle's plain copies into the tensors here: the target set after a Polyak step or a sync, the
        online set after an Adam step."""
        if self._h is not None and self._stale:
            w = self._set_struct("target")
            self._call("get_weights", self._h, abi.QC_TARGET, C.byref(w), self._stream())
        if self._h is not None and self._stale_online:
            w = self._set_struct("online")
            self._call("get_weights", self._h, abi.QC_ONLINE, C.byref(w), self._stream())

    # ----------------------------------------------------------- parameters
    def _set_pairs(self, which: str, prefix: str = "") -> List[Tuple[str, "torch.Tensor"]]:
        out = []
        for name, w, b in zip(self._names, self._ws[which], self._bs[which]):
            out += [(f"{prefix}{name}.weight", w), (f"{prefix}{name}.bias", b)]
        return out

    def _slots(self) -> List[Tuple[str, "torch.Tensor"]]:
        """The sets a load is filling, under a whole policy's key names."""
        return [p for s in self._loading for p in self._set_pairs(s, SD_PREFIX[s])]

    def state_dict(self, which: str = "online") -> Dict[str, "torch.Tensor"]:
        """Set ``which``'s parameters (``"online"``: ``critic``; ``"target"``: ``critic_target``, as the last
        Polyak step left it) under sb3_contrib's key names ``qf{i}.{0,2,4}.weight|bias`` (copies); ``"both"``:
        the two under a policy's ``critic.`` / ``critic_target.`` prefixes."""
        self._pull_target()
        if which == "both":
            return {k: t.clone() for s in SETS for k, t in self._set_pairs(s, SD_PREFIX[s])}
        return {k: t.clone() for k, t in self._set_pairs(self._which(which))}

    def load_state_dict(self, sd: Dict[str, Any], which: Optional[str] = None) -> None:
        """Load critic parameters.  A whole policy's state dict (``critic.qf0.0.weight`` ...,
        ``critic_target.qf0.0.weight`` ...; everything else ignored) fills every set whose prefix it holds, or
        with ``which`` that set alone; a critic's own dict (``qf0.0.weight`` ...) fills set ``which``, the
        online one by default.  Every key is validated before the first parameter is copied.  The packed
        weights in the handle are replaced on the current stream: a captured graph uses them at its next
        replay."""
        prefixed = any(k.startswith(p) for k in sd for p in SD_PREFIX.values())
        if which is not None:
            sets: Tuple[str, ...] = (self._which(which),)
        elif prefixed:
            sets = tuple(s for s in SETS if any(k.startswith(SD_PREFIX[s]) for k in sd))
        else:
            sets = ("online",)
        if not prefixed:
            sd = {f"{SD_PREFIX[s]}{k}": v for s in sets for k, v in sd.items()}
        if sets != SETS:
            self._pull_target()   # (a later state_dict must not read a stale set over this load)
        self._loading = sets
        try:
            self._load_slots(sd)
        finally:
            self._loading = SETS

    # --------------------------------------------------------------- launches
    def _io(self, obs: Dict[str, Any], actions):
        io = abi.PgxQcIo()
        B, keep = self._rows_into(io, obs, actions)
        return io, B, keep

    def _out(self, out, B: int, width: int) -> "torch.Tensor":
        return self._f32_out(out, B, (width,), f"out must be a contiguous f32 [>= {B}, {width}] tensor on {self.device}")

    def critic(self, obs: Dict[str, Any], actions, target: bool = False, out=None) -> "torch.Tensor":
        """Quantiles [B, n_critics, n_quantiles] of ``critic(obs, actions)`` (``target``: of
        ``critic_target``): one launch.  ``obs``: the observation dict, [B, .] each; device f32 tensors, views
        into a HER batch's rows included, are read in place.  ``out``: a contiguous f32 [>= B, n_critics *
        n_quantiles] tensor to fill (returned as it is; its rows past B are left alone)."""
        self._need_device()
        io, B, keep = self._io(obs, actions)
        q = self._out(out, B, self.n_pool)
        io.out = q.data_ptr()
        check(self.lib.pgx_qc_forward(self._h, abi.QC_TARGET if target else abi.QC_ONLINE, C.byref(io), B, self._stream()),
              "pgx_qc_forward", self.lib)
        self._keep = keep + [q]
        return q.view(B, self.n_critics, self.n_quantiles) if out is None else out

    def td_target(self, next_obs: Dict[str, Any], next_actions, next_log_prob, rewards, dones, ent_coef, out=None,
                  quantiles=None) -> "torch.Tensor":
        """``TQC.train``'s target quantiles [B, n_target]: ``critic_target(next_obs, next_actions)``, pooled,
        sorted, the lowest ``n_target`` kept, ``- ent_coef * next_log_prob``, ``rewards + (1 - dones) * gamma
        *``: one launch.  ``rewards`` / ``dones``: [B] or [B, 1] f32; ``ent_coef``: a device tensor of one
        float, read at every launch (a replayed graph sees its current value), or a number.  ``out``: a
        contiguous f32 [>= B, n_target] tensor to fill (its rows past B are left alone).  ``quantiles``
        (debug): a contiguous f32 [B, n_critics * n_quantiles] tensor that receives the unsorted pool."""
        self._need_device()
        io, B, keep = self._io(next_obs, next_actions)
        r, io.reward_stride = self._field(rewards, 1, B, "rewards")
        d, io.done_stride = self._field(dones, 1, B, "dones")
        lp, _ = self._field(next_log_prob, 1, B, "next_log_prob")
        if not lp.is_contiguous():
            lp = lp.contiguous()
        e = ent_coef if torch.is_tensor(ent_coef) else torch.as_tensor(float(ent_coef))
        if e.numel() != 1:
            raise ValueError("ent_coef must hold one float")
        e = e.detach().to(device=self.device, dtype=torch.float32).reshape(1)
        t = self._out(out, B, self.n_target)
        io.reward, io.done, io.next_log_prob, io.ent_coef, io.out = r.data_ptr(), d.data_ptr(), lp.data_ptr(), \
            e.data_ptr(), t.data_ptr()
        if quantiles is not None:
            io.quantiles_out = self._out(quantiles, B, self.n_pool).data_ptr()
        self._call("target", self._h, C.byref(io), B, self.n_target, self._stream())
        self._keep = keep + [r, d, lp, e, t, quantiles]
        return t

    def td_target_rows(self, batch: Dict[str, "torch.Tensor"], next_actions, next_log_prob, ent_coef,
                       out=None) -> "torch.Tensor":
        """``td_target`` on a HER batch (``buf.alloc_batch`` / ``buf.sample_into``): ``next_obs``,
        ``next_achieved_goal``, ``next_desired_goal``, ``reward`` and ``done`` are read from ``batch["rows"]``
        in place."""
        return self.td_target(self._batch_obs(batch, True), next_actions, next_log_prob, batch["reward"], batch["done"], ent_coef, out=out)

    def polyak_update(self, tau: float) -> None:
        """SB3's ``polyak_update(critic.parameters(), critic_target.parameters(), tau)`` on the handle's
        copies, by the rule of include/pgx.h (``t = fmaf(tau, p, t * (1 - tau))``), then the target's
        packing, on the current stream: the next target launch, eager or a replay, uses it.  Device only."""
        self._need_device()
        self._call("polyak", self._h, C.c_double(float(tau)), self._stream())
        self._stale = True

    def sync_target(self) -> None:
        """``critic_target.load_state_dict(critic.state_dict())``: the online set into the target, bit for
        bit, one launch on the current stream.  Device only."""
        self._need_device()
        self._call("sync_target", self._h, self._stream())
        self._stale = True

    # ------------------------------------------------------------ host models
    def _host_io(self, obs: Dict[str, Any], actions):
        io = abi.PgxQcIo()
        n, keep = self._host_rows_into(io, obs, actions)
        return io, n, keep

    def _host_set(self, which: str):
        self._pull_target()
        ws = [np.ascontiguousarray(t.cpu().numpy()) for t in self._ws[which]]
        bs = [np.ascontiguousarray(t.cpu().numpy()) for t in self._bs[which]]
        return self._weights_struct(ws, bs), [ws, bs]

    def forward_host(self, obs: Dict[str, Any], actions, target: bool = False) -> np.ndarray:
        """Quantiles [n, n_critics, n_quantiles] numpy f32 from the library's host model of the kernel's
        arithmetic.  A test oracle."""
        io, n, keep = self._host_io(obs, actions)
        w, keep_w = self._host_set("target" if target else "online")
        out = np.zeros((n, self.n_critics, self.n_quantiles), np.float32)
        io.out = abi.ptr(out)
        self._call("forward_host", C.byref(self._cfg), C.byref(w), C.byref(io), n)
        return out

    def td_target_host(self, next_obs: Dict[str, Any], next_actions, next_log_prob, rewards, dones, ent_coef,
                       n_target: Optional[int] = None, return_quantiles: bool = False):
        """``td_target`` [n, n_target] numpy f32 from the library's host model (the target set as the last
        Polyak step left it).  ``return_quantiles``: also the unsorted pool [n, n_critics * n_quantiles]."""
        io, n, keep = self._host_io(next_obs, next_actions)
        w, keep_w = self._host_set("target")
        f = lambda x: np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x,  # noqa: E731
                                           dtype=np.float32).reshape(-1)
        r, d, lp, e = f(rewards), f(dones), f(next_log_prob), f(ent_coef)
        if r.shape != (n,) or d.shape != (n,) or lp.shape != (n,) or e.shape != (1,):
            raise ValueError("rewards, dones and next_log_prob must hold n floats, ent_coef one")
        nt = self.n_target if n_target is None else int(n_target)
        out = np.zeros((n, max(nt, 0)), np.float32)
        pool = np.zeros((n, self.n_pool), np.float32)
        io.reward, io.done, io.next_log_prob, io.ent_coef = abi.ptr(r), abi.ptr(d), abi.ptr(lp), abi.ptr(e)
        io.reward_stride = io.done_stride = 1
        io.out, io.quantiles_out = abi.ptr(out), abi.ptr(pool)
        self._call("target_host", C.byref(self._cfg), C.byref(w), C.byref(io), n, nt)
        return (out, pool) if return_quantiles else out

    # ------------------------------------------------------------ the critic update
    def _like_online(self, device=None) -> Tuple[List["torch.Tensor"], List["torch.Tensor"]]:
        dev = self.device if device is None else device
        return ([torch.zeros_like(t, device=dev) for t in self._ws["online"]],
                [torch.zeros_like(t, device=dev) for t in self._bs["online"]])

    def _named(self, ws, bs) -> Dict[str, Any]:
        out = {}
        for name, w, b in zip(self._names, ws, bs):
            out[f"{name}.weight"], out[f"{name}.bias"] = w, b
        return out

    def _unnamed(self, d: Dict[str, Any], what: str):
        """``d`` (SB3 key names) as numpy weight and bias lists in ``_names`` order, every shape checked."""
        ws, bs = [], []
        for name, w, b in zip(self._names, self._ws["online"], self._bs["online"]):
            for key, cur, dst in ((f"{name}.weight", w, ws), (f"{name}.bias", b, bs)):
                if key not in d:
                    raise KeyError(f"{what}: missing key {key!r}")
                v = d[key]
                x = np.array(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float32, order="C")
                if x.shape != tuple(cur.shape):
                    raise ValueError(f"{what}: {key!r} has shape {x.shape}, expected {tuple(cur.shape)}")
                dst.append(x)
        return ws, bs

    def init_optimizer(self, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8) -> None:
        """``torch.optim.Adam(critic.parameters(), betas=, eps=)`` as SB3 builds it (no weight decay, no
        amsgrad): allocates the handle's gradient buffer, ``exp_avg``, ``exp_avg_sq``, the step word and the
        packing the backward reads; called again, zeroes the state.  Not a launch: call it before a capture."""
        b1, b2, e = float(betas[0]), float(betas[1]), float(eps)
        if self._h is not None:
            self._call("init_training", self._h, C.c_double(b1), C.c_double(b2), C.c_double(e))
        else:
            self.adam_step_host(0.0, self._named(*self._like_online()), betas=(b1, b2), eps=e)   # the library's checks
            zeros = lambda: self._named(*[[t.numpy() for t in x] for x in self._like_online()])  # noqa: E731
            self._cpu_state = {"exp_avg": zeros(), "exp_avg_sq": zeros(), "step": 0}
        self._opt = (b1, b2, e)

    def workspace_floats(self, batch: int) -> int:
        n = int(self.lib.pgx_qc_grad_workspace_floats(C.byref(self._cfg), int(batch)))
        if n < 0:
            check(n, "pgx_qc_grad_workspace_floats", self.lib)
        return n

    def alloc_workspace(self, max_batch: int) -> "torch.Tensor":
        """The workspace ``critic_loss_backward`` of up to ``max_batch`` rows needs (every row's activations
        and pre-activation gradients: the handle keeps no batch-sized storage), an f32 device tensor; and
        ``init_optimizer()`` with its defaults where that was not called."""
        self._need_device()
        if self._opt is None:
            self.init_optimizer()
        return torch.empty(self.workspace_floats(max_batch), dtype=torch.float32, device=self.device)

    def alloc_grad_debug(self, batch: int) -> Dict[str, "torch.Tensor"]:
        """Debug planes for ``critic_loss_backward(..., debug=)`` of ``batch`` rows: ``quantiles`` and ``dq``
        [B, n_critics * n_quantiles], ``dz`` [B, n_critics * sum(net_arch)] (critic-major, then layer)."""
        z = lambda w: torch.zeros((int(batch), w), dtype=torch.float32, device=self.device)  # noqa: E731
        return {"quantiles": z(self.n_pool), "dq": z(self.n_pool), "dz": z(self.n_critics * sum(self.net_arch))}

    def critic_loss_backward(self, obs: Dict[str, Any], actions, target_quantiles, workspace, loss=None,
                             debug: Optional[Dict[str, "torch.Tensor"]] = None) -> "torch.Tensor":
        """``critic_loss = quantile_huber_loss(critic(obs, actions), target_quantiles,
        sum_over_quantiles=False)`` and ``critic_loss.backward()`` into the handle's gradient buffer (replaced,
        never accumulated: ``zero_grad`` is implied): two launches.  ``target_quantiles``: a contiguous f32
        device tensor [B, n_target] (``td_target``'s result; any ``n_target`` in 1..n_critics * n_quantiles).
        ``workspace``: ``alloc_workspace``'s tensor.  Returns the loss, a device scalar (``loss``: a
        one-float f32 device tensor to fill instead of a new one)."""
        self._need_device()
        io = abi.PgxQcGradIo()
        B, keep = self._rows_into(io, obs, actions)
        what = f"target_quantiles must be a contiguous f32 [>= {B}, n_target] tensor on {self.device}"
        if target_quantiles is None:   # (an input: there is no new one to make)
            raise ValueError(what)
        tq = self._f32_out(target_quantiles, B, (None,), what)
        ws = workspace
        if not torch.is_tensor(ws) or ws.dtype != torch.float32 or ws.device != self.device or not ws.is_contiguous():
            raise ValueError(f"workspace must be a contiguous f32 tensor on {self.device} (alloc_workspace)")
        if loss is None:
            loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        elif not torch.is_tensor(loss) or loss.dtype != torch.float32 or loss.device != self.device or loss.numel() != 1:
            raise ValueError(f"loss must be a one-float f32 tensor on {self.device}")
        io.target_quantiles, io.workspace, io.loss = tq.data_ptr(), ws.data_ptr(), loss.data_ptr()
        io.workspace_floats = ws.numel()
        if debug is not None:
            for k in ("quantiles", "dq", "dz"):
                if debug[k].shape[0] < B or not debug[k].is_contiguous():
                    raise ValueError(f"the debug planes hold {debug[k].shape[0]} rows, the batch {B}")
                setattr(io, f"{k}_out", debug[k].data_ptr())
        check(self.lib.pgx_qc_critic_grad(self._h, C.byref(io), B, int(tq.shape[1]), self._stream()),
              "pgx_qc_critic_grad", self.lib)
        self._keep = keep + [tq, ws, loss, debug]
        return loss.view(())

    def critic_loss_backward_rows(self, batch: Dict[str, "torch.Tensor"], target_quantiles, workspace, loss=None,
                                  debug=None) -> "torch.Tensor":
        """``critic_loss_backward`` on a HER batch (``buf.alloc_batch`` / ``buf.sample_into``): ``obs``,
        ``achieved_goal``, ``desired_goal`` and ``action`` are read from ``batch["rows"]`` in place."""
        return self.critic_loss_backward(self._batch_obs(batch, False), batch["action"], target_quantiles, workspace,
                                         loss=loss, debug=debug)

    def grads(self) -> Dict[str, "torch.Tensor"]:
        """The gradient buffer as the last ``critic_loss_backward`` left it, under sb3_contrib's key names
        ``qf{i}.{0,2,4}.weight|bias`` (copies)."""
        self._need_device()
        ws, bs = self._like_online()
        w = self._weights_struct(ws, bs)
        self._call("get_grads", self._h, C.byref(w), self._stream())
        return self._named(ws, bs)

    def adam_step(self, lr) -> None:
        """``critic.optimizer.step()``: one Adam step on the online set from the gradient buffer, then its
        packing, on the current stream.  ``lr``: a one-float f32 device tensor, read at every launch (a
        replayed graph sees its current value: a schedule writes it), or a number."""
        self._need_device()
        t = lr if torch.is_tensor(lr) else torch.as_tensor(float(lr))
        if t.numel() != 1:
            raise ValueError("lr must hold one float")
        t = t.detach().to(device=self.device, dtype=torch.float32).reshape(1)
        self._call("adam_step", self._h, t.data_ptr(), self._stream())
        self._keep_lr = t
        self._stale_online = True

    def optimizer_state_dict(self) -> Dict[str, Any]:
        """``exp_avg`` and ``exp_avg_sq`` (each under the parameters' key names, copies), ``step``, ``betas``
        and ``eps``.  On a CPU device: the state this object holds (``load_optimizer_state_dict``'s)."""
        if self._opt is None:
            raise PgxError("no optimiser state: call init_optimizer first")
        if self._h is None:
            st = self._cpu_state
            return {"exp_avg": {k: torch.as_tensor(x.copy()) for k, x in st["exp_avg"].items()},
                    "exp_avg_sq": {k: torch.as_tensor(x.copy()) for k, x in st["exp_avg_sq"].items()},
                    "step": st["step"], "betas": self._opt[:2], "eps": self._opt[2]}
        m, v = self._like_online(), self._like_online()
        sm, sv = self._weights_struct(*m), self._weights_struct(*v)
        step = C.c_uint64(0)
        self._call("get_opt_state", self._h, C.byref(sm), C.byref(sv), C.byref(step), self._stream())
        return {"exp_avg": self._named(*m), "exp_avg_sq": self._named(*v), "step": int(step.value),
                "betas": self._opt[:2], "eps": self._opt[2]}

    def load_optimizer_state_dict(self, sd: Dict[str, Any]) -> None:
        """What ``optimizer_state_dict`` returned (``betas`` / ``eps`` are not read: ``init_optimizer`` sets
        them).  Every key and shape is validated before anything is written: a failed load changes nothing."""
        if self._opt is None:
            raise PgxError("no optimiser state: call init_optimizer first")
        step = int(sd["step"])
        if step < 0:
            raise ValueError("step must be >= 0")
        m = self._unnamed(sd["exp_avg"], "load_optimizer_state_dict: exp_avg")
        v = self._unnamed(sd["exp_avg_sq"], "load_optimizer_state_dict: exp_avg_sq")
        if self._h is None:
            self._cpu_state = {"exp_avg": self._named(*m), "exp_avg_sq": self._named(*v), "step": step}
            return
        sm, sv = self._weights_struct(*m), self._weights_struct(*v)
        self._call("set_opt_state", self._h, C.byref(sm), C.byref(sv), C.c_uint64(step), self._stream())
        torch.cuda.synchronize(self.device)   # (the copies read the numpy arrays above)

    def critic_grad_host(self, obs: Dict[str, Any], actions, target_quantiles, return_debug: bool = False):
        """``(loss, grads)`` -- a numpy f32 scalar and numpy arrays under the parameters' key names -- from the
        library's host model of ``critic_loss_backward`` on the online set; ``return_debug``: also the
        ``quantiles`` / ``dq`` / ``dz`` planes.  A test oracle."""
        io = abi.PgxQcGradIo()
        n, keep = self._host_rows_into(io, obs, actions)
        tq = np.ascontiguousarray(target_quantiles.detach().cpu().numpy() if torch.is_tensor(target_quantiles)
                                  else target_quantiles, dtype=np.float32)
        if tq.ndim != 2 or tq.shape[0] != n:
            raise ValueError(f"target_quantiles must be [{n}, n_target]")
        w, keep_w = self._host_set("online")
        ws = np.zeros(max(self.workspace_floats(n), 1), np.float32)
        loss = np.zeros(1, np.float32)
        dbg = {"quantiles": np.zeros((n, self.n_pool), np.float32), "dq": np.zeros((n, self.n_pool), np.float32),
               "dz": np.zeros((n, self.n_critics * sum(self.net_arch)), np.float32)}
        io.target_quantiles, io.workspace, io.loss, io.workspace_floats = abi.ptr(tq), abi.ptr(ws), abi.ptr(loss), ws.size
        io.quantiles_out, io.dq_out, io.dz_out = abi.ptr(dbg["quantiles"]), abi.ptr(dbg["dq"]), abi.ptr(dbg["dz"])
        gw = [np.zeros(tuple(t.shape), np.float32) for t in self._ws["online"]]
        gb = [np.zeros(tuple(t.shape), np.float32) for t in self._bs["online"]]
        g = self._weights_struct(gw, gb)
        self._call("critic_grad_host", C.byref(self._cfg), C.byref(w), C.byref(io), n, int(tq.shape[1]), C.byref(g))
        out = (loss[0], self._named(gw, gb))
        return out + (dbg,) if return_debug else out

    def adam_step_host(self, lr: float, grads: Dict[str, Any], params: Optional[Dict[str, Any]] = None,
                       state: Optional[Dict[str, Any]] = None, betas: Optional[Tuple[float, float]] = None,
                       eps: Optional[float] = None):
        """One Adam step by the library's host model, on copies: ``(params, state)`` after the step, from
        ``params`` (default: the online set) and ``state`` (``exp_avg`` / ``exp_avg_sq`` / ``step`` as
        ``optimizer_state_dict`` names them; default: zeros, step 0).  Nothing of this object changes.  A
        test oracle."""
        b1, b2, e = self._opt or (0.9, 0.999, 1e-8)
        if betas is not None:
            b1, b2 = float(betas[0]), float(betas[1])
        if eps is not None:
            e = float(eps)
        p = self._unnamed(self.state_dict("online") if params is None else params, "adam_step_host: params")
        g = self._unnamed(grads, "adam_step_host: grads")
        zeros = self._named(*self._like_online("cpu"))
        m = self._unnamed(zeros if state is None else state["exp_avg"], "adam_step_host: exp_avg")
        v = self._unnamed(zeros if state is None else state["exp_avg_sq"], "adam_step_host: exp_avg_sq")
        step = C.c_uint64(0 if state is None else int(state["step"]))
        structs = [self._weights_struct(*a) for a in (p, g, m, v)]
        self._call("adam_step_host", C.byref(self._cfg), *[C.byref(x) for x in structs], C.byref(step), C.c_double(float(lr)),
                   C.c_double(b1), C.c_double(b2), C.c_double(e))
        return self._named(*p), {"exp_avg": self._named(*m), "exp_avg_sq": self._named(*v), "step": int(step.value)}
