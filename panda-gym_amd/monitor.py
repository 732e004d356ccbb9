"""Device-resident VecMonitor: stable-baselines3's episode statistics over a ``PandaVecEnv``.

SB3's ``make_vec_env`` wraps every env in ``Monitor`` (the reference builds its training envs with
it, training/utils/setup_training.py:43-47), whose ``infos[i]["episode"] = {"r", "l", "t"}`` feed
``rollout/ep_rew_mean``, ``ep_len_mean`` and ``success_rate``; the reference's evaluation
(evaluation/evaluate.py:88-317 ``perform_benchmark``) scores a policy by mean episode reward,
success / collision / timeout rate, mean episode length and mean end-effector speed.  Here the
returns, lengths, outcomes, a ring of the newest ``window`` episodes and the running totals live on
the device (libpgx.so, pgx_monitor.hip; C-ABI in include/pgx.h, section "VecMonitor"): a monitored
step is the env's launches plus two more on the same stream, so it captures into a HIP graph
(``capture_steps``) and never leaves HBM (``step_tensors``).  No CPU fallback.

``EpisodeMonitor`` is the low-level binding (one handle, raw device tensors in); ``VecMonitor``
wraps an env, or a ``VecNormalize``, with it; ``evaluate`` runs a policy for an episode quota and
returns ``perform_benchmark``'s result keys.
"""
from __future__ import annotations

import ctypes as C
import inspect
import time
from typing import Any, Callable, Dict, Optional, Sequence

import numpy as np

from . import abi
from ._handle import Handle, torch
from ._native import check, load
from .normalize import VecNormalize

TOTALS_INT = ("episodes", "length_sum", "length_sum_success", "steps", "envs_open")
STATS_LAYOUT = ("episodes", "successes", "return_sum", "length_sum")   # stats_vector(), shard.gather_stats


def safe_mean(x) -> float:
    """SB3's ``safe_mean``: nan for no episodes."""
    return float("nan") if len(x) == 0 else float(np.mean(x))


def _ratio(a, b) -> float:
    return float("nan") if b == 0 else float(a) / float(b)


def combine(rows) -> Dict[str, float]:
    """One result from gathered ``stats_vector()`` rows ``[W, 4]`` (``shard.gather_stats``), or one
    row: the sums over workers and the means they give."""
    a = np.asarray(rows, dtype=np.float64).reshape(-1, len(STATS_LAYOUT)).sum(axis=0)
    ep, succ, ret, length = (float(x) for x in a)
    return {"episodes": int(ep), "successes": int(succ), "return_sum": ret, "length_sum": int(length),
            "ep_rew_mean": _ratio(ret, ep), "ep_len_mean": _ratio(length, ep), "success_rate": _ratio(succ, ep)}


def evaluation_result(totals: Dict[str, Any], episodes: Dict[str, np.ndarray], n_substeps: int) -> Dict[str, float]:
    """``perform_benchmark``'s result keys (evaluate.py:286-299) from a monitor's totals and retained
    records, rounded to 4 places as there.  Rates are over all episodes; means leave the
    non-finite episodes out (they are in no sum); ``std_reward`` is numpy's over the retained
    finite returns; ``mean_ee_speed`` is over every step of the successful episodes.  A mean over
    no episodes is nan, as ``np.mean([])``."""
    n = int(totals["episodes"])
    oc = [int(x) for x in totals["outcomes"]]
    fin = n - oc[abi.EP_NONFINITE]
    r = np.asarray(episodes["r"], dtype=np.float64)[np.asarray(episodes["outcome"]) != abi.EP_NONFINITE]
    rnd = lambda x: float(np.round(x, 4))  # noqa: E731
    return {
        "mean_reward": rnd(_ratio(totals["return_sum"], fin)),
        "std_reward": rnd(np.std(r)) if len(r) else float("nan"),
        "success_rate": rnd(_ratio(oc[abi.EP_SUCCESS], n)),
        "collision_rate": rnd(_ratio(oc[abi.EP_COLLISION], n)),
        "timeout_rate": rnd(_ratio(oc[abi.EP_TIMEOUT], n)),
        "nonfinite_rate": rnd(_ratio(oc[abi.EP_NONFINITE], n)),
        "num_episodes": n,
        "mean_ep_length": rnd(_ratio(totals["length_sum"], fin)),
        "mean_ep_length_success": rnd(_ratio(totals["length_sum_success"], oc[abi.EP_SUCCESS])),
        "mean_num_sim_steps": rnd(_ratio(int(totals["length_sum"]) * int(n_substeps), fin)),
        "mean_num_sim_steps_success": rnd(_ratio(int(totals["length_sum_success"]) * int(n_substeps),
                                                 oc[abi.EP_SUCCESS])),
        "mean_ee_speed": rnd(_ratio(totals["speed_sum_success"], totals["length_sum_success"])),
    }


def episode_count_targets(n_eval_episodes: int, n_envs: int) -> np.ndarray:
    """SB3 ``evaluate_policy``'s per-env quota: ``[(n_eval_episodes + i) // n_envs for i in range(n_envs)]``."""
    return np.array([(int(n_eval_episodes) + i) // int(n_envs) for i in range(int(n_envs))], dtype=np.int32)


class EpisodeMonitor(Handle):
    """One pgx_monitor handle for ``n_envs`` envs on ``device``: per-env return / length / speed
    accumulators, the ring of the newest ``window`` finished episodes, totals and quota."""

    _PREFIX = "pgx_monitor"

    def __init__(self, n_envs: int, obs_dim: int, window: int = 100, speed_col: int = 3, device: Any = "cuda:0",
                 lib=None):
        self._need_torch()
        self.lib = lib or load()
        self._on_device(device)
        self.n_envs, self.obs_dim, self.window, self.speed_col = int(n_envs), int(obs_dim), int(window), int(speed_col)
        self._create(abi.PgxMonitorConfig(self.n_envs, self.obs_dim, self.window, self.speed_col))

    # ------------------------------------------------------------ launches
    def step(self, io: abi.PgxMonitorIo) -> None:
        """pgx_monitor_step over the device buffers ``io`` names (two launches, no allocation)."""
        check(self.lib.pgx_monitor_step(self._h, C.byref(io), self._stream()), "pgx_monitor_step", self.lib)

    def reset(self, mask: Optional["torch.Tensor"] = None) -> None:
        """Abandon the running episodes of the envs in ``mask`` (a device tensor [N]; None: all)."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if tuple(m.shape) != (self.n_envs,):
                raise ValueError(f"mask must have shape ({self.n_envs},), got {tuple(m.shape)}")
        self._call("reset", self._h, None if m is None else C.c_void_p(m.data_ptr()), self._stream())
        self._keep_mask = m   # read by the queued launch

    def clear(self) -> None:
        """Back to the state after construction (the targets stay)."""
        self._call("clear", self._h, self._stream())

    def set_targets(self, targets: Optional[Sequence[int]]) -> None:
        """Per-env episode quota (None: none): an env that has reached it is no longer recorded."""
        t = None
        if targets is not None:
            t = np.ascontiguousarray(targets, dtype=np.int32)
            if t.shape != (self.n_envs,):
                raise ValueError(f"targets must have shape ({self.n_envs},), got {t.shape}")
        self._call("set_targets", self._h, abi.ptr(t), self._stream())

    # ------------------------------------------------------------- read-out
    def totals(self) -> Dict[str, Any]:
        """pgx_monitor_totals as a dict (``outcomes``: a list by ``abi.EP_*``).  Synchronises."""
        t = abi.PgxMonitorTotals()
        self._call("get_totals", self._h, C.byref(t), self._stream())
        out: Dict[str, Any] = {k: int(getattr(t, k)) for k in TOTALS_INT}
        out["outcomes"] = [int(x) for x in t.outcomes]
        out["return_sum"], out["speed_sum_success"] = float(t.return_sum), float(t.speed_sum_success)
        return out

    def episodes(self, max_records: Optional[int] = None) -> Dict[str, np.ndarray]:
        """The retained records, oldest first: ``r`` f32, ``l``, ``env``, ``outcome`` i32, ``step`` i64,
        ``speed_sum`` f64 (``max_records``: the newest so many).  Synchronises."""
        m = self.window if max_records is None else int(max_records)
        a = {"r": np.zeros(m, np.float32), "l": np.zeros(m, np.int32), "env": np.zeros(m, np.int32),
             "outcome": np.zeros(m, np.int32), "step": np.zeros(m, np.int64), "speed_sum": np.zeros(m, np.float64)}
        n = C.c_int32(0)
        self._call("read", self._h, m, *[abi.ptr(a[k]) for k in ("r", "l", "env", "outcome", "step", "speed_sum")],
                   C.byref(n), self._stream())
        return {k: v[:n.value].copy() for k, v in a.items()}

    def env_state(self) -> Dict[str, np.ndarray]:
        """The per-env accumulators ``ret`` f32, ``len`` i32, ``speed`` f64 and ``ep_count`` i32."""
        n = self.n_envs
        a = {"ret": np.zeros(n, np.float32), "len": np.zeros(n, np.int32), "speed": np.zeros(n, np.float64),
             "ep_count": np.zeros(n, np.int32)}
        self._call("get_env_state", self._h, *[abi.ptr(a[k]) for k in ("ret", "len", "speed", "ep_count")],
                   self._stream())
        return a

    # ------------------------------------------- array-level step (tests, tools)
    def step_arrays(self, reward, success, terminated, truncated, obs=None, terminal_obs=None, task_truncated=None,
                    nonfinite=None):
        """One pgx_monitor_step over host or device arrays (copied to fresh device buffers): returns
        the device tensors (ep_r f32 [N], ep_l i32 [N]), valid where terminated | truncated."""
        n, od, f, u8 = self.n_envs, self.obs_dim, torch.float32, torch.uint8
        opt = lambda x, s, t: None if x is None else self._dev(x, s, t)  # noqa: E731
        t = [self._dev(reward, (n,), f), self._dev(success, (n,), u8), self._dev(terminated, (n,), u8),
             self._dev(truncated, (n,), u8), opt(obs, (n, od), f), opt(terminal_obs, (n, od), f),
             opt(task_truncated, (n,), u8), opt(nonfinite, (n,), u8)]
        ep_r = torch.zeros(n, dtype=f, device=self.device)
        ep_l = torch.zeros(n, dtype=torch.int32, device=self.device)
        io = abi.PgxMonitorIo(*[None if x is None else x.data_ptr() for x in t], ep_r.data_ptr(), ep_l.data_ptr())
        self.step(io)
        self._keep = t
        return ep_r, ep_l

    def reset_arrays(self, mask=None) -> None:
        self.reset(None if mask is None else self._dev(mask, (self.n_envs,), torch.uint8))


class VecMonitor:
    """SB3 ``VecMonitor`` over a ``PandaVecEnv`` or a ``VecNormalize``, on the device; the outermost
    wrapper.  It reads the raw step buffers of the base env whatever it wraps (SB3 with ``Monitor``
    inside ``VecNormalize`` records raw returns) and returns what the wrapped object returns.

    ``step_tensors`` / ``reset_tensors`` / ``capture_steps`` are the device path; ``reset`` /
    ``step_async`` / ``step_wait`` / ``step`` the SB3 path, where a finished env's info gains
    ``"episode": {"r", "l", "t"}`` (and the ``info_keywords`` of its info), as with SB3's wrapper.
    Every other attribute forwards to the wrapped object.  ``window`` is SB3's
    ``stats_window_size``: the episodes ``episodes()`` and ``window_stats()`` see."""

    def __init__(self, venv, window: int = 100, info_keywords: Sequence[str] = ()):
        base = venv.venv if isinstance(venv, VecNormalize) else venv
        if not getattr(base, "auto_reset", True):
            raise ValueError("VecMonitor needs an env with auto_reset=True: an env that keeps its terminal state "
                             "reports the same finished episode at every step")
        self.venv, self._base = venv, base
        self.info_keywords = tuple(info_keywords)
        self.t_start = time.time()
        self._mon = EpisodeMonitor(base.num_envs, base.obs_dim, window=window, device=base.device, lib=base.lib)
        n = base.num_envs
        # ep_r f32 [N] and ep_l i32 [N] in one buffer: the SB3 path fetches both with one copy
        self._ep = torch.zeros(8 * n, dtype=torch.uint8, device=base.device)
        self.ep_r, self.ep_l = self._ep[:4 * n].view(torch.float32), self._ep[4 * n:].view(torch.int32)
        p = lambda t: t.data_ptr()  # noqa: E731
        self._io = abi.PgxMonitorIo(p(base.reward), p(base.success), p(base.terminated), p(base.truncated),
                                    p(base.obs), p(base.terminal_obs), p(base.task_trunc), p(base.nonfinite_t),
                                    p(self.ep_r), p(self.ep_l))
        self._h_ep = None

    # ------------------------------------------------------------ plumbing
    def __getattr__(self, name: str):
        if name in ("venv", "_base", "_mon"):   # (not set yet: no recursion)
            raise AttributeError(name)
        return getattr(self.venv, name)

    def close(self) -> None:
        if getattr(self, "_mon", None) is not None:
            self._mon.close()
        self.venv.close()

    def _enqueue_monitor(self) -> None:
        self._mon.step(self._io)

    # ---------------------------------------------------------- device path
    def reset_tensors(self, seed: Optional[int] = None, mask: Optional["torch.Tensor"] = None, **kwargs):
        """The wrapped ``reset_tensors`` plus VecMonitor.reset for the same envs: their running
        episodes are abandoned, not recorded."""
        if mask is not None:
            kwargs["mask"] = mask
        out = self.venv.reset_tensors(seed=seed, **kwargs)
        self._mon.reset(mask)
        return out

    def step_tensors(self, actions: "torch.Tensor"):
        """The wrapped ``step_tensors`` with the monitor's two launches behind it; returns what the
        wrapped object returns.  ``ep_r`` / ``ep_l`` hold the finished envs' return and length."""
        out = self.venv.step_tensors(actions)
        self._mon.step(self._io)
        return out

    def _enqueue_step(self, a: "torch.Tensor", what: str = "pgx_step") -> None:
        """The wrapped object's step launches and the monitor's two, on the current stream (what
        ``Actor.capture_rollout`` enqueues per step)."""
        self.venv._enqueue_step(a, what)
        self._enqueue_monitor()

    def capture_steps(self, k: int, actions: Optional["torch.Tensor"] = None, after_step=None):
        """The wrapped ``capture_steps`` with the monitor's launches behind every captured step.  The
        ring head, the step counter and the totals' parity are device words: any number of replays
        records what the same steps run eagerly record.  ``after_step``: a further callable that
        enqueues behind the monitor's launches (``RolloutBuffer.after_step``)."""
        if after_step is None:
            return self.venv.capture_steps(k, actions, after_step=self._enqueue_monitor)

        def both() -> None:
            self._enqueue_monitor()
            after_step()

        return self.venv.capture_steps(k, actions, after_step=both)

    # ------------------------------------------------------------- SB3 path
    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        out = self.venv.reset(seed=seed, options=options)
        self._mon.reset(None)
        return out

    def step_async(self, actions) -> None:
        self.venv.step_async(actions)

    def _sb3_pre_sync(self) -> None:
        self._mon.step(self._io)
        self._h_ep.copy_(self._ep, non_blocking=True)

    def step_wait(self):
        """The wrapped ``step_wait``; ``infos[i]["episode"] = {"r", "l", "t"}`` for the envs that
        finished (``t``: seconds since construction), every other key as the wrapped object reports
        it.  The monitor's launches and one more pinned copy go ahead of the step's single sync."""
        if self._h_ep is None:
            self._h_ep = torch.empty(self._ep.numel(), dtype=torch.uint8, pin_memory=True)
        self._base._pre_sync = self._sb3_pre_sync
        try:
            o, r, d, infos = self.venv.step_wait()
        finally:
            self._base._pre_sync = None
        idx = np.flatnonzero(d)
        if len(idx):
            n = self._base.num_envs
            ep_r = self._h_ep[:4 * n].view(torch.float32).numpy()
            ep_l = self._h_ep[4 * n:].view(torch.int32).numpy()
            t = round(time.time() - self.t_start, 6)
            for i in idx.tolist():
                ep = {"r": float(ep_r[i]), "l": int(ep_l[i]), "t": t}
                for k in self.info_keywords:
                    ep[k] = infos[i][k]
                infos[i]["episode"] = ep
        return o, r, d, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # ------------------------------------------------------------- read-out
    def totals(self) -> Dict[str, Any]:
        return self._mon.totals()

    def episodes(self, max_records: Optional[int] = None) -> Dict[str, np.ndarray]:
        return self._mon.episodes(max_records)

    def env_state(self) -> Dict[str, np.ndarray]:
        return self._mon.env_state()

    def set_targets(self, targets: Optional[Sequence[int]]) -> None:
        self._mon.set_targets(targets)

    def clear(self) -> None:
        self._mon.clear()

    def window_stats(self) -> Dict[str, float]:
        """SB3's logged ``safe_mean``s over the retained records: ``ep_rew_mean``, ``ep_len_mean``,
        ``success_rate``."""
        ep = self._mon.episodes()
        return {"ep_rew_mean": safe_mean(ep["r"].astype(np.float64)), "ep_len_mean": safe_mean(ep["l"]),
                "success_rate": safe_mean(ep["outcome"] == abi.EP_SUCCESS)}

    def stats_vector(self) -> np.ndarray:
        """``[episodes, successes, return_sum, length_sum]`` fp64, the row ``shard.gather_stats``
        gathers (``combine`` turns the gathered rows into one result).  ``episodes`` counts the
        episodes the two sums are over: the non-finite ones are left out."""
        t = self._mon.totals()
        return np.array([t["episodes"] - t["outcomes"][abi.EP_NONFINITE], t["outcomes"][abi.EP_SUCCESS],
                         t["return_sum"], t["length_sum"]], dtype=np.float64)

    combine = staticmethod(combine)


def evaluate(venv, policy: Callable, n_eval_episodes: int, deterministic: bool = True, poll: int = 8,
             return_episodes: bool = False):
    """Run ``policy`` (an observation dict of device tensors -> an action tensor [N, A]; called
    with ``deterministic=`` where it takes that keyword) on ``venv`` until ``n_eval_episodes``
    episodes are recorded, split over the envs as SB3's ``evaluate_policy`` splits them, and return
    ``perform_benchmark``'s result keys (``evaluation_result``); with ``return_episodes`` also the
    recorded episodes (``EpisodeMonitor.episodes``).  Steps on the tensor path; the host looks at
    ``envs_open`` every ``poll`` steps.  Effort, manipulability and jerk are not computed by the
    kernels and are not reported."""
    vm = VecMonitor(venv, window=int(n_eval_episodes))
    try:
        vm.set_targets(episode_count_targets(n_eval_episodes, vm.num_envs))
        try:
            takes = "deterministic" in inspect.signature(policy).parameters
        except (TypeError, ValueError):
            takes = False
        act = (lambda o: policy(o, deterministic=deterministic)) if takes else policy
        obs = vm.reset_tensors()
        while vm.totals()["envs_open"] > 0:
            for _ in range(max(1, int(poll))):
                obs = vm.step_tensors(act(obs))[0]
        episodes = vm.episodes()
        res = evaluation_result(vm.totals(), episodes, int(vm._base._params.n_substeps))
        return (res, episodes) if return_episodes else res
    finally:
        vm._mon.close()
