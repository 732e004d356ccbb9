"""The VecMonitor C-ABI (include/pgx.h, pgx_monitor_*) without a GPU: the ctypes mirrors against the
header's layout through gcc, the exported entry points, pgx_monitor_create's argument checks (made
before any device call), the host arithmetic of ``combine`` / ``evaluation_result`` on hand-made
records, and the numpy restatement of SB3's VecMonitor the GPU tests compare against (RefMonitor,
written from the rules of include/pgx.h, pinned here on a trace small enough to follow by hand)."""
import collections
import ctypes as C
import math
import os

import numpy as np
import pytest

from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64

MONITOR_EXPORTS = ["pgx_monitor_create", "pgx_monitor_destroy", "pgx_monitor_step", "pgx_monitor_reset",
                   "pgx_monitor_clear", "pgx_monitor_set_targets", "pgx_monitor_get_totals", "pgx_monitor_read",
                   "pgx_monitor_get_env_state"]
TIMEOUT, SUCCESS, COLLISION, NONFINITE = 0, 1, 2, 3


# ---------------------------------------------------------------- the restatement
class RefMonitor:
    """SB3 VecMonitor (f32 returns, int lengths, a loop over the done envs in ascending env id), the
    ring as ``deque(maxlen=window)``, the outcome classification, the totals and the episode quota, in
    numpy, from include/pgx.h's rules.  Sums run in plain env-then-step order; ``abs_return`` /
    ``abs_speed`` / ``summed`` carry what the fp64 bound of the GPU tests needs."""

    def __init__(self, n, window, speed_col=3, targets=None):
        self.n, self.speed_col = n, speed_col
        self.ret, self.len = np.zeros(n, F32), np.zeros(n, np.int32)
        self.speed, self.ep_count = np.zeros(n, F64), np.zeros(n, np.int32)
        self.targets = None if targets is None else np.asarray(targets, np.int64)
        self.ring = collections.deque(maxlen=window)
        self.tot = {"episodes": 0, "outcomes": [0, 0, 0, 0], "length_sum": 0, "length_sum_success": 0, "steps": 0,
                    "envs_open": self._open(), "return_sum": 0.0, "speed_sum_success": 0.0}
        self.abs_return, self.abs_speed, self.summed, self.summed_success = 0.0, 0.0, 0, 0

    def _open(self):
        return self.n if self.targets is None else int((self.ep_count < self.targets).sum())

    def set_targets(self, targets):
        self.targets = None if targets is None else np.asarray(targets, np.int64)
        self.tot["envs_open"] = self._open()

    def reset(self, mask=None):
        m = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.ret[m], self.len[m], self.speed[m] = 0, 0, 0

    def step(self, reward, success, terminated, truncated, obs=None, terminal_obs=None, task_truncated=None,
             nonfinite=None):
        n, t = self.n, self.tot
        z = np.zeros(n, np.uint8)
        task_truncated = z if task_truncated is None else task_truncated
        nonfinite = z if nonfinite is None else nonfinite
        done = (np.asarray(terminated) != 0) | (np.asarray(truncated) != 0)
        with np.errstate(invalid="ignore"):
            self.ret = self.ret + np.asarray(reward, F32)   # one f32 add
        assert self.ret.dtype == F32
        self.len += 1
        if self.speed_col >= 0:
            c = self.speed_col
            v = np.where(done[:, None], terminal_obs, obs)[:, c:c + 3].astype(F64)
            x, y, zc = v[:, 0], v[:, 1], v[:, 2]
            self.speed = self.speed + np.sqrt(x * x + y * y + zc * zc)
        t["steps"] += 1
        ep_r, ep_l = np.zeros(n, F32), np.zeros(n, np.int32)
        for i in np.flatnonzero(done).tolist():   # SB3: for i in range(len(dones)): if dones[i]
            ep_r[i], ep_l[i] = self.ret[i], self.len[i]
            if self.targets is None or self.ep_count[i] < self.targets[i]:
                if nonfinite[i] or not np.isfinite(self.ret[i]):
                    oc = NONFINITE
                elif success[i]:
                    oc = SUCCESS
                elif task_truncated[i]:
                    oc = COLLISION
                else:
                    oc = TIMEOUT
                self.ring.append((self.ret[i], int(self.len[i]), i, oc, t["steps"], float(self.speed[i])))
                t["episodes"] += 1
                t["outcomes"][oc] += 1
                if oc != NONFINITE:
                    t["length_sum"] += int(self.len[i])
                    t["return_sum"] += float(self.ret[i])
                    self.abs_return += abs(float(self.ret[i]))
                    self.summed += 1
                    if oc == SUCCESS:
                        t["length_sum_success"] += int(self.len[i])
                        t["speed_sum_success"] += float(self.speed[i])
                        self.abs_speed += abs(float(self.speed[i]))
                        self.summed_success += 1
                self.ep_count[i] += 1
            self.ret[i], self.len[i], self.speed[i] = 0, 0, 0
        t["envs_open"] = self._open()
        return ep_r, ep_l, done

    def episodes(self):
        cols = list(zip(*self.ring)) if self.ring else [[]] * 6
        return {"r": np.array(cols[0], F32), "l": np.array(cols[1], np.int32), "env": np.array(cols[2], np.int32),
                "outcome": np.array(cols[3], np.int32), "step": np.array(cols[4], np.int64),
                "speed_sum": np.array(cols[5], F64)}


def ref_evaluation(ring, n_substeps):
    """perform_benchmark's result arithmetic (evaluate.py:286-299) over a list of finished episodes
    (r, l, env, outcome, step, speed_sum), as the reference computes it from its per-episode lists;
    non-finite episodes count in the rates and in num_episodes only."""
    fin = [e for e in ring if e[3] != NONFINITE]
    succ = [e for e in ring if e[3] == SUCCESS]
    n = len(ring)
    mean = lambda x: float(np.mean(x)) if len(x) else float("nan")  # noqa: E731
    speed = sum(e[5] for e in succ) / sum(e[1] for e in succ) if succ else float("nan")
    res = {"mean_reward": mean([float(e[0]) for e in fin]), "std_reward": float(np.std([float(e[0]) for e in fin])),
           "success_rate": len(succ) / n, "collision_rate": sum(e[3] == COLLISION for e in ring) / n,
           "timeout_rate": sum(e[3] == TIMEOUT for e in ring) / n,
           "nonfinite_rate": sum(e[3] == NONFINITE for e in ring) / n,
           "mean_ep_length": mean([e[1] for e in fin]), "mean_ep_length_success": mean([e[1] for e in succ]),
           "mean_num_sim_steps": mean([e[1] * n_substeps for e in fin]),
           "mean_num_sim_steps_success": mean([e[1] * n_substeps for e in succ]), "mean_ee_speed": speed}
    res = {k: float(np.round(v, 4)) for k, v in res.items()}
    res["num_episodes"] = n
    return res


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    """ctypes mirrors of pgx_monitor_config / _io / _totals == the header's sizeof / offsetof (gcc, as C)."""
    structs = {"pgx_monitor_config": abi.PgxMonitorConfig, "pgx_monitor_io": abi.PgxMonitorIo,
               "pgx_monitor_totals": abi.PgxMonitorTotals}
    header_layout(structs)
    hdr = open(os.path.join(ROOT, "include", "pgx.h")).read()
    for name, code in (("TIMEOUT", 0), ("SUCCESS", 1), ("COLLISION", 2), ("NONFINITE", 3)):
        assert f"#define PGX_EP_{name} {code}" in hdr and getattr(abi, f"EP_{name}") == code
    assert (TIMEOUT, SUCCESS, COLLISION, NONFINITE) == (0, 1, 2, 3)


def test_library_exports_the_entry_points():
    assert_exported(MONITOR_EXPORTS)


@pytest.mark.parametrize("field,value", [("n_envs", 0), ("n_envs", -3), ("window", 0), ("window", -1),
                                         ("speed_col", 4), ("obs_dim", 5), ("obs_dim", 0)])
def test_create_rejects_bad_config_without_a_device(field, value):
    """PGX_E_INVALID comes from the argument check, before any HIP call: this runs without a GPU
    (a HIP failure would be PGX_E_HIP).  speed_col 4 with obs_dim 6, and obs_dim 5 with speed_col 3,
    are both speed_col + 3 > obs_dim."""
    lib = _native.load()
    cfg = abi.PgxMonitorConfig(64, 6, 100, 3)
    setattr(cfg, field, value)
    h = C.c_void_p()
    assert lib.pgx_monitor_create(C.byref(cfg), 0, C.byref(h)) == abi.PGX_E_INVALID
    assert not h.value
    msg = lib.pgx_last_error()
    assert b"pgx_monitor_create" in msg
    if (field, value) != ("obs_dim", 5):
        assert field.encode() in msg   # the message names the field
    else:
        assert b"speed_col" in msg
    # the null-handle checks of the other entry points
    assert lib.pgx_monitor_step(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_monitor_reset(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_monitor_clear(None, None) == abi.PGX_E_INVALID
    assert lib.pgx_monitor_set_targets(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_monitor_get_totals(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_monitor_create(None, 0, C.byref(h)) == abi.PGX_E_INVALID


def test_python_surface_is_exported():
    import inspect

    import panda_gym_amd as pg
    from panda_gym_amd import monitor as M

    sig = inspect.signature(pg.VecMonitor.__init__).parameters
    assert list(sig)[1:] == ["venv", "window", "info_keywords"]
    assert sig["window"].default == 100 and tuple(sig["info_keywords"].default) == ()
    for name in ("reset_tensors", "step_tensors", "capture_steps", "reset", "step_async", "step_wait", "step",
                 "totals", "episodes", "set_targets", "clear", "window_stats", "stats_vector", "combine"):
        assert hasattr(pg.VecMonitor, name), name
    for name in ("step", "step_arrays", "reset_arrays", "totals", "episodes", "set_targets", "clear"):
        assert hasattr(pg.EpisodeMonitor, name), name
    ev = inspect.signature(pg.evaluate).parameters
    assert list(ev)[:4] == ["venv", "policy", "n_eval_episodes", "deterministic"] and ev["deterministic"].default is True
    # the capture loops of the env and of VecNormalize share the one-step hook
    assert hasattr(pg.PandaVecEnv, "_enqueue_step") and hasattr(pg.VecNormalize, "_enqueue_step")
    assert M.episode_count_targets(20, 8).tolist() == [2, 2, 2, 2, 3, 3, 3, 3]   # (20 + i) // 8
    assert M.episode_count_targets(3, 4).tolist() == [0, 1, 1, 1]
    assert M.STATS_LAYOUT == ("episodes", "successes", "return_sum", "length_sum")


# ---------------------------------------------------------------- host arithmetic
def test_combine_sums_workers_and_divides():
    from panda_gym_amd.monitor import combine

    rows = np.array([[4.0, 1.0, -150.0, 200.0], [6.0, 3.0, -100.0, 120.0]])
    got = combine(rows)
    assert got == {"episodes": 10, "successes": 4, "return_sum": -250.0, "length_sum": 320, "ep_rew_mean": -25.0,
                   "ep_len_mean": 32.0, "success_rate": 0.4}
    one = combine(rows[0])   # a single row
    assert one["episodes"] == 4 and one["ep_rew_mean"] == -37.5 and one["success_rate"] == 0.25
    empty = combine(np.zeros((3, 4)))
    assert empty["episodes"] == 0 and all(math.isnan(empty[k]) for k in ("ep_rew_mean", "ep_len_mean", "success_rate"))


# five hand-made episodes: two successes, a timeout, a collision, one non-finite
HAND = [(F32(-3.0), 3, 0, SUCCESS, 3, 0.3), (F32(-1.0), 1, 1, SUCCESS, 4, 0.2), (F32(-50.0), 50, 2, TIMEOUT, 50, 9.0),
        (F32(-101.0), 7, 0, COLLISION, 10, 1.0), (F32(np.nan), 9, 3, NONFINITE, 9, 2.0)]
HAND_TOTALS = {"episodes": 5, "outcomes": [1, 2, 1, 1], "length_sum": 61, "length_sum_success": 4, "steps": 50,
               "envs_open": 0, "return_sum": -155.0, "speed_sum_success": 0.5}


def test_evaluation_result_on_hand_made_records():
    from panda_gym_amd.monitor import evaluation_result

    cols = list(zip(*HAND))
    eps = {"r": np.array(cols[0], F32), "l": np.array(cols[1], np.int32), "env": np.array(cols[2], np.int32),
           "outcome": np.array(cols[3], np.int32), "step": np.array(cols[4], np.int64),
           "speed_sum": np.array(cols[5], F64)}
    got = evaluation_result(HAND_TOTALS, eps, 20)
    # by hand: the four finite returns have mean -38.75 and squared deviations 1278.0625, 1425.0625,
    # 126.5625, 3875.0625 (sum 6704.75, / 4 = 1676.1875)
    want = {"mean_reward": -38.75, "std_reward": round(math.sqrt(1676.1875), 4), "success_rate": 0.4,
            "collision_rate": 0.2, "timeout_rate": 0.2, "nonfinite_rate": 0.2, "num_episodes": 5,
            "mean_ep_length": 15.25, "mean_ep_length_success": 2.0, "mean_num_sim_steps": 305.0,
            "mean_num_sim_steps_success": 40.0, "mean_ee_speed": 0.125}
    assert got == want
    assert ref_evaluation(HAND, 20) == want   # the GPU tests' restatement agrees with the hand values
    none = evaluation_result(dict(HAND_TOTALS, episodes=1, outcomes=[1, 0, 0, 0], length_sum=50, length_sum_success=0,
                                  return_sum=-50.0, speed_sum_success=0.0), {k: v[2:3] for k, v in eps.items()}, 20)
    assert none["success_rate"] == 0.0 and math.isnan(none["mean_ep_length_success"]) and math.isnan(none["mean_ee_speed"])
    assert none["mean_reward"] == -50.0 and none["std_reward"] == 0.0


def test_restatement_on_a_trace_followed_by_hand():
    """RefMonitor pinned: 3 envs, window 2, speed |v| = 1 each step, targets (2, 1, none)."""
    ref = RefMonitor(3, 2, speed_col=0, targets=None)
    obs = np.tile(np.array([[0.6, 0.0, 0.8]], F32), (3, 1))   # 0.36 + 0.64 -> 1 to rounding
    one = float(np.sqrt(F64(F32(0.6)) * F64(F32(0.6)) + 0.0 + F64(F32(0.8)) * F64(F32(0.8))))
    u8 = lambda *a: np.array(a, np.uint8)  # noqa: E731
    ref.set_targets([2, 1, 2 ** 31 - 1])
    assert ref.tot["envs_open"] == 3
    # step 1: env 1 succeeds
    r, l, d = ref.step(np.array([-1, -1, -1], F32), u8(0, 1, 0), u8(0, 1, 0), u8(0, 0, 0), obs, obs)
    assert d.tolist() == [False, True, False] and r[1] == -1 and l[1] == 1
    assert list(ref.ring) == [(F32(-1), 1, 1, SUCCESS, 1, one)] and ref.tot["envs_open"] == 2
    # step 2: every env done -- env 0 collides, env 1 is over its quota (not recorded), env 2 times out;
    # window 2 keeps the last two in env order
    r, l, d = ref.step(np.array([-100, -1, -1], F32), u8(0, 0, 0), u8(0, 0, 0), u8(1, 1, 1), obs, obs,
                       task_truncated=u8(1, 0, 0))
    assert r.tolist() == [-101.0, -1.0, -2.0] and l.tolist() == [2, 1, 2]
    assert [e[2:5] for e in ref.ring] == [(0, COLLISION, 2), (2, TIMEOUT, 2)]
    assert ref.ep_count.tolist() == [1, 1, 1] and ref.ret.tolist() == [0, 0, 0] and ref.len.tolist() == [0, 0, 0]
    assert ref.tot == {"episodes": 3, "outcomes": [1, 1, 1, 0], "length_sum": 5, "length_sum_success": 1, "steps": 2,
                       "envs_open": 2, "return_sum": -104.0, "speed_sum_success": one}
    # step 3: a NaN reward poisons env 0's return; it finishes non-finite and enters no sum
    ref.step(np.array([np.nan, -1, -1], F32), u8(0, 0, 0), u8(0, 0, 0), u8(1, 0, 0), obs, obs)
    assert ref.tot["outcomes"] == [1, 1, 1, 1] and ref.tot["episodes"] == 4 and ref.tot["return_sum"] == -104.0
    assert ref.tot["length_sum"] == 5 and ref.tot["envs_open"] == 1 and ref.ep_count.tolist() == [2, 1, 1]
    # a masked reset abandons env 2's running episode only
    ref.reset(u8(0, 0, 1))
    assert ref.len.tolist() == [0, 1, 0] and ref.ret.tolist() == [0.0, -1.0, 0.0]
