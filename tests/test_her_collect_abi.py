"""HER collection on the device (include/pgx.h, pgx_replay_set_last / _collect / _truncate_last_trajectory
/ _state / _arrays) without a GPU: the new ctypes mirrors against the header's layout through gcc, the
exported entry points, the Python surface, and RefCollect, the numpy restatement the GPU tests compare
against, written from the rules of include/pgx.h: carry -> transition -> oracle.her.HerOracle.add, plus
SB3's truncate_last_trajectory.  It is pinned on a trace small enough to follow by hand."""
import inspect
import os

import numpy as np

from oracle import her as H
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KEYS = ("observation", "achieved_goal", "desired_goal")
ERR_NO_CARRY = 1
COLLECT_EXPORTS = ["pgx_replay_set_last", "pgx_replay_collect", "pgx_replay_truncate_last_trajectory",
                   "pgx_replay_state", "pgx_replay_arrays"]


# ---------------------------------------------------------------- the restatement
class RefCollect:
    """``HerReplayBuffer``'s collection in numpy over ``HerOracle``: the carry (SB3's
    ``_last_original_obs``), ``collect`` (done = terminated | truncated, timeout = truncated &
    ~terminated with ``handle_timeout``, next_* = the terminal observation of a done env, then
    ``HerOracle.add`` and carry = the post-step observation; without a carry nothing but the error
    bit), and ``truncate_last_trajectory`` (for every env with cur_ep_start != pos: the episode
    [cur_ep_start, pos) gets its length, cur_ep_start = pos, dones[pos - 1] = 1 and, with
    ``handle_timeout``, timeouts[pos - 1] = 1)."""

    def __init__(self, n_envs, capacity, obs_dim, action_dim, handle_timeout=True, **kw):
        self.o = H.HerOracle(n_envs, capacity, obs_dim, action_dim, **kw)
        self.N, self.C, self.od, self.ad = n_envs, capacity, obs_dim, action_dim
        self.handle_timeout = bool(handle_timeout)
        self.last = None
        self.added, self.errors = 0, 0

    def set_last(self, obs):
        self.last = {k: np.array(obs[k], F32) for k in KEYS}

    def add(self, *args):
        """A direct add (``add_tensors``): the carry is not involved."""
        self.o.add(*args)
        self.added += 1

    def collect(self, action, reward, obs, terminated, truncated, terminal_obs):
        if self.last is None:
            self.errors |= ERR_NO_CARRY
            return
        te, tr = np.asarray(terminated) != 0, np.asarray(truncated) != 0
        done = te | tr
        timeout = (tr & ~te) if self.handle_timeout else np.zeros(self.N, bool)
        nxt = {k: np.where(done[:, None], np.asarray(terminal_obs[k], F32), np.asarray(obs[k], F32)) for k in KEYS}
        self.o.add(self.last["observation"], self.last["achieved_goal"], self.last["desired_goal"],
                   np.asarray(action, F32), np.asarray(reward, F32), nxt["observation"], nxt["achieved_goal"],
                   nxt["desired_goal"], done.astype(np.uint8), timeout.astype(np.uint8))
        self.last = {k: np.array(obs[k], F32) for k in KEYS}
        self.added += 1

    def truncate_last_trajectory(self):
        o, Cn = self.o, self.C
        for e in range(self.N):
            start = int(o.cur_ep_start[e])
            if start == o.pos:
                continue
            end = o.pos if o.pos > start else o.pos + Cn
            o.ep_length[np.arange(start, end) % Cn, e] = end - start
            o.cur_ep_start[e] = o.pos
            o.done[(o.pos - 1) % Cn, e] = 1
            if self.handle_timeout:
                o.timeout[(o.pos - 1) % Cn, e] = 1

    # what the device keeps, in its layout
    @property
    def pos(self):
        return self.o.pos

    def stored_done(self):
        """done * (1 - timeout), the only form the ring keeps and a sample returns."""
        return (self.o.done * (1 - self.o.timeout)).astype(F32)

    def fields(self):
        """The record's fields [C, N, ...] by their batch-row names, then the episode copies."""
        o = self.o
        return {"obs": o.obs, "achieved_goal": o.ag, "desired_goal": o.dg, "action": o.action, "reward": o.reward,
                "next_obs": o.next_obs, "next_achieved_goal": o.next_ag, "next_desired_goal": o.next_dg,
                "done": self.stored_done(), "rec_ep_start": o.ep_start.astype(np.int32),
                "rec_ep_length": o.ep_length.astype(np.int32)}

    def n_valid(self):
        return int((self.o.ep_length > 0).sum())


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    """ctypes mirrors of pgx_replay_step / pgx_replay_views == the header's sizeof / offsetof (gcc, as C)."""
    structs = {"pgx_replay_step": abi.PgxReplayStep, "pgx_replay_views": abi.PgxReplayViews}
    header_layout(structs)
    hdr = open(os.path.join(ROOT, "include", "pgx.h")).read()
    assert f"#define PGX_REPLAY_ERR_NO_CARRY {ERR_NO_CARRY}" in hdr
    assert abi.REPLAY_ERR_NO_CARRY == ERR_NO_CARRY and ERR_NO_CARRY in abi.REPLAY_ERRORS


def test_library_exports_the_entry_points():
    assert_exported(COLLECT_EXPORTS)


def test_null_handles_are_rejected_without_a_device():
    lib = _native.load()
    assert lib.pgx_replay_set_last(None, None, None, None, None) == abi.PGX_E_INVALID
    assert b"pgx_replay_set_last" in lib.pgx_last_error()
    assert lib.pgx_replay_collect(None, None, None) == abi.PGX_E_INVALID
    assert lib.pgx_replay_truncate_last_trajectory(None, 1, None) == abi.PGX_E_INVALID
    assert lib.pgx_replay_state(None, None, None, None, 0, None) == abi.PGX_E_INVALID
    assert lib.pgx_replay_arrays(None, None) == abi.PGX_E_INVALID


def test_python_surface_is_exported():
    import panda_gym_amd as pg

    B = pg.HerReplayBuffer
    for name in ("set_last", "collect_tensors", "collect_from_vec_env", "after_step", "truncate_last_trajectory",
                 "raise_device_errors", "arrays", "pos", "full", "size", "add", "add_tensors", "add_from_vec_env",
                 "sample", "sample_raw", "sample_into"):
        assert hasattr(B, name), name
    par = lambda f: list(inspect.signature(f).parameters)[1:]  # noqa: E731
    assert par(B.set_last) == ["obs"]
    assert par(B.collect_tensors) == ["action", "reward", "obs", "terminated", "truncated", "terminal_obs"]
    assert par(B.collect_from_vec_env) == ["venv", "action"]
    assert par(B.after_step) == ["venv", "actions"]
    assert inspect.signature(B.after_step).parameters["actions"].default is None
    assert par(B.truncate_last_trajectory) == []
    # the existing surface keeps its signatures
    assert par(B.add) == ["obs", "next_obs", "action", "reward", "done", "infos"]
    assert par(B.add_tensors) == ["obs", "achieved_goal", "desired_goal", "action", "reward", "next_obs",
                                  "next_achieved_goal", "next_desired_goal", "done", "timeout"]
    assert par(B.add_from_vec_env) == ["venv", "obs", "action"]


# ---------------------------------------------------------------- RefCollect, by hand
def o(x, n=2):
    return {"observation": np.full((n, 2), x, F32), "achieved_goal": np.full((n, 3), x + 0.25, F32),
            "desired_goal": np.full((n, 3), x + 0.5, F32)}


def u8(*x):
    return np.array(x, np.uint8)


def run_trace(handle_timeout):
    """2 envs x 6 steps at capacity 4.  Step i < 4 goes from observation o(i) to o(i + 1) with terminal
    observation o(100 + i); after step 3 (pos = 0 again) the open episodes are truncated and the carry
    set to o(10); steps 4 and 5 go to o(11) and o(12)."""
    ref = RefCollect(2, 4, 2, 1, handle_timeout=handle_timeout)
    f = lambda *x: np.array(x, F32)  # noqa: E731
    ref.collect(f([9], [9]), f(9, 9), o(9), u8(0, 0), u8(0, 0), o(9))     # no carry yet
    assert ref.errors == ERR_NO_CARRY and ref.added == 0 and ref.pos == 0 and ref.last is None
    assert not ref.o.obs.any() and not ref.o.ep_length.any()
    ref.errors = 0
    ref.set_last(o(0))
    #                action          reward     post-step  terminated truncated terminal
    ref.collect(f([0.5], [0.5]), f(-1, 0), o(1), u8(0, 1), u8(0, 0), o(100))   # env 1 terminated
    ref.collect(f([1.5], [1.5]), f(-1, -1), o(2), u8(0, 0), u8(1, 0), o(101))  # env 0 time limit
    ref.collect(f([2.5], [2.5]), f(-1, 0), o(3), u8(0, 1), u8(0, 1), o(102))   # env 1 both flags
    ref.collect(f([3.5], [3.5]), f(-1, -1), o(4), u8(0, 0), u8(0, 0), o(103))
    return ref, f


def test_restatement_on_a_trace_followed_by_hand():
    ref, f = run_trace(True)
    q = ref.o
    assert ref.pos == 0 and q.full and ref.added == 4
    # env 0: episode [0, 2) closed by the time limit, [2, ...) open.  env 1: [0, 1) terminated, [1, 3)
    # closed by both flags, [3, ...) open
    assert q.ep_length.T.tolist() == [[2, 2, 0, 0], [1, 2, 2, 0]]
    assert q.ep_start.T.tolist() == [[0, 0, 2, 2], [0, 1, 1, 3]]
    assert q.cur_ep_start.tolist() == [2, 3]
    # stored done: a time limit alone is not a termination; terminated wins over truncated
    assert ref.stored_done().T.tolist() == [[0, 0, 0, 0], [1, 0, 1, 0]]
    assert q.timeout.T.tolist() == [[0, 1, 0, 0], [0, 0, 0, 0]]
    # obs is the carry of the step before; next_obs the terminal observation exactly where done
    assert q.obs[:, :, 0].T.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3]]
    assert q.next_obs[:, :, 0].T.tolist() == [[1, 101, 3, 4], [100, 2, 102, 4]]
    assert q.next_ag[:, :, 0].T.tolist() == [[1.25, 101.25, 3.25, 4.25], [100.25, 2.25, 102.25, 4.25]]
    assert q.next_dg[1, 0].tolist() == [101.5] * 3 and q.dg[1, 0].tolist() == [1.5] * 3
    assert ref.last["observation"][:, 0].tolist() == [4.0, 4.0] and ref.n_valid() == 5

    # the truncate with open episodes at pos = 0: [2, 4) of env 0 and [3, 4) of env 1 get their lengths
    ref.truncate_last_trajectory()
    assert q.ep_length.T.tolist() == [[2, 2, 2, 2], [1, 2, 2, 1]] and q.cur_ep_start.tolist() == [0, 0]
    assert q.done[3].tolist() == [1, 1] and q.timeout[3].tolist() == [1, 1]   # slot pos - 1 wraps to 3
    assert ref.stored_done().T.tolist() == [[0, 0, 0, 0], [1, 0, 1, 0]]      # done * (1 - timeout) stays 0
    assert ref.n_valid() == 8 and ref.pos == 0
    before = (q.ep_length.copy(), q.done.copy(), q.timeout.copy(), q.cur_ep_start.copy())
    ref.truncate_last_trajectory()                                           # nothing open: a no-op
    assert all(np.array_equal(a, b) for a, b in zip(before, (q.ep_length, q.done, q.timeout, q.cur_ep_start)))

    ref.set_last(o(10))   # the observation of the forced reset
    # step 4 at slot 0 overwrites the first slot of env 0's [0, 2) and env 1's [0, 1): both go invalid
    ref.collect(f([4.5], [4.5]), f(-1, -1), o(11), u8(0, 0), u8(0, 0), o(104))
    assert q.ep_length.T.tolist() == [[0, 0, 2, 2], [0, 2, 2, 1]] and q.ep_start[0].tolist() == [0, 0]
    # step 5 at slot 1 overwrites env 1's [1, 3): slots 1 and 2 go invalid; env 0 terminates: [0, 2)
    ref.collect(f([5.5], [5.5]), f(0, -1), o(12), u8(1, 0), u8(0, 0), o(105))
    assert ref.pos == 2 and ref.added == 6 and ref.errors == 0
    assert q.ep_length.T.tolist() == [[2, 2, 2, 2], [0, 0, 0, 1]]
    assert q.ep_start.T.tolist() == [[0, 0, 2, 2], [0, 0, 1, 3]]
    assert q.cur_ep_start.tolist() == [2, 0]
    assert ref.stored_done().T.tolist() == [[0, 1, 0, 0], [0, 0, 1, 0]]
    assert q.obs[:, :, 0].T.tolist() == [[10, 11, 2, 3], [10, 11, 2, 3]]     # the new episodes start at o(10)
    assert q.next_obs[:, :, 0].T.tolist() == [[11, 105, 3, 4], [11, 12, 102, 4]]
    assert ref.last["desired_goal"][0].tolist() == [12.5] * 3 and ref.n_valid() == 5
    fl = ref.fields()
    assert fl["rec_ep_length"].dtype == np.int32 and fl["done"].dtype == F32
    assert fl["rec_ep_start"][2].tolist() == [2, 1]


def test_restatement_without_timeout_handling():
    """handle_timeout_termination = False: a time limit is stored as a termination, and the truncate
    marks the last transition of an open episode done."""
    ref, _ = run_trace(False)
    assert not ref.o.timeout.any()
    assert ref.stored_done().T.tolist() == [[0, 1, 0, 0], [1, 0, 1, 0]]
    ref.truncate_last_trajectory()
    assert ref.stored_done().T.tolist() == [[0, 1, 0, 1], [1, 0, 1, 1]] and not ref.o.timeout.any()
    assert ref.o.ep_length.T.tolist() == [[2, 2, 2, 2], [1, 2, 2, 1]]


def test_no_goal_is_drawn_across_a_truncation():
    """After the truncate every "future" goal slot lies in [slot, end of the truncated episode)."""
    ref, _ = run_trace(True)
    ref.truncate_last_trajectory()
    s = ref.o.sample(512, 0)
    her = s["goal_slot"] >= 0
    assert her.sum() == int(0.8 * 512)
    start, length = ref.o.ep_start[s["slot"], s["env"]], ref.o.ep_length[s["slot"], s["env"]]
    rel = (s["goal_slot"] - start) % ref.C
    cur = (s["slot"] - start) % ref.C
    assert (rel[her] >= cur[her]).all() and (rel[her] < length[her]).all()
    assert set(zip(s["slot"].tolist(), s["env"].tolist())) == {(c, e) for c in range(4) for e in range(2)}
