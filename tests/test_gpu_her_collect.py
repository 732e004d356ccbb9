"""GPU tests of the HER ring's device collection (pgx_her.hip: set_last / collect /
truncate_last_trajectory, the ring position as a device word; panda_gym_amd/her.py) against RefCollect,
the numpy restatement tests/test_her_collect_abi.py writes from the rules of include/pgx.h and pins by
hand, against the existing path (clones + add_from_vec_env) on real envs, and captured against eager.

The bar is bit-exactness everywhere: collection copies and selects, it computes nothing, so there is no
tolerance to choose.  Floats compare through their integer views (a NaN as "NaN in the same places").
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import panda_gym_amd as pg  # noqa: E402
from panda_gym_amd import abi  # noqa: E402
from panda_gym_amd._native import PgxError  # noqa: E402
from test_her_collect_abi import ERR_NO_CARRY, KEYS, RefCollect  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
DEV = "cuda:0"
FIELDS = ("obs", "achieved_goal", "desired_goal", "action", "reward", "next_obs", "next_achieved_goal",
          "next_desired_goal", "done", "rec_ep_start")
# (N, C, obs, A) -> the seed of its trace: one under which 40 steps of Bernoulli(0.15) flags show all
# four combinations and the ring ends with valid transitions to sample (at N = 1 most seeds give
# neither; both are properties of the inputs alone)
SHAPES = {(33, 7, 6, 3): 0, (48, 23, 56, 7): 0, (1, 5, 19, 4): 17}
STEPS = 40


def assert_same(got, want, what):
    """Bit for bit (floats through their integer views), NaN matching NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = got[~nan].view(np.uint32), want[~nan].view(np.uint32)
    assert np.array_equal(got, want), what


def host(t):
    return t.detach().cpu().numpy().copy()


def snapshot(buf):
    return {k: host(v) for k, v in buf.arrays().items()}


def assert_identical(a, b, what):
    """Two snapshots: every array of the blob, the records' padding included."""
    assert a.keys() == b.keys()
    for k in a:
        assert_same(a[k], b[k], f"{what} {k}")


def assert_buffer(buf, ref, what, finite=True):
    """Everything the ring keeps against RefCollect: every record field of every slot (the records'
    ep_length copy for the valid transitions: it is refreshed when an episode completes and only read
    for those), the carry, the dense bookkeeping, n_valid, pos and added."""
    a, want = snapshot(buf), ref.fields()
    valid = ref.o.ep_length > 0
    for k in FIELDS:
        assert_same(a[k], want[k], f"{what} {k}")
        assert_same(a[k][valid], want[k][valid], f"{what} {k} of the valid transitions")
    assert_same(a["rec_ep_length"][valid], want["rec_ep_length"][valid], f"{what} rec_ep_length")
    assert_same(a["ep_start"], ref.o.ep_start.astype(np.int32), f"{what} ep_start")
    assert_same(a["ep_length"], ref.o.ep_length.astype(np.int32), f"{what} ep_length")
    assert_same(a["cur_ep_start"], ref.o.cur_ep_start.astype(np.int32), f"{what} cur_ep_start")
    assert int(a["n_valid"][0]) == ref.n_valid(), what
    assert int(a["added"][0]) == ref.added and buf.pos == ref.pos == ref.added % ref.C, what
    assert buf.size() == min(ref.added, ref.C) and buf.full == (ref.added >= ref.C), what
    od = ref.od
    if ref.last is not None:
        for k in KEYS:
            assert_same(a["last_" + k], ref.last[k], f"{what} carry {k}")
        assert int(a["carry_set"][0]) == 1
    assert not a["carry"][:, od + 6:].any(), f"{what}: carry padding is not zero"
    assert not a["records"][:, :, buf.row_dim + 2:].any(), f"{what}: record padding is not zero"
    if finite:
        assert np.isfinite(a["records"][:, :, :buf.row_dim]).all() and np.isfinite(a["carry"]).all(), what
    return a


def assert_samples(buf, ref, what, batch=1031, draws=(0, 1, 2)):
    for d in draws:
        got, want = buf.sample_raw(batch, draw=d), ref.o.sample(batch, d)
        for k, w in want.items():
            assert_same(host(got[k]), w, f"{what} draw {d} field {k}")


def make_trace(N, od, A, seed, steps=STEPS):
    """Synthetic step outputs: per step (action, reward, post-step obs dict, terminated, truncated,
    terminal obs dict), then the first observation."""
    rng = np.random.default_rng(seed)
    f = lambda *s: (rng.standard_normal((N,) + s) * 0.05).astype(F32)  # noqa: E731
    obs = lambda: {"observation": f(od), "achieved_goal": f(3), "desired_goal": f(3)}  # noqa: E731
    first = obs()
    out = []
    for _ in range(steps):
        te = (rng.random(N) < 0.15).astype(np.uint8)
        tr = (rng.random(N) < 0.15).astype(np.uint8)
        out.append((f(A), f(), obs(), te, tr, obs()))
    return out, first


def flag_combinations(trace):
    return {(int(a), int(b)) for s in trace for a, b in zip(s[3], s[4])}


def make_pair(N, C, od, A, seed=3, handle_timeout=True):
    buf = pg.HerReplayBuffer(N * C, device=DEV, n_envs=N, obs_dim=od, action_dim=A, seed=seed,
                             handle_timeout_termination=handle_timeout)
    ref = RefCollect(N, C, od, A, handle_timeout=handle_timeout, her_ratio=buf.her_ratio, seed=seed)
    return buf, ref


def feed(buf, ref, step):
    buf.collect_tensors(*step)
    ref.collect(*step)


# ------------------------------------------------------------------ 1. against RefCollect
@pytest.mark.parametrize("shape", list(SHAPES))
def test_synthetic_steps_match_the_restatement(shape):
    N, C, od, A = shape
    trace, first = make_trace(N, od, A, SHAPES[shape])
    assert flag_combinations(trace) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    buf, ref = make_pair(N, C, od, A)
    buf.set_last(first)
    ref.set_last(first)
    for t, step in enumerate(trace):
        feed(buf, ref, step)
        if t % 13 == 5:
            assert_buffer(buf, ref, f"{shape} step {t}")
    assert ref.added == STEPS and ref.added // C >= 1 and ref.n_valid() > 0
    assert_buffer(buf, ref, f"{shape} end")
    assert_samples(buf, ref, f"{shape}")
    buf.raise_device_errors()
    buf.close()


def test_episodes_longer_than_a_lane_group():
    """Episodes of 19 and 37 steps with staggered ends: the collect kernel deals an episode's length
    stores and an overwritten episode's invalidation over its 16 lanes, so both loops take more than
    one pass here, at a ring (45 slots) that wraps in the 100 steps and is overwritten in mid-episode."""
    N, C, od, A, steps = 33, 45, 6, 3, 100
    trace, first = make_trace(N, od, A, 4, steps=steps)
    e = np.arange(N)
    period = np.where(e % 2 == 0, 19, 37)
    for t, step in enumerate(trace):
        end = (t + e) % period == period - 1
        step[3][:] = end & (e % 3 == 0)            # terminated
        step[4][:] = end & (e % 3 != 0)            # time limit
    buf, ref = make_pair(N, C, od, A)
    buf.set_last(first)
    ref.set_last(first)
    for t, step in enumerate(trace):
        feed(buf, ref, step)
        if t in (36, 44, 45, 63, 90):
            assert_buffer(buf, ref, f"long episodes step {t}")
    assert ref.o.ep_length.max() == 37 and (ref.o.ep_length == 19).any()
    assert_buffer(buf, ref, "long episodes end")
    assert_samples(buf, ref, "long episodes")
    buf.truncate_last_trajectory()
    ref.truncate_last_trajectory()
    assert_buffer(buf, ref, "long episodes truncated")
    buf.raise_device_errors()
    buf.close()


# ------------------------------------------------------------------ 2. against the existing path
def run_both_paths(venv, base, steps, cap, actions_of):
    """The same steps into two rings of one seed: clones + add_from_vec_env on the env itself (raw
    values), set_last + collect_from_vec_env through ``venv`` as given."""
    old = pg.HerReplayBuffer(cap * base.num_envs, env=base, device=DEV, seed=5)
    new = pg.HerReplayBuffer(cap * base.num_envs, env=base, device=DEV, seed=5)
    new.set_last(base._obs_dict())
    counts = {"terminated": 0, "truncated": 0, "collided": 0, "neither": 0}
    for t in range(steps):
        prev = {k: v.clone() for k, v in base._obs_dict().items()}
        a = actions_of(t)
        venv.step_tensors(a)
        old.add_from_vec_env(base, prev, a)
        new.collect_from_vec_env(venv, a)
        te, tr = base.terminated.bool(), base.truncated.bool()
        counts["terminated"] += int(te.sum())
        counts["truncated"] += int(tr.sum())
        counts["collided"] += int(base.task_trunc.bool().sum())
        counts["neither"] += int((~te & ~tr).sum())
    a, b = snapshot(old), snapshot(new)
    for k in a:
        if not k.startswith("last_") and k not in ("carry", "carry_set"):   # the old path keeps no carry
            assert_same(b[k], a[k], f"records and bookkeeping: {k}")
    assert np.isfinite(b["records"]).all() and np.isfinite(b["carry"]).all()
    for k, name in (("observation", "obs"), ("achieved_goal", "achieved_goal"), ("desired_goal", "desired_goal")):
        assert_same(b["last_" + k], host(getattr(base, name)), f"carry {k}")
    assert new.pos == old.pos == steps % cap and new.size() == old.size()
    for d in range(3):
        x, y = old.sample_raw(1031, draw=d), new.sample_raw(1031, draw=d)
        for k in x:
            assert_same(host(y[k]), host(x[k]), f"draw {d} field {k}")
    new.raise_device_errors()
    old.close()
    new.close()
    print("step outcomes:", counts)
    return counts


def wrap(env, wrapped):
    return pg.VecMonitor(pg.VecNormalize(env)) if wrapped else env


@pytest.mark.parametrize("wrapped", [False, True])
def test_reach_collect_equals_the_existing_path(wrapped):
    base = pg.PandaVecEnv("PandaReach-v3", num_envs=256, device=DEV, seed=11, max_episode_steps=10)
    venv = wrap(base, wrapped)
    venv.reset_tensors()
    counts = run_both_paths(venv, base, 25, 16, lambda t: base.sample_actions(t).clone())
    assert counts["truncated"] > 0 and counts["neither"] > 0
    base.close()


@pytest.mark.parametrize("wrapped", [False, True])
def test_reach_ao_collect_equals_the_existing_path(wrapped):
    """Half the envs start with the goal at the end effector and the obstacles far away, so their
    first step terminates; the others fly random actions among their obstacles."""
    from oracle.oracle import fk

    N = 64
    base = pg.PandaVecEnv("PandaReachAO-v3", num_envs=N, device=DEV, seed=1)
    venv = wrap(base, wrapped)
    venv.reset_tensors()
    com, _, _ = fk(base._cfg.model.contents, np.array(abi.NEUTRAL_Q[:7]))
    far = np.tile(np.array([99.9, 99.9, -99.9]), (N, 6, 1))
    mask = torch.arange(N, device=DEV) < N // 2
    base.reset_tensors(mask=mask, goals=np.tile(com[11] + 0.01, (N, 1)), objects=far)
    half = mask.unsqueeze(1)

    def actions_of(t):
        a = base.sample_actions(t).clone()
        return torch.where(half, torch.zeros_like(a), a) if t == 0 else a

    counts = run_both_paths(venv, base, 30, 16, actions_of)
    assert counts["terminated"] > 0 and counts["collided"] > 0 and counts["neither"] > 0
    base.close()


# ------------------------------------------------------------------ 3. captured against eager
@pytest.mark.parametrize("own_actions", [False, True])
def test_captured_collect_equals_eager(own_actions):
    N, K, C, R = 96, 6, 8, 3
    envs = [pg.PandaVecEnv("PandaReach-v3", num_envs=N, device=DEV, seed=7, max_episode_steps=4) for _ in range(2)]
    bufs = [pg.HerReplayBuffer(C * N, env=e, device=DEV, seed=9) for e in envs]
    for e, b in zip(envs, bufs):
        b.set_last(e.reset_tensors())
    cap_env, eager_env = envs
    cap_buf, eager_buf = bufs
    gen = torch.Generator(device=DEV).manual_seed(4)
    actions = None if own_actions else (torch.rand((K, N, 3), device=DEV, generator=gen) * 2 - 1).contiguous()
    base = cap_env._step_index
    g = cap_env.capture_steps(K, actions, after_step=cap_buf.after_step(cap_env, actions))
    for _ in range(R):
        g.replay()
    for _ in range(R):
        for i in range(K):
            a = actions[i] if actions is not None else eager_env.sample_actions(base + i)
            eager_env.step_tensors(a)
            eager_buf.collect_from_vec_env(eager_env, a)
    a, b = snapshot(cap_buf), snapshot(eager_buf)
    assert_identical(a, b, "captured vs eager")
    assert np.isfinite(a["records"]).all() and (a["ep_length"] > 0).any()
    assert_same(host(cap_env._outbuf), host(eager_env._outbuf), "env outputs")
    assert int(a["added"][0]) == K * R
    assert cap_buf.pos == (K * R) % C == 2 and cap_buf.size() == C and cap_buf.full
    # the device word is the truth for an eager add behind the replays: it lands in slot 18 % 8
    rng = np.random.default_rng(0)
    f = lambda *s: (rng.standard_normal((N,) + s) + 7.0).astype(F32)  # noqa: E731
    t = [f(6), f(3), f(3), f(3), f(), f(6), f(3), f(3), np.ones(N, np.uint8), np.zeros(N, np.uint8)]
    cap_buf.add_tensors(*t)
    c = snapshot(cap_buf)
    assert int(c["added"][0]) == K * R + 1 and cap_buf.pos == 3
    for name, want in zip(("obs", "achieved_goal", "desired_goal", "action", "reward", "next_obs",
                           "next_achieved_goal", "next_desired_goal"), t):
        assert_same(c[name][2], want, f"eager add behind the replays: {name}")
        for s in (1, 3):
            assert_same(c[name][s], a[name][s], f"eager add behind the replays: slot {s} {name}")
    assert (c["ep_length"][2] > 0).all() and (c["cur_ep_start"] == 3).all()
    cap_buf.raise_device_errors()
    for x in bufs + envs:
        x.close()


# ------------------------------------------------------------------ 4. truncate_last_trajectory
@pytest.mark.parametrize("handle_timeout", [True, False])
def test_truncate_last_trajectory(handle_timeout):
    N, C, od, A = 33, 16, 6, 3
    trace, first = make_trace(N, od, A, 21, steps=15)
    buf, ref = make_pair(N, C, od, A, handle_timeout=handle_timeout)
    buf.set_last(first)
    ref.set_last(first)
    for step in trace[:9]:
        feed(buf, ref, step)
    open_before = ref.o.cur_ep_start != ref.pos
    assert open_before.any() and not open_before.all()
    buf.truncate_last_trajectory()
    ref.truncate_last_trajectory()
    a = assert_buffer(buf, ref, "truncated")
    # every stored transition is valid now
    assert (a["ep_length"][:9] > 0).all() and not a["ep_length"][9:].any() and int(a["n_valid"][0]) == 9 * N
    assert (a["cur_ep_start"] == 9).all()
    assert (a["done"][8][open_before] == (0.0 if handle_timeout else 1.0)).all()
    assert_samples(buf, ref, "truncated")
    buf.truncate_last_trajectory()   # nothing is open: a no-op
    assert_identical(snapshot(buf), a, "second truncate")
    # a forced reset: new carry, and the following collects start new episodes
    buf.set_last(trace[9][2])
    ref.set_last(trace[9][2])
    for step in trace[10:]:
        feed(buf, ref, step)
    a = assert_buffer(buf, ref, "after the truncation")
    assert (a["ep_start"][9] == 9).all() and (a["rec_ep_start"][9] == 9).all()
    assert_same(a["obs"][9], trace[9][2]["observation"], "first observation behind the truncation")
    buf.truncate_last_trajectory()   # close the tail too, so that every transition can be drawn
    ref.truncate_last_trajectory()
    assert_buffer(buf, ref, "tail truncated")
    assert ref.pos == 14 and ref.n_valid() == 14 * N   # no wrap: slots compare as times
    # no relabelled goal crosses the truncation point, in either direction
    s = {k: host(v) for k, v in buf.sample_raw(4096, draw=5).items() if k in ("slot", "goal_slot")}
    her = s["goal_slot"] >= 0
    assert her.sum() == int(buf.her_ratio * 4096)
    slot, goal = s["slot"][her], s["goal_slot"][her]
    assert (goal >= slot).all() and ((slot < 9) == (goal < 9)).all()
    assert (slot < 9).any() and (slot >= 9).any() and goal.max() <= 13
    assert_samples(buf, ref, "tail truncated")
    buf.raise_device_errors()
    buf.close()


# ------------------------------------------------------------------ 5. containment
def test_non_finite_values_stay_in_their_env():
    N, C, od, A = 33, 7, 6, 3
    trace, first = make_trace(N, od, A, 8, steps=12)
    bad = 5
    trace[8][2]["observation"][bad, 2] = np.nan   # post-step observation: next_obs, then the carry and obs
    trace[9][1][bad] = np.inf                      # reward (slots 1 and 2 of the second lap: still there)
    trace[11][2]["achieved_goal"][bad, 0] = np.nan  # the last carry
    buf, ref = make_pair(N, C, od, A)
    buf.set_last(first)
    ref.set_last(first)
    for step in trace:
        feed(buf, ref, step)
    a = assert_buffer(buf, ref, "poisoned", finite=False)
    others = np.arange(N) != bad
    assert np.isfinite(a["records"][:, others]).all() and np.isfinite(a["carry"][others]).all()
    assert not np.isfinite(a["carry"][bad]).all()
    assert not np.isfinite(ref.o.next_obs[:, bad]).all() or not np.isfinite(ref.o.reward[:, bad]).all()
    buf.close()


# ------------------------------------------------------------------ 6. misuse
def test_collect_without_a_carry_is_refused():
    N, C, od, A = 33, 7, 6, 3
    trace, first = make_trace(N, od, A, 2, steps=2)
    buf, ref = make_pair(N, C, od, A)
    feed(buf, ref, trace[0])
    a = snapshot(buf)
    assert not a["records"].any() and not a["ep_length"].any() and not a["carry"].any()
    assert int(a["added"][0]) == 0 and int(a["n_valid"][0]) == 0 and int(a["carry_set"][0]) == 0
    assert int(a["errors"][0]) == ERR_NO_CARRY == ref.errors and buf.pos == 0 and buf.size() == 0
    with pytest.raises(PgxError, match="PGX_REPLAY_ERR_NO_CARRY"):
        buf.raise_device_errors()
    buf.raise_device_errors()   # cleared
    assert int(host(buf.arrays()["errors"])[0]) == 0
    buf.set_last(first)
    ref.set_last(first)
    feed(buf, ref, trace[1])
    assert_buffer(buf, ref, "after set_last")
    assert buf.pos == 1
    buf.raise_device_errors()
    buf.close()


# ------------------------------------------------------------------ 7. the env does not notice
def test_collect_in_the_step_graph_leaves_the_env_alone():
    N, steps = 128, 20
    envs = [pg.PandaVecEnv("PandaPush-v3", num_envs=N, device=DEV, seed=13, max_episode_steps=8) for _ in range(2)]
    buf = pg.HerReplayBuffer(16 * N, env=envs[0], device=DEV, seed=1)
    buf.set_last(envs[0].reset_tensors())
    envs[1].reset_tensors()
    acts = [torch.zeros((1, N, envs[0].action_dim), device=DEV) for _ in envs]
    graphs = [envs[0].capture_steps(1, acts[0], after_step=buf.after_step(envs[0], acts[0])),
              envs[1].capture_steps(1, acts[1])]
    gen = torch.Generator(device=DEV).manual_seed(6)
    for t in range(steps):
        a = torch.rand(acts[0].shape, device=DEV, generator=gen) * 2 - 1
        for x, g in zip(acts, graphs):
            x.copy_(a)
            g.replay()
        out = [host(e._outbuf) for e in envs]
        assert np.array_equal(out[0], out[1]), f"step {t}: the env's outputs differ with the collect behind it"
        assert np.isfinite(host(envs[0]._out_f32)).all()
    assert buf.pos == steps % 16 and buf.full
    buf.raise_device_errors()
    buf.close()
    for e in envs:
        e.close()
