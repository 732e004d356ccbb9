"""GPU tests of the device VecMonitor (pgx_monitor.hip, panda_gym_amd/monitor.py) against RefMonitor,
the numpy restatement of SB3's VecMonitor, of the ring as deque(maxlen=window), of the outcome
classification and of the episode quota that tests/test_monitor_abi.py writes from the rules of
include/pgx.h and pins by hand.

Bars.  Bit-exact: ep_r / ep_l where done, the ring's contents and order (r, l, env, outcome, step,
speed_sum), the per-env accumulators and ep_count, every integer total, envs_open.  (A NaN return
is compared as "NaN in the same places": the payload of a NaN is not part of the rules.)  The fp64
sums return_sum and speed_sum_success: |device - restatement| <= E * 2^-53 * sum|x| over the E summed
episodes, the worst case of any summation order; the same sequence twice gives identical bits; with
integer (sparse) returns the sums are equal outright.
Measured on an MI355X over every test here: return_sum equal to the restatement's in every
comparison; speed_sum_success within 6 % of its bar at worst (1.4e-14 against 2.3e-13).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from panda_gym_amd import abi  # noqa: E402
from panda_gym_amd import monitor as M  # noqa: E402
from test_monitor_abi import RefMonitor, ref_evaluation  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
INT_TOTALS = ("episodes", "length_sum", "length_sum_success", "steps", "envs_open")
OD = 7   # an odd row length: the speed columns 3..5 sit at no aligned offset


def assert_same(got, want, what):
    """Bit for bit (floats through their integer views), NaN matching NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        iv = np.uint32 if got.dtype == F32 else np.uint64
        got, want = got[~nan].view(iv), want[~nan].view(iv)
    assert np.array_equal(got, want), what


def assert_totals(got, ref, what, integer_returns=False):
    for k in INT_TOTALS:
        assert got[k] == ref.tot[k], (what, k, got[k], ref.tot[k])
    assert got["outcomes"] == ref.tot["outcomes"], (what, got["outcomes"], ref.tot["outcomes"])
    for k, e, mag in (("return_sum", ref.summed, ref.abs_return), ("speed_sum_success", ref.summed_success,
                                                                   ref.abs_speed)):
        err, bar = abs(got[k] - ref.tot[k]), e * 2.0 ** -53 * mag
        print(f"{what}: {k} device {got[k]!r} restatement {ref.tot[k]!r} |diff| {err:.3e} bar {bar:.3e}")
        assert err <= bar, (what, k, got[k], ref.tot[k], err, bar)
    if integer_returns:
        assert got["return_sum"] == ref.tot["return_sum"], what


def assert_state(mon, ref, what, integer_returns=False):
    """Ring, per-env state and totals of a monitor (EpisodeMonitor or VecMonitor) against the restatement."""
    got, want = mon.episodes(), ref.episodes()
    for k in ("env", "l", "outcome", "step", "r", "speed_sum"):
        assert_same(got[k], want[k], f"{what} ring {k}")
    st = mon.env_state()
    assert_same(st["ret"], ref.ret, f"{what} ret")
    assert_same(st["len"], ref.len, f"{what} len")
    assert_same(st["speed"], ref.speed, f"{what} speed")
    assert_same(st["ep_count"], ref.ep_count, f"{what} ep_count")
    assert_totals(mon.totals(), ref, what, integer_returns)


# ------------------------------------------------------------------ array level
STEPS, ALL_DONE_STEP, NAN_STEP = 12, 5, 9


def make_trace(n, seed, sparse=False):
    """12 steps of synthetic step outputs.  Env e is done wherever (t + e) % 3 == 2, at a few random
    steps more, and -- every env -- at step 5; the flags of (t, e) follow code (t + e) % 4: 0 none,
    1 success (half of them with the collision flag too: success wins), 2 collision, 3 the guard's flag
    (with success set: non-finite wins).  So env 0 alone meets every outcome (done at 2, 5, 8, 11 with
    codes 2, 1, 0, 3).  One reward, of env n // 2 at step 9, is NaN."""
    rng = np.random.default_rng(seed)
    t_, e_ = np.meshgrid(np.arange(STEPS), np.arange(n), indexing="ij")
    done = ((t_ + e_) % 3 == 2) | (rng.random((STEPS, n)) < 0.1)
    done[ALL_DONE_STEP] = True
    terminated = done & (rng.random((STEPS, n)) < 0.5)
    truncated = done & (~terminated | (rng.random((STEPS, n)) < 0.2))
    code = (t_ + e_) % 4
    success = (code == 1) | (code == 3)
    task = (code == 2) | ((code == 1) & (rng.random((STEPS, n)) < 0.5))
    nonfinite = code == 3
    if sparse:
        reward = -(rng.random((STEPS, n)) < 0.8).astype(F32)
    else:
        reward = rng.standard_normal((STEPS, n)).astype(F32)
    reward[NAN_STEP, n // 2] = np.nan
    obs = rng.standard_normal((STEPS, n, OD)).astype(F32)
    tobs = rng.standard_normal((STEPS, n, OD)).astype(F32)
    u8 = lambda x: x.astype(np.uint8)  # noqa: E731
    return [dict(reward=reward[t], success=u8(success[t]), terminated=u8(terminated[t]), truncated=u8(truncated[t]),
                 obs=obs[t], terminal_obs=tobs[t], task_truncated=u8(task[t]), nonfinite=u8(nonfinite[t]))
            for t in range(STEPS)]


def run_trace(n, window, targets, trace, what, integer_returns=False, every_step=True):
    mon = M.EpisodeMonitor(n, OD, window=window, device="cuda:0")
    ref = RefMonitor(n, window, targets=targets)
    if targets is not None:
        mon.set_targets(targets)
        assert mon.totals()["envs_open"] == ref.tot["envs_open"]
    for t, s in enumerate(trace):
        ep_r, ep_l = mon.step_arrays(**s)
        r, l, done = ref.step(**s)
        if every_step or t == len(trace) - 1:
            assert_same(ep_r.cpu().numpy()[done], r[done], f"{what} step {t} ep_r")
            assert_same(ep_l.cpu().numpy()[done], l[done], f"{what} step {t} ep_l")
            assert_state(mon, ref, f"{what} step {t}", integer_returns)
    return mon, ref


@pytest.mark.parametrize("targets", ["none", "quota"])
@pytest.mark.parametrize("window", [4, 100])
@pytest.mark.parametrize("n", [1, 63, 257, 1000])
def test_records_totals_and_state_vs_restatement(n, window, targets):
    """One wave, a ragged block, crossing a block, several slabs (1000 envs: four slabs of 256), with a
    ring that overflows within the all-done step (window 4; across slab boundaries at 1000) and one
    that does not at the small sizes (window 100).  "quota": targets 0, 1 and 2 by env id."""
    tg = None if targets == "none" else (np.arange(n) % 3).astype(np.int32)
    mon, ref = run_trace(n, window, tg, make_trace(n, 100 + n), f"n={n} window={window} {targets}")
    if tg is None:
        assert min(ref.tot["outcomes"]) > 0, ref.tot["outcomes"]   # every outcome code occurred
        assert ref.tot["episodes"] >= 4 * n and ref.tot["envs_open"] == n
    else:
        assert np.array_equal(ref.ep_count, tg) and ref.tot["envs_open"] == 0   # every quota filled, none exceeded
    assert len(ref.ring) == min(window, ref.tot["episodes"])
    mon.close()


def test_nan_return_is_classified_without_the_guard_flag():
    """The NaN reward reaches an episode whose own flags say otherwise: that episode is recorded as
    non-finite and enters no sum (restatement and device alike)."""
    n = 63
    trace = make_trace(n, 7)
    e = n // 2
    t_end = next(t for t in range(NAN_STEP, STEPS) if trace[t]["terminated"][e] | trace[t]["truncated"][e])
    assert trace[t_end]["nonfinite"][e] == 0   # code (t + e) % 4 != 3 there: only the return says so
    mon, ref = run_trace(n, 1000, None, trace, "nan", every_step=False)
    eps = mon.episodes()
    hit = (eps["env"] == e) & (eps["step"] == t_end + 1)
    assert hit.sum() == 1 and eps["outcome"][hit][0] == abi.EP_NONFINITE and np.isnan(eps["r"][hit][0])
    assert np.isfinite(mon.totals()["return_sum"])
    mon.close()


@pytest.mark.parametrize("n", [257, 1000])
def test_same_sequence_twice_gives_identical_bits_and_sparse_sums_are_exact(n):
    trace = make_trace(n, 3)
    a, ref = run_trace(n, 100, None, trace, "first", every_step=False)
    b, _ = run_trace(n, 100, None, trace, "second", every_step=False)
    ta, tb = a.totals(), b.totals()
    assert ta == tb and F64(ta["return_sum"]).view(np.uint64) == F64(tb["return_sum"]).view(np.uint64)
    assert F64(ta["speed_sum_success"]).view(np.uint64) == F64(tb["speed_sum_success"]).view(np.uint64)
    ea, eb = a.episodes(), b.episodes()
    for k in ea:
        assert_same(ea[k], eb[k], k)
    a.close()
    b.close()
    # sparse rewards: the returns are integers, any order gives the same sum
    c, cref = run_trace(n, 100, None, make_trace(n, 4, sparse=True), "sparse", integer_returns=True, every_step=False)
    assert c.totals()["return_sum"] == cref.tot["return_sum"] and float(cref.tot["return_sum"]).is_integer()
    assert cref.tot["return_sum"] < 0
    c.close()


def test_masked_reset_and_clear():
    n, window = 257, 100
    trace = make_trace(n, 11)
    tg = (np.arange(n) % 3 + 1).astype(np.int32)
    mon = M.EpisodeMonitor(n, OD, window=window, device="cuda:0")
    ref = RefMonitor(n, window, targets=tg)
    mon.set_targets(tg)
    for s in trace[:3]:
        mon.step_arrays(**s)
        ref.step(**s)
    mask = (np.random.default_rng(0).random(n) < 0.4).astype(np.uint8)
    before = mon.env_state()
    mon.reset_arrays(mask)
    ref.reset(mask)
    after = mon.env_state()
    keep = mask == 0
    assert (before["len"][~keep] > 0).any() and (before["len"][keep] > 0).any()   # abandoned: exactly the masked
    for k in ("ret", "len", "speed"):
        assert_same(after[k][keep], before[k][keep], f"unmasked {k}")
        assert not after[k][~keep].any()
    assert_same(after["ep_count"], before["ep_count"], "ep_count")
    assert_state(mon, ref, "after masked reset")
    for t, s in enumerate(trace[3:7]):
        mon.step_arrays(**s)
        ref.step(**s)
        assert_state(mon, ref, f"after masked reset, step {t}")
    mon.reset_arrays(None)   # all
    ref.reset(None)
    assert_state(mon, ref, "after full reset")
    # clear: the state at create (the targets stay), and it runs on from there like a new handle
    mon.clear()
    fresh = RefMonitor(n, window, targets=tg)
    assert_state(mon, fresh, "after clear")
    t = mon.totals()
    assert t["episodes"] == 0 and t["steps"] == 0 and t["return_sum"] == 0.0 and t["envs_open"] == n
    assert len(mon.episodes()["r"]) == 0
    for i, s in enumerate(trace[7:]):
        mon.step_arrays(**s)
        fresh.step(**s)
        assert_state(mon, fresh, f"after clear, step {i}")
    mon.set_targets(None)
    assert mon.totals()["envs_open"] == n
    assert len(mon.episodes(max_records=3)["r"]) == 3   # the newest three
    assert_same(mon.episodes(max_records=3)["env"], fresh.episodes()["env"][-3:], "newest three")
    mon.close()


# ------------------------------------------------------------------ with envs
@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    return pg


def _raw(env):
    torch.cuda.synchronize()
    c = lambda t: t.cpu().numpy().copy()  # noqa: E731
    return dict(reward=c(env.reward), success=c(env.success), terminated=c(env.terminated), truncated=c(env.truncated),
                obs=c(env.obs), terminal_obs=c(env.terminal_obs), task_truncated=c(env.task_trunc),
                nonfinite=c(env.nonfinite_t))


def _assert_env_equal(a, b, what):
    """Every step output of env ``a`` bit for bit env ``b``'s."""
    for k in ("obs", "achieved_goal", "desired_goal", "reward", "success", "terminated", "truncated", "task_trunc"):
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
    done = (b.terminated | b.truncated).bool()
    for k in ("terminal_obs", "terminal_ag", "terminal_dg"):
        assert torch.equal(getattr(a, k)[done], getattr(b, k)[done]), (what, k)


@pytest.mark.parametrize("env_id", ["PandaReach-v3", "PandaReachDense-v3"])
def test_tensor_path(pg, env_id):
    """257 envs, 4-step episodes staggered by a masked reset after two steps, 10 steps: records and
    totals against the restatement fed the bare env's outputs; the monitored env bit for bit the bare one."""
    n = 257
    kw = dict(num_envs=n, device="cuda:0", seed=3, max_episode_steps=4)
    bare, inner = pg.PandaVecEnv(env_id, **kw), pg.PandaVecEnv(env_id, **kw)
    vm = pg.VecMonitor(inner, window=100)
    ref = RefMonitor(n, 100)
    assert vm.num_envs == n and vm.obs_dim == 6 and vm.action_dim == 3   # forwarded
    bare.reset_tensors()
    o = vm.reset_tensors()
    assert o["observation"].data_ptr() == inner.obs.data_ptr()
    sparse = env_id == "PandaReach-v3"
    episodes = 0
    for t in range(10):
        if t == 2:
            mask = (torch.arange(n, device="cuda:0") % 2 == 0)
            bare.reset_tensors(mask=mask)
            vm.reset_tensors(mask=mask)
            ref.reset(mask.cpu().numpy())
        a = bare.sample_actions(t).clone()
        bare.step_tensors(a)
        out = vm.step_tensors(a)
        _assert_env_equal(inner, bare, f"{env_id} step {t}")
        assert out[1].data_ptr() == inner.reward.data_ptr() and out[0]["observation"].data_ptr() == inner.obs.data_ptr()
        raw = _raw(bare)
        r, l, done = ref.step(**raw)
        episodes += int(done.sum())
        assert_same(vm.ep_r.cpu().numpy()[done], r[done], f"{env_id} step {t} ep_r")
        assert_same(vm.ep_l.cpu().numpy()[done], l[done], f"{env_id} step {t} ep_l")
        assert_state(vm, ref, f"{env_id} step {t}", integer_returns=sparse)
    assert episodes == ref.tot["episodes"] >= 2 * n and set(ref.episodes()["l"].tolist()) <= {2, 4}
    assert ref.tot["speed_sum_success"] >= 0.0 and (ref.speed > 0).any()
    ws = vm.window_stats()
    eps = ref.episodes()
    assert ws["ep_rew_mean"] == float(np.mean(eps["r"].astype(F64))) and ws["ep_len_mean"] == float(np.mean(eps["l"]))
    assert ws["success_rate"] == float(np.mean(eps["outcome"] == 1))
    sv = vm.stats_vector()
    assert sv.tolist() == [ref.tot["episodes"], ref.tot["outcomes"][1], vm.totals()["return_sum"], ref.tot["length_sum"]]
    assert pg.VecMonitor.combine(np.stack([sv, sv]))["episodes"] == 2 * ref.tot["episodes"]
    bare.close()
    vm.close()


def test_tensor_path_over_vecnormalize(pg):
    """VecMonitor(VecNormalize(env)): the returns recorded are the raw ones, what comes back is
    VecNormalize's own output bit for bit."""
    n = 257
    kw = dict(num_envs=n, device="cuda:0", seed=4, max_episode_steps=4)
    bare = pg.PandaVecEnv("PandaReachDense-v3", **kw)
    alone = pg.VecNormalize(pg.PandaVecEnv("PandaReachDense-v3", **kw))
    vm = pg.VecMonitor(pg.VecNormalize(pg.PandaVecEnv("PandaReachDense-v3", **kw)), window=100)
    ref = RefMonitor(n, 100)
    bare.reset_tensors()
    oa, ov = alone.reset_tensors(), vm.reset_tensors()
    for k in oa:
        assert torch.equal(oa[k], ov[k]), k
    with pytest.raises(ValueError, match="mask"):
        vm.reset_tensors(mask=torch.ones(n, dtype=torch.uint8, device="cuda:0"))
    for t in range(10):
        a = bare.sample_actions(t).clone()
        bare.step_tensors(a)
        xa, xv = alone.step_tensors(a), vm.step_tensors(a)
        for k in xa[0]:
            assert torch.equal(xa[0][k], xv[0][k]), (t, k)
        for i in range(1, 5):
            assert torch.equal(xa[i], xv[i]), (t, i)
        assert not torch.equal(xv[1], bare.reward)   # normalised rewards came back ...
        r, l, done = ref.step(**_raw(bare))          # ... and raw ones were recorded
        assert_same(vm.ep_r.cpu().numpy()[done], r[done], f"step {t} ep_r")
        assert_state(vm, ref, f"over VecNormalize step {t}")
    for x, y in zip(alone.get_stats(), vm.get_stats()):   # forwarded; the statistics moved alike
        assert np.array_equal(x, y)
    assert ref.tot["episodes"] == 2 * n
    bare.close()
    alone.close()
    vm.close()


def test_reach_ao_runs_and_outcomes_add_up(pg):
    n = 64
    vm = pg.VecMonitor(pg.PandaVecEnv("PandaReachAO-v3", num_envs=n, device="cuda:0", seed=2, max_episode_steps=2))
    vm.reset_tensors()
    for t in range(5):
        vm.step_tensors(vm.sample_actions(t))
    t = vm.totals()
    assert t["steps"] == 5 and t["episodes"] >= 2 * n and sum(t["outcomes"]) == t["episodes"]
    assert t["outcomes"][abi.EP_NONFINITE] == 0 and np.isfinite(t["return_sum"])
    eps = vm.episodes()
    assert len(eps["r"]) == 100 and (np.diff(eps["step"]) >= 0).all()
    vm.close()


def test_auto_reset_false_is_rejected(pg):
    env = pg.PandaVecEnv("PandaReach-v3", num_envs=8, device="cuda:0", auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset"):
        pg.VecMonitor(env)
    env.close()


def test_sb3_path(pg):
    """8 envs, 3-step episodes, 7 steps: infos[i]["episode"] at steps 3 and 6 exactly, l == 3, r the
    f32 running sum of the env's rewards, t non-decreasing; everything else the bare env's."""
    n = 8
    kw = dict(num_envs=n, device="cuda:0", seed=5, max_episode_steps=3)
    bare = pg.PandaVecEnv("PandaReach-v3", **kw)
    vm = pg.VecMonitor(pg.PandaVecEnv("PandaReach-v3", **kw), info_keywords=("is_success",))
    bare.seed(5)
    vm.seed(5)
    ob, ov = bare.reset(), vm.reset()
    for k in ob:
        assert np.array_equal(ob[k], ov[k])
    rng = np.random.default_rng(0)
    run = np.zeros(n, F32)
    last_t = 0.0
    for step in range(1, 8):
        a = rng.uniform(-1, 1, (n, 3)).astype(F32)
        obs, reward, done, infos = bare.step(a)
        o, r, d, winfos = vm.step(a)
        for k in obs:
            assert_same(o[k], obs[k], f"obs {k}")
        assert_same(r, reward, "reward")
        assert np.array_equal(d, done) and done.all() == (step in (3, 6)) and done.any() == (step in (3, 6))
        run = run + reward
        for i in range(n):
            a_i, b_i = dict(infos[i]), dict(winfos[i])
            ep = b_i.pop("episode", None)
            assert (ep is not None) == (step in (3, 6)), (step, i)
            ta, tb = a_i.pop("terminal_observation", None), b_i.pop("terminal_observation", None)
            assert a_i == b_i, (step, i)
            assert (ta is None) == (tb is None)
            if ta is not None:
                for k in ta:
                    assert_same(tb[k], ta[k], f"terminal {k}")
            if ep is not None:
                assert set(ep) == {"r", "l", "t", "is_success"} and ep["l"] == 3 and type(ep["l"]) is int
                assert type(ep["r"]) is float and F32(ep["r"]) == run[i] and ep["is_success"] == a_i["is_success"]
                assert ep["t"] >= last_t >= 0.0
                last_t = ep["t"]
        if step in (3, 6):
            run[:] = 0
    assert vm.totals()["episodes"] == 2 * n and vm.totals()["steps"] == 7
    assert vm._base._pre_sync is None   # the hook is set for the wrapper's own step_wait only
    bare.close()
    vm.close()


@pytest.mark.parametrize("k,replays", [(3, 2), (1, 4)])
def test_captured_steps_equal_eager_steps(pg, k, replays):
    """capture_steps(k) replayed `replays` times leaves ring, totals and accumulators bit-equal to the
    same k * replays steps run eagerly; k = 1 is the odd length a parity scheme could get wrong."""
    n = 64
    kw = dict(num_envs=n, device="cuda:0", seed=9, max_episode_steps=2)
    eager = pg.VecMonitor(pg.PandaVecEnv("PandaReachDense-v3", **kw), window=100)
    graphed = pg.VecMonitor(pg.PandaVecEnv("PandaReachDense-v3", **kw), window=100)
    eager.reset_tensors(seed=9)
    graphed.reset_tensors(seed=9)
    acts = torch.empty((k, n, 3), device="cuda:0")
    for i in range(k):
        acts[i].copy_(eager.sample_actions(i))
    g = graphed.capture_steps(k, acts)
    assert graphed.totals()["steps"] == 0   # capture runs nothing
    for rep in range(replays):
        for i in range(k):
            eager.step_tensors(acts[i])
        g.replay()
        torch.cuda.synchronize()
        ta, tb = eager.totals(), graphed.totals()
        assert ta == tb, (rep, ta, tb)
        assert F64(ta["return_sum"]).view(np.uint64) == F64(tb["return_sum"]).view(np.uint64)
        ea, eb = eager.episodes(), graphed.episodes()
        sa, sb = eager.env_state(), graphed.env_state()
        for key in ea:
            assert_same(eb[key], ea[key], f"replay {rep} ring {key}")
        for key in sa:
            assert_same(sb[key], sa[key], f"replay {rep} {key}")
        assert torch.equal(eager.ep_r, graphed.ep_r) and torch.equal(eager.ep_l, graphed.ep_l)
    t = eager.totals()
    assert t["steps"] == k * replays and t["episodes"] == n * (k * replays // 2) > 0
    eager.close()
    graphed.close()


def test_captured_steps_over_vecnormalize(pg):
    n, k = 64, 2
    kw = dict(num_envs=n, device="cuda:0", seed=6, max_episode_steps=2)
    eager = pg.VecMonitor(pg.VecNormalize(pg.PandaVecEnv("PandaReachDense-v3", **kw)))
    graphed = pg.VecMonitor(pg.VecNormalize(pg.PandaVecEnv("PandaReachDense-v3", **kw)))
    eager.reset_tensors(seed=6)
    graphed.reset_tensors(seed=6)
    acts = torch.empty((k, n, 3), device="cuda:0")
    for i in range(k):
        acts[i].copy_(eager.sample_actions(i))
    g = graphed.capture_steps(k, acts)
    for rep in range(2):
        for i in range(k):
            eager.step_tensors(acts[i])
        g.replay()
        torch.cuda.synchronize()
    assert eager.totals() == graphed.totals() and eager.totals()["episodes"] == 2 * n
    for x, y in zip(eager.get_stats(), graphed.get_stats()):
        assert np.array_equal(x, y)
    assert torch.equal(eager.venv._n["reward"], graphed.venv._n["reward"])
    eager.close()
    graphed.close()


def test_her_add_from_monitored_env_stores_the_bare_envs_rows(pg):
    from panda_gym_amd.her import HerReplayBuffer

    n = 64
    kw = dict(num_envs=n, device="cuda:0", seed=1, max_episode_steps=5)
    bare = pg.PandaVecEnv("PandaReach-v3", **kw)
    vm = pg.VecMonitor(pg.PandaVecEnv("PandaReach-v3", **kw))
    bufs = [HerReplayBuffer(100 * n, env=e, device="cuda:0", seed=2) for e in (bare, vm)]
    bare.reset_tensors()
    vm.reset_tensors()
    for t in range(12):
        a = bare.sample_actions(t).clone()
        o_b = {k: v.clone() for k, v in bare._obs_dict().items()}
        o_v = {k: v.clone() for k, v in vm._obs_dict().items()}
        bare.step_tensors(a)
        vm.step_tensors(a)
        bufs[0].add_from_vec_env(bare, o_b, a)
        bufs[1].add_from_vec_env(vm, o_v, a)
    x, y = bufs[0].sample_raw(2048, draw=0), bufs[1].sample_raw(2048, draw=0)
    for k in ("rows", "slot", "env", "goal_slot"):
        assert torch.equal(x[k], y[k]), k
    for a_, b_ in zip(bufs[0]._arrays(), bufs[1]._arrays()):
        assert torch.equal(a_, b_)
    assert vm.totals()["episodes"] == 2 * n
    for b in bufs:
        b.close()
    bare.close()
    vm.close()


@pytest.mark.parametrize("kind", ["random", "seek"])
def test_evaluate_fills_the_quota_and_matches_the_restatement(pg, kind):
    """8 envs, 20 episodes of 3 steps, a fixed random policy: per-env counts are evaluate_policy's
    targets, and every result key equals the restatement run over the same steps of a bare env.
    "seek" repeats it with a policy that heads for the goal, so that the keys over successful
    episodes (length, sim steps, EE speed) are numbers and not nan."""
    n, episodes = 8, 20
    kw = dict(num_envs=n, device="cuda:0", seed=12, max_episode_steps=3)
    env, bare = pg.PandaVecEnv("PandaReach-v3", **kw), pg.PandaVecEnv("PandaReach-v3", **kw)
    noise = torch.as_tensor(np.random.default_rng(5).uniform(-1, 1, (64, n, 3)).astype(F32), device="cuda:0")
    calls, acts = [], []

    def policy(obs, deterministic=False):
        assert deterministic is True and obs["observation"].shape == (n, 6) and obs["observation"].is_cuda
        a = noise[len(calls)]
        if kind == "seek":   # the EE moves 0.05 * action per step
            a = ((obs["desired_goal"] - obs["achieved_goal"]) / 0.05).clamp(-1, 1).contiguous()
        calls.append(1)
        acts.append(a.clone())
        return a

    res, eps = pg.evaluate(env, policy, episodes, return_episodes=True)
    if kind == "seek":
        assert res["success_rate"] > 0 and np.isfinite(res["mean_ee_speed"]) and res["mean_ee_speed"] > 0
    targets = np.array([(episodes + i) // n for i in range(n)])
    assert res["num_episodes"] == episodes and len(eps["r"]) == episodes
    assert np.array_equal(np.bincount(eps["env"], minlength=n), targets)
    assert 9 <= len(calls) <= 16 and len(calls) % 8 == 0   # 3 episodes of 3 steps, looked at every 8 steps
    ref = RefMonitor(n, episodes, targets=targets)
    bare.reset_tensors()
    for t in range(len(calls)):
        bare.step_tensors(acts[t])
        ref.step(**_raw(bare))
    assert np.array_equal(ref.ep_count, targets) and ref.tot["envs_open"] == 0
    want = ref_evaluation(list(ref.ring), 20)
    assert set(res) == set(want)
    for k in want:
        print(f"evaluate {k}: {res[k]!r} restatement {want[k]!r}")
        assert res[k] == want[k] or (np.isnan(res[k]) and np.isnan(want[k])), (k, res[k], want[k])
    for k in ("r", "l", "env", "outcome", "step", "speed_sum"):
        assert_same(eps[k], ref.episodes()[k], f"evaluate ring {k}")
    assert res["mean_ep_length"] == 3.0 and res["mean_num_sim_steps"] == 60.0
    assert res["success_rate"] + res["collision_rate"] + res["timeout_rate"] + res["nonfinite_rate"] == pytest.approx(1)
    assert env.step_tensors(acts[0])[1].shape == (n,)   # the env is the caller's: still open
    env.close()
    bare.close()
