"""GPU: the per-env non-finite guard (PandaVecEnv(nonfinite=...), pgx_config.nonfinite_guard;
DESIGN.md section 4).  A NaN / inf is injected into one env through the writable state views
(``q``, ``qd``, ``object`` only) between two steps:

* with the guard off the env writes non-finite observations and nothing says so (what the guard
  is for; the default, unchanged);
* with it on, the step that would have stored the non-finite state flags the env, reports a fixed
  finite step and resets the env exactly as a time-limit truncation at that step would have (a twin
  handle truncated by its TimeLimit in the same step is the reference, bit for bit), and no other
  env of the batch differs by a bit, then or in the steps after;
* envs that stay finite never see the guard: a guarded and an unguarded handle agree bit for bit.

A NaN joint velocity does not survive a step as a NaN (the velocity clamp's fminf / fmaxf turn it
into +-max_coord_vel), so the guard checks the state a step loads as well as the state it stores;
``test_off_launders_a_nan_velocity`` pins that behaviour of the unguarded step.

One deviation from "the same reset as a truncation": that reset keeps the cube's velocity
(resetBasePositionAndOrientation), and a caught env's is not fit to keep, so the guard zeroes it.
The twin's cube velocity is therefore set to zero too (an ``object`` write of that one env) before
the rollouts are compared further; every other row is compared as it comes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import panda_gym_amd as pg  # noqa: E402
from panda_gym_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

N, J, SEED = 64, 37, 11   # env J: lane 37 of the one-lane wave, row 1 of wave 9 in the 16-lane layout
NAN, INF = float("nan"), float("inf")

CONFIGS = {
    "reach_narrow": ("PandaReach-v3", dict(lanes_per_env=1)),
    "reach_wide": ("PandaReach-v3", dict(lanes_per_env=16)),
    "push": ("PandaPush-v3", dict(lanes_per_env=16, full_manifold=True)),
    "reach_ao": ("PandaReachAO-v3", dict()),
}
OUTPUTS = ("obs", "achieved_goal", "desired_goal", "reward", "success", "terminated", "truncated", "task_trunc")
TERMINAL = ("terminal_obs", "terminal_ag", "terminal_dg")
STATE = ("q", "qd", "qc", "goal", "object", "elapsed", "episode")


def _make(cfg, nonfinite="off", n=N, **kw):
    env_id, base = CONFIGS[cfg]
    v = pg.PandaVecEnv(env_id, num_envs=n, device="cuda:0", seed=SEED, nonfinite=nonfinite, **{**base, **kw})
    v.reset_tensors(seed=SEED)
    return v


def _errors(v) -> int:
    return int(v.state()["errors"].item())


def _assert_same(a, b, what, terminal="all"):
    """Every output and state row of the two handles, bit for bit; ``terminal="done"``: the terminal
    rows only of the envs that finished in this step (the others' are left from earlier steps)."""
    for k in OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
    done = (a.terminated | a.truncated).bool()
    for k in TERMINAL:
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x, y) if terminal == "all" else torch.equal(x[done], y[done]), (what, k)
    sa, sb = a.state(), b.state()
    for k in STATE:
        assert torch.equal(sa[k], sb[k]), (what, k)
    assert torch.equal(sa["contacts"], sb["contacts"]), (what, "contacts")
    if "manifolds" in sa:
        assert torch.equal(sa["manifolds"][0], sb["manifolds"][0]), (what, "manifold count")
    if "obstacles" in sa:
        assert torch.equal(sa["obstacles"], sb["obstacles"]), (what, "obstacles")


# ------------------------------------------------------------------ 1: invisible to finite envs
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_guard_is_invisible_to_finite_envs(cfg):
    a, b = _make(cfg, "reset"), _make(cfg, "off")
    try:
        assert a._cfg.nonfinite_guard == 1 and b._cfg.nonfinite_guard == 0
        for t in range(30):
            act = a.sample_actions(t)
            a.step_tensors(act)
            b.step_tensors(act)
            _assert_same(a, b, (cfg, t))
            assert not a.nonfinite().any() and not b.nonfinite().any()
        assert "_nf<" in a.step_kernel() and "_nf<" not in b.step_kernel()
        assert _errors(a) == 0 and _errors(b) == 0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 2, 3: catch, report, reset
def _catch_report_reset(cfg, key, row, value, n=N, j=J, **kw):
    a, b = _make(cfg, "reset", n=n, **kw), _make(cfg, "off", n=n, **kw)
    try:
        T = a.spec.max_episode_steps
        for t in range(5):
            act = a.sample_actions(t)
            a.step_tensors(act)
            b.step_tensors(act)
        _assert_same(a, b, (cfg, "before"))
        a.state()[key][row, j] = value
        b.state()["elapsed"][j] = T - 1   # the twin's env j truncates, and auto-resets, in the same step
        act = a.sample_actions(5)
        a.step_tensors(act)
        b.step_tensors(act)
        # ---- the flagged step
        mask = a.nonfinite()
        assert mask[j] and mask.sum() == 1, np.flatnonzero(mask)
        assert torch.equal(a.nonfinite_t.bool().cpu(), torch.as_tensor(mask))
        assert _errors(a) == abi.ERR_NONFINITE and _errors(b) == 0
        assert int(a.truncated[j]) == 1 and int(a.terminated[j]) == 0 and int(a.success[j]) == 0
        assert float(a.reward[j]) == 0.0 and int(a.task_trunc[j]) == 0
        assert torch.equal(a.terminal_obs[j], a.obs[j])
        assert torch.equal(a.terminal_ag[j], a.achieved_goal[j])
        assert torch.equal(a.terminal_dg[j], a.desired_goal[j])
        for k in OUTPUTS[:4] + TERMINAL:
            assert bool(torch.isfinite(getattr(a, k)).all()), k
        # ---- env j was reset as the twin's TimeLimit reset it
        sa, sb = a.state(), b.state()
        for k in STATE:
            x, y = sa[k][..., j], sb[k][..., j]
            assert bool(torch.isfinite(x.double()).all()), k
            if k == "object" and a.spec.task != abi.TASK_REACH and a.spec.task != abi.TASK_REACH_AO:
                # (the module docstring: the guard's reset does not keep the cube's velocity)
                assert torch.equal(x[:7], y[:7]), k
                assert bool((x[7:] == 0).all()) and bool(torch.isfinite(y[7:]).all()), k
                sb["object"][7:, j] = 0.0
            else:
                assert torch.equal(x, y), (k, x, y)
        assert int(sa["elapsed"][j]) == 0
        assert torch.equal(sa["contacts"][:, j], sb["contacts"][:, j])
        if "manifolds" in sa:
            assert torch.equal(sa["manifolds"][0, j], sb["manifolds"][0, j]) and float(sa["manifolds"][0, j]) == 0.0
        if "obstacles" in sa:
            assert torch.equal(sa["obstacles"][:, j], sb["obstacles"][:, j])
        if a.reset_rng == "pcg64":   # the reset drew from env j's stream, as the twin's
            assert np.array_equal(a.rng_streams(), b.rng_streams())
        # ---- every other env: untouched, in this step ...
        others = torch.ones(n, dtype=torch.bool, device=a.device)
        others[j] = False
        for k in OUTPUTS:
            assert torch.equal(getattr(a, k)[others], getattr(b, k)[others]), k
        # ---- ... and, with env j, in the steps after
        a.state()["errors"].zero_()
        for t in range(6, 26):
            act = a.sample_actions(t)
            a.step_tensors(act)
            b.step_tensors(act)
            _assert_same(a, b, (cfg, key, t), terminal="done")
            assert not a.nonfinite().any()
        assert _errors(a) == 0
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_catch_report_reset_qd_nan(cfg):
    _catch_report_reset(cfg, "qd", 3, NAN)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_catch_report_reset_q_inf(cfg):
    _catch_report_reset(cfg, "q", 0, INF)


@pytest.mark.parametrize("row,value", [(7, NAN), (0, INF)], ids=["linvel_nan", "pos_inf"])
def test_catch_report_reset_object(row, value):
    _catch_report_reset("push", "object", row, value)


def test_catch_report_reset_pcg64_stream():
    _catch_report_reset("reach_wide", "qd", 3, NAN, reset_rng="pcg64")


def test_catch_report_reset_with_env_order():
    """1024 envs: the heavy-first env order runs (pgx_launch_step_arm); env j in the second XCD's
    range of envs (128 per XCD at this size)."""
    _catch_report_reset("reach_wide", "qd", 3, NAN, n=1024, j=128 + 69, full_manifold=True)


# ------------------------------------------------------------------ 4: off is today
@pytest.mark.parametrize("cfg,key,row,value", [("reach_wide", "q", 0, INF), ("reach_narrow", "q", 0, INF),
                                               ("push", "object", 7, NAN), ("push", "object", 0, INF)])
def test_off_lets_the_nan_through(cfg, key, row, value):
    """The default: nothing flags the env, and its observation is non-finite."""
    v = _make(cfg, "off")
    try:
        for t in range(5):
            v.step_tensors(v.sample_actions(t))
        v.state()[key][row, J] = value
        v.step_tensors(v.sample_actions(5))
        assert _errors(v) == 0 and not v.nonfinite().any()
        assert not bool(torch.isfinite(v.obs[J]).all())
        assert not bool(torch.isfinite(v.state()[key][:, J]).all())
        others = torch.ones(N, dtype=torch.bool, device=v.device)
        others[J] = False
        assert bool(torch.isfinite(v.obs[others]).all())
        v.raise_device_errors()   # nothing to raise
    finally:
        v.close()


@pytest.mark.parametrize("cfg", ["reach_wide", "push"])
def test_off_launders_a_nan_velocity(cfg):
    """The default with a NaN joint velocity: the substeps clamp the joint velocities to
    +-max_coord_vel with fminf / fmaxf, which return the other operand for a NaN, so the env's state
    and observation come out finite -- and wrong (every joint driven at the clamp), with nothing said.
    This is why the guard also checks what a step loads (test_catch_report_reset_qd_nan): the
    epilogue's values alone would pass."""
    v, twin = _make(cfg, "off"), _make(cfg, "off")
    try:
        for t in range(5):
            act = v.sample_actions(t)
            v.step_tensors(act)
            twin.step_tensors(act)
        v.state()["qd"][3, J] = NAN
        act = v.sample_actions(5)
        v.step_tensors(act)
        twin.step_tensors(act)
        assert _errors(v) == 0 and not v.nonfinite().any()
        assert bool(torch.isfinite(v.obs).all()) and bool(torch.isfinite(v.state()["q"]).all())
        assert not torch.equal(v.state()["q"][:, J], twin.state()["q"][:, J])
        others = torch.ones(N, dtype=torch.bool, device=v.device)
        others[J] = False
        assert torch.equal(v.obs[others], twin.obs[others])
    finally:
        v.close()
        twin.close()


# ------------------------------------------------------------------ 5: host surface
def _host_env(mode):
    v = pg.PandaVecEnv("PandaReach-v3", num_envs=N, device="cuda:0", seed=SEED, nonfinite=mode)
    v.reset(seed=SEED)
    rng = np.random.default_rng(0)
    acts = rng.uniform(-1, 1, (3, N, v.action_dim)).astype(np.float32)
    for t in range(2):
        _, _, _, infos = v.step(acts[t])
        assert all("nonfinite" not in i for i in infos)
    v.state()["qd"][3, J] = NAN
    return v, acts[2]


def test_step_wait_reset_mode_marks_infos():
    v, act = _host_env("reset")
    try:
        obs, rew, done, infos = v.step(act)
        assert [i for i, info in enumerate(infos) if info.get("nonfinite")] == [J]
        info = infos[J]
        assert info["nonfinite"] is True and info["TimeLimit.truncated"] is True and info["is_success"] is False
        assert done[J] and rew[J] == 0.0
        for k, x in info["terminal_observation"].items():
            assert np.isfinite(x).all() and np.array_equal(x, obs[k][J]), k
        assert all(np.isfinite(x).all() for x in obs.values()) and np.isfinite(rew).all()
        assert v.nonfinite_resets == 1 and _errors(v) == 0
        _, _, _, infos = v.step(act)
        assert all("nonfinite" not in i for i in infos) and v.nonfinite_resets == 1
    finally:
        v.close()


def test_step_wait_raise_mode_names_the_env():
    v, act = _host_env("raise")
    try:
        with pytest.raises(pg.envs.PgxError, match=rf"PGX_ERR_NONFINITE.*\b{J}\b"):
            v.step(act)
        assert _errors(v) == 0   # raised and cleared; the device reset the env all the same
        assert bool(torch.isfinite(v.state()["q"]).all()) and bool(torch.isfinite(v.obs).all())
        v.step(act)              # and the batch goes on
    finally:
        v.close()


def test_raise_device_errors_on_the_device_path():
    """step_tensors never looks; raise_device_errors does: silent in "reset", raising in "raise"."""
    for mode in ("reset", "raise"):
        v = _make("reach_wide", mode)
        try:
            v.step_tensors(v.sample_actions(0))
            v.state()["q"][0, J] = INF
            v.step_tensors(v.sample_actions(1))
            if mode == "reset":
                v.raise_device_errors()
            else:
                with pytest.raises(pg.envs.PgxError, match=rf"\b{J}\b"):
                    v.raise_device_errors()
            assert v.nonfinite_resets == 1 and _errors(v) == 0
        finally:
            v.close()


@pytest.mark.parametrize("mode", ["raise", "reset"])
def test_single_env_facade(mode):
    env = pg.PandaEnv("PandaReach-v3", device="cuda:0", seed=3, nonfinite=mode)
    try:
        env.reset(seed=3)
        a = np.full(3, 0.25, dtype=np.float32)
        _, _, _, truncated, info = env.step(a)
        assert not truncated and "nonfinite" not in info
        env._vec.state()["qd"][3, 0] = NAN
        if mode == "raise":
            with pytest.raises(pg.envs.PgxError, match="PGX_ERR_NONFINITE"):
                env.step(a)
        else:
            _, r, terminated, truncated, info = env.step(a)
            assert truncated and not terminated and r == 0.0 and info["nonfinite"] is True
            assert info["is_success"] is False
        obs, _ = env.reset(seed=4)   # the caller resets: finite again
        assert all(np.isfinite(x).all() for x in obs.values())
        obs, r, _, truncated, info = env.step(a)
        assert all(np.isfinite(x).all() for x in obs.values()) and not truncated and "nonfinite" not in info
    finally:
        env.close()


def test_captured_steps_keep_the_sticky_bit():
    v = _make("reach_wide", "reset")
    try:
        v.step_tensors(v.sample_actions(0))
        g = v.capture_steps(4)
        ep0 = int(v.state()["episode"][J])
        v.state()["qd"][3, J] = NAN
        g.replay()
        torch.cuda.synchronize()
        assert _errors(v) == abi.ERR_NONFINITE   # caught in the first of the four: the word is sticky
        assert not v.nonfinite().any()           # (the mask is the last step's)
        st = v.state()
        for k in ("q", "qd", "qc", "goal"):
            assert bool(torch.isfinite(st[k]).all()), k
        assert bool(torch.isfinite(v.obs).all()) and bool(torch.isfinite(v.reward).all())
        assert int(st["elapsed"][J]) == 3 and int(st["episode"][J]) == ep0 + 1
        v.raise_device_errors()
        assert _errors(v) == 0
    finally:
        v.close()


# ------------------------------------------------------------------ 6: no auto-reset
def _same_nan_aware(x, y):
    return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))


@pytest.mark.parametrize("cfg,key,row,value", [("reach_narrow", "qd", 3, NAN), ("reach_wide", "q", 0, INF),
                                               ("push", "object", 7, NAN)])
def test_no_auto_reset_handle_flags_and_keeps_state(cfg, key, row, value):
    """auto_reset=False: flag, bit and the fixed step as ever, the env's state as the physics left it
    (the same rows as an unguarded handle's with the same injection), and the host's reset brings
    it back."""
    a, b = _make(cfg, "reset", auto_reset=False), _make(cfg, "off", auto_reset=False)
    try:
        for t in range(3):
            act = a.sample_actions(t)
            a.step_tensors(act)
            b.step_tensors(act)
        for v in (a, b):
            v.state()[key][row, J] = value
        act = a.sample_actions(3)
        a.step_tensors(act)
        b.step_tensors(act)
        mask = a.nonfinite()
        assert mask[J] and mask.sum() == 1 and _errors(a) == abi.ERR_NONFINITE and _errors(b) == 0
        assert int(a.truncated[J]) == 1 and int(a.terminated[J]) == 0 and int(a.success[J]) == 0
        assert float(a.reward[J]) == 0.0
        sa, sb = a.state(), b.state()
        for k in STATE:
            assert _same_nan_aware(sa[k].double(), sb[k].double()), k
        assert int(sa["elapsed"][J]) == 4 and torch.equal(sa["episode"], sb["episode"])
        if key != "qd":   # (a NaN joint velocity leaves the step as the finite clamp value, see above)
            assert not bool(torch.isfinite(sa[key][:, J]).all())
        m = torch.zeros(N, dtype=torch.bool, device=a.device)
        m[J] = True
        a.state()["errors"].zero_()
        a.reset_tensors(mask=m)
        sa = a.state()
        for k in ("q", "qd", "qc", "goal", "object"):
            assert bool(torch.isfinite(sa[k]).all()), k
        assert bool(torch.isfinite(a.obs).all()) and int(sa["elapsed"][J]) == 0
        a.step_tensors(a.sample_actions(4))
        assert not a.nonfinite().any() and _errors(a) == 0 and bool(torch.isfinite(a.obs).all())
    finally:
        a.close()
        b.close()
