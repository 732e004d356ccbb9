"""GPU tests of the critic update (pgx_quantile_critic.hip: qc_grad_rows_kernel, qc_wgrad_kernel, the Adam
kernels): the loss, every gradient tensor and the debug planes (quantiles, dq, each hidden layer's dZ) against
the library's host model bit for bit over both row tiles with tails, head widths of one and two tiles, padded
widths, dense, strided, subnormal and -0 inputs; the entry's quantiles against critic(); a HER batch read in
place; three Adam steps (parameters, exp_avg, exp_avg_sq, step) against the host model in every bit; the
captured update sample_into -> action_log_prob_rows -> td_target_rows -> critic_loss_backward_rows ->
adam_step -> polyak_update replayed after everything it reads has changed; and containment (canaries, rows
past B, refusals that launch nothing, a NaN row).  The host models are pinned without a GPU in
test_critic_update_abi.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import panda_gym_amd as pg
from panda_gym_amd import abi
from test_action_log_prob_abi import make_gaussian
from test_actor_abi import bits
from test_critic_update_abi import grad_batch, online
from test_quantile_critic_abi import make_qc, n_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CANARY = 12345.0
PAD = 64


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def guarded(n):
    """n f32 between PAD canary floats on each side: (the whole, the view)."""
    flat = torch.full((2 * PAD + n,), CANARY, dtype=torch.float32, device=DEV)
    return flat, flat[PAD:PAD + n]


def intact(flat, n):
    f = host(flat)
    return bool((f[:PAD] == CANARY).all() and (f[PAD + n:] == CANARY).all())


class Run:
    """One critic_loss_backward with the workspace, the loss and the debug planes (two rows more than B)
    between canaries."""

    def __init__(self, qc, obs, act, tq, B, spare=2):
        self.B, self.need = B, qc.workspace_floats(B)
        self.fw, ws = guarded(self.need)
        self.fl, loss = guarded(1)
        widths = {"quantiles": qc.n_pool, "dq": qc.n_pool, "dz": qc.n_critics * sum(qc.net_arch)}
        self.fd = {k: guarded((B + spare) * w) for k, w in widths.items()}
        debug = {k: v[1].view(B + spare, widths[k]) for k, v in self.fd.items()}
        self.widths, self.spare = widths, spare
        out = qc.critic_loss_backward(obs, act, tq, ws, loss=loss, debug=debug)
        assert out.dim() == 0 and out.data_ptr() == loss.data_ptr()
        torch.cuda.synchronize()
        self.loss = host(loss)[0]
        self.planes = {k: host(v)[:B] for k, v in debug.items()}
        self.tails = {k: host(v)[B:] for k, v in debug.items()}
        self.grads = {k: host(v) for k, v in qc.grads().items()}

    def contained(self):
        return intact(self.fw, self.need) and intact(self.fl, 1) and all((t == CANARY).all() for t in self.tails.values()) \
            and all(intact(f, (self.B + self.spare) * self.widths[k]) for k, (f, _) in self.fd.items())


def assert_equals_host(qc, run, obs, act, tq, what=""):
    loss, grads, planes = qc.critic_grad_host(obs, act, tq, return_debug=True)
    assert np.isfinite(loss) and bits(run.loss) == bits(loss), (what, run.loss, loss)
    for k in ("quantiles", "dq", "dz"):
        assert np.array_equal(bits(run.planes[k]), bits(planes[k])), (what, k)
    for k, v in grads.items():
        assert run.grads[k].shape == v.shape and np.array_equal(bits(run.grads[k]), bits(v)), (what, k)
    assert any(np.abs(v).max() > 0 for v in grads.values())


# ------------------------------------------------------------------ 1. kernel == host model
# B (1, 3, 15, 16: the 16-row tile; from 17 rows on the 32-row tile, with tails of 17, 1 and 1 rows and 4100 = 128
# tiles and 4 rows, 65 loss segments), obs_dim, action_dim (K 15, 16, 29), net_arch (padded widths 20 and 300; three
# layers of 512), n_critics, n_quantiles (a head of one tile and of two; T = 1)
CASES = [(1, 6, 3, (16,), 1, 1), (3, 7, 3, (20, 300), 2, 17), (15, 6, 3, (256, 256), 2, 25), (16, 19, 4, (16,), 1, 25),
         (17, 6, 3, (512, 512, 512), 2, 17), (33, 19, 4, (256, 256), 2, 25), (257, 7, 3, (20, 300), 2, 25),
         (4100, 7, 3, (33, 7), 2, 25)]


@pytest.mark.parametrize("B,od,A,arch,nc,nq", CASES, ids=[f"B{c[0]}-K{c[1] + 6 + c[2]}-{'x'.join(map(str, c[3]))}-{c[4]}x{c[5]}"
                                                          for c in CASES])
def test_loss_grads_and_planes_equal_host_model_bit_for_bit(B, od, A, arch, nc, nq):
    rng = np.random.default_rng(B + od + nq)
    qc, _ = make_qc(od, A, arch, nc, nq, device=DEV, seed=B)
    qc.init_optimizer()
    for nt in n_targets(nc, nq) if B <= 16 else [max(nc * nq - 2 * nc, 1)]:
        obs, act, tq = grad_batch(rng, B, od, A, nt)
        run = Run(qc, obs, act, dev(tq), B)
        assert_equals_host(qc, run, obs, act, tq, nt)
        assert run.contained()
        # the entry's quantiles are critic()'s
        assert np.array_equal(bits(run.planes["quantiles"]), bits(host(qc.critic(obs, act)).reshape(B, -1)))
    st = qc.optimizer_state_dict()   # the gradient buffer's neighbours in the handle
    assert st["step"] == 0 and not any(host(v).any() for w in ("exp_avg", "exp_avg_sq") for v in st[w].values())
    qc.close()


@pytest.mark.parametrize("B", [17, 33])
def test_both_row_tiles_give_the_same_bits(monkeypatch, B):
    """PGX_QC_TILE (read at every launch) forces the 16- or the 32-row tile: 33 rows are three tiles of 16 with
    a one-row tail, or one of 32 and one of a single row.  The order of every sum depends on the shapes alone."""
    rng = np.random.default_rng(3)
    qc, _ = make_qc(19, 4, (96, 40), 2, 25, device=DEV, seed=3)
    qc.init_optimizer()
    obs, act, tq = grad_batch(rng, B, 19, 4, 46)
    default = Run(qc, obs, act, dev(tq), B)
    assert_equals_host(qc, default, obs, act, tq)
    for tile in ("16", "32"):
        monkeypatch.setenv("PGX_QC_TILE", tile)
        run = Run(qc, obs, act, dev(tq), B)
        assert bits(run.loss) == bits(default.loss) and run.contained()
        for k, v in default.grads.items():
            assert np.array_equal(bits(run.grads[k]), bits(v)), (tile, k)
        for k, v in default.planes.items():
            assert np.array_equal(bits(run.planes[k]), bits(v)), (tile, k)
    qc.close()


def test_strided_subnormal_and_negative_zero_inputs():
    rng = np.random.default_rng(5)
    B, od, A = 31, 6, 3
    qc, sd = make_qc(od, A, (96,), 2, 25, device=DEV, seed=5)
    for p in ("critic.", "critic_target."):
        sd[f"{p}qf0.0.bias"][:48] = 0.0   # sums of tiny products stay subnormal where the bias is 0
    qc.load_state_dict(sd)
    qc.init_optimizer()
    obs, act, tq = grad_batch(rng, B, od, A, 46)
    obs["observation"][::3, 1] = F32(-0.0)
    obs["observation"][1::3, 2] = F32(1e-41)      # subnormal
    obs["achieved_goal"][::2, 0] = F32(-3e-39)    # subnormal
    obs["desired_goal"][:, 2] = F32(-0.0)
    act[::4, 0] = F32(-0.0)
    act[1::4, 1] = F32(2e-42)
    for k in obs:   # a row whose every input is tiny
        obs[k][7] = (rng.standard_normal(obs[k].shape[1]) * 1e-39).astype(F32)
    act[7] = (rng.standard_normal(A) * 1e-39).astype(F32)
    tq[3, :4] = np.array([-0.0, 1e-41, -2e-40, 0.0], F32)
    dense = Run(qc, obs, act, dev(tq), B)
    assert_equals_host(qc, dense, obs, act, tq)
    # the same rows inside wider tensors: row strides above the widths
    wide = lambda a: torch.cat([torch.full((B, 2), CANARY, device=DEV), dev(a), torch.full((B, 3), CANARY, device=DEV)],  # noqa: E731
                               dim=1)[:, 2:2 + a.shape[1]]
    views = {k: wide(v) for k, v in obs.items()}
    assert views["observation"].stride(0) == od + 5 and not views["observation"].is_contiguous()
    strided = Run(qc, views, wide(act), dev(tq), B)
    assert bits(strided.loss) == bits(dense.loss) and strided.contained()
    for k, v in dense.grads.items():
        assert np.array_equal(bits(strided.grads[k]), bits(v)), k
    qc.close()


# ------------------------------------------------------------------ 2. a HER batch in place
def fill_ring(buf, rng, N, od, A, steps):
    for t in range(steps):
        done = (np.arange(N) % 4 == t % 4).astype(np.uint8)
        f = lambda *s: (rng.standard_normal((N,) + s) * 0.5).astype(F32)  # noqa: E731
        buf.add_tensors(f(od), f(3), f(3), f(A), f(), f(od), f(3), f(3), done)


def batch_views(b):
    return {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}


def test_a_her_batch_read_in_place_equals_dense_copies_and_the_host_model():
    rng = np.random.default_rng(11)
    N, od, A, B = 16, 6, 3, 64
    buf = pg.HerReplayBuffer(N * 8, device=DEV, n_envs=N, obs_dim=od, action_dim=A, seed=3)
    fill_ring(buf, rng, N, od, A, 26)
    b = buf.alloc_batch(B)
    buf.sample_into(b, draw=0)
    assert b["rows"].stride(0) == buf.row_stride > od and not b["obs"].is_contiguous()
    qc, _ = make_qc(od, A, (96, 40), 2, 25, drop=2, device=DEV, seed=11)
    ws = qc.alloc_workspace(B)   # (and init_optimizer with its defaults)
    tq = dev((rng.standard_normal((B, qc.n_target)) * 1.5).astype(F32))
    rows_before = b["rows"].clone()
    loss_rows = host(qc.critic_loss_backward_rows(b, tq, ws)).copy()
    g_rows = {k: host(v) for k, v in qc.grads().items()}
    dense = {k: v.contiguous() for k, v in batch_views(b).items()}
    loss_dense = host(qc.critic_loss_backward(dense, b["action"].contiguous(), tq, ws)).copy()
    g_dense = {k: host(v) for k, v in qc.grads().items()}
    want_loss, want = qc.critic_grad_host({k: host(v) for k, v in dense.items()}, host(b["action"]), host(tq))
    assert np.isfinite(want_loss) and bits(loss_rows) == bits(loss_dense) == bits(want_loss)
    for k, v in want.items():
        assert np.array_equal(bits(g_rows[k]), bits(v)) and np.array_equal(bits(g_dense[k]), bits(v)), k
    assert torch.equal(b["rows"], rows_before)   # read only
    qc.close()
    buf.close()


# ------------------------------------------------------------------ 3. Adam
def assert_state_equals(qc, params, st, what=""):
    got = qc.state_dict("online")
    opt = qc.optimizer_state_dict()
    assert opt["step"] == st["step"], what
    for k, v in params.items():
        assert np.array_equal(bits(host(got[k])), bits(v)), (what, k)
        assert np.array_equal(bits(host(opt["exp_avg"][k])), bits(st["exp_avg"][k])), (what, k)
        assert np.array_equal(bits(host(opt["exp_avg_sq"][k])), bits(st["exp_avg_sq"][k])), (what, k)


def test_three_adam_steps_equal_the_host_model_in_every_bit():
    rng = np.random.default_rng(13)
    B, od, A, arch = 33, 7, 3, (20, 300)
    qc, sd = make_qc(od, A, arch, 2, 17, drop=2, device=DEV, seed=13)
    ref, _ = make_qc(od, A, arch, 2, 17, drop=2, seed=13)
    ws = qc.alloc_workspace(B)
    lr = dev(np.zeros(1, F32))
    x = grad_batch(rng, B, od, A, 1)
    tgt_in = (x[0], x[1], rng.standard_normal(B).astype(F32), rng.standard_normal(B).astype(F32), np.zeros(B, F32),
              dev(np.array([0.2], F32)))
    target_before = host(qc.td_target(*tgt_in)).copy()
    p, st = online(sd), None
    for i, rate in enumerate((3e-4, 1e-3, 0.0)):   # the learning rate is read at every launch
        obs, act, tq = grad_batch(rng, B, od, A, qc.n_target)
        loss = host(qc.critic_loss_backward(obs, act, dev(tq), ws)).copy()
        lr.fill_(rate)
        before = qc.state_dict("online") if rate == 0.0 else None
        qc.adam_step(lr)
        ref.load_state_dict(p, which="online")
        want_loss, grads = ref.critic_grad_host(obs, act, tq)
        assert bits(loss) == bits(want_loss), i
        p, st = ref.adam_step_host(float(F32(rate)), grads, params=p, state=st)
        assert_state_equals(qc, p, st, i)
        if before is not None:   # lr = 0: not a bit of a parameter moves, the moments and the step do
            assert all(torch.equal(v, qc.state_dict("online")[k]) for k, v in before.items())
    assert st["step"] == 3 and any(not np.array_equal(p[k], online(sd)[k]) for k in p)
    # the packed online set the kernels read is that plain copy, the transposed packing included
    ref.load_state_dict(p, which="online")
    obs, act, tq = grad_batch(rng, B, od, A, qc.n_target)
    assert np.array_equal(bits(host(qc.critic(obs, act))), bits(ref.forward_host(obs, act)))
    run = Run(qc, obs, act, dev(tq), B)
    assert_equals_host(ref, run, obs, act, tq)
    # the target set is left alone
    for k, v in qc.state_dict("target").items():
        assert np.array_equal(bits(host(v)), bits(sd["critic_target." + k])), k
    assert np.array_equal(bits(host(qc.td_target(*tgt_in))), bits(target_before))
    qc.close()


def test_optimizer_state_round_trips_and_init_again_zeroes_it():
    rng = np.random.default_rng(15)
    qc, sd = make_qc(6, 3, (16, 8), 2, 5, device=DEV, seed=15)
    ws = qc.alloc_workspace(8)
    obs, act, tq = grad_batch(rng, 8, 6, 3, qc.n_target)
    for _ in range(2):
        qc.critic_loss_backward(obs, act, dev(tq), ws)
        qc.adam_step(1e-3)
    st = qc.optimizer_state_dict()
    assert st["step"] == 2 and any(host(v).any() for v in st["exp_avg"].values())
    qc.init_optimizer()
    zero = qc.optimizer_state_dict()
    assert zero["step"] == 0 and not any(host(v).any() for w in ("exp_avg", "exp_avg_sq") for v in zero[w].values())
    bad = {"exp_avg": dict(st["exp_avg"]), "exp_avg_sq": dict(st["exp_avg_sq"]), "step": 2}
    bad["exp_avg_sq"]["qf1.4.bias"] = torch.zeros(6)
    with pytest.raises(ValueError, match="qf1.4.bias"):
        qc.load_optimizer_state_dict(bad)
    assert qc.optimizer_state_dict()["step"] == 0   # a failed load changes nothing
    qc.load_optimizer_state_dict(st)
    got = qc.optimizer_state_dict()
    assert got["step"] == 2
    for w in ("exp_avg", "exp_avg_sq"):
        for k, v in st[w].items():
            assert torch.equal(got[w][k], v), (w, k)
    qc.close()


# ------------------------------------------------------------------ 4. the captured update
def test_captured_update_equals_eager_after_everything_it_reads_changed():
    """sample_into -> action_log_prob_rows -> td_target_rows -> critic_loss_backward_rows -> adam_step ->
    polyak_update in one graph.  Replayed after the ring, the actor's weights, ent_coef and lr have changed, it
    equals the eager chain from the same state in every bit, and the gradient is the host model's on the batch
    it drew; two replays take two Adam steps."""
    rng = np.random.default_rng(23)
    N, od, A, B = 16, 6, 3, 64
    buf = pg.HerReplayBuffer(N * 8, device=DEV, n_envs=N, obs_dim=od, action_dim=A, seed=3)
    fill_ring(buf, rng, N, od, A, 13)
    actor = make_gaussian(od, A, (96, 40), rng, device=DEV, n_envs=1)[0]
    qc, _ = make_qc(od, A, (96, 40), 2, 25, drop=2, device=DEV, seed=23)
    ws = qc.alloc_workspace(B)
    b = buf.alloc_batch(B)
    act = torch.zeros((B, A), dtype=torch.float32, device=DEV)
    lp = torch.zeros((B,), dtype=torch.float32, device=DEV)
    target = torch.zeros((B, qc.n_target), dtype=torch.float32, device=DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    ent, lr = dev(np.array([0.2], F32)), dev(np.array([3e-4], F32))

    def chain():
        buf.sample_into(b, draw=0)
        actor.action_log_prob_rows(b, out=(act, lp))
        qc.td_target_rows(b, act, lp, ent, out=target)
        qc.critic_loss_backward_rows(b, target, ws, loss=loss)
        qc.adam_step(lr)
        qc.polyak_update(0.05)

    def snapshot():
        torch.cuda.synchronize()
        out = [host(t).copy() for t in (b["rows"], act, lp, target, loss)]
        out += [host(v) for v in qc.grads().values()] + [host(v) for v in qc.state_dict("both").values()]
        opt = qc.optimizer_state_dict()
        return out + [host(v) for w in ("exp_avg", "exp_avg_sq") for v in opt[w].values()] + [np.array([opt["step"]], F32)]

    chain()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    fill_ring(buf, rng, N, od, A, 9)   # another batch behind the same draw
    actor.load_state_dict({k: (host(v) * F32(0.7)).astype(F32) for k, v in actor.state_dict().items()})
    ent.fill_(0.55)
    lr.fill_(1e-3)
    weights, opt, word = qc.state_dict("both"), qc.optimizer_state_dict(), actor.log_prob_noise_step
    assert opt["step"] == 1
    g.replay()
    replayed = snapshot()
    assert qc.optimizer_state_dict()["step"] == 2
    # the gradient of the replay: the host model on the batch it drew, with the parameters it started from
    ref, _ = make_qc(od, A, (96, 40), 2, 25, drop=2, seed=23)
    ref.load_state_dict({k: host(v) for k, v in weights.items()})
    want_loss, want = ref.critic_grad_host({k: host(v) for k, v in batch_views(b).items()}, host(b["action"]), replayed[3])
    assert bits(replayed[4]) == bits(want_loss)
    for k, v in qc.grads().items():
        assert np.array_equal(bits(host(v)), bits(want[k])), k
    # eager from the same state
    qc.load_state_dict(weights)
    qc.load_optimizer_state_dict(opt)
    actor.log_prob_noise_step = word
    chain()
    eager = snapshot()
    assert len(eager) == len(replayed)
    for i, (x, y) in enumerate(zip(replayed, eager)):
        assert np.array_equal(bits(x), bits(y)), i
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert qc.optimizer_state_dict()["step"] == 4 and np.isfinite(host(loss)).all()
    for x in (actor, qc, buf):
        x.close()


# ------------------------------------------------------------------ 5. containment
def test_a_nan_row_poisons_loss_and_gradients_and_leaves_the_parameters_until_the_step():
    rng = np.random.default_rng(29)
    B, od, A = 33, 6, 3
    qc, sd = make_qc(od, A, (96, 40), 2, 25, drop=2, device=DEV, seed=29)
    qc.init_optimizer()
    obs, act, tq = grad_batch(rng, B, od, A, qc.n_target)
    tq[5, 7] = np.nan
    run = Run(qc, obs, act, dev(tq), B)
    assert np.isnan(run.loss) and run.contained()
    want_loss, want, planes = qc.critic_grad_host(obs, act, tq, return_debug=True)
    assert np.isnan(want_loss)
    others = np.arange(B) != 5
    assert np.isnan(run.planes["dq"][5]).all() and np.array_equal(bits(run.planes["dq"][others]), bits(planes["dq"][others]))
    for k, v in want.items():   # (a NaN's payload is not pinned: equal where finite, NaN where NaN)
        assert np.array_equal(run.grads[k], v, equal_nan=True), k
    for c in range(2):   # the head sums over every row: all of it is NaN
        assert np.isnan(run.grads[f"qf{c}.4.weight"]).all() and np.isnan(run.grads[f"qf{c}.4.bias"]).all()
    for k, v in qc.state_dict("online").items():
        assert np.array_equal(bits(host(v)), bits(sd["critic." + k])), k
    qc.adam_step(1e-3)
    after = qc.state_dict("online")
    assert all(torch.isnan(after[f"qf{c}.4.bias"]).all() for c in range(2))
    qc.close()


def test_refusals_name_the_field_and_launch_nothing():
    rng = np.random.default_rng(31)
    B = 4
    qc, _ = make_qc(6, 3, (16,), 2, 5, device=DEV)
    obs, act, tq = grad_batch(rng, B, 6, 3, 6)
    t = {"obs": dev(obs["observation"]), "achieved_goal": dev(obs["achieved_goal"]), "desired_goal": dev(obs["desired_goal"]),
         "action": dev(act), "target_quantiles": dev(tq)}
    need = qc.workspace_floats(B)
    fw, ws = guarded(need)
    fl, loss = guarded(1)

    def io(**over):
        x = abi.PgxQcGradIo()
        for k, v in t.items():
            setattr(x, k, v.data_ptr())
        x.workspace, x.loss, x.workspace_floats = ws.data_ptr(), loss.data_ptr(), need
        x.obs_stride, x.achieved_goal_stride, x.desired_goal_stride, x.action_stride = 6, 3, 3, 3
        for k, v in over.items():
            setattr(x, k, v)
        return x

    lib, s = qc.lib, qc._stream()
    assert lib.pgx_qc_critic_grad(qc._h, C.byref(io()), B, 6, s) == abi.PGX_E_INVALID   # before init_optimizer
    assert b"pgx_qc_init_training" in lib.pgx_last_error()
    lr = dev(np.array([1e-3], F32))
    assert lib.pgx_qc_adam_step(qc._h, lr.data_ptr(), s) == abi.PGX_E_INVALID and b"pgx_qc_init_training" in lib.pgx_last_error()
    with pytest.raises(pg.PgxError, match="init_training"):
        qc.grads()
    qc.init_optimizer()
    for x, n, k, word in ((io(workspace_floats=need - 1), B, 6, b"workspace_floats"), (io(), 0, 6, b"B must be > 0"),
                          (io(), B, 11, b"n_target"), (io(), B, 0, b"n_target"), (io(loss=None), B, 6, b"null loss"),
                          (io(target_quantiles=None), B, 6, b"null target_quantiles"), (io(obs_stride=5), B, 6, b"obs_stride"),
                          (io(workspace=None), B, 6, b"null workspace")):
        assert lib.pgx_qc_critic_grad(qc._h, C.byref(x), n, k, s) == abi.PGX_E_INVALID
        assert b"pgx_qc_critic_grad" in lib.pgx_last_error() and word in lib.pgx_last_error()
    assert lib.pgx_qc_adam_step(qc._h, None, s) == abi.PGX_E_INVALID and b"null lr" in lib.pgx_last_error()
    with pytest.raises(ValueError, match="workspace"):
        qc.critic_loss_backward(obs, act, dev(tq), torch.zeros(need, dtype=torch.float64, device=DEV))
    with pytest.raises(pg.PgxError, match="workspace_floats"):
        qc.critic_loss_backward(obs, act, dev(tq), torch.zeros(need - 1, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    assert (host(fw) == CANARY).all() and (host(fl) == CANARY).all()   # nothing was launched
    assert not any(host(v).any() for v in qc.grads().values()) and qc.optimizer_state_dict()["step"] == 0
    assert lib.pgx_qc_critic_grad(qc._h, C.byref(io()), B, 6, s) == abi.PGX_OK
    torch.cuda.synchronize()
    want_loss, want = qc.critic_grad_host(obs, act, tq)
    assert bits(host(loss)) == bits(want_loss) and intact(fw, need) and intact(fl, 1)
    for k, v in qc.grads().items():
        assert np.array_equal(bits(host(v)), bits(want[k])), k
    qc.close()
