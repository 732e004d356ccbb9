"""GPU tests of the device quantile critics (pgx_quantile_critic.hip): the forward kernel against the
library's host model bit for bit for both parameter sets (K order, padding, a head of two tiles, the tails of
the 16- and the 32-row tile), the one-launch truncated target against pgx_qc_target_host bit for bit (the
order rule on crafted biases, done rows, a NaN row that disturbs nothing else), a HER batch read in place
against dense copies, the Polyak step against a libm-fmaf restatement of the header's rule, a captured
td_target replayed after the batch, ent_coef and the weights changed, the refusals on a live handle, and
that nothing but the output is written (canaries, rows past B).  The host models themselves are pinned
without a GPU in test_quantile_critic_abi.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import panda_gym_amd as pg
from panda_gym_amd import abi
from test_actor_abi import bits, fmaf, random_obs
from test_quantile_critic_abi import crafted_bias_dict, make_qc, n_targets, random_qc_state_dict, target_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
CANARY = 12345.0
PAD = 64


def host(t):
    return t.detach().cpu().numpy()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def guarded(rows, width):
    """A contiguous [rows, width] f32 view with PAD canary floats in front of and behind it."""
    flat = torch.full((2 * PAD + rows * width,), CANARY, dtype=torch.float32, device=DEV)
    return flat, flat[PAD:PAD + rows * width].view(rows, width)


def canaries_intact(flat, rows, width):
    f = host(flat)
    return bool((f[:PAD] == CANARY).all() and (f[PAD + rows * width:] == CANARY).all())


def batch(rng, n, od, A):
    return random_obs(rng, n, od), rng.uniform(-1, 1, (n, A)).astype(F32)


# ------------------------------------------------------------------ 1. forward == host model
# B (1, 15: the 16-row tile; from 17 rows on the 32-row tile, with tails of 17, 1, 1 and 4 rows; the 16-row
# tile's tails: test_both_row_tiles_with_a_tail), obs_dim, action_dim (K 15, 16, 29), net_arch, n_critics,
# n_quantiles (head of one tile and of two)
FORWARD = [(1, 6, 3, (16,), 1, 1), (15, 7, 3, (16,), 5, 17), (17, 19, 4, (256, 256), 2, 25), (33, 6, 3, (512, 512, 512), 2, 16),
           (257, 6, 3, (400, 300), 2, 32), (33, 19, 4, (16,), 5, 25), (4100, 7, 3, (33, 7), 2, 25)]


@pytest.mark.parametrize("B,od,A,arch,nc,nq", FORWARD, ids=[f"B{c[0]}-K{c[1] + 6 + c[2]}-{'x'.join(map(str, c[3]))}-{c[4]}x{c[5]}"
                                                            for c in FORWARD])
def test_forward_equals_host_model_bit_for_bit(B, od, A, arch, nc, nq):
    rng = np.random.default_rng(B + od + nq)
    qc, _ = make_qc(od, A, arch, nc, nq, device=DEV, seed=B)
    obs, act = batch(rng, B, od, A)
    got = {}
    for target in (False, True):
        flat, out = guarded(B + 3, nc * nq)   # three rows more than B: left alone
        assert qc.critic(obs, act, target=target, out=out) is out
        want = qc.forward_host(obs, act, target=target)
        g = host(out)
        assert np.isfinite(want).all() and np.array_equal(bits(g[:B]), bits(want.reshape(B, -1))), target
        assert (g[B:] == CANARY).all() and canaries_intact(flat, B + 3, nc * nq)
        got[target] = g[:B].copy()
    assert not np.array_equal(got[False], got[True])   # the sets differ: a kernel reading the wrong one fails above
    q = qc.critic(obs, act)   # without out: a fresh [B, n_critics, n_quantiles]
    assert tuple(q.shape) == (B, nc, nq) and np.array_equal(bits(host(q).reshape(B, -1)), bits(got[False]))
    qc.close()


@pytest.mark.parametrize("tile", ["16", "32"])
def test_both_row_tiles_with_a_tail(monkeypatch, tile):
    """PGX_QC_TILE (read at every launch) forces the 16- or the 32-row tile; the library takes 32 from 17 rows
    on.  33 rows are three tiles of 16 with a one-row tail, or one of 32 and one of a single row."""
    rng = np.random.default_rng(3)
    qc, _ = make_qc(19, 4, (96, 40), 2, 25, device=DEV, seed=3)
    obs, act = batch(rng, 33, 19, 4)
    x = target_inputs(rng, 33)
    default = host(qc.critic(obs, act)).copy()
    monkeypatch.setenv("PGX_QC_TILE", tile)
    assert np.array_equal(bits(host(qc.critic(obs, act))), bits(default))
    assert np.array_equal(bits(default), bits(qc.forward_host(obs, act)))
    flat, out = guarded(33, qc.n_target)
    qc.td_target(obs, act, x["next_log_prob"], x["rewards"], x["dones"], dev(np.array([0.2], F32)), out=out)
    want = qc.td_target_host(obs, act, x["next_log_prob"], x["rewards"], x["dones"], 0.2)
    assert np.array_equal(bits(host(out)), bits(want)) and canaries_intact(flat, 33, qc.n_target)
    qc.close()


def test_forward_with_subnormal_and_negative_zero_inputs():
    rng = np.random.default_rng(5)
    B, od, A = 31, 6, 3
    qc, sd = make_qc(od, A, (96,), 2, 25, device=DEV, seed=5)
    for p in ("critic.", "critic_target."):
        sd[f"{p}qf0.0.bias"][:48] = 0.0   # sums of tiny products stay subnormal where the bias is 0
    qc.load_state_dict(sd)
    obs, act = batch(rng, B, od, A)
    obs["observation"][::3, 1] = F32(-0.0)
    obs["observation"][1::3, 2] = F32(1e-41)      # subnormal
    obs["achieved_goal"][::2, 0] = F32(-3e-39)    # subnormal
    obs["desired_goal"][:, 2] = F32(-0.0)
    act[::4, 0] = F32(-0.0)
    act[1::4, 1] = F32(2e-42)
    for k in obs:   # a row whose every input is tiny
        obs[k][7] = (rng.standard_normal(obs[k].shape[1]) * 1e-39).astype(F32)
    act[7] = (rng.standard_normal(A) * 1e-39).astype(F32)
    for target in (False, True):
        want = qc.forward_host(obs, act, target=target)
        assert np.isfinite(want).all()
        assert np.array_equal(bits(host(qc.critic(obs, act, target=target))), bits(want)), target
    qc.close()


# ------------------------------------------------------------------ 2. target == host model
# B, n_critics, n_quantiles (T = 1, 50, 64, 65, 128), net_arch
TARGET = [(1, 1, 1, (16,)), (15, 2, 25, (256, 256)), (17, 2, 32, (16,)), (33, 5, 13, (33, 7)), (257, 4, 32, (16,)),
          (4100, 2, 25, (16,))]


@pytest.mark.parametrize("B,nc,nq,arch", TARGET, ids=[f"B{c[0]}-T{c[1] * c[2]}" for c in TARGET])
def test_target_equals_host_model_bit_for_bit(B, nc, nq, arch):
    rng = np.random.default_rng(B * 7 + nq)
    T = nc * nq
    qc, _ = make_qc(6, 3, arch, nc, nq, device=DEV, seed=B + 1)
    obs, act = batch(rng, B, 6, 3)
    x = target_inputs(rng, B)   # dones 0, 1, 0, 1, ...
    ent = dev(np.array([0.37], F32))
    for k in n_targets(nc, nq):   # 1, T - 2 n_critics, T
        qc.n_target = k
        flat, out = guarded(B + 2, k)
        pool = torch.zeros((B, T), dtype=torch.float32, device=DEV)
        assert qc.td_target(obs, act, x["next_log_prob"], x["rewards"], x["dones"], ent, out=out, quantiles=pool) is out
        want, want_pool = qc.td_target_host(obs, act, x["next_log_prob"], x["rewards"], x["dones"], 0.37, n_target=k,
                                            return_quantiles=True)
        g = host(out)
        assert np.array_equal(bits(host(pool)), bits(want_pool)), k
        assert np.isfinite(want).all() and np.array_equal(bits(g[:B]), bits(want)), k
        assert (g[B:] == CANARY).all() and canaries_intact(flat, B + 2, k)
        done = x["dones"] == 1   # reward + 0 * t2: the reward itself
        assert np.array_equal(bits(g[:B][done]), bits(np.repeat(x["rewards"][done, None], k, axis=1)))
    qc.close()


@pytest.mark.parametrize("B,nc,nq", [(17, 2, 25), (33, 5, 13), (15, 4, 32)], ids=["T50", "T65", "T128"])
def test_the_order_rule_on_crafted_biases(B, nc, nq):
    """The pool is the crafted biases (duplicates, -0 beside +0, a descending run, subnormals, infinities),
    whatever the matmul does; with reward -0, done 0, gamma 1, ent_coef 0 and a positive log-probability the
    output is the sorted pool itself."""
    rng = np.random.default_rng(7)
    T = nc * nq
    qc = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(16,), n_critics=nc, n_quantiles=nq,
                           top_quantiles_to_drop_per_net=0, gamma=1.0, device=DEV)
    sd, crafted = crafted_bias_dict(qc, rng)
    qc.load_state_dict(sd)
    obs, act = batch(rng, B, 6, 3)
    lp, r, d = np.abs(rng.standard_normal(B)).astype(F32), np.full(B, -0.0, F32), np.zeros(B, F32)
    pool = torch.zeros((B, T), dtype=torch.float32, device=DEV)
    got = host(qc.td_target(obs, act, lp, r, d, dev(np.zeros(1, F32)), quantiles=pool))
    assert np.array_equal(bits(host(pool)), bits(np.tile(crafted, (B, 1))))
    want = qc.td_target_host(obs, act, lp, r, d, 0.0)
    assert np.array_equal(bits(got), bits(want))
    zeros = np.flatnonzero(want[0] == 0)
    assert list(bits(want[0][zeros])) == [0x80000000, 0x80000000, 0, 0]
    qc.n_target = T - 2 * nc   # a truncated target is the head of the same order
    part = host(qc.td_target(obs, act, lp, r, d, dev(np.zeros(1, F32))))
    assert np.array_equal(bits(part), bits(want[:, :T - 2 * nc]))
    qc.close()


def test_a_nan_row_disturbs_no_other_row():
    """NaN in one row's next_log_prob, and in another row's observation (relu(NaN) = +0 by the contract's
    v > 0 ? v : +0, so that row stays finite and equals the host model): all their n_target outputs are
    written, every other row is bit-identical to the run without, the canaries stay."""
    rng = np.random.default_rng(9)
    B = 33
    qc, _ = make_qc(6, 3, (96, 40), 2, 25, drop=2, device=DEV, seed=9)
    obs, act = batch(rng, B, 6, 3)
    x = target_inputs(rng, B)
    ent = dev(np.array([0.2], F32))
    clean = host(qc.td_target(obs, act, x["next_log_prob"], x["rewards"], x["dones"], ent)).copy()
    lp = x["next_log_prob"].copy()
    lp[5] = np.nan
    obs["observation"][10, 2] = np.nan   # (rows 5 and 10: done = 1 and 0)
    flat, out = guarded(B, qc.n_target)
    qc.td_target(obs, act, lp, x["rewards"], x["dones"], ent, out=out)
    g = host(out)
    others = np.ones(B, bool)
    others[[5, 10]] = False
    assert np.array_equal(bits(g[others]), bits(clean[others]))
    assert np.isnan(g[5]).all()   # every slot of the row written (none still holds the canary)
    want = qc.td_target_host(obs, act, lp, x["rewards"], x["dones"], 0.2)
    assert np.isfinite(g[10]).all() and np.array_equal(bits(g[10]), bits(want[10])) and not np.array_equal(g[10], clean[10])
    assert canaries_intact(flat, B, qc.n_target)
    qc.close()


# ------------------------------------------------------------------ 3. a HER batch in place
def test_a_her_batch_read_in_place_equals_dense_copies():
    rng = np.random.default_rng(11)
    N, od, A, B = 16, 6, 3, 64
    buf = pg.HerReplayBuffer(N * 8, device=DEV, n_envs=N, obs_dim=od, action_dim=A, seed=3)
    for t in range(26):
        done = (np.arange(N) % 4 == t % 4).astype(np.uint8)
        f = lambda *s: (rng.standard_normal((N,) + s) * 0.5).astype(F32)  # noqa: E731
        buf.add_tensors(f(od), f(3), f(3), f(A), f(), f(od), f(3), f(3), done)   # (no timeouts: done stays 1)
    b = buf.alloc_batch(B)
    buf.sample_into(b, draw=0)
    assert b["rows"].stride(0) == buf.row_stride > od and not b["next_obs"].is_contiguous()
    qc, _ = make_qc(od, A, (96, 40), 2, 25, drop=2, device=DEV, seed=11)
    nxt_a, lp = dev(rng.uniform(-1, 1, (B, A)).astype(F32)), dev(rng.standard_normal(B).astype(F32))
    ent = dev(np.array([0.3], F32))
    rows_before = b["rows"].clone()
    in_place = host(qc.td_target_rows(b, nxt_a, lp, ent)).copy()
    nxt = {"observation": b["next_obs"].contiguous(), "achieved_goal": b["next_achieved_goal"].contiguous(),
           "desired_goal": b["next_desired_goal"].contiguous()}
    dense = host(qc.td_target(nxt, nxt_a, lp, b["reward"].contiguous(), b["done"].contiguous(), ent))
    assert np.isfinite(dense).all() and np.array_equal(bits(in_place), bits(dense))
    want = qc.td_target_host({k: host(v) for k, v in nxt.items()}, host(nxt_a), host(lp), host(b["reward"]),
                             host(b["done"]), 0.3)
    assert np.array_equal(bits(in_place), bits(want))
    assert host(b["done"]).any() and not host(b["done"]).all()
    # the obs side: critic(...) on the batch's views
    views = {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}
    q_views = host(qc.critic(views, b["action"])).copy()
    q_dense = host(qc.critic({k: v.contiguous() for k, v in views.items()}, b["action"].contiguous()))
    assert np.array_equal(bits(q_views), bits(q_dense))
    assert np.array_equal(bits(q_views), bits(qc.forward_host({k: host(v) for k, v in views.items()}, host(b["action"]))))
    assert torch.equal(b["rows"], rows_before)   # read only
    qc.close()
    buf.close()


# ------------------------------------------------------------------ 4. Polyak
def restated_polyak(online, target, tau):
    """t = fmaf((float)tau, p, t * (float)(1.0 - tau)) per element, the product rounded first (libm fmaf)."""
    tf, keep_f = float(F32(tau)), F32(1.0 - tau)
    out = {}
    for k, t in target.items():
        keep = (np.asarray(t, F32) * keep_f).astype(F32).ravel()
        p = np.asarray(online[k], F32).ravel()
        out[k] = np.array([fmaf(tf, float(p[i]), float(keep[i])) for i in range(p.size)], F32).reshape(t.shape)
    return out


def test_polyak_update_and_sync_target():
    rng = np.random.default_rng(13)
    B = 17
    qc, sd = make_qc(7, 3, (16, 8), 2, 17, device=DEV, seed=13)
    obs, act = batch(rng, B, 7, 3)
    online = {k[len("critic."):]: v for k, v in sd.items() if k.startswith("critic.")}
    want = {k[len("critic_target."):]: v for k, v in sd.items() if k.startswith("critic_target.")}
    qc.polyak_update(0.0)   # tau = 0: the target's bits stay
    for k, v in qc.state_dict("target").items():
        assert np.array_equal(bits(host(v)), bits(want[k])), k
    for step in range(3):   # three in a row: packing again must not accumulate anything
        qc.polyak_update(0.02)
        want = restated_polyak(online, want, 0.02)
        got = qc.state_dict("target")
        for k in want:
            assert np.array_equal(bits(host(got[k])), bits(want[k])), (step, k)
        # the packed target the kernels read is that plain copy: forward == host model on those parameters
        ref = pg.QuantileCritic(obs_dim=7, action_dim=3, net_arch=(16, 8), n_critics=2, n_quantiles=17, device="cpu")
        ref.load_state_dict(want, which="target")
        assert np.array_equal(bits(host(qc.critic(obs, act, target=True))), bits(ref.forward_host(obs, act, target=True)))
    for k, v in qc.state_dict("online").items():   # the online set is left alone
        assert np.array_equal(bits(host(v)), bits(online[k])), k
    assert np.array_equal(bits(host(qc.critic(obs, act))), bits(qc.forward_host(obs, act)))
    qc.polyak_update(1.0)   # tau = 1: fmaf(1, p, t * 0) = p
    assert np.array_equal(bits(host(qc.critic(obs, act, target=True))), bits(host(qc.critic(obs, act))))
    # a hard copy after the sets were made to differ again
    qc.load_state_dict(random_qc_state_dict(qc, rng, which="online"), which="target")
    assert not np.array_equal(host(qc.critic(obs, act, target=True)), host(qc.critic(obs, act)))
    qc.sync_target()
    assert np.array_equal(bits(host(qc.critic(obs, act, target=True))), bits(host(qc.critic(obs, act))))
    for k, v in qc.state_dict("target").items():
        assert np.array_equal(bits(host(v)), bits(online[k])), k
    qc.close()


# ------------------------------------------------------------------ 5. capture
def test_captured_td_target_sees_the_batch_ent_coef_and_weights_of_its_replay():
    rng = np.random.default_rng(17)
    B, od, A = 64, 6, 3
    qc, _ = make_qc(od, A, (96, 40), 2, 25, drop=2, device=DEV, seed=17)

    def fresh():
        obs, act = batch(rng, B, od, A)
        x = target_inputs(rng, B)
        return [obs["observation"], obs["achieved_goal"], obs["desired_goal"], act, x["next_log_prob"], x["rewards"], x["dones"]]

    bufs = [dev(a) for a in fresh()]
    ent = dev(np.array([0.2], F32))
    flat, out = guarded(B, qc.n_target)

    def enqueue():
        o = {"observation": bufs[0], "achieved_goal": bufs[1], "desired_goal": bufs[2]}
        return qc.td_target(o, bufs[3], bufs[4], bufs[5], bufs[6], ent, out=out)

    enqueue()
    first = host(out).copy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one launch: a single chain
        enqueue()
    # another batch, another entropy coefficient, other online weights, then a Polyak step into the target
    for t, a in zip(bufs, fresh()):
        t.copy_(dev(a))
    ent.fill_(0.55)
    qc.load_state_dict(random_qc_state_dict(qc, rng, which="online"))
    qc.polyak_update(0.3)
    g.replay()
    replayed = host(out).copy()
    assert not np.array_equal(replayed, first)
    eager = host(enqueue()).copy()
    assert np.array_equal(bits(replayed), bits(eager))
    want = qc.td_target_host({"observation": host(bufs[0]), "achieved_goal": host(bufs[1]), "desired_goal": host(bufs[2])},
                             host(bufs[3]), host(bufs[4]), host(bufs[5]), host(bufs[6]), host(ent))
    assert np.array_equal(bits(replayed), bits(want))
    assert canaries_intact(flat, B, qc.n_target)
    qc.close()


# ------------------------------------------------------------------ 6. refusals on a live handle
def test_device_entry_points_refuse_bad_launches():
    qc, _ = make_qc(6, 3, (16,), 2, 5, device=DEV)
    B = 4
    t = {k: torch.zeros(s, dtype=torch.float32, device=DEV) for k, s in
         {"obs": (B, 6), "achieved_goal": (B, 3), "desired_goal": (B, 3), "action": (B, 3), "reward": (B,), "done": (B,),
          "next_log_prob": (B,), "ent_coef": (1,)}.items()}
    flat, out = guarded(B, 10)

    def io(**over):
        x = abi.PgxQcIo()
        for k, v in t.items():
            setattr(x, k, v.data_ptr())
        x.out = out.data_ptr()
        x.obs_stride, x.achieved_goal_stride, x.desired_goal_stride, x.action_stride = 6, 3, 3, 3
        x.reward_stride = x.done_stride = 1
        for k, v in over.items():
            setattr(x, k, v)
        return x

    lib, s = qc.lib, qc._stream()
    for x, n, k, word in ((io(obs_stride=5), B, 10, b"obs_stride"), (io(), 0, 10, b"B must be > 0"), (io(), B, 11, b"n_target"),
                          (io(), B, 0, b"n_target"), (io(ent_coef=None), B, 10, b"null ent_coef"),
                          (io(done_stride=0), B, 10, b"done_stride")):
        assert lib.pgx_qc_target(qc._h, C.byref(x), n, k, s) == abi.PGX_E_INVALID
        assert b"pgx_qc_target" in lib.pgx_last_error() and word in lib.pgx_last_error()
    x = io(action_stride=2)
    assert lib.pgx_qc_forward(qc._h, abi.QC_ONLINE, C.byref(x), B, s) == abi.PGX_E_INVALID
    assert b"action_stride" in lib.pgx_last_error()
    assert lib.pgx_qc_forward(qc._h, 2, C.byref(io()), B, s) == abi.PGX_E_INVALID
    assert b"which" in lib.pgx_last_error()
    assert lib.pgx_qc_polyak(qc._h, 1.5, s) == abi.PGX_E_INVALID and b"tau" in lib.pgx_last_error()
    torch.cuda.synchronize()
    assert (host(flat) == CANARY).all()   # nothing was launched
    assert lib.pgx_qc_target(qc._h, C.byref(io()), B, 10, s) == abi.PGX_OK
    torch.cuda.synchronize()
    z = np.zeros
    want = qc.td_target_host({"observation": z((B, 6), F32), "achieved_goal": z((B, 3), F32), "desired_goal": z((B, 3), F32)},
                             z((B, 3), F32), z(B, F32), z(B, F32), z(B, F32), 0.0)
    assert np.array_equal(bits(host(out)), bits(want)) and canaries_intact(flat, B, 10)
    qc.close()
