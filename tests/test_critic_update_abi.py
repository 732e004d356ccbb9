"""The critic update's C-ABI (include/pgx.h, "QuantileCritic, the critic update") without a GPU: the new
struct's layout through gcc, the exports, every refusal naming its field (the launch check is one function
for pgx_qc_critic_grad and its host twin, reached here through the twin), and the arithmetic:
pgx_qc_critic_grad_host bit for bit against a numpy + libm-fmaf restatement of the header's orders (k
ascending inside the loss, o ascending for dA, b ascending for dW and db, the row-loss segments of 64),
crafted d of 0, -0, +-1 and beyond, units at +-0 and dead units, and against torch autograd in fp64;
pgx_qc_adam_step_host bit for bit against the stated f32 sequence in numpy and against torch.optim.Adam.

The fp64 bounds follow one rule: the host model's largest error may be FACTOR times torch f32's largest
error on the same problem plus one ulp of the largest value, FACTOR being twice the largest ratio measured
over the shapes below ("Critic update on the device": the measured ratios)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import panda_gym_amd as pg
from abi_checks import assert_exported, header_layout
from panda_gym_amd import _native, abi
from test_actor_abi import bits, chain, fmaf, random_obs
from test_quantile_critic_abi import good_config, make_qc, n_targets, qc_features

F32 = np.float32
EXPORTS = ["pgx_qc_grad_workspace_floats", "pgx_qc_init_training", "pgx_qc_critic_grad", "pgx_qc_get_grads",
           "pgx_qc_adam_step", "pgx_qc_get_opt_state", "pgx_qc_set_opt_state", "pgx_qc_critic_grad_host",
           "pgx_qc_adam_step_host"]
# Twice the largest measured ratio (host model's largest error) / (torch f32 autograd's largest error) against
# fp64 over GRAD_CASES, eight draws per shape (DESIGN.md has the table): 9.3 for the gradients (K29-16-5x25-B17:
# the loss chains 115 targets one after the other where torch sums them in blocks), 3.1 for the loss.
GRAD_FACTOR = 18.6
LOSS_FACTOR = 6.2
# The same for three Adam steps against an fp64 restatement: 1.0 measured.
ADAM_FACTOR = 2.0


# ---------------------------------------------------------------- helpers shared with the GPU tests
def online(sd):
    return {k[len("critic."):]: v for k, v in sd.items() if k.startswith("critic.")}


def up(n, m):
    return (n + m - 1) // m * m


def restated_grad(qc, sd, obs, act, tq):
    """loss, grads, planes by the header's rules, one libm fmaf at a time.  sd: the online set's own keys."""
    x = qc_features(obs, act)
    B, nl, nc, nq, nt = x.shape[0], len(qc.net_arch), qc.n_critics, qc.n_quantiles, tq.shape[1]
    inv = F32(1.0) / F32(B * nc * nq * nt)
    widths = list(qc.net_arch) + [nq]
    grads, rl = {}, np.zeros(B, F32)
    quant, dq_all = np.zeros((B, nc, nq), F32), np.zeros((B, nc, nq), F32)
    dz_all = [[None] * nl for _ in range(nc)]
    with np.errstate(all="ignore"):
        lt_all = np.zeros((B, nc, nq), F32)
        for c in range(nc):
            Ws = [np.asarray(sd[f"qf{c}.{2 * l}.weight"], F32) for l in range(nl + 1)]
            bs = [np.asarray(sd[f"qf{c}.{2 * l}.bias"], F32) for l in range(nl + 1)]
            acts = [x]   # acts[l]: the input of Linear l
            for l in range(nl):
                y = np.array([[chain(acts[l][b], Ws[l][o], bs[l][o]) for o in range(widths[l])] for b in range(B)], F32)
                acts.append(np.where(y > 0, y, F32(0.0)).astype(F32))
            q = np.array([[chain(acts[nl][b], Ws[nl][o], bs[nl][o]) for o in range(nq)] for b in range(B)], F32)
            dz = np.zeros((B, nq), F32)
            for b in range(B):
                for j in range(nq):
                    tau = (F32(j) + F32(0.5)) / F32(nq)
                    a_l = a_g = 0.0
                    for k in range(nt):
                        d = F32(tq[b, k] - q[b, j])
                        w = np.abs(F32(tau - (F32(1.0) if d < 0 else F32(0.0))))
                        ad = np.abs(d)
                        huber = F32(ad - F32(0.5)) if ad > 1 else F32(F32(d * d) * F32(0.5))
                        clamp = F32(-1.0) if d < -1 else (F32(1.0) if d > 1 else d)
                        a_l = fmaf(float(w), float(huber), a_l)
                        a_g = fmaf(float(w), float(clamp), a_g)
                    lt_all[b, c, j] = a_l
                    dz[b, j] = F32(-inv) * F32(a_g)
            quant[:, c], dq_all[:, c] = q, dz
            for l in range(nl, -1, -1):
                out, inn = Ws[l].shape
                dW, db = np.zeros((out, inn), F32), np.zeros(out, F32)
                for o in range(out):
                    for k in range(inn):
                        acc = 0.0
                        for b in range(B):
                            acc = fmaf(float(dz[b, o]), float(acts[l][b, k]), acc)
                        for _ in range(B, up(B, 4)):
                            acc = fmaf(0.0, 0.0, acc)
                        dW[o, k] = acc
                    acc = 0.0
                    for b in range(B):
                        acc = fmaf(float(dz[b, o]), 1.0, acc)
                    for _ in range(B, up(B, 4)):
                        acc = fmaf(0.0, 0.0, acc)
                    db[o] = acc
                grads[f"qf{c}.{2 * l}.weight"], grads[f"qf{c}.{2 * l}.bias"] = dW, db
                if l == 0:
                    break
                prev = np.zeros((B, inn), F32)
                for b in range(B):
                    for k in range(inn):
                        acc = 0.0
                        for o in range(out):
                            acc = fmaf(float(dz[b, o]), float(Ws[l][o, k]), acc)
                        for _ in range(out, up(out, 16)):
                            acc = fmaf(0.0, 0.0, acc)
                        prev[b, k] = acc if acts[l][b, k] > 0 else 0.0
                dz = prev
                dz_all[c][l - 1] = prev
        for b in range(B):
            s = F32(0.0)
            for v in lt_all[b].reshape(-1):
                s = F32(s + v)
            rl[b] = s
        total = F32(0.0)
        for b0 in range(0, B, 64):
            seg = F32(0.0)
            for v in rl[b0:b0 + 64]:
                seg = F32(seg + v)
            total = F32(total + seg)
        loss = F32(total * inv)
    planes = {"quantiles": quant.reshape(B, -1), "dq": dq_all.reshape(B, -1),
              "dz": np.concatenate([dz_all[c][l] for c in range(nc) for l in range(nl)], axis=1)}
    return loss, grads, planes


def autograd(qc, sd, obs, act, tq, dtype):
    """loss and gradients of quantile_huber_loss(critic(obs, act), tq.unsqueeze(1), sum_over_quantiles=False)
    through torch autograd on the CPU, as sb3_contrib writes it."""
    x = torch.as_tensor(qc_features(obs, act)).to(dtype)
    ps = {k: torch.as_tensor(np.asarray(v, F32)).to(dtype).requires_grad_(True) for k, v in sd.items()}
    nl = len(qc.net_arch)
    qs = []
    for c in range(qc.n_critics):
        h = x
        for l in range(nl + 1):
            h = torch.nn.functional.linear(h, ps[f"qf{c}.{2 * l}.weight"], ps[f"qf{c}.{2 * l}.bias"])
            if l < nl:
                h = torch.relu(h)
        qs.append(h)
    cur = torch.stack(qs, dim=1)
    target = torch.as_tensor(tq).to(dtype).unsqueeze(1)
    nq = cur.shape[-1]
    tau = (torch.arange(nq, dtype=dtype) + 0.5) / nq
    delta = target.unsqueeze(-2) - cur.unsqueeze(-1)
    a = delta.abs()
    huber = torch.where(a > 1, a - 0.5, delta ** 2 * 0.5)
    loss = (torch.abs(tau.view(1, 1, -1, 1) - (delta.detach() < 0).to(dtype)) * huber).mean()
    loss.backward()
    return loss.detach().numpy(), {k: p.grad.numpy() for k, p in ps.items()}


def restated_adam(params, grads, state, lr, betas=(0.9, 0.999), eps=1e-8):
    """One step of the header's f32 sequence in numpy; returns new (params, state)."""
    step = state["step"] + 1

    def power(beta):
        p, s, n = 1.0, float(beta), step
        while n:
            if n & 1:
                p = p * s
            s = s * s
            n >>= 1
        return p

    bc1, bc2 = F32(1.0 - power(betas[0])), F32(1.0 - power(betas[1]))
    step_size, c2 = F32(lr) / bc1, np.sqrt(bc2)
    omb1, b2, omb2, e = F32(1.0 - betas[0]), F32(betas[1]), F32(1.0 - betas[1]), F32(eps)
    new_p, m_out, v_out = {}, {}, {}
    with np.errstate(all="ignore"):
        for k, p in params.items():
            p, g = np.asarray(p, F32), np.asarray(grads[k], F32)
            m = state["exp_avg"][k] + (g - state["exp_avg"][k]) * omb1
            v = state["exp_avg_sq"][k] * b2 + omb2 * (g * g)
            u = step_size * (m / (np.sqrt(v) / c2 + e))
            new_p[k] = np.where(u == 0, p, p - u).astype(F32)
            m_out[k], v_out[k] = m.astype(F32), v.astype(F32)
    return new_p, {"exp_avg": m_out, "exp_avg_sq": v_out, "step": step}


def zero_state(params):
    z = lambda: {k: np.zeros_like(np.asarray(v, F32)) for k, v in params.items()}  # noqa: E731
    return {"exp_avg": z(), "exp_avg_sq": z(), "step": 0}


def grad_batch(rng, n, od, A, nt, spread=1.5):
    obs, act = random_obs(rng, n, od), rng.uniform(-1, 1, (n, A)).astype(F32)
    return obs, act, (rng.standard_normal((n, nt)) * spread).astype(F32)   # |d| on both sides of 1


# ---------------------------------------------------------------- the C-ABI
def test_struct_layout_matches_header():
    header_layout({"pgx_qc_grad_io": abi.PgxQcGradIo})


def test_library_exports_the_entry_points():
    assert_exported(EXPORTS)


def test_python_surface_is_exported():
    for name in ("alloc_workspace", "critic_loss_backward", "critic_loss_backward_rows", "grads", "init_optimizer",
                 "adam_step", "optimizer_state_dict", "load_optimizer_state_dict", "critic_grad_host", "adam_step_host"):
        assert hasattr(pg.QuantileCritic, name), name
    assert list(inspect.signature(pg.QuantileCritic.critic_loss_backward).parameters)[1:5] == [
        "obs", "actions", "target_quantiles", "workspace"]
    assert list(inspect.signature(pg.QuantileCritic.critic_loss_backward_rows).parameters)[1:4] == [
        "batch", "target_quantiles", "workspace"]
    sig = inspect.signature(pg.QuantileCritic.init_optimizer).parameters
    assert sig["betas"].default == (0.9, 0.999) and sig["eps"].default == 1e-8
    q = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8,), device="cpu")
    z = np.zeros((4, 3), F32)
    for call in (lambda: q.alloc_workspace(4), lambda: q.critic_loss_backward(random_obs(np.random.default_rng(0), 4, 6), z, z, z),
                 q.grads, lambda: q.adam_step(1e-3)):
        with pytest.raises(pg.PgxError, match="no CPU fallback"):
            call()


def test_workspace_floats():
    """B rows of: K16 features, per critic the A_l and dZ_l planes (widths up to 16), 16 for the loss terms."""
    lib = _native.load()
    cfg = good_config()   # K = 15, one hidden layer of 16, 2 critics x 5 quantiles
    assert lib.pgx_qc_grad_workspace_floats(C.byref(cfg), 7) == 7 * (16 + 2 * (2 * 16 + 16) + 16)
    q = pg.QuantileCritic(obs_dim=19, action_dim=4, net_arch=(20, 300), n_critics=2, n_quantiles=17, device="cpu")
    assert q.workspace_floats(4100) == 4100 * (32 + 2 * (2 * (32 + 304) + 32) + 16)
    assert lib.pgx_qc_grad_workspace_floats(C.byref(cfg), 0) == abi.PGX_E_INVALID and b"B must be > 0" in lib.pgx_last_error()
    cfg.n_critics = 6
    assert lib.pgx_qc_grad_workspace_floats(C.byref(cfg), 4) == abi.PGX_E_INVALID and b"n_critics" in lib.pgx_last_error()
    assert lib.pgx_qc_grad_workspace_floats(None, 4) == abi.PGX_E_INVALID


def _grad_call(n=3, n_target=4):
    """Everything pgx_qc_critic_grad_host takes, valid: (cfg, weights, io, n, n_target, grads, keep-alive)."""
    cfg = good_config()
    rng = np.random.default_rng(0)
    w, g, keep = abi.PgxQcWeights(), abi.PgxQcWeights(), []
    for c in range(2):
        for l, shape in enumerate([(16, 15), (5, 16)]):
            for s, scale in ((w, 1.0), (g, 0.0)):
                W, b = (rng.standard_normal(shape) * scale).astype(F32), (rng.standard_normal(shape[0]) * scale).astype(F32)
                s.weight[c][l], s.bias[c][l] = W.ctypes.data, b.ctypes.data
                keep += [W, b]
    need = _native.load().pgx_qc_grad_workspace_floats(C.byref(cfg), n)
    arrays = {"obs": (n, 6), "achieved_goal": (n, 3), "desired_goal": (n, 3), "action": (n, 3),
              "target_quantiles": (n, n_target), "workspace": (need,), "loss": (1,)}
    io = abi.PgxQcGradIo()
    for k, shape in arrays.items():
        a = np.zeros(shape, F32)
        setattr(io, k, a.ctypes.data)
        keep.append(a)
    io.workspace_floats = need
    io.obs_stride, io.achieved_goal_stride, io.desired_goal_stride, io.action_stride = 6, 3, 3, 3
    return cfg, w, io, n, n_target, g, keep


BAD_LAUNCH = [("obs", None, b"null obs"), ("achieved_goal", None, b"null achieved_goal"),
              ("desired_goal", None, b"null desired_goal"), ("action", None, b"null action"),
              ("target_quantiles", None, b"null target_quantiles"), ("workspace", None, b"null workspace"),
              ("loss", None, b"null loss"), ("B", 0, b"B must be > 0"), ("B", -3, b"B must be > 0"),
              ("n_target", 0, b"n_target"), ("n_target", 11, b"n_target"), ("obs_stride", 5, b"obs_stride"),
              ("achieved_goal_stride", 2, b"achieved_goal_stride"), ("desired_goal_stride", 0, b"desired_goal_stride"),
              ("action_stride", 2, b"action_stride"), ("workspace_floats", -1, b"workspace_floats is below"),
              ("workspace_floats", 0, b"workspace_floats is below")]


@pytest.mark.parametrize("field,value,words", BAD_LAUNCH, ids=[f"{b[0]}={b[1]}" for b in BAD_LAUNCH])
def test_launch_checks_refuse_without_a_device(field, value, words):
    """pgx_qc_check_grad_launch, the one function pgx_qc_critic_grad and its host twin call in front of
    anything else: every refusal names its field (a workspace one float short included); the valid call
    passes."""
    lib = _native.load()
    cfg, w, io, n, n_target, g, keep = _grad_call()
    assert lib.pgx_qc_critic_grad_host(C.byref(cfg), C.byref(w), C.byref(io), n, n_target, C.byref(g)) == abi.PGX_OK
    if field == "B":
        n = value
    elif field == "n_target":
        n_target = value
    elif field == "workspace_floats":
        io.workspace_floats = io.workspace_floats - 1 if value == -1 else value
    else:
        setattr(io, field, value)
    assert lib.pgx_qc_critic_grad_host(C.byref(cfg), C.byref(w), C.byref(io), n, n_target, C.byref(g)) == abi.PGX_E_INVALID
    msg = lib.pgx_last_error()
    assert b"pgx_qc_critic_grad_host" in msg and words in msg, msg


def test_launch_checks_keep_their_order():
    """Every field bad at once: the first of the ladder wins, and as each is mended, the next.  The pointers and
    the strides at the ladder's two ends are checked by code the other batch launches share, this launch's own
    pointers in between: the winner for any set of bad fields stays the one it was."""
    lib = _native.load()
    cfg, w, io, n, n_target, g, keep = _grad_call()
    ladder = [("obs", None, b"null obs"), ("achieved_goal", None, b"null achieved_goal"),
              ("desired_goal", None, b"null desired_goal"), ("action", None, b"null action"),
              ("target_quantiles", None, b"null target_quantiles"), ("workspace", None, b"null workspace"),
              ("loss", None, b"null loss"), ("B", 0, b"B must be > 0"), ("obs_stride", 5, b"obs_stride"),
              ("achieved_goal_stride", 2, b"achieved_goal_stride"), ("desired_goal_stride", 0, b"desired_goal_stride"),
              ("action_stride", 2, b"action_stride"), ("n_target", 0, b"n_target"),
              ("workspace_floats", 0, b"workspace_floats is below")]
    call = {"B": n, "n_target": n_target}
    good = {f: call[f] if f in call else getattr(io, f) for f, _, _ in ladder}

    def put(field, value):
        if field in call:
            call[field] = value
        else:
            setattr(io, field, value)

    for field, value, _ in ladder:
        put(field, value)
    for field, _, words in ladder:
        rc = lib.pgx_qc_critic_grad_host(C.byref(cfg), C.byref(w), C.byref(io), call["B"], call["n_target"], C.byref(g))
        assert rc == abi.PGX_E_INVALID and words in lib.pgx_last_error(), (field, lib.pgx_last_error())
        put(field, good[field])
    assert lib.pgx_qc_critic_grad_host(C.byref(cfg), C.byref(w), C.byref(io), n, n_target, C.byref(g)) == abi.PGX_OK


@pytest.mark.parametrize("b1,b2,eps,word", [(1.0, 0.999, 1e-8, b"beta1"), (-0.1, 0.999, 1e-8, b"beta1"),
                                            (0.9, 1.0, 1e-8, b"beta2"), (0.9, float("nan"), 1e-8, b"beta2"),
                                            (0.9, 0.999, 0.0, b"eps"), (0.9, 0.999, float("inf"), b"eps")])
def test_adam_constants_are_checked_by_name(b1, b2, eps, word):
    lib = _native.load()
    cfg, w, io, n, n_target, g, keep = _grad_call()
    step = C.c_uint64(0)
    args = [C.byref(cfg), C.byref(w), C.byref(g), C.byref(g), C.byref(g), C.byref(step), 1e-3]
    assert lib.pgx_qc_adam_step_host(*args, b1, b2, eps) == abi.PGX_E_INVALID
    assert b"pgx_qc_adam_step_host" in lib.pgx_last_error() and word in lib.pgx_last_error()
    assert step.value == 0
    q = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(8,), device="cpu")
    with pytest.raises(pg.PgxError, match=word.decode()):
        q.init_optimizer(betas=(b1, b2), eps=eps)


def test_null_handles_and_pointers_are_rejected():
    lib = _native.load()
    cfg, w, io, n, n_target, g, keep = _grad_call()
    step = C.c_uint64(0)
    lr = np.zeros(1, F32)
    for rc in (lib.pgx_qc_init_training(None, 0.9, 0.999, 1e-8), lib.pgx_qc_critic_grad(None, C.byref(io), n, n_target, None),
               lib.pgx_qc_get_grads(None, C.byref(g), None), lib.pgx_qc_adam_step(None, lr.ctypes.data, None),
               lib.pgx_qc_get_opt_state(None, C.byref(g), C.byref(g), C.byref(step), None),
               lib.pgx_qc_set_opt_state(None, C.byref(g), C.byref(g), 0, None),
               lib.pgx_qc_critic_grad_host(C.byref(cfg), C.byref(w), None, n, n_target, C.byref(g)),
               lib.pgx_qc_critic_grad_host(C.byref(cfg), None, C.byref(io), n, n_target, C.byref(g)),
               lib.pgx_qc_critic_grad_host(C.byref(cfg), C.byref(w), C.byref(io), n, n_target, None),
               lib.pgx_qc_adam_step_host(C.byref(cfg), C.byref(w), C.byref(g), C.byref(g), C.byref(g), None, 1e-3, 0.9,
                                         0.999, 1e-8)):
        assert rc == abi.PGX_E_INVALID
        assert b"null" in lib.pgx_last_error()


# ---------------------------------------------------------------- the arithmetic contract: loss and gradient
# obs_dim, action_dim (K 15, 16, 29), net_arch, n_critics, n_quantiles, rows, every n_target of n_targets() or
# T - 2 n_critics alone
GRAD_CASES = [(6, 3, (16,), 1, 1, 1, True), (7, 3, (20, 300), 2, 17, 3, False), (19, 4, (16,), 5, 25, 17, False),
              (6, 3, (256, 256), 1, 16, 3, False), (7, 3, (24, 16, 8), 2, 32, 17, True), (6, 3, (16,), 2, 25, 3, True)]
GRAD_IDS = [f"K{c[0] + 6 + c[1]}-{'x'.join(map(str, c[2]))}-{c[3]}x{c[4]}-B{c[5]}" for c in GRAD_CASES]


@pytest.mark.parametrize("od,A,arch,nc,nq,n,every", GRAD_CASES, ids=GRAD_IDS)
def test_grad_host_model_equals_the_restatement_bit_for_bit(od, A, arch, nc, nq, n, every):
    rng = np.random.default_rng(od * 1000 + nc * 100 + nq)
    qc, sd = make_qc(od, A, arch, nc, nq, seed=od + nq)
    for nt in n_targets(nc, nq) if every else [max(nc * nq - 2 * nc, 1)]:
        obs, act, tq = grad_batch(rng, n, od, A, nt)
        loss, grads, planes = qc.critic_grad_host(obs, act, tq, return_debug=True)
        want_loss, want, want_planes = restated_grad(qc, online(sd), obs, act, tq)
        assert np.isfinite(loss) and bits(loss) == bits(want_loss), (nt, loss, want_loss)
        for k in ("quantiles", "dq", "dz"):
            assert np.array_equal(bits(planes[k]), bits(want_planes[k])), (nt, k)
        assert list(grads) == list(qc.state_dict("online"))
        for k, v in grads.items():   # torch shapes: the padded columns of width 20 / 300 exist nowhere here
            assert v.shape == want[k].shape and np.array_equal(bits(v), bits(want[k])), (nt, k)
        assert any(np.abs(v).max() > 0 for v in grads.values())
    assert np.array_equal(bits(planes["quantiles"]), bits(qc.forward_host(obs, act).reshape(n, -1)))


def test_crafted_differences_zero_one_and_beyond():
    """The last Linear's weights are -0 and the last hidden width is 16, so q IS the bias (+0 and 0.5): the
    targets put d at -0, +0, +-1 exactly and on both sides of them.  d = +-0 and the Huber branch |d| = 1
    (quadratic: 0.5, slope 1) meet fp64 autograd, which takes the same branches."""
    rng = np.random.default_rng(5)
    qc, sd = make_qc(6, 3, (16,), 2, 4, seed=5)
    for c in range(2):
        sd[f"critic.qf{c}.2.weight"] = np.full((4, 16), -0.0, F32)
        sd[f"critic.qf{c}.2.bias"] = np.array([0.0, 0.5, 0.0, 0.5], F32)
    qc.load_state_dict(sd)
    obs, act, _ = grad_batch(rng, 3, 6, 3, 1)
    tq = np.array([[-0.0, 0.0, 1.0, -1.0, 1.5, -0.5, 2.5, -3.0]] * 3, F32)
    tq[1] += F32(0.5)
    loss, grads, planes = qc.critic_grad_host(obs, act, tq, return_debug=True)
    assert np.array_equal(bits(planes["quantiles"]), bits(np.tile(np.array([0.0, 0.5], F32), (3, 4))))
    want_loss, want, want_planes = restated_grad(qc, online(sd), obs, act, tq)
    assert bits(loss) == bits(want_loss) and np.array_equal(bits(planes["dq"]), bits(want_planes["dq"]))
    for k, v in grads.items():
        assert np.array_equal(bits(v), bits(want[k])), k
    l64, g64 = autograd(qc, online(sd), obs, act, tq, torch.float64)
    assert abs(float(loss) - float(l64)) <= 4 * np.spacing(F32(l64))
    for k, v in grads.items():
        assert np.abs(v - g64[k]).max() <= 8 * np.spacing(F32(np.abs(g64[k]).max())), k
    # one element by hand: B = 1, one critic, one quantile, one target, d = 1: w = 0.5, huber 0.5, clamp 1
    one = pg.QuantileCritic(obs_dim=6, action_dim=3, net_arch=(16,), n_critics=1, n_quantiles=1,
                            top_quantiles_to_drop_per_net=0, device="cpu")
    s1 = {k: np.zeros(tuple(v.shape), F32) for k, v in one.state_dict("online").items()}
    one.load_state_dict(s1)
    o1, a1, _ = grad_batch(rng, 1, 6, 3, 1)
    loss, grads, planes = one.critic_grad_host(o1, a1, np.array([[1.0]], F32), return_debug=True)
    assert loss == F32(0.25) and planes["dq"][0, 0] == F32(-0.5) and grads["qf0.2.bias"][0] == F32(-0.5)


def test_units_at_zero_and_dead_units_pass_nothing():
    """First-layer units with zero weights: bias +0 and -0 (pre-activation exactly +-0) and -100 (dead for the
    whole batch).  Their rows of dW_0 and db_0 and their columns of dW_1 are exactly zero, as torch's
    threshold_backward leaves them; everything equals the restatement."""
    rng = np.random.default_rng(6)
    qc, sd = make_qc(6, 3, (20, 16), 2, 5, seed=6)
    for c in range(2):
        sd[f"critic.qf{c}.0.weight"][:3] = 0.0
        sd[f"critic.qf{c}.0.bias"][:3] = np.array([0.0, -0.0, -100.0], F32)
    qc.load_state_dict(sd)
    obs, act, tq = grad_batch(rng, 5, 6, 3, 6)
    loss, grads, planes = qc.critic_grad_host(obs, act, tq, return_debug=True)
    want_loss, want, want_planes = restated_grad(qc, online(sd), obs, act, tq)
    assert bits(loss) == bits(want_loss)
    for k, v in grads.items():
        assert np.array_equal(bits(v), bits(want[k])), k
    for c in range(2):
        assert not grads[f"qf{c}.0.weight"][:3].any() and not grads[f"qf{c}.0.bias"][:3].any()
        assert not grads[f"qf{c}.2.weight"][:, :3].any() and grads[f"qf{c}.2.weight"][:, 3:].any()
        assert not planes["dz"][:, c * 36:c * 36 + 3].any()
    _, g64 = autograd(qc, online(sd), obs, act, tq, torch.float64)
    for c in range(2):
        assert not g64[f"qf{c}.0.weight"][:3].any() and not g64[f"qf{c}.0.bias"][:3].any()


def measured_errors(qc, sd, obs, act, tq):
    """(host model's, torch f32 autograd's) largest error against fp64 autograd, and the largest |value|, for
    the loss and over every gradient tensor."""
    loss, grads = qc.critic_grad_host(obs, act, tq)
    l64, g64 = autograd(qc, sd, obs, act, tq, torch.float64)
    l32, g32 = autograd(qc, sd, obs, act, tq, torch.float32)
    e_host = max(np.abs(grads[k].astype(np.float64) - g64[k]).max() for k in g64)
    e_t32 = max(np.abs(g32[k].astype(np.float64) - g64[k]).max() for k in g64)
    top = max(np.abs(g64[k]).max() for k in g64)
    return (abs(float(loss) - float(l64)), abs(float(l32) - float(l64)), abs(float(l64))), (e_host, e_t32, top)


def ensemble_errors(od, A, arch, nc, nq, n, seeds=8):
    """measured_errors over `seeds` parameter sets and batches of one shape, the largest of each figure: a
    single draw's ratio is luck (torch's f32 loss can land on the fp64 value), the largest over a few is not."""
    runs = []
    for seed in range(seeds):
        rng = np.random.default_rng(1000 + seed)
        qc, sd = make_qc(od, A, arch, nc, nq, seed=seed)
        obs, act, tq = grad_batch(rng, n, od, A, max(nc * nq - 2 * nc, 1))
        runs.append(measured_errors(qc, online(sd), obs, act, tq))
    return [tuple(max(r[i][j] for r in runs) for j in range(3)) for i in range(2)]


@pytest.mark.parametrize("od,A,arch,nc,nq,n,every", GRAD_CASES, ids=GRAD_IDS)
def test_grad_host_model_against_fp64_autograd(od, A, arch, nc, nq, n, every):
    for what, factor, (e_host, e_t32, top) in zip(("loss", "grads"), (LOSS_FACTOR, GRAD_FACTOR),
                                                  ensemble_errors(od, A, arch, nc, nq, n)):
        print(f"{what}: host {e_host:.3e} torch-f32 {e_t32:.3e} ratio {e_host / e_t32:.2f} top {top:.3e}")
        assert e_host <= factor * e_t32 + np.spacing(F32(top)), what


# ---------------------------------------------------------------- the arithmetic contract: Adam
def adam_problem(seed=0):
    rng = np.random.default_rng(seed)
    qc, sd = make_qc(7, 3, (20, 12), 2, 5, seed=seed)
    params = online(sd)
    grads = [{k: (rng.standard_normal(v.shape) * 10.0 ** rng.integers(-6, 1)).astype(F32) for k, v in params.items()}
             for _ in range(3)]
    grads[1]["qf0.0.bias"][:4] = 0.0   # g = 0 behind a non-zero first step
    return qc, params, grads


def test_adam_host_model_equals_the_stated_sequence_bit_for_bit():
    qc, params, grads = adam_problem()
    qc.init_optimizer()
    p, st = params, None
    want_p, want_st = params, zero_state(params)
    for i, g in enumerate(grads):
        p, st = qc.adam_step_host(3e-4, g, params=p, state=st)
        want_p, want_st = restated_adam(want_p, g, want_st, 3e-4)
        assert st["step"] == i + 1 == want_st["step"]
        for k in params:
            assert np.array_equal(bits(p[k]), bits(want_p[k])), (i, k)
            assert np.array_equal(bits(st["exp_avg"][k]), bits(want_st["exp_avg"][k])), (i, k)
            assert np.array_equal(bits(st["exp_avg_sq"][k]), bits(want_st["exp_avg_sq"][k])), (i, k)
    assert any(not np.array_equal(p[k], params[k]) for k in params)
    for k, v in qc.state_dict("online").items():   # on copies: the object's own parameters stay
        assert np.array_equal(bits(v.numpy()), bits(params[k])), k
    # other constants reach the arithmetic
    p2, _ = qc.adam_step_host(3e-4, grads[0], params=params, betas=(0.5, 0.9), eps=1e-3)
    w2, _ = restated_adam(params, grads[0], zero_state(params), 3e-4, betas=(0.5, 0.9), eps=1e-3)
    assert all(np.array_equal(bits(p2[k]), bits(w2[k])) for k in params)
    assert not all(np.array_equal(p2[k], restated_adam(params, grads[0], zero_state(params), 3e-4)[0][k]) for k in params)


def test_a_zero_learning_rate_leaves_every_bit_of_the_parameters():
    qc, params, grads = adam_problem(1)
    params["qf0.0.bias"][:2] = np.array([-0.0, 0.0], F32)   # p - (+-0) would turn a -0 into +0
    grads[0]["qf0.0.bias"][:2] = np.array([-1.0, 1.0], F32)
    p, st = qc.adam_step_host(0.0, grads[0], params=params)
    assert st["step"] == 1 and any(v.any() for v in st["exp_avg"].values())
    for k in params:
        assert np.array_equal(bits(p[k]), bits(params[k])), k


def test_adam_against_torch_and_fp64():
    """Three steps from zero state: the host model and torch.optim.Adam (CPU, f32) against an fp64 restatement
    of the same update, the host model held to ADAM_FACTOR times torch's error plus one ulp."""
    qc, params, grads = adam_problem(2)
    tp = {k: torch.nn.Parameter(torch.as_tensor(v.copy())) for k, v in params.items()}
    opt = torch.optim.Adam(list(tp.values()), lr=3e-4)
    p, st = params, None
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    m64 = {k: np.zeros_like(v) for k, v in p64.items()}
    v64 = {k: np.zeros_like(v) for k, v in p64.items()}
    for i, g in enumerate(grads):
        p, st = qc.adam_step_host(3e-4, g, params=p, state=st)
        for k, t in tp.items():
            t.grad = torch.as_tensor(g[k].copy())
        opt.step()
        for k in p64:
            g64 = g[k].astype(np.float64)
            m64[k] = 0.9 * m64[k] + 0.1 * g64
            v64[k] = 0.999 * v64[k] + 0.001 * g64 * g64
            denom = np.sqrt(v64[k]) / np.sqrt(1 - 0.999 ** (i + 1)) + 1e-8
            p64[k] = p64[k] - 3e-4 / (1 - 0.9 ** (i + 1)) * m64[k] / denom
    e_host = max(np.abs(p[k] - p64[k]).max() for k in p64)
    e_torch = max(np.abs(tp[k].detach().numpy() - p64[k]).max() for k in p64)
    top = max(np.abs(p64[k]).max() for k in p64)
    print(f"adam: host {e_host:.3e} torch-f32 {e_torch:.3e} ratio {e_host / e_torch:.2f} top {top:.3e}")
    assert e_host <= ADAM_FACTOR * e_torch + np.spacing(F32(top))


# ---------------------------------------------------------------- the optimiser state
def test_optimizer_state_round_trips_and_a_failed_load_changes_nothing():
    qc, params, grads = adam_problem(3)
    with pytest.raises(pg.PgxError, match="init_optimizer"):
        qc.optimizer_state_dict()
    qc.init_optimizer(betas=(0.8, 0.99), eps=1e-6)
    sd0 = qc.optimizer_state_dict()
    assert sd0["step"] == 0 and sd0["betas"] == (0.8, 0.99) and sd0["eps"] == 1e-6
    assert list(sd0["exp_avg"]) == list(params) and not any(v.any() for v in sd0["exp_avg_sq"].values())
    _, st = qc.adam_step_host(1e-3, grads[0], params=params)
    qc.load_optimizer_state_dict(st)
    got = qc.optimizer_state_dict()
    assert got["step"] == 1
    for which in ("exp_avg", "exp_avg_sq"):
        for k in params:
            assert np.array_equal(bits(got[which][k].numpy()), bits(st[which][k])), (which, k)
    for fault in ("shape", "missing", "step"):
        bad = {"exp_avg": dict(st["exp_avg"]), "exp_avg_sq": dict(st["exp_avg_sq"]), "step": 7}
        if fault == "shape":
            bad["exp_avg_sq"]["qf1.4.bias"] = np.zeros(6, F32)
        elif fault == "missing":
            del bad["exp_avg_sq"]["qf1.4.bias"]
        else:
            bad["step"] = -1
        with pytest.raises((ValueError, KeyError)):
            qc.load_optimizer_state_dict(bad)
        again = qc.optimizer_state_dict()
        assert again["step"] == 1
        for which in ("exp_avg", "exp_avg_sq"):
            for k in params:
                assert np.array_equal(bits(again[which][k].numpy()), bits(st[which][k])), (fault, which, k)
