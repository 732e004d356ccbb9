"""What TQC's critic update costs per gradient step, the device entries against torch autograd and Adam:
python tools/bench_critic_update.py [--batches 256 4096] [--arch 256 256] [--critics 2] [--quantiles 25]
[--drop 2] [--rounds 12] [--window 200] [--out profiles/bench_critic_update.json]

One process, legs alternated, medians with min / max over ``--rounds`` windows of ``--window`` calls (device
events around each window, which ends in a synchronise), every leg warmed up first, Reach dims (obs 6, action
3), the same seeded weights in every leg.  Per batch size:
  fused         ``QuantileCritic.critic_loss_backward`` + ``adam_step``: the loss, the gradient, the step
  torch         the same lines in torch ops: the critics' forward, ``quantile_huber_loss`` as sb3_contrib writes
                it, ``backward()`` and ``torch.optim.Adam(capturable=True).step()`` with a device ``lr``
each eager and as the replay of one captured graph of ``--window`` calls (``torch.cuda.graph``), as
microseconds per call; where torch's capture fails the leg reports eager alone and ``capture_failed`` says
why.  ``grad`` / ``adam``: the two device entries on their own.  ``update``: the whole captured update,
``sample_into -> action_log_prob_rows -> td_target_rows -> critic_loss_backward_rows -> adam_step ->
polyak_update``, per replayed update.  No figure is a bar: the numbers are reported with their window
spreads.  One JSON line (also written to --out).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402

F = torch.nn.functional
OD, A = 6, 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)} if v else None


class TorchUpdate:
    """sb3_contrib's critic forward, quantile_huber_loss(sum_over_quantiles=False), backward and Adam."""

    def __init__(self, sd, nc, nl, dev):
        self.p = [[(torch.nn.Parameter(sd[f"critic.qf{c}.{2 * l}.weight"].to(dev).clone()),
                    torch.nn.Parameter(sd[f"critic.qf{c}.{2 * l}.bias"].to(dev).clone())) for l in range(nl + 1)]
                  for c in range(nc)]
        self.lr = torch.full((), 3e-4, device=dev)
        self.opt = torch.optim.Adam([t for net in self.p for wb in net for t in wb], lr=self.lr, capturable=True)

    def loss(self, obs, act, target):
        x = torch.cat([obs["achieved_goal"], obs["desired_goal"], obs["observation"], act], dim=1)
        qs = []
        for net in self.p:
            h = x
            for W, b in net[:-1]:
                h = F.relu(F.linear(h, W, b))
            qs.append(F.linear(h, *net[-1]))
        cur = torch.stack(qs, dim=1)
        nq = cur.shape[-1]
        tau = (torch.arange(nq, device=cur.device, dtype=torch.float32) + 0.5) / nq
        delta = target.unsqueeze(1).unsqueeze(-2) - cur.unsqueeze(-1)
        a = delta.abs()
        huber = torch.where(a > 1, a - 0.5, delta ** 2 * 0.5)
        return (torch.abs(tau.view(1, 1, -1, 1) - (delta.detach() < 0).float()) * huber).mean()

    def step(self, obs, act, target):
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(obs, act, target)
        loss.backward()
        self.opt.step()
        return loss


def capture(fn, W):
    """One graph of W calls, or (None, why) where the capture fails."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # outside capture first: libraries pick their algorithms, Adam builds its state
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(W):
                keep = fn()
        g._keep = keep
        g.replay()
        torch.cuda.synchronize()
        return g, None
    except Exception as e:  # noqa: BLE001  (reported, not hidden: the leg then has no captured figure)
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {str(e).splitlines()[0][:200]}"


def run_legs(legs, rounds, W):
    """legs: name -> callable of one call.  Microseconds per call, eager and captured, legs alternated."""
    graphs, failed = {}, {}
    for k, fn in legs.items():
        graphs[k], why = capture(fn, W)
        if why:
            failed[k] = why
    for fn in legs.values():
        for _ in range(W):
            fn()
    torch.cuda.synchronize()
    us = {(k, m): [] for k in legs for m in ("eager", "graph")}
    for _ in range(rounds):
        for k, fn in legs.items():
            us[(k, "eager")].append(timed(lambda: [fn() for _ in range(W)]) / W * 1e3)
            if graphs[k] is not None:
                us[(k, "graph")].append(timed(graphs[k].replay) / W * 1e3)
    out = {"us_per_call": {m: {k: stats(us[(k, m)]) for k in legs} for m in ("eager", "graph")}}
    if failed:
        out["capture_failed"] = failed
    return out


def bench(B, arch, nc, nq, drop, rounds, W):
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    qc = pg.QuantileCritic(obs_dim=OD, action_dim=A, net_arch=arch, n_critics=nc, n_quantiles=nq,
                           top_quantiles_to_drop_per_net=drop, gamma=0.98, device=dev)
    sd = {}
    for k, v in qc.state_dict("both").items():
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        sd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    qc.load_state_dict(sd)
    ws = qc.alloc_workspace(B)
    tu = TorchUpdate(sd, nc, len(arch), dev)
    t = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32), device=dev)  # noqa: E731
    obs = {"observation": t(B, OD), "achieved_goal": t(B, 3), "desired_goal": t(B, 3)}
    act, target = torch.tanh(t(B, A)), t(B, qc.n_target) * 1.5
    loss = torch.zeros(1, device=dev)
    lr = torch.full((1,), 3e-4, device=dev)

    # the two legs compute the same thing (the torch one to f32 reassociation): the loss and one gradient
    a = float(qc.critic_loss_backward(obs, act, target, ws, loss=loss))
    # (autograd.grad, not backward(): no gradient accumulator of the parameters outlives this check on the
    # default stream, where the captured leg below could not run it)
    tl = tu.loss(obs, act, target)
    g_torch, = torch.autograd.grad(tl, tu.p[0][0][0])
    tl = float(tl.detach())
    err = float((qc.grads()["qf0.0.weight"] - g_torch).abs().max())
    if not (abs(a - tl) <= 1e-5 * max(abs(a), 1.0) and err <= 1e-4 * max(float(g_torch.abs().max()), 1e-6)):
        raise SystemExit(f"bench_critic_update: the legs disagree (loss {a} / {tl}, max |dW| difference {err:.3e})")
    del g_torch
    res = {"batch": B, "loss": a, "max_abs_grad_fused_minus_torch": err, "workspace_mib": ws.numel() * 4 / 2 ** 20}

    def fused():
        qc.critic_loss_backward(obs, act, target, ws, loss=loss)
        qc.adam_step(lr)

    res["critic_update"] = run_legs({"fused": fused, "torch": lambda: tu.step(obs, act, target)}, rounds, W)
    res["parts"] = run_legs({"grad": lambda: qc.critic_loss_backward(obs, act, target, ws, loss=loss),
                             "adam": lambda: qc.adam_step(lr)}, rounds, W)

    # the whole update of a gradient step on a HER batch, captured
    N = 16
    buf = pg.HerReplayBuffer(N * 64, device=dev, n_envs=N, obs_dim=OD, action_dim=A, seed=3)
    for step in range(60):
        done = (np.arange(N) % 4 == step % 4).astype(np.uint8)
        f = lambda *s: (rng.standard_normal((N,) + s) * 0.5).astype(np.float32)  # noqa: E731
        buf.add_tensors(f(OD), f(3), f(3), f(A), f(), f(OD), f(3), f(3), done)
    actor = pg.Actor(obs_dim=OD, action_dim=A, n_envs=1, net_arch=arch, kind="gaussian", device=dev)
    asd = {}
    for k, v in actor.state_dict().items():
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        asd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s * 0.5).astype(np.float32))
    actor.load_state_dict(asd)
    b = buf.alloc_batch(B)
    nact, lp = torch.zeros((B, A), device=dev), torch.zeros((B,), device=dev)
    tgt = torch.zeros((B, qc.n_target), device=dev)
    ent = torch.full((1,), 0.2, device=dev)

    def update():
        buf.sample_into(b, draw=0)
        actor.action_log_prob_rows(b, out=(nact, lp))
        qc.td_target_rows(b, nact, lp, ent, out=tgt)
        qc.critic_loss_backward_rows(b, tgt, ws, loss=loss)
        qc.adam_step(lr)
        qc.polyak_update(0.05)

    res["update"] = run_legs({"fused": update}, rounds, W)
    res["update_loss_finite"] = bool(torch.isfinite(loss).all())
    dims = [OD + 6 + A] + list(arch) + [nq]
    res["grad_flops"] = 6 * B * nc * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    for x in (actor, qc, buf):
        x.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--arch", type=int, nargs="+", default=[256, 256])
    ap.add_argument("--critics", type=int, default=2)
    ap.add_argument("--quantiles", type=int, default=25)
    ap.add_argument("--drop", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_critic_update: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_critic_update", "device": torch.cuda.get_device_name(0), "net_arch": a.arch,
           "n_critics": a.critics, "n_quantiles": a.quantiles, "top_quantiles_to_drop_per_net": a.drop,
           "obs_dim": OD, "action_dim": A, "rounds": a.rounds, "window_calls": a.window,
           "tile_env": os.environ.get("PGX_QC_TILE"),
           "runs": [bench(B, tuple(a.arch), a.critics, a.quantiles, a.drop, a.rounds, a.window) for B in a.batches]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
