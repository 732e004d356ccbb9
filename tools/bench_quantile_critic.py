"""What TQC's truncated TD target costs per gradient step, the device critics against their torch restatement:
python tools/bench_quantile_critic.py [--batches 256 4096] [--arch 256 256] [--critics 2] [--quantiles 25]
[--drop 2] [--rounds 12] [--window 200] [--out profiles/bench_quantile_critic.json]

One process, legs alternated, medians with min / max over ``--rounds`` windows of ``--window`` calls (device
events around each window, which ends in a synchronise), every leg warmed up first, Reach dims (obs 6, action
3), the same seeded weights in every leg.  Per batch size:
  fused         ``QuantileCritic.td_target``: one launch
  torch         the same lines restated in torch ops: cat, the Linears, relu, stack, reshape, sort, slice and
                the four arithmetic ops of ``TQC.train``'s no_grad block
each eager and as the replay of one captured graph of ``--window`` calls (``torch.cuda.graph``), as
microseconds per call.  ``bar``: the captured fused launch's median is below the captured torch
restatement's -- the strongest alternative a user has -- by more than the larger min-max window spread of
the two legs.  Also ``critic`` (``QuantileCritic.critic`` alone against the torch forward up to the stack)
and ``polyak`` (``polyak_update`` against torch's ``mul_`` / ``add_`` loop over the parameter list), captured
and eager, and the target's FLOPs from the shapes.  One JSON line (also written to --out).  Needs a GPU."""
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
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


class TorchCritics:
    """sb3_contrib's critic_target forward and TQC.train's no_grad block in torch ops."""

    def __init__(self, sd, prefix, nc, nl, n_target, gamma, dev):
        self.p = [[(sd[f"{prefix}qf{c}.{2 * l}.weight"].to(dev), sd[f"{prefix}qf{c}.{2 * l}.bias"].to(dev))
                   for l in range(nl + 1)] for c in range(nc)]
        self.n_target, self.gamma = n_target, gamma

    def params(self):
        return [t for net in self.p for wb in net for t in wb]

    def quantiles(self, obs, act):
        x = torch.cat([obs["achieved_goal"], obs["desired_goal"], obs["observation"], act], dim=1)
        qs = []
        for net in self.p:
            h = x
            for W, b in net[:-1]:
                h = F.relu(F.linear(h, W, b))
            qs.append(F.linear(h, *net[-1]))
        return torch.stack(qs, dim=1)

    def td_target(self, obs, act, lp, r, d, ent):
        z, _ = torch.sort(self.quantiles(obs, act).reshape(act.shape[0], -1))
        z = z[:, :self.n_target]
        t = z - ent * lp.reshape(-1, 1)
        return r.reshape(-1, 1) + (1 - d.reshape(-1, 1)) * self.gamma * t


def capture(fn, W):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # once outside capture: libraries pick their algorithms
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(W):
            keep = fn()
    g._keep = keep
    g.replay()
    torch.cuda.synchronize()
    return g


def run_legs(legs, rounds, W):
    """legs: name -> callable of one call.  Microseconds per call, eager and captured, legs alternated."""
    graphs = {k: capture(fn, W) for k, fn in legs.items()}
    for fn in legs.values():
        for _ in range(W):
            fn()
    torch.cuda.synchronize()
    us = {(k, m): [] for k in legs for m in ("eager", "graph")}
    for _ in range(rounds):
        for k, fn in legs.items():
            us[(k, "eager")].append(timed(lambda: [fn() for _ in range(W)]) / W * 1e3)
            us[(k, "graph")].append(timed(graphs[k].replay) / W * 1e3)
    return us


def verdict(us, ours, theirs):
    spread = lambda v: max(v) - min(v)  # noqa: E731
    gap = statistics.median(us[(theirs, "graph")]) - statistics.median(us[(ours, "graph")])
    noise = max(spread(us[(ours, "graph")]), spread(us[(theirs, "graph")]))
    return {"us_per_call": {m: {k: stats(us[(k, m)]) for k in (ours, theirs)} for m in ("eager", "graph")},
            "gap_graph_torch_minus_fused_us": gap, "larger_window_spread_us": noise, "bar": gap > noise}


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
    tq = TorchCritics(sd, "critic_target.", nc, len(arch), qc.n_target, 0.98, dev)
    online = TorchCritics(sd, "critic.", nc, len(arch), qc.n_target, 0.98, dev)
    t = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32), device=dev)  # noqa: E731
    obs = {"observation": t(B, OD), "achieved_goal": t(B, 3), "desired_goal": t(B, 3)}
    act, lp, r = torch.tanh(t(B, A)), t(B), t(B)
    d = (torch.arange(B, device=dev) % 5 == 0).float()
    ent = torch.full((1,), 0.2, device=dev)
    out = torch.zeros((B, qc.n_target), device=dev)
    q_out = torch.zeros((B, nc * nq), device=dev)

    # the two legs compute the same thing (the torch one to f32 reassociation)
    a, b = qc.td_target(obs, act, lp, r, d, ent, out=out), tq.td_target(obs, act, lp, r, d, ent)
    err = float((a - b).abs().max())
    scale = float(b.abs().max())
    if not err <= 1e-4 * max(scale, 1.0):
        raise SystemExit(f"bench_quantile_critic: the legs disagree (max |fused - torch| = {err:.3e})")

    res = {"batch": B, "max_abs_fused_minus_torch": err}
    us = run_legs({"fused": lambda: qc.td_target(obs, act, lp, r, d, ent, out=out),
                   "torch": lambda: tq.td_target(obs, act, lp, r, d, ent)}, rounds, W)
    res["td_target"] = verdict(us, "fused", "torch")
    us = run_legs({"fused": lambda: qc.critic(obs, act, target=True, out=q_out),
                   "torch": lambda: tq.quantiles(obs, act)}, rounds, W)
    res["critic"] = verdict(us, "fused", "torch")

    def torch_polyak(tau=0.02):
        for p, tp in zip(online.params(), tq.params()):
            tp.mul_(1 - tau)
            tp.add_(p, alpha=tau)

    us = run_legs({"fused": lambda: qc.polyak_update(0.02), "torch": torch_polyak}, rounds, W)
    res["polyak"] = verdict(us, "fused", "torch")
    dims = [OD + 6 + A] + list(arch) + [nq]
    res["td_target_flops"] = 2 * B * nc * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
    tile = {"16": 16, "32": 32}.get(os.environ.get("PGX_QC_TILE"), 32 if B > 16 else 16)
    res["workgroups"] = (B + tile - 1) // tile
    qc.close()
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
        raise SystemExit("bench_quantile_critic: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_quantile_critic", "device": torch.cuda.get_device_name(0), "net_arch": a.arch,
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
