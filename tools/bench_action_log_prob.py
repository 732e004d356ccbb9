"""What SB3's ``actor.action_log_prob`` costs per gradient step, the device actors against their torch restatement:
python tools/bench_action_log_prob.py [--batches 256 4096] [--arch 256 256] [--rounds 12] [--window 200]
[--out profiles/bench_action_log_prob.json]

One process, legs alternated, medians with min / max over ``--rounds`` windows of ``--window`` calls (device
events around each window, which ends in a synchronise), every leg warmed up first, Reach dims (obs 6, action
3), the same seeded weights in every leg.  Per batch size:
  gaussian      ``Actor.action_log_prob`` (one launch, noise from the device stream) against SB3's
                ``SquashedDiagGaussianDistribution.log_prob_from_params`` lines in torch ops on a noise buffer
                made beforehand (the torch leg draws nothing)
  gsde          ``SdeActor.action_log_prob`` (one launch) against ``StateDependentNoiseDistribution``'s lines in
                torch ops: ``mm`` for the noise and the variance, the ``log1p`` inverse of the squash
  tiles         the two device entries with the 16- and the 32-row tile forced (PGX_ACTOR_LP_TILE /
                PGX_SDE_LP_TILE, read at every launch)
  chain         ``buf.sample_into`` + ``SdeActor.action_log_prob_rows`` + ``QuantileCritic.td_target_rows`` on a
                HER batch, three launches, against the same chain with the torch gSDE restatement in the middle
each eager and as the replay of one captured graph of ``--window`` calls (``torch.cuda.graph``), as
microseconds per call.  ``bar``: the captured device entry's median is below the captured torch restatement's
by more than the larger min-max window spread of the two legs.  One JSON line (also written to --out).  Needs a
GPU."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402
from bench_quantile_critic import run_legs, stats, verdict  # noqa: E402

F = torch.nn.functional
OD, A = 6, 3
EPS = 1.1920929e-7


def features(obs):
    return torch.cat([obs["achieved_goal"], obs["desired_goal"], obs["observation"]], dim=1)


def trunk(x, layers):
    for W, b in layers:
        x = F.relu(F.linear(x, W, b))
    return x


def torch_gaussian(p, obs, eps):
    """sac/policies.py Actor.action_log_prob with the squashed Gaussian, on given noise."""
    h = trunk(features(obs), p["trunk"])
    mean = F.linear(h, *p["mu"])
    log_std = torch.clamp(F.linear(h, *p["log_std"]), -20.0, 2.0)
    std = torch.exp(log_std)
    g = mean + std * eps
    a = torch.tanh(g)
    lp = (-((g - mean) ** 2) / (2 * std * std) - log_std - 0.9189385).sum(1)
    return a, lp - torch.log(1 - a ** 2 + 1e-6).sum(1)


def torch_gsde(p, obs, clip_mean=2.0):
    """The same with use_sde=True: get_noise on the one exploration_mat, the variance, the inverse of the squash."""
    h = trunk(features(obs), p["trunk"])
    mean = F.hardtanh(F.linear(h, *p["mu"]), -clip_mean, clip_mean)
    noise = torch.mm(h, p["Eb"])
    var = torch.mm(h ** 2, p["std"] ** 2)
    scale = torch.sqrt(var + 1e-6)
    a = torch.tanh(mean + noise)
    x = a.clamp(-1.0 + EPS, 1.0 - EPS)
    g = 0.5 * (x.log1p() - (-x).log1p())
    lp = (-((g - mean) ** 2) / (2 * scale * scale) - torch.log(scale) - 0.9189385).sum(1)
    return a, lp - torch.log(1 - torch.tanh(g) ** 2 + 1e-6).sum(1)


def seeded(policy, rng, log_std=None):
    sd = {}
    for k, v in policy.state_dict().items():
        if k == "log_std" and v.dim() == 2 and log_std is not None:
            sd[k] = torch.full(tuple(v.shape), log_std)
            continue
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        sd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    policy.load_state_dict(sd)
    return sd


def with_tile(var, tile, fn):
    def call():
        if tile is None:
            os.environ.pop(var, None)
        else:
            os.environ[var] = tile
        return fn()
    return call


def bench(B, arch, rounds, W):
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    nl = len(arch)
    t = lambda *s: torch.as_tensor(rng.standard_normal(s).astype(np.float32), device=dev)  # noqa: E731
    obs = {"observation": t(B, OD), "achieved_goal": t(B, 3), "desired_goal": t(B, 3)}
    act, lp = torch.zeros((B, A), device=dev), torch.zeros((B,), device=dev)
    res = {"batch": B}

    ga = pg.Actor(obs_dim=OD, action_dim=A, n_envs=1, net_arch=arch, kind="gaussian", device=dev)
    sd = seeded(ga, rng)
    gp = {"trunk": [(sd[f"latent_pi.{2 * i}.weight"].to(dev), sd[f"latent_pi.{2 * i}.bias"].to(dev)) for i in range(nl)],
          "mu": (sd["mu.weight"].to(dev), sd["mu.bias"].to(dev)),
          "log_std": (sd["log_std.weight"].to(dev), sd["log_std.bias"].to(dev))}
    eps = t(B, A)
    a0, l0 = ga.action_log_prob(obs, eps=eps)
    a1, l1 = torch_gaussian(gp, obs, eps)
    res["gaussian_max_abs_fused_minus_torch"] = [float((a0 - a1).abs().max()), float((l0 - l1).abs().max())]
    g_fused = lambda: ga.action_log_prob(obs, out=(act, lp))  # noqa: E731
    us = run_legs({"fused": with_tile("PGX_ACTOR_LP_TILE", None, g_fused), "torch": lambda: torch_gaussian(gp, obs, eps)},
                  rounds, W)
    res["gaussian"] = verdict(us, "fused", "torch")

    sa = pg.SdeActor(obs_dim=OD, action_dim=A, n_envs=1, net_arch=arch, device=dev)
    sd = seeded(sa, rng, log_std=-3.0)
    sa.reset_batch_noise()
    sp = {"trunk": [(sd[f"latent_pi.{2 * i}.weight"].to(dev), sd[f"latent_pi.{2 * i}.bias"].to(dev)) for i in range(nl)],
          "mu": (sd["mu.0.weight"].to(dev), sd["mu.0.bias"].to(dev)), "Eb": sa.exploration_mat, "std": sa.std}
    a0, l0 = sa.action_log_prob(obs)
    a1, l1 = torch_gsde(sp, obs)
    res["gsde_max_abs_fused_minus_torch"] = [float((a0 - a1).abs().max()), float((l0 - l1).abs().max())]
    s_fused = lambda: sa.action_log_prob(obs, out=(act, lp))  # noqa: E731
    us = run_legs({"fused": with_tile("PGX_SDE_LP_TILE", None, s_fused), "torch": lambda: torch_gsde(sp, obs)}, rounds, W)
    res["gsde"] = verdict(us, "fused", "torch")

    us = run_legs({"gaussian16": with_tile("PGX_ACTOR_LP_TILE", "16", g_fused),
                   "gaussian32": with_tile("PGX_ACTOR_LP_TILE", "32", g_fused),
                   "gsde16": with_tile("PGX_SDE_LP_TILE", "16", s_fused),
                   "gsde32": with_tile("PGX_SDE_LP_TILE", "32", s_fused)}, rounds, W)
    res["tiles_graph_us_per_call"] = {k: stats(us[(k, "graph")]) for k in ("gaussian16", "gaussian32", "gsde16", "gsde32")}
    for var in ("PGX_ACTOR_LP_TILE", "PGX_SDE_LP_TILE"):
        os.environ.pop(var, None)

    # the chain of a gradient step's no-grad half on a HER batch
    N = 16
    buf = pg.HerReplayBuffer(N * 64, device=dev, n_envs=N, obs_dim=OD, action_dim=A, seed=3)
    for step in range(60):
        done = (np.arange(N) % 4 == step % 4).astype(np.uint8)
        f = lambda *s: (rng.standard_normal((N,) + s) * 0.5).astype(np.float32)  # noqa: E731
        buf.add_tensors(f(OD), f(3), f(3), f(A), f(), f(OD), f(3), f(3), done)
    qc = pg.QuantileCritic(obs_dim=OD, action_dim=A, net_arch=arch, device=dev)
    seeded_qc = {}
    for k, v in qc.state_dict("both").items():
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        seeded_qc[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    qc.load_state_dict(seeded_qc)
    b = buf.alloc_batch(B)
    ent = torch.full((1,), 0.2, device=dev)
    target = torch.zeros((B, qc.n_target), device=dev)
    nxt = {"observation": b["next_obs"], "achieved_goal": b["next_achieved_goal"], "desired_goal": b["next_desired_goal"]}

    def chain_fused():
        buf.sample_into(b, draw=0)
        sa.action_log_prob_rows(b, out=(act, lp))
        return qc.td_target_rows(b, act, lp, ent, out=target)

    def chain_torch():
        buf.sample_into(b, draw=0)
        a, l = torch_gsde(sp, nxt)
        return qc.td_target_rows(b, a, l, ent, out=target), a, l

    us = run_legs({"fused": chain_fused, "torch": chain_torch}, rounds, W)
    res["chain"] = verdict(us, "fused", "torch")
    for x in (ga, sa, qc, buf):
        x.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--arch", type=int, nargs="+", default=[256, 256])
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_action_log_prob: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_action_log_prob", "device": torch.cuda.get_device_name(0), "net_arch": a.arch, "obs_dim": OD,
           "action_dim": A, "rounds": a.rounds, "window_calls": a.window,
           "runs": [bench(B, tuple(a.arch), a.rounds, a.window) for B in a.batches]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
