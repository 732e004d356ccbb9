"""What gSDE exploration costs inside the step loop, the device gSDE actor against its torch restatement:
python tools/bench_sde_actor.py [--env PandaReach-v3] [--envs 4096] [--arch 256 256] [--rounds 12]
[--window 200] [--train-freq 8] [--out profiles/bench_sde_actor.json]

One process, legs alternated, medians with min / max over ``--rounds`` windows of ``--window`` (device
events around each window, which ends in a synchronise), warm-up past the first episode, episode phases
staggered, the same seeded weights in every leg.  Everything timed is the replay of a captured graph:
  forward_alone   ``--window`` forwards on the observation buffers as they stand, no env step:
      sde     SdeActor's kernel (trunk, mu, the per-env noise chain, tanh)
      torch   the same forward in torch ops (cat, linears, relu, hardtanh, bmm over [N, H, A], add, tanh, copy
              into the action buffer)
      actor   pg.Actor's plain Gaussian forward (state-dependent log_std head, device eps): the cost of gSDE
              is ``sde - actor``
  reset_alone     ``--window`` resamples of every env's matrix:
      sde     SdeActor.reset_noise (one launch)
      torch   ``torch.mul(torch.randn((N, H, A)), std, out=E)``
  rollout         ``--window`` closed-loop steps as ``window / train_freq`` rollouts of one resample and
                  ``train_freq`` steps (SB3 collect_rollouts with ``sde_sample_freq=-1``), ms per step:
      step    the env step alone on actions recorded from the device gSDE loop
      sde     SdeActor.capture_rollout
      torch   the torch restatement in its place (randn resample, torch forward, env step)
``bar_forward`` / ``bar_rollout``: the device leg is faster than the torch leg by more than three times the
larger min-max window spread of the two.  One JSON line (also written to --out).  Needs a GPU."""
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def spread(v):
    return max(v) - min(v)


class TorchSdeActor:
    """SB3's gSDE actor forward and sample_weights in torch ops, writing persistent buffers."""

    def __init__(self, sd, n, H, A, clip, dev):
        self.p = {k: v.to(dev) for k, v in sd.items()}
        self.n_layers = sum(1 for k in sd if k.startswith("latent_pi.") and k.endswith(".weight"))
        self.clip, self.n, self.H, self.A, self.dev = clip, n, H, A, dev
        self.std = torch.exp(self.p["log_std"])
        self.E = torch.zeros((n, H, A), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((n, A), dtype=torch.float32, device=dev)

    def reset_noise(self):
        torch.mul(torch.randn((self.n, self.H, self.A), device=self.dev), self.std, out=self.E)

    def __call__(self, obs):
        p = self.p
        h = torch.cat([obs["achieved_goal"], obs["desired_goal"], obs["observation"]], dim=1)
        for i in range(self.n_layers):
            h = F.relu(F.linear(h, p[f"latent_pi.{2 * i}.weight"], p[f"latent_pi.{2 * i}.bias"]))
        mean = F.hardtanh(F.linear(h, p["mu.0.weight"], p["mu.0.bias"]), -self.clip, self.clip)
        noise = torch.bmm(h.unsqueeze(1), self.E).squeeze(1)
        self.actions.copy_(torch.tanh(mean + noise))
        return self.actions


def capture(fn, warm=True):
    """fn's launches as one graph; the torch ops run once outside capture first (libraries pick algorithms)."""
    if warm:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn(1)
        torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn(None)
    return g


def bench(env_id, N, arch, rounds, W, K):
    dev = "cuda:0"
    legs = ("step", "sde", "torch")
    env = {leg: pg.PandaVecEnv(env_id, num_envs=N, device=dev, seed=0) for leg in legs}
    od, A, H = env["sde"].obs_dim, env["sde"].action_dim, arch[-1]
    rng = np.random.default_rng(0)
    sde = pg.SdeActor(env=env["sde"], net_arch=arch, seed=1)
    sd = {}
    for k, v in sde.state_dict().items():
        if k == "log_std":
            sd[k] = torch.full(tuple(v.shape), -3.0)
        else:
            s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
            sd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    sde.load_state_dict(sd)
    tsde = TorchSdeActor(sd, N, H, A, sde.clip_mean, dev)
    gauss = pg.Actor(env=env["sde"], net_arch=arch, kind="gaussian", seed=1)
    gsd = {}
    for k, v in gauss.state_dict().items():
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        gsd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    gauss.load_state_dict(gsd)
    obs = {leg: e.reset_tensors(episode_phase="staggered") for leg, e in env.items()}
    horizon = int(env["sde"].spec.max_episode_steps)

    # W steps of the device gSDE loop's own actions, for the step-alone leg (an env of its own)
    rec_env = pg.PandaVecEnv(env_id, num_envs=N, device=dev, seed=0)
    rec = pg.SdeActor(env=rec_env, net_arch=arch, seed=1)
    rec.load_state_dict(sd)
    recorded = torch.empty((W, N, A), dtype=torch.float32, device=dev)
    o = rec_env.reset_tensors(episode_phase="staggered")
    for i in range(W):
        if i % K == 0:
            rec.reset_noise()
        recorded[i].copy_(rec(o))
        o = rec_env.step_tensors(recorded[i])[0]
    torch.cuda.synchronize()
    rec.close()
    rec_env.close()

    def torch_rollouts(n):
        e, o = env["torch"], obs["torch"]
        for j in range(W if n is None else K * n):
            if j % K == 0:
                tsde.reset_noise()
            e._enqueue_step(tsde(o), "pgx_step (capture)")

    graphs = {"step": env["step"].capture_steps(W, recorded),
              "sde": sde.capture_rollout(env["sde"], W, sde_sample_freq=K),
              "torch": capture(torch_rollouts)}
    for leg in legs:   # warm-up: past the first episode of every phase
        for _ in range(horizon // W + 2):
            graphs[leg].replay()
    torch.cuda.synchronize()
    roll = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            roll[leg].append(timed(graphs[leg].replay) / W)
    for e in env.values():
        e.raise_device_errors()

    # the forwards and the resamples alone, on the observation buffers as they stand: graphs of W launches
    o_sde, o_torch = env["sde"]._obs_dict(), env["torch"]._obs_dict()
    alone = {
        ("forward", "sde"): capture(lambda n: [sde._launch(o_sde, False) for _ in range(n or W)], warm=False),
        ("forward", "torch"): capture(lambda n: [tsde(o_torch) for _ in range(n or W)]),
        ("forward", "actor"): capture(lambda n: [gauss._launch(o_sde, False, None) for _ in range(n or W)], warm=False),
        ("reset", "sde"): capture(lambda n: [sde.reset_noise() for _ in range(n or W)], warm=False),
        ("reset", "torch"): capture(lambda n: [tsde.reset_noise() for _ in range(n or W)]),
    }
    for g in alone.values():
        g.replay()
    torch.cuda.synchronize()
    ms = {k: [] for k in alone}
    for _ in range(rounds):
        for k, g in alone.items():
            ms[k].append(timed(g.replay) / W)

    med = lambda v: statistics.median(v)  # noqa: E731
    fwd_gap = med(ms[("forward", "torch")]) - med(ms[("forward", "sde")])
    fwd_noise = max(spread(ms[("forward", "torch")]), spread(ms[("forward", "sde")]))
    roll_gap = med(roll["torch"]) - med(roll["sde"])
    roll_noise = max(spread(roll["torch"]), spread(roll["sde"]))
    dims = [od + 6] + list(arch)
    flops = 2 * N * (sum(dims[i] * dims[i + 1] for i in range(len(arch))) + 2 * A * H)
    out = {"env_id": env_id, "n_envs": N, "net_arch": list(arch), "obs_dim": od, "action_dim": A, "rounds": rounds,
           "window": W, "train_freq": K, "matrix_bytes": 4 * N * H * A,
           "forward_alone_ms": {leg: stats(ms[("forward", leg)]) for leg in ("sde", "torch", "actor")},
           "gsde_over_gaussian_forward_ms": med(ms[("forward", "sde")]) - med(ms[("forward", "actor")]),
           "reset_alone_ms": {leg: stats(ms[("reset", leg)]) for leg in ("sde", "torch")},
           "rollout_ms_per_step": {leg: stats(roll[leg]) for leg in legs},
           "forward_gap_torch_minus_sde_ms": fwd_gap, "forward_larger_window_spread_ms": fwd_noise,
           "bar_forward": fwd_gap > 3.0 * fwd_noise,
           "rollout_gap_torch_minus_sde_ms": roll_gap, "rollout_larger_window_spread_ms": roll_noise,
           "bar_rollout": roll_gap > 3.0 * roll_noise,
           "forward_flops": flops, "noise_generation": sde.noise_generation,
           "step_kernel": env["step"].step_kernel()}
    sde.close()
    gauss.close()
    for e in env.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env", default="PandaReach-v3")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--arch", type=int, nargs="+", default=[256, 256])
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--train-freq", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sde_actor: no HIP device (there is no CPU fallback)")
    if a.window % a.train_freq:
        raise SystemExit("bench_sde_actor: --window must be a multiple of --train-freq")
    res = {"tool": "bench_sde_actor", "device": torch.cuda.get_device_name(0),
           "run": bench(a.env, a.envs, tuple(a.arch), a.rounds, a.window, a.train_freq)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
