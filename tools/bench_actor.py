"""What a policy inside the step loop costs per env step, the device actor against its torch restatement:
python tools/bench_actor.py [--env PandaReach-v3] [--envs 4096] [--arch 256 256] [--rounds 12]
[--window 200] [--out profiles/bench_actor.json]

One process, legs alternated, medians with min / max over ``--rounds`` windows of ``--window`` steps
(device events around each window, which ends in a synchronise), warm-up past the first episode of every
leg, episode phases staggered, Gaussian actor with the same seeded weights in every leg:
  bare          the env step alone, actions from a static buffer of uniform random ones
  bare_recorded the env step alone, actions from a static buffer recorded from the device actor's own loop
  actor         plus the device actor (one launch, device noise), closed loop
  torch         plus the same forward restated in torch ops (cat, 4 linear, relu, clamp, exp, randn, tanh,
                copy into the action buffer), closed loop
each eager (``step_tensors``) and as the replay of one captured graph of ``--window`` steps
(``capture_steps`` / ``Actor.capture_rollout`` / the torch ops under ``torch.cuda.graph``), as ms per step
and as ms added over ``bare`` (and over ``bare_recorded``) of the same mode in the same run.  ``bar``: the
captured device actor adds less than the captured torch restatement -- the strongest alternative -- by
more than the larger min-max window spread of the two legs.  The step's own time depends on the actions it is given (``bare`` steps on
uniform random ones, the policy legs on what the policy chose), so ``added`` holds that difference too;
``forward_alone_ms`` is each forward by itself, a graph of ``--window`` launches with no env step between
them.  Also the forward's FLOPs from the shapes.  One JSON line (also written to --out).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402

LEGS = ("bare", "bare_recorded", "actor", "torch")
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


class TorchActor:
    """SB3's SAC actor forward in torch ops on the env's buffers, writing a persistent action buffer."""

    def __init__(self, sd, n, A, dev):
        self.p = {k: v.to(dev) for k, v in sd.items()}
        self.n_layers = sum(1 for k in sd if k.startswith("latent_pi.") and k.endswith(".weight"))
        self.actions = torch.zeros((n, A), dtype=torch.float32, device=dev)

    def __call__(self, obs):
        p = self.p
        h = torch.cat([obs["achieved_goal"], obs["desired_goal"], obs["observation"]], dim=1)
        for i in range(self.n_layers):
            h = F.relu(F.linear(h, p[f"latent_pi.{2 * i}.weight"], p[f"latent_pi.{2 * i}.bias"]))
        mean = F.linear(h, p["mu.weight"], p["mu.bias"])
        log_std = torch.clamp(F.linear(h, p["log_std.weight"], p["log_std.bias"]), -20.0, 2.0)
        self.actions.copy_(torch.tanh(mean + torch.exp(log_std) * torch.randn_like(mean)))
        return self.actions


def bench(env_id, N, arch, rounds, W):
    dev = "cuda:0"
    modes = ("eager", "graph")
    env = {(leg, m): pg.PandaVecEnv(env_id, num_envs=N, device=dev, seed=0) for leg in LEGS for m in modes}
    od, A = env[("bare", "eager")].obs_dim, env[("bare", "eager")].action_dim
    rng = np.random.default_rng(0)
    actor = {m: pg.Actor(env=env[("actor", m)], net_arch=arch, kind="gaussian", seed=1) for m in modes}
    sd = {}
    for k, v in actor["eager"].state_dict().items():
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        sd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    for a in actor.values():
        a.load_state_dict(sd)
    tactor = {m: TorchActor(sd, N, A, dev) for m in modes}
    gen = torch.Generator(device=dev).manual_seed(2)
    static = (torch.rand((W, N, A), device=dev, generator=gen) * 2 - 1).contiguous()
    obs = {key: e.reset_tensors(episode_phase="staggered") for key, e in env.items()}

    def eager_window(leg):
        e = env[(leg, "eager")]
        o = obs[(leg, "eager")]
        for i in range(W):
            a = buffers[leg][i] if leg in buffers else (actor["eager"](o) if leg == "actor" else tactor["eager"](o))
            o = e.step_tensors(a)[0]

    # W steps of the device actor's own actions, for bare_recorded (an env of its own, so open loop)
    rec_env = pg.PandaVecEnv(env_id, num_envs=N, device=dev, seed=0)
    rec_actor = pg.Actor(env=rec_env, net_arch=arch, kind="gaussian", seed=1)
    rec_actor.load_state_dict(sd)
    recorded = torch.empty_like(static)
    o = rec_env.reset_tensors(episode_phase="staggered")
    for i in range(W):
        recorded[i].copy_(rec_actor(o))
        o = rec_env.step_tensors(recorded[i])[0]
    torch.cuda.synchronize()
    rec_actor.close()
    rec_env.close()
    buffers = {"bare": static, "bare_recorded": recorded}

    horizon = int(env[("bare", "eager")].spec.max_episode_steps)
    for leg in LEGS:   # warm-up: past the first episode of every phase
        for _ in range(horizon // W + 2):
            eager_window(leg)
    torch.cuda.synchronize()

    graphs = {"bare": env[("bare", "graph")].capture_steps(W, static),
              "bare_recorded": env[("bare_recorded", "graph")].capture_steps(W, recorded),
              "actor": actor["graph"].capture_rollout(env[("actor", "graph")], W)}
    e, o, t = env[("torch", "graph")], obs[("torch", "graph")], tactor["graph"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # the ops once outside capture: libraries pick their algorithms
        t(o)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(W):
            e._enqueue_step(t(o), "pgx_step (capture)")
    graphs["torch"] = g
    for leg in LEGS:
        for _ in range(horizon // W + 2):
            graphs[leg].replay()
    torch.cuda.synchronize()

    ms = {(leg, m): [] for leg in LEGS for m in modes}
    for _ in range(rounds):
        for leg in LEGS:
            ms[(leg, "eager")].append(timed(lambda: eager_window(leg)) / W)
            ms[(leg, "graph")].append(timed(graphs[leg].replay) / W)
    for e in env.values():
        e.raise_device_errors()

    # the forwards alone, on the observation buffers as they stand: graphs of W launches, no env step
    fwd = {}
    for leg, e_key, fn in (("actor", ("actor", "eager"), lambda o: actor["eager"]._launch(o, False, None)),
                           ("torch", ("torch", "eager"), tactor["eager"])):
        o = env[e_key]._obs_dict()
        torch.cuda.synchronize()
        fg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(fg):
            for _ in range(W):
                fn(o)
        fg.replay()
        torch.cuda.synchronize()
        fwd[leg] = (fg, [])
    for _ in range(rounds):
        for leg in fwd:
            fwd[leg][1].append(timed(fwd[leg][0].replay) / W)

    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = lambda v: max(v) - min(v)  # noqa: E731
    added = {m: {leg: med[(leg, m)] - med[("bare", m)] for leg in ("actor", "torch")} for m in modes}
    added_rec = {m: {leg: med[(leg, m)] - med[("bare_recorded", m)] for leg in ("actor", "torch")} for m in modes}
    gap = added["graph"]["torch"] - added["graph"]["actor"]
    noise = max(spread(ms[("actor", "graph")]), spread(ms[("torch", "graph")]))
    dims = [od + 6] + list(arch)
    flops = 2 * N * (sum(dims[i] * dims[i + 1] for i in range(len(arch))) + 2 * A * dims[-1])
    out = {"env_id": env_id, "n_envs": N, "net_arch": list(arch), "kind": "gaussian", "obs_dim": od, "action_dim": A,
           "rounds": rounds, "window_steps": W,
           "ms_per_step": {m: {leg: stats(ms[(leg, m)]) for leg in LEGS} for m in modes},
           "added_ms_per_step": added, "added_over_bare_recorded_ms_per_step": added_rec,
           "gap_graph_torch_minus_actor_ms": gap, "larger_window_spread_ms": noise,
           "bar": gap > noise, "forward_alone_ms": {leg: stats(v) for leg, (_, v) in fwd.items()}, "forward_flops": flops,
           "noise_steps": {m: a.noise_step for m, a in actor.items()},
           "step_kernel": env[("bare", "eager")].step_kernel()}
    for a in actor.values():
        a.close()
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_actor: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_actor", "device": torch.cuda.get_device_name(0),
           "run": bench(a.env, a.envs, tuple(a.arch), a.rounds, a.window)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
