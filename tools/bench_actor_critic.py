"""What PPO's policy costs on the device, the actor-critic kernels against their torch restatement:
python tools/bench_actor_critic.py [--env PandaReach-v3] [--envs 4096] [--arch 256 256] [--rounds 12]
[--window 200] [--out profiles/bench_actor_critic.json]

One process, one GPU, legs alternated, medians with min / max over ``--rounds`` windows of ``--window``
steps (device events around each window, which ends in a synchronise), warm-up before the first timed
window, episode phases staggered, ``net_arch`` for both trunks, the same seeded weights in every leg:
  forward   the forward alone (action, clipped action, value, log_prob), a graph of ``--window`` launches
            with no env step between them: the device kernel; the torch restatement (cat, two
            nn.Sequential trunks, the heads, randn, Normal.log_prob, clamp, copies into persistent
            buffers) captured the same way; the restatement eager
  values    the values launch alone on the terminal-observation buffers, a graph of ``--window`` launches:
            with the truncated flags of ``--window`` recorded steady-state steps as its ``need`` mask against
            no mask and against an all-zero mask (a step in which no env was cut off), and the share of
            workgroup tiles the recorded flags touch
  rollout   SB3's collect_rollouts for ``--window`` steps as one graph, ms per step: ``capture_steps`` on the
            clipped actions recorded from the device policy's own loop (the env alone); the device
            ``ActorCritic.capture_rollout``; the same enqueue sequence with the torch restatement in place of
            the two kernels (its terminal values unmasked)
and the ratios torch / device.  No target is fixed in advance; where the device path is not faster the
ratio says so.  One JSON line (also written to --out).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402
from panda_gym_amd.rollout import step_buffers, terminal_observation  # noqa: E402

nn = torch.nn


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


class TorchActorCritic:
    """SB3's ActorCriticPolicy forward in torch ops on the env's buffers, writing persistent outputs."""

    def __init__(self, sd, n, in_dim, arch, A, dev):
        def trunk(net):
            layers, k = [], in_dim
            for i, w in enumerate(arch):
                lin = nn.Linear(k, w)
                lin.weight.data.copy_(sd[f"mlp_extractor.{net}.{2 * i}.weight"])
                lin.bias.data.copy_(sd[f"mlp_extractor.{net}.{2 * i}.bias"])
                layers += [lin, nn.ReLU()]
                k = w
            return nn.Sequential(*layers).to(dev)

        self.pi, self.vf = trunk("policy_net"), trunk("value_net")
        self.action_net, self.value_net = nn.Linear(arch[-1], A).to(dev), nn.Linear(arch[-1], 1).to(dev)
        for mod, name in ((self.action_net, "action_net"), (self.value_net, "value_net")):
            mod.weight.data.copy_(sd[f"{name}.weight"])
            mod.bias.data.copy_(sd[f"{name}.bias"])
        self.log_std = sd["log_std"].to(dev)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        self.actions, self.clipped_actions, self.values, self.log_probs = z(n, A), z(n, A), z(n), z(n)
        self.terminal_values, self.last_values = z(n), z(n)

    @staticmethod
    def features(obs):
        return torch.cat([obs["achieved_goal"], obs["desired_goal"], obs["observation"]], dim=1)

    @torch.no_grad()
    def __call__(self, obs):
        x = self.features(obs)
        mean = self.action_net(self.pi(x))
        dist = torch.distributions.Normal(mean, torch.exp(self.log_std), validate_args=False)
        a = mean + dist.scale * torch.randn_like(mean)
        self.actions.copy_(a)
        self.clipped_actions.copy_(torch.clamp(a, -1.0, 1.0))
        self.values.copy_(self.value_net(self.vf(x)).flatten())
        self.log_probs.copy_(dist.log_prob(a).sum(dim=1))

    @torch.no_grad()
    def predict_values(self, obs, out):
        out.copy_(self.value_net(self.vf(self.features(obs))).flatten())


def graph_of(fn, warm=True):
    if warm:   # the ops once outside capture, on a side stream: libraries pick their algorithms
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def bench(env_id, N, arch, rounds, W):
    dev = "cuda:0"
    legs = ("bare_recorded", "device", "torch")
    env = {leg: pg.PandaVecEnv(env_id, num_envs=N, device=dev, seed=0) for leg in legs}
    od, A = env["device"].obs_dim, env["device"].action_dim
    rng = np.random.default_rng(0)
    ac = pg.ActorCritic(env=env["device"], net_arch=list(arch), seed=1)
    sd = {}
    for k, v in ac.state_dict().items():
        s = 1.0 / np.sqrt(v.shape[1]) if v.dim() == 2 else 0.5
        sd[k] = torch.as_tensor((rng.standard_normal(tuple(v.shape)) * s).astype(np.float32))
    sd["log_std"] = torch.full((A,), -0.5)
    ac.load_state_dict(sd)
    tac = TorchActorCritic(sd, N, od + 6, arch, A, dev)
    obs = {leg: e.reset_tensors(episode_phase="staggered") for leg, e in env.items()}
    horizon = int(env["device"].spec.max_episode_steps)

    # W steady-state steps of the device policy's own loop on an env of its own: the clipped actions for the
    # bare leg, the truncated flags and terminal observations for the values legs
    rec_env = pg.PandaVecEnv(env_id, num_envs=N, device=dev, seed=0)
    rec_ac = pg.ActorCritic(env=rec_env, net_arch=list(arch), seed=1)
    rec_ac.load_state_dict(sd)
    recorded = torch.empty((W, N, A), dtype=torch.float32, device=dev)
    flags = torch.empty((W, N), dtype=torch.uint8, device=dev)
    o = rec_env.reset_tensors(episode_phase="staggered")
    for i in range(horizon + W):
        rec_ac(o)
        o = rec_env.step_tensors(rec_ac.clipped_actions)[0]
        if i >= horizon:
            recorded[i - horizon].copy_(rec_ac.clipped_actions)
            flags[i - horizon].copy_(rec_env.truncated)
    torch.cuda.synchronize()
    tobs = {k: v.clone() for k, v in terminal_observation(rec_env).items()}
    rec_ac.close()
    rec_env.close()
    tile = 32 if N >= 4096 else 16
    f = flags.cpu().numpy().astype(bool)
    pad = (-N) % tile
    touched = np.pad(f, ((0, 0), (0, pad))).reshape(W, -1, tile).any(axis=2)
    mask_stats = {"tile_envs": tile, "truncated_envs_per_step": float(f.sum(axis=1).mean()),
                  "tiles_touched_share": float(touched.mean()), "steps_without_a_flag_share": float((~f.any(axis=1)).mean())}

    # ---- the forward alone
    o = env["device"]._obs_dict()
    fwd = {"device": graph_of(lambda: [ac._launch(o, False, None) for _ in range(W)], warm=False),
           "torch_graph": graph_of(lambda: [tac(o) for _ in range(W)])}
    runs = {"device": fwd["device"].replay, "torch_graph": fwd["torch_graph"].replay,
            "torch_eager": lambda: [tac(o) for _ in range(W)]}
    # ---- the values launch alone
    pv = torch.zeros(N, dtype=torch.float32, device=dev)
    no_flag = torch.zeros(N, dtype=torch.uint8, device=dev)
    val = {"masked": graph_of(lambda: [ac._launch_values(tobs, flags[i], pv) for i in range(W)], warm=False),
           "unmasked": graph_of(lambda: [ac._launch_values(tobs, None, pv) for _ in range(W)], warm=False),
           "no_flag": graph_of(lambda: [ac._launch_values(tobs, no_flag, pv) for _ in range(W)], warm=False),
           "torch_graph": graph_of(lambda: [tac.predict_values(tobs, pv) for _ in range(W)])}
    runs.update({f"values_{k}": g.replay for k, g in val.items()})
    # ---- the rollout
    buf = {leg: pg.RolloutBuffer(W, env=env[leg], device=dev, gamma=0.99, gae_lambda=0.9) for leg in ("device", "torch")}
    for leg, b in buf.items():
        b.set_last(obs[leg])
    roll = {"bare_recorded": env["bare_recorded"].capture_steps(W, recorded),
            "device": ac.capture_rollout(env["device"], buf["device"])}
    e, b = env["torch"], buf["torch"]
    t_obs, t_rew, t_term, t_trunc = step_buffers(e)
    t_tobs = terminal_observation(e)

    def torch_rollout():
        for _ in range(W):
            tac(t_obs)
            e._enqueue_step(tac.clipped_actions, "pgx_step (capture)")
            tac.predict_values(t_tobs, tac.terminal_values)
            b._launch_add(tac.actions, t_rew, tac.values, tac.log_probs, tac.terminal_values, t_obs, t_term, t_trunc)
        tac.predict_values(t_obs, tac.last_values)
        b.enqueue_returns_and_advantage(tac.last_values)

    roll["torch"] = graph_of(torch_rollout, warm=False)   # (warm already; a warm run here would step the env)

    def replay_rollout(leg):
        if leg in buf:
            buf[leg].reset()
        roll[leg].replay()

    runs.update({f"rollout_{leg}": (lambda leg=leg: replay_rollout(leg)) for leg in legs})
    for name, fn in runs.items():   # warm-up: clocks, caches, and the rollouts past the first episode of every phase
        for _ in range(horizon // W + 2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            ms[name].append(timed(fn) / W)
    for leg in buf:
        buf[leg].raise_device_errors()
    for x in env.values():
        x.raise_device_errors()
    med = {k: statistics.median(v) for k, v in ms.items()}
    added = {leg: med[f"rollout_{leg}"] - med["rollout_bare_recorded"] for leg in ("device", "torch")}
    dims = [od + 6] + list(arch)
    trunk_flops = sum(dims[i] * dims[i + 1] for i in range(len(arch)))
    out = {"env_id": env_id, "n_envs": N, "net_arch": {"pi": list(arch), "vf": list(arch)}, "obs_dim": od, "action_dim": A,
           "rounds": rounds, "window_steps": W,
           "forward_alone_ms": {k: stats(ms[k]) for k in ("device", "torch_graph", "torch_eager")},
           "forward_ratio_torch_graph_over_device": med["torch_graph"] / med["device"],
           "forward_ratio_torch_eager_over_device": med["torch_eager"] / med["device"],
           "forward_flops": 2 * N * (2 * trunk_flops + (A + 1) * dims[-1]),
           "values_alone_ms": {k: stats(ms[f"values_{k}"]) for k in val}, "values_mask": mask_stats,
           "values_ratio_unmasked_over_masked": med["values_unmasked"] / med["values_masked"],
           "values_ratio_unmasked_over_no_flag": med["values_unmasked"] / med["values_no_flag"],
           "values_ratio_torch_graph_over_unmasked": med["values_torch_graph"] / med["values_unmasked"],
           "rollout_ms_per_step": {leg: stats(ms[f"rollout_{leg}"]) for leg in legs},
           "rollout_added_over_bare_recorded_ms_per_step": added,
           "rollout_added_ratio_torch_over_device": added["torch"] / added["device"],
           "rollout_ratio_torch_over_device": med["rollout_torch"] / med["rollout_device"],
           "noise_steps": ac.noise_step, "step_kernel": env["device"].step_kernel()}
    for x in buf.values():
        x.close()
    ac.close()
    for x in env.values():
        x.close()
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
        raise SystemExit("bench_actor_critic: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_actor_critic", "device": torch.cuda.get_device_name(0),
           "run": bench(a.env, a.envs, tuple(a.arch), a.rounds, a.window)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
