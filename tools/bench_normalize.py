"""What the device VecNormalize adds to a step: python tools/bench_normalize.py [--envs 4096 256]
[--window 50] [--rounds 24] [--out profiles/bench_normalize.json]

Times the headline loop (PandaReach-v3, Philox random policy, episode phases staggered, as bench.py
times it) three ways in one process, in alternating windows of ``--window`` steps (device events
around each window, which ends in a synchronise), ``--rounds`` windows per leg:
  bare       PandaVecEnv.step_tensors
  wrapper    VecNormalize.step_tensors (the env step plus pgx_norm_step's two launches)
  torch_ops  the env step plus the same arithmetic as torch ops on device tensors (TorchNormalize
             below: fp64 running statistics, three keys, returns, clips, terminal rows)
and the replay of capture_steps(--window) with and without the wrapper.  Reports per leg the median
over windows of ms per step, and the added time of wrapper and torch_ops over bare.  One JSON line
(also written to --out).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402


class TorchNormalize:
    """VecNormalize.step_wait's arithmetic as torch ops (what a user writes without the kernels)."""

    def __init__(self, env, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8):
        self.env, self.clip_obs, self.clip_reward, self.gamma, self.eps = env, clip_obs, clip_reward, gamma, epsilon
        kw = dict(dtype=torch.float64, device=env.device)
        self.keys = {"observation": (env.obs, env.terminal_obs), "achieved_goal": (env.achieved_goal, env.terminal_ag),
                     "desired_goal": (env.desired_goal, env.terminal_dg)}
        self.mean = {k: torch.zeros(v[0].shape[1], **kw) for k, v in self.keys.items()}
        self.var = {k: torch.ones(v[0].shape[1], **kw) for k, v in self.keys.items()}
        self.count = {k: torch.full((), 1e-4, **kw) for k in self.keys}
        self.ret_mean, self.ret_var, self.ret_count = torch.zeros((), **kw), torch.ones((), **kw), torch.full((), 1e-4, **kw)
        self.returns = torch.zeros(env.num_envs, **kw)
        self.out = {}

    @staticmethod
    def _update(mean, var, count, x):
        x = x.double()
        n = x.shape[0]
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        delta = bm - mean
        tot = count + n
        m2 = var * count + bv * n + delta * delta * count * n / tot
        return mean + delta * n / tot, m2 / tot, tot

    def step(self):
        env = self.env
        done = (env.terminated | env.truncated).bool()
        for k, (x, t) in self.keys.items():
            self.mean[k], self.var[k], self.count[k] = self._update(self.mean[k], self.var[k], self.count[k], x)
            den = torch.sqrt(self.var[k] + self.eps)
            self.out[k] = ((x.double() - self.mean[k]) / den).clamp(-self.clip_obs, self.clip_obs).float()
            tn = ((t.double() - self.mean[k]) / den).clamp(-self.clip_obs, self.clip_obs).float()
            self.out["terminal_" + k] = torch.where(done.unsqueeze(1), tn, t)
        self.returns = self.returns * self.gamma + env.reward.double()
        self.ret_mean, self.ret_var, self.ret_count = self._update(self.ret_mean, self.ret_var, self.ret_count,
                                                                   self.returns)
        self.out["reward"] = (env.reward.double() / torch.sqrt(self.ret_var + self.eps)).clamp(
            -self.clip_reward, self.clip_reward).float()
        self.returns = torch.where(done, torch.zeros_like(self.returns), self.returns)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench(n, window, rounds):
    mk = lambda: pg.PandaVecEnv("PandaReach-v3", num_envs=n, device="cuda:0", seed=0)  # noqa: E731
    bare, inner, tenv = mk(), mk(), mk()
    wrap = pg.VecNormalize(inner)
    tnorm = TorchNormalize(tenv)
    T = int(bare.spec.max_episode_steps)
    step = {"bare": 0, "wrapper": 0, "torch_ops": 0}

    def run(leg, k):
        for _ in range(k):
            t = step[leg]
            if leg == "bare":
                bare.step_tensors(bare.sample_actions(t))
            elif leg == "wrapper":
                wrap.step_tensors(inner.sample_actions(t))
            else:
                tenv.step_tensors(tenv.sample_actions(t))
                tnorm.step()
            step[leg] = t + 1

    bare.reset_tensors(episode_phase="staggered")
    wrap.reset_tensors(episode_phase="staggered")
    tenv.reset_tensors(episode_phase="staggered")
    for leg in step:   # warm-up: past the first episode of every phase
        run(leg, T + 20)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in step}
    for _ in range(rounds):
        for leg in step:
            ms[leg].append(timed(lambda: run(leg, window)) / window)
    # graph replay, with and without the wrapper (the draws of capture time repeat: a timing loop only)
    graphs = {"bare": bare.capture_steps(window), "wrapper": wrap.capture_steps(window)}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    gms = {leg: [] for leg in graphs}
    for _ in range(rounds):
        for leg, g in graphs.items():
            gms[leg].append(timed(g.replay) / window)
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    gmed = {leg: statistics.median(v) for leg, v in gms.items()}
    spread = {leg: [min(v), max(v)] for leg, v in ms.items()}
    out = {"n_envs": n, "steps_per_leg": window * rounds, "window": window,
           "ms_per_step_median": med, "ms_per_step_min_max": spread,
           "added_ms_wrapper": med["wrapper"] - med["bare"], "added_ms_torch_ops": med["torch_ops"] - med["bare"],
           "graph_ms_per_step_median": gmed, "graph_added_ms_wrapper": gmed["wrapper"] - gmed["bare"],
           "step_kernel": bare.step_kernel()}
    wrap.close()
    bare.close()
    tenv.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normalize: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_normalize", "env_id": "PandaReach-v3", "device": torch.cuda.get_device_name(0),
           "runs": [bench(n, a.window, a.rounds) for n in a.envs]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
