"""What the device RolloutBuffer costs, against the same operations in plain torch: python
tools/bench_rollout.py [--configs PandaReach-v3:4096:64 PandaReachAO-v3:8192:32] [--rounds 12]
[--out profiles/bench_rollout.json]

Per config (env id : envs : n_steps), in one process, legs alternated, medians with min / max over
``--rounds`` windows (device events around each window, which ends in a synchronise), warm-up first:
  collect   one rollout of n_steps env steps (Philox random policy, episode phases staggered) three
            ways -- bare (the step alone), device (plus RolloutBuffer's add, one launch) and torch
            (plus the torch restatement of add: slice stores of the carry and the step's values, the
            bootstrap as a masked expression, the new carry) -- eagerly and as the replay of
            capture_steps(n_steps); reported as ms per step and as ms added over bare in the same run
  gae       compute_returns_and_advantage: the one launch against SB3's loop in torch ops
  epoch     one epoch of get(4096): the permutation launch plus one gather per minibatch, against
            torch.randperm plus one fancy-index gather per stored field and minibatch (from arrays
            flattened once outside the window, as SB3 flattens once per rollout)
For the device legs also the algorithmic bytes (computed from the shapes, below) over the time and
their share of the 8 TB/s HBM peak.  The torch legs are the comparison, not code under test.
One JSON line (also written to --out).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
KEYS = ("observation", "achieved_goal", "desired_goal")
GAMMA, LAMBDA, BATCH = 0.99, 0.95, 4096


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def algorithmic_bytes(N, T, od, ad):
    """Bytes each operation has to move, from the shapes (f32 everywhere, u8 flags)."""
    V = od + 6 + ad
    add = N * (4 * (od + 7) + 4 * ad + 4 * 4 + 2 + 4 * (od + 6)      # read: carry, action, 4 scalars, flags, new obs
               + 4 * V + 4 * 4 + 4 * (od + 7))                       # write: record, 4 planes, carry
    gae = 4 * N * (3 * T + 2) + 4 * N * 2 * T                        # read 3 planes + 2 rows, write 2 planes
    M = N * T
    epoch = 4 * M + 4 * M + 2 * 4 * M * (V + 4)                      # permutation out, indices in, rows in and out
    return {"add_per_step": add, "gae": gae, "epoch": epoch}


class TorchRollout:
    """The plain-torch restatement: the baseline."""

    def __init__(self, T, N, od, ad, dev):
        z = lambda *s: torch.zeros((T, N) + s, device=dev)  # noqa: E731
        self.T, self.N = T, N
        self.a = {"observation": z(od), "achieved_goal": z(3), "desired_goal": z(3), "action": z(ad), "reward": z(),
                  "episode_start": z(), "value": z(), "log_prob": z(), "advantage": z(), "return": z()}
        self.last = {"observation": torch.zeros(N, od, device=dev), "achieved_goal": torch.zeros(N, 3, device=dev),
                     "desired_goal": torch.zeros(N, 3, device=dev)}
        self.last_start = torch.ones(N, device=dev)

    def add(self, t, action, reward, value, log_prob, obs, te, tr, tv):
        a = self.a
        for k in KEYS:
            a[k][t].copy_(self.last[k])
        a["episode_start"][t].copy_(self.last_start)
        a["action"][t].copy_(action)
        a["value"][t].copy_(value)
        a["log_prob"][t].copy_(log_prob)
        timeout = (tr != 0) & (te == 0)
        a["reward"][t].copy_(reward + GAMMA * tv * timeout)
        for k in KEYS:
            self.last[k].copy_(obs[k])
        self.last_start.copy_((te | tr) != 0)

    def gae(self, last_values, dones):
        a, T = self.a, self.T
        last = 0
        for t in reversed(range(T)):
            if t == T - 1:
                nnt, nv = 1.0 - dones, last_values
            else:
                nnt, nv = 1.0 - a["episode_start"][t + 1], a["value"][t + 1]
            delta = a["reward"][t] + GAMMA * nv * nnt - a["value"][t]
            last = delta + GAMMA * LAMBDA * nnt * last
            a["advantage"][t] = last
        a["return"] = a["advantage"] + a["value"]

    def flatten(self):
        f = lambda x: x.swapaxes(0, 1).reshape((self.T * self.N,) + tuple(x.shape[2:])).contiguous()  # noqa: E731
        self.flat = {k: f(self.a[k]) for k in KEYS + ("action", "value", "log_prob", "advantage", "return")}

    def epoch(self, batch):
        M = self.T * self.N
        perm = torch.randperm(M, device=self.last_start.device)
        for s in range(0, M, batch):
            idx = perm[s:s + batch]
            yield {k: v[idx] for k, v in self.flat.items()}


def bench(env_id, N, T, rounds):
    dev = torch.device("cuda:0")
    LEGS = ("bare", "device", "torch")
    env = {leg: pg.PandaVecEnv(env_id, num_envs=N, device="cuda:0", seed=0) for leg in LEGS}
    od, ad = env["bare"].obs_dim, env["bare"].action_dim
    rb = pg.RolloutBuffer(T, env=env["device"], gamma=GAMMA, gae_lambda=LAMBDA)
    tb = TorchRollout(T, N, od, ad, dev)
    g = torch.Generator(device="cuda:0").manual_seed(0)
    values, log_probs, tvs = (torch.randn(T, N, device=dev, generator=g) for _ in range(3))
    last_values = torch.randn(N, device=dev, generator=g)
    step = dict.fromkeys(LEGS, 0)

    def rollout(leg):
        e = env[leg]
        if leg == "device":
            rb.reset()
        for t in range(T):
            a = e.sample_actions(step[leg])
            step[leg] += 1
            obs, reward, te, tr, _ = e.step_tensors(a)
            if leg == "device":
                rb.add_from_vec_env(e, a, values[t], log_probs[t], tvs[t])
            elif leg == "torch":
                tb.add(t, a, reward, values[t], log_probs[t], obs, te, tr, tvs[t])

    horizon = int(env["bare"].spec.max_episode_steps)
    for leg in LEGS:
        obs = env[leg].reset_tensors(episode_phase="staggered")
        if leg == "device":
            rb.set_last(obs)
        elif leg == "torch":
            for k in KEYS:
                tb.last[k].copy_(obs[k])
    for leg in LEGS:   # warm-up: past the first episode of every phase
        for _ in range(horizon // T + 2):
            rollout(leg)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            ms[leg].append(timed(lambda: rollout(leg)) / T)

    # the same three as graph replays (the draws of capture time repeat: a timing loop only)
    actions = {leg: torch.zeros(T, N, ad, device=dev).uniform_(-1, 1, generator=g) for leg in LEGS}
    count = [0]

    def torch_hook():
        t, e = count[0], env["torch"]
        tb.add(t, actions["torch"][t], e.reward, values[t], log_probs[t], e._obs_dict(), e.terminated, e.truncated, tvs[t])
        count[0] = t + 1

    graphs = {"bare": env["bare"].capture_steps(T, actions["bare"]),
              "device": env["device"].capture_steps(T, actions["device"], after_step=rb.after_step(
                  env["device"], actions["device"], values, log_probs, tvs)),
              "torch": env["torch"].capture_steps(T, actions["torch"], after_step=torch_hook)}

    def replay(leg):
        if leg == "device":
            rb.reset()
        graphs[leg].replay()

    for leg in LEGS:
        replay(leg)
    torch.cuda.synchronize()
    gms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            gms[leg].append(timed(lambda: replay(leg)) / T)
    pos, full = rb.pos, rb.full
    rb.raise_device_errors()

    # GAE: both buffers are full; REPS launches per window
    REPS = 10
    dones = tb.last_start.clone()
    gae = {"device": [], "torch": []}
    rb.enqueue_returns_and_advantage(last_values)
    tb.gae(last_values, dones)
    torch.cuda.synchronize()
    for _ in range(rounds):
        gae["device"].append(timed(lambda: [rb.enqueue_returns_and_advantage(last_values) for _ in range(REPS)]) / REPS)
        gae["torch"].append(timed(lambda: [tb.gae(last_values, dones) for _ in range(REPS)]) / REPS)
    rb.raise_device_errors()

    # one epoch of minibatches
    tb.flatten()
    ep = {"device": [], "torch": []}
    for _ in range(2):
        for _b in rb.get(BATCH):
            pass
        for _b in tb.epoch(BATCH):
            pass
    torch.cuda.synchronize()
    for _ in range(rounds):
        ep["device"].append(timed(lambda: [None for _b in rb.get(BATCH)]))
        ep["torch"].append(timed(lambda: [None for _b in tb.epoch(BATCH)]))

    by = algorithmic_bytes(N, T, od, ad)
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    gmed = {leg: statistics.median(v) for leg, v in gms.items()}

    def rate(nbytes, t_ms):
        if t_ms <= 0:
            return {"bytes": nbytes, "GB_per_s": None, "share_of_hbm_peak": None}
        bps = nbytes / (t_ms * 1e-3)
        return {"bytes": nbytes, "GB_per_s": bps / 1e9, "share_of_hbm_peak": bps / HBM_PEAK}

    added = {"eager": {leg: med[leg] - med["bare"] for leg in ("device", "torch")},
             "graph": {leg: gmed[leg] - gmed["bare"] for leg in ("device", "torch")}}
    gd, gt, ed, et = (statistics.median(x) for x in (gae["device"], gae["torch"], ep["device"], ep["torch"]))
    out = {"env_id": env_id, "n_envs": N, "n_steps": T, "obs_dim": od, "action_dim": ad, "rounds": rounds,
           "minibatch": BATCH, "minibatches_per_epoch": -(-N * T // BATCH),
           "collect_ms_per_step": {leg: stats(v) for leg, v in ms.items()},
           "collect_graph_ms_per_step": {leg: stats(v) for leg, v in gms.items()},
           "added_ms_per_step": added,
           "add_rate": {k: rate(by["add_per_step"], added[k]["device"]) for k in ("eager", "graph")},
           "gae_ms": {leg: stats(v) for leg, v in gae.items()}, "gae_rate": rate(by["gae"], gd),
           "epoch_ms": {leg: stats(v) for leg, v in ep.items()}, "epoch_rate": rate(by["epoch"], ed),
           "torch_over_device": {"collect_eager_ms_per_step": med["torch"] / med["device"],
                                 "collect_graph_ms_per_step": gmed["torch"] / gmed["device"],
                                 "gae": gt / gd, "epoch": et / ed},
           "pos_after_replay": pos, "full_after_replay": full, "step_kernel": env["bare"].step_kernel()}
    rb.close()
    for e in env.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+", default=["PandaReach-v3:4096:64", "PandaReachAO-v3:8192:32"])
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout: no HIP device (there is no CPU fallback)")
    runs = []
    for c in a.configs:
        env_id, n, t = c.split(":")
        runs.append(bench(env_id, int(n), int(t), a.rounds))
    res = {"tool": "bench_rollout", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "runs": runs}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
