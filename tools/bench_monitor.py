"""What the device VecMonitor adds to a step: python tools/bench_monitor.py [--envs 4096 256]
[--window 50] [--rounds 24] [--out profiles/bench_monitor.json]

Times the headline loop (PandaReach-v3, Philox random policy, episode phases staggered, as bench.py
times it) three ways in one process, in alternating windows of ``--window`` steps (device events
around each window, which ends in a synchronise), ``--rounds`` windows per leg:
  bare       PandaVecEnv.step_tensors
  monitor    VecMonitor.step_tensors (the env step plus pgx_monitor_step's two launches)
  normalize  VecNormalize.step_tensors (the env step plus pgx_norm_step's two launches)
and, alternated the same way, the replay of capture_steps(--window) of each leg.  Reports per leg the
median and min / max over windows of ms per step and the added time of monitor and normalize over
bare, eagerly and in the graph: the yardstick is the monitor's added time against VecNormalize's in
the same run.  The bare leg runs the step kernel of the library as it is (``step_kernel`` names it).
One JSON line (also written to --out).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402

LEGS = ("bare", "monitor", "normalize")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench(n, window, rounds):
    mk = lambda: pg.PandaVecEnv("PandaReach-v3", num_envs=n, device="cuda:0", seed=0)  # noqa: E731
    env = {"bare": mk()}
    env["monitor"] = pg.VecMonitor(mk())
    env["normalize"] = pg.VecNormalize(mk())
    T = int(env["bare"].spec.max_episode_steps)
    step = dict.fromkeys(LEGS, 0)

    def run(leg, k):
        e = env[leg]
        for _ in range(k):
            e.step_tensors(e.sample_actions(step[leg]))
            step[leg] += 1

    for leg in LEGS:
        env[leg].reset_tensors(episode_phase="staggered")
    for leg in LEGS:   # warm-up: past the first episode of every phase
        run(leg, T + 20)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            ms[leg].append(timed(lambda: run(leg, window)) / window)
    # graph replay of each leg (the draws of capture time repeat: a timing loop only)
    graphs = {leg: env[leg].capture_steps(window) for leg in LEGS}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    gms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            gms[leg].append(timed(graphs[leg].replay) / window)
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    gmed = {leg: statistics.median(v) for leg, v in gms.items()}
    totals = env["monitor"].totals()
    out = {"n_envs": n, "steps_per_leg": window * rounds, "window": window,
           "ms_per_step_median": med, "ms_per_step_min_max": {leg: [min(v), max(v)] for leg, v in ms.items()},
           "added_ms_monitor": med["monitor"] - med["bare"], "added_ms_normalize": med["normalize"] - med["bare"],
           "graph_ms_per_step_median": gmed,
           "graph_ms_per_step_min_max": {leg: [min(v), max(v)] for leg, v in gms.items()},
           "graph_added_ms_monitor": gmed["monitor"] - gmed["bare"],
           "graph_added_ms_normalize": gmed["normalize"] - gmed["bare"],
           "monitor_episodes": totals["episodes"], "monitor_steps": totals["steps"],
           "step_kernel": env["bare"].step_kernel()}
    for leg in LEGS:
        env[leg].close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_monitor: no HIP device (there is no CPU fallback)")
    res = {"tool": "bench_monitor", "env_id": "PandaReach-v3", "device": torch.cuda.get_device_name(0),
           "runs": [bench(n, a.window, a.rounds) for n in a.envs]}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
