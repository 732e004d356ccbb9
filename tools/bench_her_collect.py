"""What collecting into the HER ring costs per env step, the device collect against the existing path:
python tools/bench_her_collect.py [--configs PandaReach-v3:4096 ...] [--rounds 12] [--window 50]
[--kernel-stats reach.csv ...] [--out profiles/bench_her_collect.json]

Per config (env id : envs; capacity per env such that the ring holds about 2^20 transitions, the
reference's buffer_size), in one process, legs alternated, medians with min / max over ``--rounds``
windows of ``--window`` steps (device events around each window, which ends in a synchronise), warm-up
past the first episode, episode phases staggered, Philox random policy:
  bare      the env step alone
  existing  plus three clones of the observation before the step and add_from_vec_env behind it
            (INTEGRATION.md's off-policy loop before this tool: torch.where x 3, flag conversions,
            pgx_replay_add)
  collect   plus collect_from_vec_env (one collect launch reading the env's buffers in place)
each as ms per step and as ms added over bare in the same run; ``collect`` and ``bare`` also as the
replay of capture_steps(window) (the existing path cannot be captured: its ring position is a host
argument).  ``bar`` says whether collect adds less than existing by more than the larger min-max
window spread of the two legs.  Also the algorithmic bytes of one collect (from the shapes, below)
and, given ``--kernel-stats`` (per config the CSV of a separate ``rocprofv3 --kernel-trace --stats`` run
of this tool over that config alone), over collect_kernel's average time.  One JSON line (also written
to --out).  Needs a GPU."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import panda_gym_amd as pg  # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s
RING = 1 << 20      # transitions, the reference's buffer_size
EAGER, GRAPH = ("bare", "existing", "collect"), ("bare", "collect")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def collect_bytes(N, od, ad):
    """Bytes one collect launch has to move, from the shapes: it reads the carry, the action, the
    reward, two flags and the post-step observation (the terminal one instead for the next_* of a done
    env: the same size) and writes the record's row_dim + 2 floats and the carry."""
    o = od + 6
    row = 2 * od + ad + 14
    return N * (4 * o + 4 * ad + 4 + 2 + 4 * o + 4 * (row + 2) + 4 * o)


def bench(env_id, N, rounds, W):
    cap = max(RING // N, 2)
    env = {leg: pg.PandaVecEnv(env_id, num_envs=N, device="cuda:0", seed=0) for leg in EAGER}
    od, ad = env["bare"].obs_dim, env["bare"].action_dim
    buf = {leg: pg.HerReplayBuffer(cap * N, env=env[leg], device="cuda:0", seed=1) for leg in ("existing", "collect")}
    step = dict.fromkeys(EAGER, 0)

    def window(leg):
        e = env[leg]
        for _ in range(W):
            a = e.sample_actions(step[leg])
            step[leg] += 1
            if leg == "existing":
                prev = {k: v.clone() for k, v in e._obs_dict().items()}
                e.step_tensors(a)
                buf[leg].add_from_vec_env(e, prev, a)
            else:
                e.step_tensors(a)
                if leg == "collect":
                    buf[leg].collect_from_vec_env(e, a)

    horizon = int(env["bare"].spec.max_episode_steps)
    for leg in EAGER:
        obs = env[leg].reset_tensors(episode_phase="staggered")
        if leg == "collect":
            buf[leg].set_last(obs)
    for leg in EAGER:   # warm-up: past the first episode of every phase
        for _ in range(horizon // W + 2):
            window(leg)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in EAGER}
    for _ in range(rounds):
        for leg in EAGER:
            ms[leg].append(timed(lambda: window(leg)) / W)

    # bare and collect as graph replays (the draws of capture time repeat: a timing loop only)
    graphs = {"bare": env["bare"].capture_steps(W),
              "collect": env["collect"].capture_steps(W, after_step=buf["collect"].after_step(env["collect"]))}
    for leg in GRAPH:
        graphs[leg].replay()
    torch.cuda.synchronize()
    gms = {leg: [] for leg in GRAPH}
    for _ in range(rounds):
        for leg in GRAPH:
            gms[leg].append(timed(graphs[leg].replay) / W)
    for b in buf.values():
        b.raise_device_errors()

    med = {leg: statistics.median(v) for leg, v in ms.items()}
    gmed = {leg: statistics.median(v) for leg, v in gms.items()}
    spread = lambda v: max(v) - min(v)  # noqa: E731
    added = {"eager": {leg: med[leg] - med["bare"] for leg in ("existing", "collect")},
             "graph": {"collect": gmed["collect"] - gmed["bare"]}}
    # the bar: collect adds less than existing, by more than the larger window spread of the two legs;
    # for the replay, the replayed collect against the eager existing path (there is no captured one)
    gap = {"eager": added["eager"]["existing"] - added["eager"]["collect"],
           "graph": added["eager"]["existing"] - added["graph"]["collect"]}
    noise = {"eager": max(spread(ms["existing"]), spread(ms["collect"])),
             "graph": max(spread(ms["existing"]), spread(gms["collect"]))}
    out = {"env_id": env_id, "n_envs": N, "capacity_per_env": cap, "ring_transitions": cap * N, "obs_dim": od,
           "action_dim": ad, "rounds": rounds, "window_steps": W,
           "eager_ms_per_step": {leg: stats(v) for leg, v in ms.items()},
           "graph_ms_per_step": {leg: stats(v) for leg, v in gms.items()},
           "added_ms_per_step": added, "gap_ms_per_step": gap, "larger_window_spread_ms": noise,
           "bar": {k: gap[k] > noise[k] for k in gap},
           "collect_bytes": collect_bytes(N, od, ad),
           "added_after": {leg: b._state()[0] for leg, b in buf.items()},
           "step_kernel": env["bare"].step_kernel()}
    for b in buf.values():
        b.close()
    for e in env.values():
        e.close()
    return out


def kernel_times(path):
    """Average ns per launch of the ring's kernels from a rocprofv3 --stats CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in ("collect_kernel", "add_kernel", "count_kernel", "scan_blocks_kernel", "scatter_kernel"):
                if f"::{k}(" in row["Name"] and "RingPtrs" in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                              "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", nargs="+",
                    default=["PandaReach-v3:4096", "PandaPickAndPlace-v3:16384", "PandaReachAO-v3:8192"])
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--kernel-stats", nargs="+", default=None, help="one rocprofv3 stats CSV per config, in order")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_her_collect: no HIP device (there is no CPU fallback)")
    runs = []
    for c in a.configs:
        env_id, n = c.split(":")
        runs.append(bench(env_id, int(n), a.rounds, a.window))
    res = {"tool": "bench_her_collect", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "runs": runs}
    if a.kernel_stats:
        if len(a.kernel_stats) != len(runs):
            raise SystemExit("bench_her_collect: --kernel-stats takes one CSV per config")
        for run, path in zip(runs, a.kernel_stats):
            kt = kernel_times(path)
            run["kernel_stats"] = kt
            if "collect_kernel" in kt:
                bps = run["collect_bytes"] / (kt["collect_kernel"]["average_ns"] * 1e-9)
                run["collect_rate"] = {"GB_per_s": bps / 1e9, "share_of_hbm_peak": bps / HBM_PEAK}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
