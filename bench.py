"""Benchmark: aggregate env-steps/s of PandaReach at 4096 envs per GPU (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--envs 4096] [--dump-outputs DIR] [--full]

One step = one batched env step of all envs on the GPU: device Philox random
actions (pgx_sample_actions) + the fused IK/physics/obs/reward/auto-reset
kernel (pgx_step).  Inputs and state stay resident in HBM.  For N > 1 the
driver launches one process per GPU (torch.distributed.run); envs are sharded
by global id (rank r owns ids [r*E, (r+1)*E)), nothing is exchanged on the step
path, and the timed region is bracketed by barriers with the max over ranks.

A plain run sets up, warms up, times the K steps and rank 0 prints one JSON line with the
headline (``value`` env-steps/s, ``ms_per_step``).  ``--dump-outputs DIR`` also writes what the
last timed step returned to its caller (actions, obs, goals, reward, flags) as DIR/<name>.npy;
with the same arguments the inputs, and so these arrays, are the same from run to run.

``--full`` adds every other leg to that line: the roofline of the step kernel (algorithmic
bytes from SURVEY.md §8d over the HIP-event kernel time), the HIP-graph replay, ReachAO, the
Push / PickAndPlace / HER legs, the SB3 host path and a CPU baseline (the fp64 oracle = CPU
restatement, not PyBullet, timed on this host).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md chip table (8.0 TB/s spec)
VALU_PEAK_TFLOPS = 157.3         # FP32 vector peak (spec)
EPISODE_STEPS = 50               # the TimeLimit: terminal outputs and reset writes amortised over an episode


def alg_bytes_per_env_step(task: str, obs_dim: int, action_dim: int, robot_points: int) -> dict:
    """HBM bytes one env-step must move: the state it carries -- q, qd and the
    cached link pose qc (f32 x 7 each), the fp64 goal, the contact warm-start cache (feature id,
    impulse) of the robot budget's slots and, with an object, the cube's 13 floats and its 4
    object-scene slots; ReachAO's 6 obstacle centres; the TimeLimit and episode counters --
    read and written back (the goal and obstacles only on a reset), the action read, and the
    outputs written: obs, achieved / desired goal, reward, success / terminated / truncated
    (+ ReachAO's task flag), the terminal obs / goals on an episode's last step."""
    obj = task in ("push", "pick_and_place")
    ao = task == "reach_ao"
    state = 3 * 7 * 4 + 8 + 2 * 4 * (robot_points + (4 if obj else 0)) + (13 * 4 if obj else 0)
    read = state + 24 + (72 if ao else 0) + 4 * action_dim
    out = 4 * obs_dim + 12 + 12 + 4 + 3 + (1 if ao else 0)
    reset = (4 * obs_dim + 24 + 24 + (72 if ao else 0)) / EPISODE_STEPS
    write = state + out + reset
    return {"read": read, "write": write, "total": read + write}
PROFILE_JSON = os.path.join(ROOT, "profiles", "pmc_step_kernel.json")
# algorithmic FLOPs per env-step, op-counted in the oracle and frozen (oracle/count_flops.py)
FLOPS_JSON = os.path.join(ROOT, "tests", "golden", "flops_per_env_step.json")


def alg_flops() -> dict:
    """config key -> algorithmic FLOPs per env-step (tests/golden/flops_per_env_step.json)."""
    with open(FLOPS_JSON) as f:
        doc = json.load(f)
    return {k: v["flops_per_env_step"] for k, v in doc["configs"].items()}


def pmc(name: str, envs=None):
    """profiles/<name>.json (tools/pmc_summary_r3.py), or None when absent or for another batch."""
    p = os.path.join(ROOT, "profiles", name + ".json")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        doc = json.load(f)
    if envs is not None and doc.get("num_envs") != envs:
        return None
    return doc


def pmc_kernel_ok(doc, kernel: str) -> bool:
    """The PMC summary names this kernel: its full name, or (older summaries) the tail of the
    template argument list after '<'."""
    k = doc.get("kernel")
    return k is None or k == kernel or (not k.startswith("step_kernel") and kernel.endswith("<" + k))


def pmc_for(name: str, envs: int, kernel: str):
    """The PMC summary when it was taken on this batch and this kernel (else None)."""
    doc = pmc(name, envs)
    if doc and not pmc_kernel_ok(doc, kernel):
        return None
    return doc


def hbm_roofline(alg_bytes: float, ms: float, prof, kernel: str) -> dict:
    """Algorithmic bytes of one launch over its time, against the HBM peak; traffic = the PMC bytes."""
    ach = alg_bytes / (ms * 1e-3) / 1e9
    return {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "traffic": prof["hbm_bytes_per_launch"] if prof else None, "alg_bytes_per_launch": alg_bytes,
            "kernel": kernel, "traffic_source": prof["source"] if prof else None}


def valu_roofline(key: str, env_steps_per_s: float, what: str) -> dict:
    """rate x algorithmic FLOPs per env-step / the FP32 vector peak.  The count is
    the minimal (recursive: CRBA + Newton-Euler + Cholesky) formulation's; the oracle's Jacobian
    form of the same dynamics is reported beside it, labelled, and not used for the fraction."""
    fl = alg_flops()[key]
    with open(FLOPS_JSON) as f:
        jac = json.load(f)["configs"][key].get("jacobian", {}).get("flops_per_env_step")
    ach = env_steps_per_s * fl / 1e12
    return {"bound": "valu", "achieved": ach, "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / VALU_PEAK_TFLOPS,
            "alg_flops_per_env_step": fl, "formulation": "recursive (CRBA + Newton-Euler + Cholesky)",
            "jacobian_form_flops_per_env_step": jac, "rate": what,
            "source": os.path.relpath(FLOPS_JSON, ROOT) + f" [{key}] (fp64 oracle op-count, oracle/count_flops.py)"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--envs", type=int, default=4096, help="envs per GPU")
    ap.add_argument("--env-id", default="PandaReach-v3")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg (step-kernel time and rooflines, HIP-graph replay, ReachAO, "
                         "Push / PickAndPlace, HER, SB3 host path, CPU baselines); the options below shape those legs")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=12.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--kernel-launches", type=int, default=200, help="launches for the kernel-time measurement")
    ap.add_argument("--no-her", action="store_true", help="skip the HER relabel leg (BASELINE configs[3])")
    ap.add_argument("--her-calls", type=int, default=50)
    ap.add_argument("--no-tasks", action="store_true", help="skip the Push / PickAndPlace legs (configs[2], [3])")
    ap.add_argument("--task-steps", type=int, default=200)
    ap.add_argument("--no-ao", action="store_true", help="skip the sharded ReachAO leg (configs[4])")
    ap.add_argument("--no-graph", action="store_true", help="skip the HIP-graph replay of the headline loop")
    ap.add_argument("--ao-envs", type=int, default=8192, help="ReachAO envs per GPU (65536 over 8 GPUs)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="process group for N > 1 (gloo: collective tensors on the host, so several ranks "
                         "can share one GPU for a rehearsal of the multi-GPU path)")
    return ap.parse_args()


def host_cores() -> dict:
    """The host's core counts: nproc (os.cpu_count), the cores this process may run on
    (sched_getaffinity), the CPU share the GPU box grants a one-GPU job (OMP_NUM_THREADS, which
    the box sets to its share) and the CPU model."""
    nproc = os.cpu_count() or 1
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:   # pragma: no cover
        avail = nproc
    share = os.environ.get("OMP_NUM_THREADS")
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:   # pragma: no cover
        pass
    return {"nproc": nproc, "affinity": avail, "omp_num_threads": int(share) if share and share.isdigit() else None,
            "cpu_model": model}


CPU_THREADS_MAX = 64   # thread cap of the CPU baseline where no OMP_NUM_THREADS share is set


def cpu_baseline(venv, seconds: float):
    """fp64 oracle on the host cores (threads; ctypes releases the GIL) over a bounded sample: one
    thread per core this process may use, capped by the box's CPU share for a one-GPU job
    (OMP_NUM_THREADS, set there to the share) -- the GPU box's nproc counts the whole machine."""
    import concurrent.futures as cf

    from oracle import oracle as O

    n = venv.num_envs
    hc = host_cores()
    # the box's one-GPU share (OMP_NUM_THREADS); without one, the affinity mask capped at CPU_THREADS_MAX
    threads = min(hc["affinity"], CPU_THREADS_MAX) if hc["omp_num_threads"] is None \
        else min(hc["affinity"], hc["omp_num_threads"])
    threads = max(1, threads)

    def run(n_envs: int, n_threads: int, budget: float):
        shards = np.array_split(np.arange(n_envs), n_threads)
        envs = []
        for sh in shards:
            cfg = type(venv._cfg).from_buffer_copy(venv._cfg)
            cfg.n_envs = len(sh)
            cfg.env_id_offset = int(sh[0])
            e = O.OracleVecEnv(cfg, len(sh))
            e.reset()
            envs.append(e)
        steps = 0
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(n_threads) as ex:
            while time.perf_counter() - t0 < budget and steps < 200:
                list(ex.map(lambda e: e.step(e.sample_actions(steps)), envs))
                steps += 1
        return steps, time.perf_counter() - t0

    steps, dt = run(n, threads, seconds)
    # one core (BASELINE.md section 2's single-core figure): a 256-env slice of the same workload
    n1 = min(n, 256)
    steps1, dt1 = run(n1, 1, max(2.0, seconds / 4))
    return {"value": n * steps / dt, "unit": "env-steps/s", "cores": threads, "kind": "port", **hc,
            "single_core": {"value": n1 * steps1 / dt1, "unit": "env-steps/s", "cores": 1,
                            "sample": f"{n1} envs x {steps1} steps = {n1 * steps1} env-steps in {dt1:.1f} s on one thread"},
            "cores_note": "'cores' is the CPU share the GPU box grants one GPU (OMP_NUM_THREADS), not the whole "
                          "machine (nproc): the multi-thread leg is capped at that share by design",
            "sample": f"fp64 C oracle (CPU restatement, not PyBullet): {n} PandaReach envs x {steps} steps "
                      f"= {n * steps} env-steps in {dt:.1f} s on {threads} host threads (nproc {hc['nproc']}, "
                      f"{hc['affinity']} in this process's affinity, OMP_NUM_THREADS {hc['omp_num_threads']}: "
                      f"the box's CPU share for one GPU; {hc['cpu_model']})"}


# HER relabel leg: 16384 envs x one 50-step episode each in a 64-slot ring
# (SB3 never validates an episode whose length equals the ring size), PickAndPlace rows
# (obs 19, action 4), B = 2^20 samples per call, "future", her_ratio 0.8.
HER_N, HER_C, HER_EP, HER_OD, HER_AD, HER_B = 16384, 64, 50, 19, 4, 1 << 20


def her_alg_bytes(B: int, nbv: int, row_dim: int, row_stride: int) -> int:
    """Algorithmic HBM bytes of one sample() call (DESIGN.md "HER relabelling").

    Per draw: valid-list entry 4 B, the transition's row 4*row_dim B, the batch row written
    4*row_stride B; relabelled draws also read ep_start/ep_length 8 B and the goal 12 B."""
    return B * (4 + 4 * row_dim + 4 * row_stride) + nbv * (8 + 12)


def her_leg(dev, calls: int, with_cpu: bool):
    from panda_gym_amd.her import HerReplayBuffer

    N, C, B = HER_N, HER_C, HER_B
    buf = HerReplayBuffer(N * C, device=dev, n_envs=N, obs_dim=HER_OD, action_dim=HER_AD, seed=0,
                          reward_type="sparse", goal_selection_strategy="future", n_sampled_goal=4)
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g, device=dev) * 0.3 - 0.15  # noqa: E731
    for t in range(HER_EP):  # one full 50-step episode per env (PickAndPlace time limit), ends by time-out
        done = torch.full((N,), int(t == HER_EP - 1), dtype=torch.uint8, device=dev)
        buf.add_tensors(r(N, HER_OD), r(N, 3), r(N, 3), r(N, HER_AD), -torch.ones(N, device=dev), r(N, HER_OD),
                        r(N, 3), r(N, 3), done, done)
    out = buf.alloc_batch(B, with_indices=False)   # what a learner consumes: the rows, no index outputs
    buf.sample_into(out)
    for _ in range(3):
        buf.sample_into(out)
    # one add() (ring write + valid-list refresh) timed separately: it is the other half of a step
    obs_args = [r(N, HER_OD), r(N, 3), r(N, 3), r(N, HER_AD), r(N), r(N, HER_OD), r(N, 3), r(N, 3)]
    zero = torch.zeros(N, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record(stream)
    for _ in range(calls):
        buf.sample_into(out)
    e1.record(stream)
    torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1) / calls
    # 10 adds back to back (the ring holds 64 slots, 50 used: no episode is overwritten), HIP events
    # over the span; the host's Python path per add alone (argument checks, ctypes) beside it
    n_add = 10
    torch.cuda.synchronize(dev)
    t_host = time.perf_counter()
    e0.record(stream)
    for _ in range(n_add):
        buf.add_tensors(*obs_args, zero, zero)
    e1.record(stream)
    t_host = (time.perf_counter() - t_host) / n_add
    torch.cuda.synchronize(dev)
    add_ms = e0.elapsed_time(e1) / n_add
    nbv = int(buf.her_ratio * B)
    n_valid = int(buf._arrays()[2].item())
    if n_valid != N * HER_EP:
        raise RuntimeError(f"HER ring holds {n_valid} valid transitions, expected {N * HER_EP}")
    alg = her_alg_bytes(B, nbv, buf.row_dim, buf.row_stride)
    achieved = alg / (ms * 1e-3) / 1e9
    prof = pmc("pmc_sample_kernel")
    if prof and prof.get("alg_bytes_per_launch") != alg:
        prof = None
    res = {"metric": "HER relabels/s (virtual transitions, future, her_ratio 0.8)", "value": nbv / (ms * 1e-3),
           "unit": "relabels/s", "samples_per_s": B / (ms * 1e-3), "ms_per_call": ms, "calls": calls,
           "ms_per_add": add_ms, "host_ms_per_add_issue": t_host * 1e3,
           "config": {"workload": f"HER ring {N} envs x {HER_EP}-step episodes ({C} slots), obs {HER_OD}, "
                                  f"action {HER_AD}, B={B} "
                                  f"(BASELINE configs[3] relabel leg)", "batch": B, "relabels_per_call": nbv},
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": achieved / HBM_PEAK_GBS, "traffic": prof["hbm_bytes_per_launch"] if prof else None,
                        "kernel": "sample_kernel", "alg_bytes_per_call": alg,
                        "traffic_source": prof["source"] if prof else None}}
    if with_cpu:
        from oracle import her as H

        orc = H.HerOracle(N, C, HER_OD, HER_AD, seed=0)
        # the numpy restatement samples its own ring of the same shape (contents do not change the work)
        z = np.zeros
        for t in range(HER_EP):
            d = np.full(N, int(t == HER_EP - 1), np.uint8)
            orc.add(z((N, HER_OD), np.float32), z((N, 3), np.float32), z((N, 3), np.float32),
                    z((N, HER_AD), np.float32), z(N, np.float32), z((N, HER_OD), np.float32),
                    z((N, 3), np.float32), z((N, 3), np.float32), d, d)
        bs = 1 << 16
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 5.0:
            orc.sample(bs, n)
            n += 1
        dt = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": int(buf.her_ratio * bs) * n / dt, "unit": "relabels/s", "cores": 1,
                               "kind": "port",
                               "sample": f"numpy restatement of SB3 HerReplayBuffer.sample (oracle/her.py), "
                                         f"{n} calls of B=2^16 on the same ring shape, 1 thread"}
    buf.close()
    return res


def task_leg(dev, env_id: str, n: int, steps: int, contacts: bool = True, flops_key: str = "",
             full_manifold=None):
    """env-steps/s of one more task config on this GPU (device random policy, in-kernel
    auto-reset), timed like the main leg: barrier-free single GPU, HIP events bracketing.
    ``full_manifold=False``: the 4-point robot budget (reduced fidelity, for comparison only)."""
    import panda_gym_amd as pg

    venv = pg.PandaVecEnv(env_id, num_envs=n, device=dev, seed=1, contacts=contacts, full_manifold=full_manifold)
    obs_dim, act_dim, budget = venv.obs_dim, venv.action_dim, venv.robot_contact_budget()
    venv.reset_tensors(episode_phase="staggered")
    T = venv.spec.max_episode_steps
    for t in range(T):   # one whole episode: every env has auto-reset once, at its own step
        venv.step_tensors(venv.sample_actions(t))
    kname = venv.step_kernel()
    stream = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record(stream)
    for t in range(steps):
        venv.step_tensors(venv.sample_actions(T + t))
    e1.record(stream)
    torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1) / steps
    venv.close()
    res = {"env_id": env_id, "envs": n, "contacts": contacts, "robot_points": budget, "value": n / (ms * 1e-3),
           "unit": "env-steps/s", "kernel": kname,
           "ms_per_step": ms, "steps": steps,
           "policy": "device Philox random actions (sample_actions + step per step), episode phases staggered "
                     "(every step auto-resets ~N/50 envs), timed after one whole episode"}
    if flops_key:
        res["roofline_valu"] = valu_roofline(flops_key, res["value"], "env-steps/s of this leg (sample + step)")
    alg = None
    if flops_key in ("push", "pick_and_place"):
        alg = alg_bytes_per_env_step(flops_key, obs_dim, act_dim, budget)["total"]
    if alg:
        prof = pmc("pmc_object_kernel_" + ("push" if flops_key == "push" else "pnp"), n)
        if budget <= 4:
            res["fidelity"] = "reduced: 4 robot contact points per env (not the per-pair manifold rule)"
        if prof and (prof.get("robot_points", 4) != budget or not pmc_kernel_ok(prof, kname)):
            prof = None   # PMC of another budget's / another kernel
        res["roofline"] = hbm_roofline(alg * n, ms, prof, kname)
    return res


def host_path_leg(dev, env_id: str, n: int, steps: int):
    """The SB3-facing path (PCIe-inclusive, never ``value``): numpy actions in through
    ``step_async`` (pinned H2D), ``step_wait`` returns numpy obs / rewards / dones and the
    per-env infos list SB3's VecEnv protocol requires (D2H of every output + Python dicts).
    The actions are drawn on the host by numpy, as a policy's would arrive."""
    import panda_gym_amd as pg

    venv = pg.PandaVecEnv(env_id, num_envs=n, device=dev, seed=2)
    venv.reset()
    rng = np.random.default_rng(0)
    acts = rng.uniform(-1.0, 1.0, (steps + 10, n, venv.action_dim)).astype(np.float32)
    for t in range(10):
        venv.step(acts[t])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for t in range(steps):
        venv.step(acts[10 + t])
    el = time.perf_counter() - t0
    venv.close()
    return {"env_id": env_id, "envs": n, "value": n * steps / el, "unit": "env-steps/s",
            "ms_per_step": el / steps * 1e3, "steps": steps,
            "path": "VecEnv.step_async/step_wait with numpy in and out (pinned H2D / D2H, SB3 infos list)"}


def state_digest(venv, dist, world: int) -> str:
    """sha256 over every env's final observation bits in global env order: per env the sum of the
    int32 views of its obs row (order-independent and exact), gathered from every rank.  A sharded
    run and one handle holding all the envs give the same digest iff they agree env for env."""
    import hashlib

    per_env = venv.obs.contiguous().view(torch.int32).to(torch.int64).sum(1).cpu()
    if dist is not None and world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, per_env.numpy())
        per_env = torch.from_numpy(np.concatenate(parts))
    return hashlib.sha256(per_env.numpy().astype("<i8").tobytes()).hexdigest()


def sharded_leg(dev, env_id: str, n: int, steps: int, warmup: int, dist, rank: int, world: int,
                coll_dev=None):
    """Every rank steps its own shard of ``n`` envs (global ids [rank*n, (rank+1)*n)); the timed
    region is barrier-bracketed and the max over ranks is taken, like the headline leg.  Used for
    BASELINE configs[4] (ReachAO, 65536 envs as 8192 per GPU on 8 GPUs)."""
    import panda_gym_amd as pg
    from panda_gym_amd.shard import max_over_ranks, shard_offset

    venv = pg.PandaVecEnv(env_id, num_envs=n, device=dev, seed=1, env_id_offset=shard_offset(rank, n))
    ab = alg_bytes_per_env_step("reach_ao", venv.obs_dim, venv.action_dim, venv.robot_contact_budget())["total"]
    venv.reset_tensors(episode_phase="staggered")

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(venv.spec.max_episode_steps + warmup):
        venv.step_tensors(venv.sample_actions())
    kname = venv.step_kernel()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        venv.step_tensors(venv.sample_actions())
    torch.cuda.synchronize(dev)
    barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0, dist, coll_dev)
    digest = state_digest(venv, dist, world)
    venv.close()
    value = world * n * steps / elapsed
    return {"env_id": env_id, "envs_per_gpu": n, "global_envs": world * n, "n_gpus": world,
            "value": value, "unit": "env-steps/s", "ms_per_step": elapsed / steps * 1e3,
            "steps": steps, "warmup": warmup, "scaling": "weak",
            "policy": "device Philox random actions, in-kernel collision / success / TimeLimit auto-reset, "
                      "episode phases staggered, timed after one whole episode + warmup",
            "kernel": kname,
            "obs_digest": digest,
            "roofline_valu": valu_roofline("reach_ao", value / world, "env-steps/s per GPU of this leg"),
            # state, obstacles, contact cache, 56-float obs
            "roofline": hbm_roofline(ab * n, elapsed / steps * 1e3, pmc_for("pmc_reach_ao_kernel", n, kname), kname)}


def launch_ranks(n: int) -> int:
    """``--gpus N`` without a torch.distributed launcher: run N ranks (one per GPU) as a child
    torch.distributed.run job on this node and return its exit code.  Nothing here has touched
    the GPU, and the launcher is a child process, not an exec."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


DUMP_MAX_BYTES = 64 << 20   # cap of one --dump-outputs directory


def dump_outputs(out_dir: str, venv, rank: int, world: int) -> None:
    """``--dump-outputs DIR``: what the last timed step handed its caller -- the actions
    sample_actions drew and step_tensors' obs dict, reward, terminated, truncated, success -- one
    DIR/<name>.npy each (f32; the uint8 flags as 0.0 / 1.0), rows in env order.  Past the size cap
    a fixed seeded sample of the envs is written, their indices in env_index.npy.  With several
    ranks each writes its own shard as <name>.rank<r>.npy."""
    obs = venv._obs_dict()
    arrays = {"actions": venv._actions, "observation": obs["observation"], "achieved_goal": obs["achieved_goal"],
              "desired_goal": obs["desired_goal"], "reward": venv.reward, "terminated": venv.terminated,
              "truncated": venv.truncated, "success": venv.success}
    n = venv.num_envs
    row_bytes = sum(4 * t[0].numel() for t in arrays.values()) + 8
    rows = None
    if n * row_bytes * world > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // (row_bytes * world)
        rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
    os.makedirs(out_dir, exist_ok=True)
    sfx = f".rank{rank}" if world > 1 else ""
    for name, t in arrays.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, name + sfx + ".npy"), a if rows is None else a[rows])
    if rows is not None:
        np.save(os.path.join(out_dir, "env_index" + sfx + ".npy"), rows.astype(np.float64))


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world} ranks were launched")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # gloo rehearsal on one box: ranks share the GPUs there are (device_count does not initialise HIP)
    local_dev = local if args.dist_backend == "nccl" else local % max(1, torch.cuda.device_count())
    if world > 1:
        import torch.distributed as dist

        torch.cuda.set_device(local_dev)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_dev))
        else:
            dist.init_process_group("gloo")
    dev = torch.device("cuda", local_dev)
    torch.cuda.set_device(dev)
    coll_dev = dev if args.dist_backend == "nccl" else None   # where the collective tensors live

    import panda_gym_amd as pg
    from panda_gym_amd.shard import max_over_ranks, shard_offset

    E = args.envs
    venv = pg.PandaVecEnv(args.env_id, num_envs=E, device=dev, seed=args.seed,
                          env_id_offset=shard_offset(rank, E))
    # steady state: staggered episode phases (global env g starts its TimeLimit counter at g mod 50),
    # so every step auto-resets ~E/50 envs as in a long VecEnv rollout, and one whole episode before
    # the warmup steps, so every env has reset once and no env still holds the at-rest start pose --
    # any window of steps is then the steady-state mix (with all envs in phase, a 20-step window is
    # a fixed, cheaper slice of the episode; profiles/r04)
    venv.reset_tensors(episode_phase="staggered")

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(venv.spec.max_episode_steps + args.warmup):
        venv.step_tensors(venv.sample_actions())
    kname = venv.step_kernel()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        venv.step_tensors(venv.sample_actions())
    torch.cuda.synchronize(dev)
    barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0, dist, coll_dev)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, venv, rank, world)
    total = world * E * args.steps
    line = {
        "metric": "aggregate env-steps/s, PandaReach 4096 envs @1 GPU; 1/2/4/8-GPU scaling",
        "value": total / elapsed, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "steady_state": f"episode phases staggered (env g starts its TimeLimit counter at g mod "
                        f"{venv.spec.max_episode_steps}: every step auto-resets ~{E // venv.spec.max_episode_steps} "
                        f"envs), timed after {venv.spec.max_episode_steps} + {args.warmup} untimed steps "
                        f"(every env has auto-reset at least once)",
        "kernel": kname,
        "vs_baseline": None, "dtype": "f32",
        "data": "synthetic: device Philox random policy U[-1,1)^3, 50-step episodes with in-kernel auto-reset",
        "config": {"workload": f"{args.env_id} (ee control, sparse reward), {E} envs per GPU, the "
                               f"reference's scene: table / plane contacts of the robot (BASELINE configs[1])",
                   "envs_per_gpu": E, "global_envs": world * E, "parallelism": f"env-sharded x{world}"},
    }
    if args.full:
        line.update(full_legs(args, venv, dev, dist, rank, world, coll_dev, kname))
    if rank == 0:
        print(json.dumps(line), flush=True)
    venv.close()
    if dist is not None:
        dist.destroy_process_group()


def full_legs(args, venv, dev, dist, rank: int, world: int, coll_dev, kname: str) -> dict:
    """``--full``: every leg beside the headline, run after it on the same handle; rank 0 gets the
    fields they add to the result line (the other ranks an empty dict)."""
    from panda_gym_amd.shard import gather_stats

    E = venv.num_envs
    # episode statistics all-gather (outside the timed region; 16 B per rank over xGMI)
    stats = gather_stats([float(venv.truncated.sum()), float(venv.success.sum()), float(venv.reward.sum()),
                          float(args.steps)], dist, coll_dev).sum(0)

    # kernel time of pgx_step alone (HIP events on the launch stream = torch's current stream),
    # on the same random-policy workload: the actions are drawn up front
    K = args.kernel_launches
    acts = torch.empty((K, E, venv.action_dim), dtype=torch.float32, device=dev)
    base = venv._step_index
    for k in range(K):
        acts[k].copy_(venv.sample_actions(base + k))   # a fresh Philox draw per launch, as in the timed loop
    stream = torch.cuda.current_stream(dev)
    # first-to-last span of K back-to-back launches per launch (launch gaps included; event pairs
    # around each launch measured 3 % above rocprof's kernel average: an event record adds its own
    # gap, profiles/r04/bench_v3.json)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    ev0.record(stream)
    for k in range(K):
        venv.step_tensors(acts[k])
    ev1.record(stream)
    torch.cuda.synchronize(dev)
    kernel_ms = ev0.elapsed_time(ev1) / K
    # the same random-policy loop replayed from a HIP graph (capture_steps: sample + step per step, no
    # host launches in between; the replays repeat the capture's draws while the state moves on)
    graph = None
    if not args.no_graph:
        G, R = venv.spec.max_episode_steps, 10
        g = venv.capture_steps(G)
        g.replay()
        torch.cuda.synchronize(dev)
        ev0.record(stream)
        for _ in range(R):
            g.replay()
        ev1.record(stream)
        torch.cuda.synchronize(dev)
        gms = ev0.elapsed_time(ev1) / (R * G)
        graph = {"ms_per_step": gms, "value": E / (gms * 1e-3), "unit": "env-steps/s per GPU",
                 "steps_per_graph": G, "replays": R,
                 "path": "PandaVecEnv.capture_steps: sample_actions + pgx_step x 50 in one HIP graph"}
        del g
    # configs[4]: ReachAO sharded over every rank (collective timing: all ranks take part)
    ao = None if args.no_ao else sharded_leg(dev, "PandaReachAO-v3", args.ao_envs, args.task_steps, 20, dist, rank,
                                            world, coll_dev)

    if rank == 0:
        traffic = None
        # the binding roofline: algorithmic FLOPs (op-counted in the oracle, frozen) over the
        # kernel's own launch time (HIP events on the launch stream)
        fkey = {"PandaReach-v3": "reach_table", "PandaPush-v3": "push", "PandaPickAndPlace-v3": "pick_and_place",
                "PandaReachAO-v3": "reach_ao"}.get(args.env_id)
        alg_bytes = alg_bytes_per_env_step(fkey or "reach_table", venv.obs_dim, venv.action_dim,
                                           venv.robot_contact_budget())["total"] * E
        achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
        valu = None
        if fkey:
            valu = valu_roofline(fkey, E / (kernel_ms * 1e-3), "env-steps/s of the step kernel alone (kernel_ms)")
            valu["binding"] = True
        if os.path.exists(PROFILE_JSON):
            with open(PROFILE_JSON) as f:
                prof = json.load(f)
            if prof.get("num_envs") == E and pmc_kernel_ok(prof, kname):
                traffic = prof.get("hbm_bytes_per_launch")
                ins = prof.get("valu_lane_ops_per_launch")
                if ins and valu:
                    # what the hardware issued (PMC SQ_INSTS_VALU x 64 lanes, the redundant lanes
                    # of the 16-lane rows included), next to the algorithmic count
                    valu["issued"] = {"lane_ops_per_env_step": ins / E,
                                      "tflops_equiv": 2.0 * ins / (kernel_ms * 1e-3) / 1e12,
                                      "redundancy": ins / E / valu["alg_flops_per_env_step"],
                                      "cycles_per_valu_instr": prof.get("cycles_per_valu_instr"),
                                      "stall_split": prof.get("stall_split"),
                                      "source": os.path.relpath(PROFILE_JSON, ROOT)}
        line = {
            # the step kernel alone: HIP events over --kernel-launches back-to-back launches on the launch
            # stream right after the timed window (launch gaps included; rocprof's kernel average,
            # profiles/, is the gap-free duration)
            "kernel_ms": kernel_ms,
            # HBM is reported as the contract asks but does not bind this kernel: a step is ~200 B of
            # state against a long dependent VALU chain per env, so the
            # kernel is latency / VALU-issue bound; roofline_valu is the figure that measures it
            "roofline": {"bound": "hbm", "binding": False,
                         "binds": "dependent VALU issue of one wave per SIMD (see roofline_valu)",
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "kernel": kname,
                         "kernel_ms": kernel_ms,
                         "alg_bytes_per_launch": alg_bytes},
            "roofline_valu": valu,
            "episode_stats_last_step": {"truncated": float(stats[0]), "success": float(stats[1]),
                                        "reward_sum": float(stats[2])},
        }
        if graph is not None:
            line["graph_replay"] = graph
        if ao is not None:
            line["reach_ao"] = ao
        if world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(venv, args.cpu_baseline_seconds)
        if world == 1 and not args.no_her:
            line["her_relabel"] = her_leg(dev, args.her_calls, not args.no_cpu_baseline)
        if world == 1 and not args.no_tasks:
            line["tasks"] = [task_leg(dev, "PandaPush-v3", 4096, args.task_steps, flops_key="push"),   # configs[2]
                             task_leg(dev, "PandaPickAndPlace-v3", 16384, args.task_steps,            # configs[3]
                                      flops_key="pick_and_place"),
                             task_leg(dev, args.env_id, E, args.task_steps, contacts=False,           # no table
                                      flops_key="reach_no_table"),
                             # the round-3 robot budget (4 points), for comparison only
                             task_leg(dev, "PandaPush-v3", 4096, args.task_steps, flops_key="push", full_manifold=False),
                             task_leg(dev, "PandaPickAndPlace-v3", 16384, args.task_steps, flops_key="pick_and_place",
                                      full_manifold=False)]
            line["sb3_host_path"] = host_path_leg(dev, args.env_id, E, 100)
        return line
    return {}


if __name__ == "__main__":
    main()
