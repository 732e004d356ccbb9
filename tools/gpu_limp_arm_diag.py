"""Where the limp arm's qd deviation from the fp64 oracle comes from (DESIGN.md section 6 "limp
arm", profiles/r10/limp_arm_per_substep.log): tests/test_gpu_limp_arm.py's ballistic step of
PandaReachJoints-v3 with 1 and with 20 substeps, gravity only / qd0 +-1 / qd0 +-10 / every env at
the neutral pose, both layouts; per dof the median, the largest and the signed mean of
qd - qd64, device and fp32 oracle.  Needs a GPU:  python tools/gpu_limp_arm_diag.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import panda_gym_amd as pg
from oracle import oracle as O
import limp_arm as L
import test_gpu_limp_arm as T

pg.load_native()
n = 256
for substeps in (1, 20):
    for label, qd_scale, spread in (("gravity only (qd0 = 0)", 0.0, 0.4), ("qd0 +-1", 1.0, 0.4), ("qd0 +-10", 10.0, 0.4),
                                    ("neutral pose, qd0 +-1", 1.0, 0.0)):
        for lanes in (16, 1):
            v = T._make(pg, "PandaReachJoints-v3", n, 0.0, lanes, n_substeps=substeps)
            q0, qd0 = L.start_state(v._cfg, n, 7, spread, qd_max=qd_scale)
            T._inject(v, q0, qd0)
            r64, r32 = T._oracles(O, v)
            o64, o32, q, qd, obs = T._step_all(v, r64, r32, torch.zeros((n, 7), device="cuda:0"))
            v.close()
            ed, ef = np.abs(qd - r64.qd), np.abs(r32.qd - r64.qd)
            print(f"substeps {substeps} {label} lanes {lanes}: qd p50/p99/max device {L.fmt(L.pcts(ed))} | fp32 {L.fmt(L.pcts(ef))}")
            print("    p50 per dof device", L.fmt(np.median(ed, 0)), "| fp32", L.fmt(np.median(ef, 0)))
            print("    max per dof device", L.fmt(np.max(ed, 0)), "| fp32", L.fmt(np.max(ef, 0)))
            # signed mean error per dof: a bias (a wrong constant) shows as |mean| ~ p50
            print("    mean signed per dof device", " / ".join(f"{x:+.1e}" for x in (qd - r64.qd).mean(0)),
                  "| fp32", " / ".join(f"{x:+.1e}" for x in (r32.qd - r64.qd).mean(0)))
