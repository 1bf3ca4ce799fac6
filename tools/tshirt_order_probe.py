#!/usr/bin/env python3
"""fold_tshirt throughput per cloth kernel mode, in one process (bench.py's fold_tshirt workload has no kernel-mode leg).

Modelled on bench.py's bench_fold_tshirt: 4 envs, one "step" = one env.step_diff (40 x 50 substeps) + the backward of the reward to
the pick-and-place action; 2 warm-up and 5 timed steps per mode.  One JSON line per mode:
    0   order v2, several workgroups per env (the default)
    3   reference order, several workgroups per env (csrc/cloth_cluster_ref.hip)
    1   reference order, one 1024-lane workgroup per env (forward and adjoint)
with substeps/s and the mean forward / backward kernel time per call (CUDA events around the launches, ClothSimulator.profile).
usage: python tools/tshirt_order_probe.py [--modes 0,3,1] [--envs 4] [--steps 5] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MACRO = 40   # robot steps per step_diff (bench.py's MACRO)


def probe(mode, B, steps, warmup, device="cuda:0"):
    from unidom_amd.envs.fold_cloth_tshirt_env import DefaultConf
    from unidom_amd.envs.registration import env_functions
    conf = DefaultConf()
    conf.kernel_mode = mode
    env = env_functions["fold_tshirt"](batch_size=B, conf=conf, aux_reward=True, device=device)
    sim = env.simulator
    _, st = env.reset(np.array([0, 5], np.uint32))
    g = torch.Generator(device=device).manual_seed(0)
    xm = st.x.mean(1)
    off = (torch.rand((B, 2), device=device, generator=g) - 0.5) * 0.2
    act = torch.stack([xm[:, 0] + off[:, 0], torch.zeros_like(off[:, 0]), xm[:, 2] + off[:, 1],
                       xm[:, 0] - off[:, 0], torch.zeros_like(off[:, 0]), xm[:, 2] - off[:, 1]], -1).contiguous().requires_grad_(True)

    def one():
        act.grad = None
        _, reward, _, _ = env.step_diff(act, st)
        reward.sum().backward()

    for _ in range(warmup):
        one()
    sim.profile = {"fwd": [], "bwd": []}
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    prof, sim.profile = sim.profile, None
    assert torch.isfinite(act.grad).all()
    sim.check_status()
    k_ms = {k: float(np.mean([a.elapsed_time(b) for a, b in vv])) for k, vv in prof.items() if vv}
    units = B * MACRO * sim.substeps * steps
    return {"probe": "tshirt_order", "kernel_mode": mode, "several_workgroups": sim.launch_envs(64) < 64, "envs": B,
            "particles": int(st.x.shape[1]), "steps": steps, "warmup": warmup, "substeps_per_sec": units / dt,
            "ms_per_step": dt / steps * 1e3, "fwd_ms": k_ms.get("fwd"), "bwd_ms": k_ms.get("bwd"),
            "fwd_calls_per_step": len(prof["fwd"]) // steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="0,3,1")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for m in (int(s) for s in a.modes.split(",")):
        print(json.dumps(probe(m, a.envs, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
