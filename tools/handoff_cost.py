#!/usr/bin/env python
"""What SimpleMPMSimulator.device_handoff costs and what a captured update wins back.

For pour_water and shape_rope at the bench shapes (32 envs; pour_water: one APG update of ep_len 3; shape_rope: one env.step_diff plus
the backward of its reward, bench.py's unit for that workload), on ONE non-default stream, ms per update for
    host     eager, the overflow flag carried from forward to backward by the host (side stream, pinned memory, event)
    device   eager, device_handoff: the backward takes clip bit 2 and enqueues the restore pass and the (here empty) recompute pass
    graph    device_handoff, the update replayed as one HIP graph
and, for the two eager modes, the span of the backward call per simulator step: HIP events around ud_mpm_step_bwd on its stream, in a
run of its own.  That span is the call's kernels PLUS the launch gaps between them -- an upper bound of the kernel time, and the
figure in which the second pass's near-empty launches show; kernel time proper comes from tools/kernel_stats.sh on the same workload.
Each figure: `--warmup` untimed updates, then `--repeats` windows, each ended by a device synchronise, of as many updates as fill
`--window` seconds (counted from a first timed update, at least 2); median and min..max of the windows.  The modes of a workload alternate window by window, so that drift hits them alike.

    python tools/handoff_cost.py [--workloads pour_water,shape_rope] [--modes host,device,graph] [--out profiles/handoff_cost.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class PourWater:
    """one APG update (policy, 3 x step_diff, loss, backward, clip, Adam)"""
    unit = "APG update, ep_len 3"

    def __init__(self, B, handoff, device):
        from unidom_amd.algorithms.apg.core import APG
        from unidom_amd.envs.registration import env_functions
        from unidom_amd.utils import prng
        self.env = env_functions["pour_water"](batch_size=B, seed=0, aux_reward=True, device=device)
        self.env.simulator.device_handoff = handoff
        _, self.state = self.env.reset(prng.PRNGKey(0))
        self.learner = APG(self.env, 3, learning_rate=1e-4, max_gradient_norm=0.3, seed=0)
        self.sim = self.env.simulator
        self.graphed = False

    def capture(self):
        self.learner.capture(self.state)
        self.graphed = True

    def update(self):
        if self.graphed:
            self.learner.minimize_captured()
        else:
            self.learner.minimize(self.state)


class ShapeRope:
    """one env.step_diff (30 simulator steps of 133 substeps) + the backward of the reward to the push action"""
    unit = "step_diff + backward"

    def __init__(self, B, handoff, device):
        from unidom_amd.envs.registration import env_functions
        self.env = env = env_functions["shape_rope"](batch_size=B, seed=0, device=device)
        env.simulator.device_handoff = handoff
        env.build_reset_state()
        self.st, self.sim = env.state, env.simulator
        N = self.sim.n_particles
        g = torch.Generator(device=device).manual_seed(0)
        mid = self.st.x[:, N // 2]
        ang = torch.rand((B,), device=device, generator=g) * 6.2831853
        off = torch.stack([torch.cos(ang), torch.zeros_like(ang), torch.sin(ang)], -1)
        self.act = torch.cat([mid - 0.02 * off, mid + 0.08 * off], -1).contiguous().requires_grad_(True)
        self.graph = None

    def _once(self):
        _, reward, _, _ = self.env.step_diff(self.act, self.st)
        (self.grad,) = torch.autograd.grad(reward.sum(), self.act)

    def capture(self):
        dev = self.act.device
        for _ in range(2):
            self._once()
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=torch.cuda.current_stream(dev)):
            self._once()

    def update(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self._once()


WORKLOADS = {"pour_water": PourWater, "shape_rope": ShapeRope}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pour_water,shape_rope")
    ap.add_argument("--modes", default="host,device,graph")
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handoff_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("handoff_cost: needs the GPU")
    dev = torch.device("cuda", 0)
    lines = [f"# tools/handoff_cost.py  {torch.cuda.get_device_name(dev)}  envs={args.envs} warmup={args.warmup} "
             f"windows={args.repeats} x {args.window} s  (ms per update: median  min..max of the windows)"]
    work = torch.cuda.Stream(dev)
    with torch.cuda.stream(work):
        for name in args.workloads.split(","):
            runs = {}
            for mode in args.modes.split(","):
                w = WORKLOADS[name](args.envs, mode != "host", dev)
                for _ in range(args.warmup):
                    w.update()
                torch.cuda.synchronize(dev)
                if mode == "graph":
                    t0 = time.perf_counter()
                    try:
                        w.capture()
                        w.update()
                        torch.cuda.synchronize(dev)
                        lines.append(f"{name:11s} graph   captured in {time.perf_counter() - t0:.1f} s")
                    except Exception as e:     # a refusal is a result: the table says so instead of a time
                        lines.append(f"{name:11s} graph   not captured: {type(e).__name__}: {e}")
                        continue
                runs[mode] = w
            ms = {m: [] for m in runs}
            updates = {}
            for m, w in runs.items():          # updates per window, from one timed update
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                w.update()
                torch.cuda.synchronize(dev)
                updates[m] = max(2, int(args.window / (time.perf_counter() - t0)))
            for _ in range(args.repeats):
                for m, w in runs.items():
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(updates[m]):
                        w.update()
                    torch.cuda.synchronize(dev)
                    ms[m].append((time.perf_counter() - t0) * 1e3 / updates[m])
            for m, v in ms.items():
                lines.append(f"{name:11s} {m:7s} {statistics.median(v):9.2f} ms per update ({WORKLOADS[name].unit})   {min(v):.2f}..{max(v):.2f}  ({updates[m]} updates per window)")
            for m in ("host", "device"):       # span of the step calls (kernels + launch gaps): events around each call, eager, a run of its own
                if m not in runs:
                    continue
                w = runs[m]
                w.sim.profile = {"fwd": [], "bwd": []}
                for _ in range(2):
                    w.update()
                torch.cuda.synchronize(dev)
                prof, w.sim.profile = w.sim.profile, None
                t = {k: float(np.mean([a.elapsed_time(b) for a, b in v])) for k, v in prof.items() if v}
                lines.append(f"{name:11s} {m:7s} backward call span {t['bwd']:.3f} ms, forward call span {t['fwd']:.3f} ms per simulator step (events around the call: kernels + launch gaps; {len(prof['bwd'])} steps)")
            for m, w in runs.items():
                w.sim.check_status()
                if m != "host":
                    lines.append(f"{name:11s} {m:7s} env-steps whose backward recomputed the grid: {w.sim.grid_recomputed_env_steps()}")
                else:
                    lines.append(f"{name:11s} {m:7s} steps whose backward recomputed the grid (whole batch): {w.sim.grid_ckpt_overflows}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
