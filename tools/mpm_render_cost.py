#!/usr/bin/env python
"""What the MPM renderer costs (csrc/mpm_render.hip: one setup launch and one tile launch per call, one workgroup per frame and
32 x 32 pixel tile, LDS z-buffer with a 64-bit LDS atomic minimum; no global atomics, no clear pass).

On one device and one stream, 640 x 480 frames, device events around MPMEnv.render_batch:
    whip_rope, 1 frame          67 particles as spheres, one box
    shape_rope, 1 frame         582 particles as spheres, one box
    pour_soup, 1 frame          7631 particles as points, two cut hollow spheres (sphere-traced); the same frame with the bowls' march
                                taken out (a handle with n_prims = 0) shows what the march costs
    shape_rope, T frames        the render call of one step_with_render: env 0 of every entry of info["state_list"]
    whip_rope, 32 envs          render_batch of a 32-env state
Beside each: the forward rollout (step_diff, no gradient) that produces those states, timed in the same session.
Each figure is the median (min..max) of `--repeats` calls timed one by one with device events after `--warmup` untimed calls; the
output tensors come from torch's caching allocator inside the call.

    python tools/mpm_render_cost.py [--repeats 20] [--warmup 5] [--out profiles/mpm_render_cost.txt] [--png DIR]

--png DIR writes the frames as PNG files (PIL) for a human to look at: the reset frame of every env and the frames of the step.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def save_png(directory, name, rgb):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(rgb)).save(os.path.join(directory, name))   # the MPM envs return RGB, as the reference


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpm_render_cost.txt"))
    ap.add_argument("--png", default=None, metavar="DIR")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mpm_render_cost: needs the GPU")
    if args.repeats < 20:
        sys.exit("mpm_render_cost: at least 20 repeats")
    from unidom_amd.engine.mpm_render import MpmRenderer
    from unidom_amd.envs.registration import env_functions
    dev = torch.device("cuda", 0)
    key = np.array([0, 7], np.uint32)
    lines = [f"# tools/mpm_render_cost.py  {torch.cuda.get_device_name(dev)}  640 x 480 frames, warmup={args.warmup}, median (min..max) of "
             f"{args.repeats} calls, device events around each call",
             "# built: tile kernel, one workgroup per (frame, 32 x 32 tile), LDS z-buffer (8 KiB) + survivor list (4 KiB), 64-bit LDS atomic minimum; "
             "arena 20 B per particle and frame, 48 B per primitive and frame; no global atomics, no clear pass"]

    def row(label, frames, t, t_roll=None, what=""):
        tail = "" if t_roll is None else f"   rollout {t_roll[0]:8.3f} ms ({t_roll[1]:.3f}..{t_roll[2]:.3f}) {what}-> render / rollout = {t[0] / t_roll[0]:.3f}"
        lines.append(f"  {label:36s} {t[0]:8.3f} ms ({t[1]:.3f}..{t[2]:.3f})   {frames:3d} frames, {t[0] / frames * 1e3:8.1f} us each{tail}")

    def make(name, B):
        env = env_functions[name](batch_size=B, seed=1)
        _, state = env.reset(key)
        if name.startswith("shape_rope"):
            a = torch.tensor([[0.45, 0.0, 0.45, 0.55, 0.0, 0.5]] * B, device=dev)
        else:
            a = torch.zeros((B, env.action_size), device=dev)
            a[:, 0] = 0.3
        return env, state, a

    with torch.no_grad():
        for name in ("whip_rope", "shape_rope", "pour_soup"):
            env, state, a = make(name, 1)
            r = env._renderer(state)
            lines.append(f"{name} ({r.n_particles} particles as {'points' if r.conf.mode else 'spheres'}, {r.n_prims} "
                         f"{'cut hollow spheres' if r.prim_kind else 'boxes'})")
            t_roll = timed(lambda: env.step_diff(a, state), args.warmup, args.repeats)
            t_one = timed(lambda: env.render_batch(state), args.warmup, args.repeats)
            row("1 frame", 1, t_one, t_roll, "(one step_diff forward) ")
            if args.png:
                save_png(args.png, f"{name}_reset.png", env.render(state)[0])
            if name == "pour_soup":
                bare = MpmRenderer(r.n_particles, np.zeros((0, 3), np.float32), r.prim_kind, env._render_conf(), device=dev)
                t_bare = timed(lambda: bare.frames(state.x), args.warmup, args.repeats)
                row("1 frame without the two bowls", 1, t_bare)
                lines.append(f"  the bowls' sphere trace (K = 64, eps = 1e-4): {t_one[0] - t_bare[0]:.3f} ms of {t_one[0]:.3f} ms "
                             f"= {100 * (t_one[0] - t_bare[0]) / t_one[0]:.0f} % of the frame")
            if name == "shape_rope":
                info = env.step_diff(a, state)[3]
                sl = info["state_list"]
                T = int(sl.x.shape[0])
                sl0 = sl._replace(x=sl.x[:, 0].contiguous(), primitives=[p._replace(position=p.position[:, 0].contiguous(), rotation=p.rotation[:, 0].contiguous())
                                                                         for p in sl.primitives])
                row(f"{T} frames (one step_with_render)", T, timed(lambda: env.render_batch(sl0), args.warmup, args.repeats), t_roll, "(the step_diff that makes them) ")
                if args.png:
                    for k, img in enumerate(env.step_with_render(a, state)[3]["img_list"]):
                        save_png(args.png, f"shape_rope_step_{k:02d}.png", img)
        if args.png:
            for name in ("shape_rope_hard", "pour_water"):
                env, state, _ = make(name, 1)
                save_png(args.png, f"{name}_reset.png", env.render(state)[0])
        env32, s32, a32 = make("whip_rope", 32)
        lines.append("whip_rope, 32 envs")
        row("render_batch, 32 envs", 32, timed(lambda: env32.render_batch(s32), args.warmup, args.repeats),
            timed(lambda: env32.step_diff(a32, s32), args.warmup, args.repeats), "(one step_diff forward, 32 envs) ")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
