#!/usr/bin/env python
"""What the cloth renderer costs (csrc/cloth_render.hip: one setup launch and one tile launch per call, one workgroup per frame and
32 x 32 pixel tile, LDS z-buffer with a 64-bit LDS atomic minimum; no global atomics, no clear pass).

On one device and one stream, 640 x 480 frames:
    fold_cloth1, 1 frame        ClothEnv.render_batch of one env (840 faces)
    fold_cloth1, 40 frames      the render call of one step_with_render: env 0 of the 40 macro states (12 000 workgroups)
    fold_tshirt, 1 frame        6536 faces
    fold_cloth1, 32 envs        render_batch of a 32-env state
    step_diff forward           the rollout whose states the 40 frames draw (no gradient), for scale
Each figure is the median (min..max) of `--repeats` calls timed one by one with device events after `--warmup` untimed calls; the
output tensors come from torch's caching allocator inside the call.  Next to each time: the bytes the call must write (colour 3 B and
depth 4 B per pixel) over the time, as a fraction of the HBM peak rate.

    python tools/cloth_render_cost.py [--repeats 20] [--warmup 5] [--out profiles/cloth_render_cost.txt] [--png DIR]

--png DIR writes the frames as PNG files (PIL) for a human to look at: the reset frame of both tasks and the 40 frames of the step.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes/s, MI355X specification


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


def save_png(directory, name, bgr):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(os.path.join(directory, name))   # the env returns BGR, as the reference


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloth_render_cost.txt"))
    ap.add_argument("--png", default=None, metavar="DIR")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cloth_render_cost: needs the GPU")
    if args.repeats < 20:
        sys.exit("cloth_render_cost: at least 20 repeats")
    from unidom_amd.envs.fold_cloth1_env import FoldCloth1Env
    from unidom_amd.envs.fold_cloth_tshirt_env import FoldTshirtEnv
    dev = torch.device("cuda", 0)
    lines = [f"# tools/cloth_render_cost.py  {torch.cuda.get_device_name(dev)}  640 x 480 frames, warmup={args.warmup}, median (min..max) of "
             f"{args.repeats} calls, device events around each call; HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s",
             "# built: tile kernel, one workgroup per (frame, 32 x 32 tile), LDS z-buffer (8 KiB) + survivor list (4 KiB), ds_min_u64; arena 20 B per "
             "vertex and frame; no global atomics, no clear pass"]

    def row(label, frames, t):
        wb = frames * 640 * 480 * 7
        lines.append(f"  {label:34s} {t[0]:8.3f} ms ({t[1]:.3f}..{t[2]:.3f})   {frames:5d} frames, {t[0] / frames * 1e3:8.1f} us each; writes "
                     f"{wb / 1e6:7.1f} MB -> {wb / t[0] / 1e9:5.2f} TB/s = {100 * wb / (t[0] * 1e-3) / HBM_PEAK:4.1f} % of HBM peak")

    with torch.no_grad():
        env = FoldCloth1Env(2)
        _, state = env.reset(np.array([0, 1], np.uint32))
        one = state._replace(x=state.x[:1], primitive0=state.primitive0[:1])
        lines.append(f"fold_cloth1 ({len(env.simulator.indices)} faces, {env.simulator.N ** 2} vertices)")
        row("1 frame", 1, timed(lambda: env.render_batch(one), args.warmup, args.repeats))
        p = state.x[:, 100]
        actions = torch.cat([p, p + torch.tensor([0.1, 0.0, 0.1], device=p.device)], -1)
        t_step = timed(lambda: env.step_diff(actions, state, want_lists=True), args.warmup, args.repeats)
        sl = env.step_diff(actions, state, want_lists=True)[3]["state_list"]
        sl0 = sl._replace(x=sl.x[:, 0].contiguous(), primitive0=sl.primitive0[:, 0].contiguous())
        row("40 frames (one step_with_render)", 40, timed(lambda: env.render_batch(sl0), args.warmup, args.repeats))
        lines.append(f"  {'step_diff forward, 2 envs, lists':34s} {t_step[0]:8.3f} ms ({t_step[1]:.3f}..{t_step[2]:.3f})   the rollout those 40 frames draw")
        if args.png:
            save_png(args.png, "fold_cloth1_reset.png", env.render(state)[0])
            for k, img in enumerate(env.step_with_render(actions, state)[3]["img_list"]):
                save_png(args.png, f"fold_cloth1_step_{k:02d}.png", img)
        env32 = FoldCloth1Env(32)
        _, s32 = env32.reset(np.array([0, 1], np.uint32))
        row("render_batch, 32 envs", 32, timed(lambda: env32.render_batch(s32), args.warmup, args.repeats))
        tenv = FoldTshirtEnv(1)
        _, ts = tenv.reset(np.array([0, 3], np.uint32))
        lines.append(f"fold_tshirt ({len(tenv.simulator.indices)} faces, {tenv.simulator.N ** 2} vertices)")
        row("1 frame", 1, timed(lambda: tenv.render_batch(ts), args.warmup, args.repeats))
        if args.png:
            save_png(args.png, "fold_tshirt_reset.png", tenv.render(ts)[0])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
