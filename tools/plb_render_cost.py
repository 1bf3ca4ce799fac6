#!/usr/bin/env python3
"""Cost of the PLB renderer in the reference's own setting (rope.yml: 1500 particles, a 168^3 volume, a 512 x 512 image, spp 50) for B = 1 and
B = 12: bake, G-buffer and image timed separately with HIP events on the stream (warm-up, then the median of --runs runs), and one whole
`plb_unfold --env rope` sweep with the render's share of it.  Writes profiles/plb_render_cost.txt.

    python tools/plb_render_cost.py [--runs 20] [--out profiles/plb_render_cost.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from unidom_amd.algorithms import plb_unfold  # noqa: E402
from unidom_amd.engine.plb_render import PlbRenderer, render_conf_of  # noqa: E402
from unidom_amd.engine.plb_simulator import PlbSimulator, RopeConf  # noqa: E402


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_render_cost.txt"))
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    conf = RopeConf()
    rc = render_conf_of(conf)
    lines = [f"# tools/plb_render_cost.py on {torch.cuda.get_device_name(0)}: RopeConf reset state, {conf.n_particles} particles, volume {rc.voxel_res}, "
             f"image {rc.image_res}, spp {rc.spp}, max_ray_depth {rc.max_ray_depth}; HIP events, 3 warm-up runs, median (min .. max) of {args.runs} runs, ms"]
    for B in (1, 12):
        sim = PlbSimulator(conf, batch_size=B)
        state = sim.reset()
        r = PlbRenderer(conf, rc, batch_size=B)
        for name, fn in (("bake", lambda: r.bake(state)), ("gbuffer", lambda: r.gbuffer(state)), ("image", lambda: r.image(state))):
            med, lo, hi = timed(fn, args.runs)
            lines.append(f"B={B:<2d} {name:<8s} {med:10.3f}  ({lo:.3f} .. {hi:.3f})   per env {med / B:.3f}")
            print(lines[-1], flush=True)
        del r, sim
    if not args.no_sweep:
        # one whole sweep, the render inside it timed by events around PlbRenderer.render: bake + image only -- the renderer's creation
        # (its arenas' allocation, on PlbSimulator.render's first call) is part of the sweep's wall clock, not of this span
        span = {}
        orig = PlbRenderer.render

        def render(self, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(self, *a, **kw)
            e1.record()
            span["ev"] = (e0, e1)
            return out
        PlbRenderer.render = render
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = plb_unfold.unfold(conf, render_conf=rc)
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
        finally:
            PlbRenderer.render = orig
        rms = span["ev"][0].elapsed_time(span["ev"][1])
        lines.append(f"unfold sweep (12 envs, 1060 actions, one render; one run, wall clock incl. the creation of both handles): {total:.1f} ms, render (bake + image) "
                     f"{rms:.1f} ms = {100 * rms / total:.1f} % ; coverages {res['coverage'].tolist()} -> max_acxel {res['max_acxel']}")
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
