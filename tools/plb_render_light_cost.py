#!/usr/bin/env python3
"""Cost of the four instances of the PLB renderer's image kernel (unlit, roulette, lit, lit + roulette) in the reference's setting (a 168^3
volume, a 512 x 512 image, spp 50) on the Torus scene (TorusConf reset state, torus.yml's camera) for B = 1 and B = 12, and of one
`plb_release --env torus` sweep (8 envs, the final frame only).  HIP events on the stream, warm-up, then the median of --runs runs.

--parent-so PATH: a libunidom_hip.so built from the parent commit (for instance `git worktree add ../parent HEAD~1 && make -C
../parent/unidom_amd/csrc`).  Its unlit image is then timed in the same session, twice, interleaved with two timings of this tree's unlit
instance: the distance between the parent's two medians is the run-to-run spread the unlit instance is held against.  The libraries are
driven through the C ABI directly (the parent's has no ud_plb_render_set_light, which the package insists on).

    python tools/plb_render_light_cost.py [--runs 20] [--parent-so PATH] [--out profiles/plb_render_light_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from unidom_amd import _lib  # noqa: E402
from unidom_amd.algorithms import plb_release  # noqa: E402
from unidom_amd.engine.plb_render import render_conf_of  # noqa: E402
from unidom_amd.engine.plb_simulator import PlbSimulator, TorusConf  # noqa: E402


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


class RawRenderer:
    """create / bake / image of one library through ctypes."""

    def __init__(self, L, conf, rc, B, state):
        M, P = _lib.RENDER_MAX_PRIM, len(conf.prim_radius)
        pad = lambda seq, fill: (list(seq)[:P] + [fill] * M)[:M]
        cc = _lib.ud_plb_render_conf(
            dx=float(rc.dx), voxel_res=(C.c_int * 3)(*rc.voxel_res), bake_size=int(rc.bake_size), sdf_threshold=float(rc.sdf_threshold),
            image_res=(C.c_int * 2)(*rc.image_res), spp=int(rc.spp), max_ray_depth=int(rc.max_ray_depth),
            camera_pos=(C.c_double * 3)(*rc.camera_pos), camera_rot=(C.c_double * 2)(*rc.camera_rot), n_primitives=P,
            prim_kind=(C.c_int * M)(*pad(conf.prim_kind, 0)), prim_radius=(C.c_double * M)(*pad(conf.prim_radius, 0.0)),
            prim_h=(C.c_double * M)(*pad(conf.prim_h, 0.0)), prim_color=(C.c_float * 3 * M)(*[(C.c_float * 3)(*c) for c in pad(conf.prim_color, (0.3, 0.3, 0.3))]),
            n_particles=int(conf.n_particles), max_envs=B)
        self.L, self.B, self.h = L, B, C.c_void_p()
        L.ud_last_error.restype = C.c_char_p
        for name, n in (("ud_plb_render_create", 2), ("ud_plb_render_destroy", 1), ("ud_plb_render_set_light", 2)):
            if hasattr(L, name):
                getattr(L, name).argtypes = [C.c_void_p] * n
        L.ud_plb_render_bake.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.ud_plb_render_image.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_uint] + [C.c_void_p] * 2
        self._ok(L.ud_plb_render_create(C.byref(cc), C.byref(self.h)))
        W, H = rc.image_res
        self.x, self.pp = state.x.contiguous(), state.prim_pos.contiguous()
        self.color = torch.full((conf.n_particles,), int(conf.particle_color), dtype=torch.int32, device="cuda")
        self.bbox, self.status = torch.empty((B, 2, 3), device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
        self.img = torch.empty((B, H, W, 3), device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        self._ok(L.ud_plb_render_bake(self.h, B, p(self.x), p(self.color), p(self.bbox), p(self.status), None))
        torch.cuda.synchronize()
        assert not bool(self.status.any()), "the Torus rod does not fit the volume"

    def _ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.ud_last_error().decode())

    def set_light(self, light, roulette, direction):
        ll = _lib.ud_plb_render_light(use_directional_light=int(light), use_roulette=int(roulette), light_direction=(C.c_double * 3)(*direction))
        self._ok(self.L.ud_plb_render_set_light(self.h, C.byref(ll)))

    def image(self):
        p = lambda t: C.c_void_p(t.data_ptr())
        self._ok(self.L.ud_plb_render_image(self.h, self.B, p(self.pp), None, None, 0, 0, p(self.img), None))

    def close(self):
        self.L.ud_plb_render_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_render_light_cost.txt"))
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    conf = TorusConf()
    rc = render_conf_of(conf)
    new = _lib.lib()
    parent = C.CDLL(os.path.abspath(args.parent_so)) if args.parent_so else None
    lines = [f"# tools/plb_render_light_cost.py on {torch.cuda.get_device_name(0)}: TorusConf reset state, {conf.n_particles} particles, volume {rc.voxel_res}, "
             f"image {rc.image_res}, spp {rc.spp}, max_ray_depth {rc.max_ray_depth}, camera {rc.camera_pos}, light {rc.light_direction}; image call only; "
             f"HIP events, 3 warm-up runs, median (min .. max) of {args.runs} runs, ms"]

    def say(B, name, t, note=""):
        lines.append(f"B={B:<2d} {name:<28s} {t[0]:10.3f}  ({t[1]:.3f} .. {t[2]:.3f})   per env {t[0] / B:.3f}{note}")
        print(lines[-1], flush=True)

    for B in (1, 12):
        state = PlbSimulator(conf, batch_size=B).reset()
        rn = RawRenderer(new, conf, rc, B, state)
        unlit = []
        if parent is not None:
            rp = RawRenderer(parent, conf, rc, B, state)
            par = []
            for k in (1, 2):                                  # parent, this tree, parent, this tree
                par.append(timed(rp.image, args.runs)); say(B, f"unlit, parent commit (run {k})", par[-1])
                unlit.append(timed(rn.image, args.runs)); say(B, f"unlit, this commit (run {k})", unlit[-1])
            assert torch.equal(rp.img, rn.img), "the unlit image differs from the parent's"
            spread = abs(par[0][0] - par[1][0])
            worst = max(abs(u[0] - p[0]) for u in unlit for p in par)
            lines.append(f"B={B:<2d} parent's run-to-run spread (between its two medians) {spread:.3f} ms; largest |this - parent| over the four pairs of medians "
                         f"{worst:.3f} ms; this / parent (means of the medians) {(unlit[0][0] + unlit[1][0]) / (par[0][0] + par[1][0]):.4f}; images bit-equal")
            print(lines[-1], flush=True)
            rp.close()
        else:
            unlit.append(timed(rn.image, args.runs)); say(B, "unlit, this commit", unlit[-1])
        base = statistics.mean(u[0] for u in unlit)
        for name, light, roulette in (("roulette", 0, 1), ("lit", 1, 0), ("lit + roulette", 1, 1)):
            rn.set_light(light, roulette, rc.light_direction)
            t = timed(rn.image, args.runs)
            say(B, name, t, f"   x {t[0] / base:.2f} of unlit")
        rn.close()
    if not args.no_sweep:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = plb_release.release(conf, num_envs=8, render_conf=rc)
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
        lines.append(f"plb_release sweep (8 envs, 600 actions, the final frame only; one run, wall clock incl. the creation of both handles): {total:.1f} ms; "
                     f"max_x {[round(float(v), 4) for v in res['max_x']]}")
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
