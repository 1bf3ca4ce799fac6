"""The small scene of the PLB renderer tests (tests/test_plb_render_cpu.py, tests/test_plb_render_gpu.py) and its twin results, computed once
per process and shared (never modified by a test).

Shapes: the smallest at which the kernels can still go wrong -- 96 particles in a blob about 0.06 wide, dx = 1/150, a non-cubic volume
(24, 20, 28) so that an axis mix-up shows, a non-square image (24, 16) so that aspect / transposition errors show, more than one 8 x 8 pixel tile
and a ragged one, three different clouds of which the last is wider than the volume (status 1), one Sphere and one rotated Capsule in view,
spp 2."""
import functools

import numpy as np

from plb_render_twin import RenderTwin, prims_of
from unidom_amd.engine.plb_render import RenderConf

N = 96
B = 3
SPP = 2
COLOR = (150 << 16) + 150          # rope.yml's first colour; per particle below: two colours, so that the colour bytes of the minimum matter


class SceneConf:
    """The PlbConf-like fields the renderer reads."""
    n_particles = N
    prim_kind = (0, 1)
    prim_radius = (0.012, 0.007)
    prim_h = (0.0, 0.03)
    prim_shape = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    prim_color = ((0.7, 0.7, 0.7), (0.8, 0.3, 0.2))
    particle_color = COLOR


def render_conf(**kw):
    base = dict(dx=1.0 / 150, voxel_res=(24, 20, 28), image_res=(24, 16), spp=SPP, camera_pos=(0.5, 0.1, 0.66), camera_rot=(0.2, 0.0))
    base.update(kw)
    return RenderConf(**base)


@functools.lru_cache(maxsize=None)
def scene():
    rng = np.random.default_rng(7)
    x = np.empty((B, N, 3))
    x[0] = (rng.random((N, 3)) - 0.5) * (0.05, 0.04, 0.06) + (0.5, 0.06, 0.5)
    x[1] = (rng.random((N, 3)) - 0.5) * (0.04, 0.03, 0.07) + (0.505, 0.055, 0.49)
    x[2] = (rng.random((N, 3)) - 0.5) * (0.2, 0.03, 0.05) + (0.5, 0.06, 0.5)       # 30 cells wide: more than voxel_res[0] = 24
    color = np.where(np.arange(N) % 3 == 0, 100, COLOR).astype(np.int32)
    th = 0.6                                                                        # the Capsule, turned about z
    prim_pos = np.array([[[0.458, 0.05, 0.51], [0.543, 0.06, 0.5]], [[0.46, 0.055, 0.5], [0.54, 0.065, 0.51]], [[0.458, 0.05, 0.51], [0.543, 0.06, 0.5]]])
    prim_rot = np.array([[[1.0, 0.0, 0.0, 0.0], [np.cos(th / 2), 0.0, 0.0, np.sin(th / 2)]]] * B)
    x.setflags(write=False); color.setflags(write=False); prim_pos.setflags(write=False); prim_rot.setflags(write=False)
    return dict(x=x, color=color, prim_pos=prim_pos, prim_rot=prim_rot)


@functools.lru_cache(maxsize=None)
def twin():
    return RenderTwin(render_conf())


@functools.lru_cache(maxsize=None)
def twin_bake():
    s = scene()
    return twin().bake(s["x"], s["color"])


def twin_prims(b):
    s = scene()
    return prims_of(SceneConf, s["prim_pos"][b], s["prim_rot"][b])


@functools.lru_cache(maxsize=None)
def twin_gbuffer():
    return [twin().gbuffer(e, twin_prims(b)) for b, e in enumerate(twin_bake())]


@functools.lru_cache(maxsize=None)
def twin_image(seed=0, spp=SPP, nudge=0):
    return [twin().image(e, twin_prims(b), spp=spp, seed=seed, nudge=nudge) for b, e in enumerate(twin_bake())]
