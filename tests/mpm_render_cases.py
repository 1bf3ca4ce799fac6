"""Scenes for the MPM renderer's tests and the f64 closed forms its twin is held to: the hand-made kernel scene (every path of
csrc/mpm_render.hip in three frames of 1030 particles and two primitives), its copy with cut hollow spheres, and the smallest frame."""
import math

import numpy as np

from cloth_render_cases import SIZES, plane_depth_f64, rays_f64, sphere_depth_f64, unproject   # noqa: F401  (re-exported for the tests)
from mpm_render_twin import Conf

KERNEL_SIZES = [(50, 38), (37, 29)]
N_SHEET, N_PARTICLES = 1020, 1030
EDGE = dict(tie_lo=1020, tie_hi=1021, corner=1022, reach_in=1023, outside=1024, behind=1025, sunk=1026, near=1027, nan=1028, front=1029)
BOX_SIZES = np.array([[0.06, 0.03, 0.05], [0.08, 0.0, 0.06]], np.float32)            # the second is a plate
BOWL_SIZES = np.array([[0.09, 0.0, 0.008], [0.08, 0.0, 0.008]], np.float32)
CAM_SIM = np.array([0.9, 1.0, 0.5])                                                   # Conf.camera_pos in sim order


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[math.cos(0.5 * angle)], math.sin(0.5 * angle) * a])


def rot_f64(q):
    """the rotation matrix of the unit quaternion (w, x, y, z): local -> sim"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def local_rays_f64(conf, pos, q):
    """(o [3], dl [3,H,W]) in f64: the camera and the pixel rays in the primitive's local frame; depth t is the point o + t dl"""
    rx, ry, cam = rays_f64(conf)
    R, P = cam["R"], cam["P"]
    D = [R[0, c] * rx + R[1, c] * ry - R[2, c] for c in range(3)]
    Ds = np.stack([D[0], D[2], D[1]])
    A = rot_f64(q).T
    o = A @ (P[[0, 2, 1]] - np.asarray(pos, np.float64))
    return o, np.einsum("ab,bhw->ahw", A, Ds)


def box_depth_f64(conf, pos, q, size):
    """f64 slab test: entry depth [H,W], nan where the ray misses"""
    o, dl = local_rays_f64(conf, pos, q)
    s = np.asarray(size, np.float64)
    with np.errstate(all="ignore"):
        t1 = (-s[:, None, None] - o[:, None, None]) / dl
        t2 = (s[:, None, None] - o[:, None, None]) / dl
        tnear, tfar = np.minimum(t1, t2).max(0), np.maximum(t1, t2).min(0)
    return np.where((tnear <= tfar) & (tnear >= conf.znear), tnear, np.nan)


def bowl_sdf_f64(size, p):
    r, h, t = (float(v) for v in size)
    w = math.sqrt(r * r - h * h)
    q0, q1 = np.sqrt(p[0] * p[0] + p[2] * p[2]), p[1]
    return np.where(h * q0 < w * q1, np.sqrt((q0 - w) ** 2 + (q1 - h) ** 2) - t, np.abs(np.sqrt(q0 * q0 + q1 * q1) - r) - t)


def bowl_outer_f64(conf, pos, q, size):
    """(depth, ok) [H,W]: the f64 ray-sphere depth for radius r + t, and where that entry point lies on the outer lower hemisphere
    (local y < 0) with the ray's incidence cosine >= 0.5"""
    o, dl = local_rays_f64(conf, pos, q)
    rb = float(size[0]) + float(size[2])
    dep = sphere_depth_f64(conf, pos, rb)
    with np.errstate(invalid="ignore"):
        p = o[:, None, None] + dep * dl
        cosang = -(p * dl).sum(0) / (rb * np.sqrt((dl * dl).sum(0)))
        ok = np.isfinite(dep) & (dep >= conf.znear) & (p[1] < -1e-3) & (cosang >= 0.5)
    return dep, ok


def _along(centre, f):
    """the point at f times the way from the camera to `centre` (sim order)"""
    return (CAM_SIM + f * (np.asarray(centre, np.float64) - CAM_SIM)).tolist()


def kernel_scene(W, H, kind=0, mode=0, point_size=1):
    """(conf, x [3,1030,3] f32, prim_pos [3,2,3], prim_rot [3,2,4], sizes [2,3]).  Particles 0..1019: a 34 x 30 sheet above the ground,
    rippled differently in each frame.  Then (EDGE): two at one position (the lower index wins), one on the tile corner at pixel (32, 32),
    one centred left of the image whose disc reaches in, one wholly outside, one behind primitive 0, one half sunk in the ground, one
    with znear < d < znear + r (dropped in sphere mode), one with a NaN coordinate (dropped), one in front of primitive 1.
    kind 0: a box and a plate (zero half size), both rotated; kind 1: two cut hollow spheres, the second tilted towards the camera."""
    conf = Conf(width=W, height=H, mode=mode, prim_kind=kind, radius=0.012, point_size=point_size,
                particle_color=(0.5, 0.5, 0.5, 1.0) if mode == 0 else (100 / 255, 100 / 255, 249 / 255, 125 / 255))
    P = lambda a, b, d: unproject(conf, a, b, d)
    sizes = BOX_SIZES if kind == 0 else BOWL_SIZES
    i, j = np.meshgrid(np.arange(34), np.arange(30), indexing="ij")
    xs, pos, rot = [], [], []
    gu, gv = (int(0.25 * W) + 0.5) / W, (int(0.77 * H) + 0.5) / H                         # a pixel centre that sees the ground
    gd = float(plane_depth_f64(conf, conf.ground_z)[int(0.77 * H), int(0.25 * W)])
    for m, (dx, amp) in enumerate([(0.0, 0.01), (0.03, 0.02), (-0.05, 0.0)]):
        c0, c1 = np.array([0.35 + dx, 0.12, 0.55]), np.array([0.62 + dx, 0.16 + 0.02 * m, 0.4])
        if kind == 0:
            q0, q1 = quat((1, 2, 3), 0.7 + 0.3 * m), quat((3, -1, 2), -1.1 + 0.2 * m)
        else:
            q0, q1 = quat((1, 0, 2), 0.15 + 0.1 * m), quat((0.2, 0, 1), -1.0 - 0.2 * m)
        sheet = np.stack([0.15 + 0.7 * i / 33 + dx, 0.04 + amp * np.sin(0.9 * i + 0.5 * j), 0.15 + 0.7 * j / 29], -1).reshape(-1, 3)
        edge = [P(0.3, 0.3, 0.5), P(0.3, 0.3, 0.5), P(32 / W, 32 / H, 0.3), P(-0.01, 0.4, 0.3), P(1.6, 0.5, 0.5), _along(c0, 1.25),
                P(gu, gv, gd), P(0.5, 0.5, 0.06), [0.4, float("nan"), 0.4], _along(c1, 0.6)]
        xs.append(np.concatenate([sheet, np.asarray(edge)]))
        pos.append([c0, c1])
        rot.append([q0, q1])
    x = np.asarray(xs, np.float32)
    assert x.shape == (3, N_PARTICLES, 3)
    return conf, x, np.asarray(pos, np.float32), np.asarray(rot, np.float32), sizes.copy()


def single_particle(W, H, mode=0):
    """(conf, x [1,1,3]): one particle, no primitive (a handle with n_prims = 0)"""
    conf = Conf(width=W, height=H, mode=mode, radius=0.03)
    return conf, np.asarray([[unproject(conf, 0.4, 0.45, 0.6)]], np.float32)
