"""The cloth renderer's specification: the operation order of the ud_cloth_render_* block of include/unidom_hip.h restated in NumPy
f32, one operation per rounding (NumPy neither contracts nor reassociates; its f32 divide and sqrt are correctly rounded).  The
kernels of csrc/cloth_render.hip are held bit-equal to this in colour, depth and triangle id (tests/test_cloth_render_gpu.py); this
file is held to f64 geometry and to its stated properties by tests/test_cloth_render_cpu.py.

render(conf, faces, vertices, spheres) -> (color [H,W,3] u8, depth [H,W] f32, tri [H,W] i32) in the returned orientation (mirrored
left-right, channels reversed); `unmirrored=True` gives the render before py_render.py:110-111 (RGB, column u at u).
"""
import math

import numpy as np

f32 = np.float32


class Conf:
    """ud_cloth_render_conf with its defaults (positions in the render frame, z up)."""
    width, height = 640, 480
    yfov = math.pi / 3.0
    znear = 0.05
    camera_pos = (0.9, 0.5, 1.0)
    camera_target = (0.6, 0.5, 0.0)
    camera_up = (0.0, 0.0, 1.0)
    ground_min = (-0.02, -0.04)
    ground_max = (0.98, 0.96)
    ground_z = -0.02
    cloth_color = (0.12, 0.2, 0.35)
    ground_color = (0.3, 0.2, 0.12)
    sphere_color = (0.35, 0.05, 0.05)

    def __init__(self, **kw):
        for k, v in kw.items():
            assert hasattr(type(self), k), k
            setattr(self, k, v)


def camera_f64(conf):
    """look_at (py_render.py:50-70) and the pinhole constants in f64: R (rows x, y, z), P, fx, fy, cx, cy."""
    P, T, U = (np.asarray(v, np.float64) for v in (conf.camera_pos, conf.camera_target, conf.camera_up))
    z = P - T
    z = z / math.sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2])
    x = np.array([U[1] * z[2] - U[2] * z[1], U[2] * z[0] - U[0] * z[2], U[0] * z[1] - U[1] * z[0]])
    x = x / math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]])
    t = math.tan(0.5 * conf.yfov)
    W, H = conf.width, conf.height
    return dict(R=np.stack([x, y, z]), P=P, fx=(0.5 * W) / ((W / H) * t), fy=(0.5 * H) / t, cx=0.5 * W, cy=0.5 * H)


class _K:
    """the handle's f32 constants (ClothRenderK)"""

    def __init__(self, conf):
        c = camera_f64(conf)
        self.W, self.H = int(conf.width), int(conf.height)
        self.R = c["R"].astype(f32)
        self.P = c["P"].astype(f32)
        self.fx, self.fy, self.cx, self.cy = f32(c["fx"]), f32(c["fy"]), f32(c["cx"]), f32(c["cy"])
        self.znear = f32(conf.znear)
        self.gmin = np.asarray(conf.ground_min, np.float64).astype(f32)
        self.gmax = np.asarray(conf.ground_max, np.float64).astype(f32)
        self.gz = f32(conf.ground_z)
        co, ci = math.cos(math.pi / 6.0), math.cos(math.pi / 16.0)
        self.cos_outer, self.cos_range, self.inv_pi = f32(co), f32(ci - co), f32(1.0 / math.pi)
        self.col = [np.asarray(v, f32) for v in (conf.cloth_color, conf.sphere_color, conf.ground_color)]


def _eye(k, p):
    """sim-order points [..., 3] -> eye frame (three arrays)"""
    p = np.asarray(p, f32)
    q = [p[..., 0] - k.P[0], p[..., 2] - k.P[1], p[..., 1] - k.P[2]]
    return [(k.R[r, 0] * q[0] + k.R[r, 1] * q[1]) + k.R[r, 2] * q[2] for r in range(3)]


def _edge(p, q, ip, iq, px, py):
    if ip < iq:
        return (q[0] - p[0]) * (py - p[1]) - (q[1] - p[1]) * (px - p[0])
    return -((p[0] - q[0]) * (py - q[1]) - (p[1] - q[1]) * (px - q[0]))


def _lit(k, n, e):
    ne = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]
    flip = ne > 0
    n = [np.where(flip, -c, c) for c in n]
    ndl_d = np.maximum(n[2], f32(0))
    r2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    rl = np.sqrt(r2)
    ndl_s = np.maximum(-((n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]) / rl, f32(0))
    cosang = -e[2] / rl
    s = np.minimum(np.maximum((cosang - k.cos_outer) / k.cos_range, f32(0)), f32(1))
    spot = (s * s) * (f32(3) - f32(2) * s)
    return f32(0.05) + (f32(1) * ndl_d + ((f32(10) * spot) * ndl_s) / r2) * k.inv_pi


def render(conf, faces, vertices, spheres=None, unmirrored=False):
    with np.errstate(all="ignore"):
        return _render(conf, faces, vertices, spheres, unmirrored)


def _render(conf, faces, vertices, spheres, unmirrored):
    k = _K(conf)
    W, H = k.W, k.H
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    verts = np.asarray(vertices, f32).reshape(-1, 3)
    xe, ye, ze = _eye(k, verts)
    d = -ze
    sx = k.cx + (k.fx * xe) / d
    sy = k.cy - (k.fy * ye) / d

    # ---- mesh: nearest depth, then lowest index (ascending loop + strict <)
    zbuf = np.full((H, W), np.inf, f32)
    tri = np.full((H, W), -1, np.int32)
    for t, (ia, ib, ic) in enumerate(faces):
        if not (d[ia] >= k.znear and d[ib] >= k.znear and d[ic] >= k.znear):
            continue
        A, B, C = (sx[ia], sy[ia]), (sx[ib], sy[ib]), (sx[ic], sy[ic])
        area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
        if not (area > 0 or area < 0):
            continue
        s = f32(1) if area > 0 else f32(-1)
        lx = max(np.ceil(min(A[0], B[0], C[0]) - f32(0.5)), f32(0))
        hx = min(np.floor(max(A[0], B[0], C[0]) - f32(0.5)), f32(W - 1))
        ly = max(np.ceil(min(A[1], B[1], C[1]) - f32(0.5)), f32(0))
        hy = min(np.floor(max(A[1], B[1], C[1]) - f32(0.5)), f32(H - 1))
        if not (lx <= hx and ly <= hy):
            continue
        x0, x1, y0, y1 = int(lx), int(hx), int(ly), int(hy)
        px = (np.arange(x0, x1 + 1, dtype=np.int32).astype(f32) + f32(0.5))[None, :]
        py = (np.arange(y0, y1 + 1, dtype=np.int32).astype(f32) + f32(0.5))[:, None]
        e0, e1, e2 = _edge(B, C, ib, ic, px, py), _edge(C, A, ic, ia, px, py), _edge(A, B, ia, ib, px, py)
        esum = (e0 + e1) + e2
        dep = esum / ((e0 / d[ia] + e1 / d[ib]) + e2 / d[ic])
        cov = (s * e0 >= 0) & (s * e1 >= 0) & (s * e2 >= 0) & (s * esum > 0) & (dep >= k.znear)
        zs, ts = zbuf[y0:y1 + 1, x0:x1 + 1], tri[y0:y1 + 1, x0:x1 + 1]
        win = cov & (dep < zs)
        zs[win] = dep[win]
        ts[win] = t
    best = np.where(tri >= 0, zbuf, f32(0)).astype(f32)

    # ---- per pixel: spheres, ground
    rx = np.broadcast_to((((np.arange(W, dtype=np.int32).astype(f32) + f32(0.5)) - k.cx) / k.fx)[None, :], (H, W))
    ry = np.broadcast_to(((k.cy - (np.arange(H, dtype=np.int32).astype(f32) + f32(0.5))) / k.fy)[:, None], (H, W))
    sn = [np.zeros((H, W), f32) for _ in range(3)]
    qa = (rx * rx + ry * ry) + f32(1)
    for sp in (np.zeros((0, 4), f32) if spheres is None else np.asarray(spheres, f32).reshape(-1, 4)):
        r = sp[3]
        if not (r > 0):
            continue
        cxe, cye, cze = _eye(k, sp[:3])
        tc = ((rx * cxe + ry * cye) - cze) / qa
        qx, qy, qz = cxe - tc * rx, cye - tc * ry, cze + tc
        h2 = r * r - ((qx * qx + qy * qy) + qz * qz)
        ts = tc - np.sqrt(h2 / qa)
        take = (h2 >= 0) & (ts >= k.znear) & ((tri == -1) | (ts < best))
        tri = np.where(take, np.int32(-2), tri)
        best = np.where(take, ts, best)
        for a, v in enumerate(((ts * rx - cxe) / r, (ts * ry - cye) / r, (-ts - cze) / r)):
            sn[a] = np.where(take, v, sn[a])
    D = [(k.R[0, c] * rx + k.R[1, c] * ry) - k.R[2, c] for c in range(3)]
    tg = (k.gz - k.P[2]) / D[2]
    hx, hy = k.P[0] + tg * D[0], k.P[1] + tg * D[1]
    take = ((D[2] < 0) & (tg >= k.znear) & (hx >= k.gmin[0]) & (hx <= k.gmax[0]) & (hy >= k.gmin[1]) & (hy <= k.gmax[1])
            & ((tri == -1) | (tg < best)))
    tri = np.where(take, np.int32(-3), tri)
    best = np.where(take, tg, best).astype(f32)

    # ---- shading
    e = [best * rx, best * ry, -best]
    tid = np.maximum(tri, 0)
    if len(faces):
        ia, ib, ic = faces[tid, 0], faces[tid, 1], faces[tid, 2]
        u = [xe[ib] - xe[ia], ye[ib] - ye[ia], d[ia] - d[ib]]
        v = [xe[ic] - xe[ia], ye[ic] - ye[ia], d[ia] - d[ic]]
        n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ok = ln > 0
        n = [np.where(ok, n[0] / ln, f32(0)), np.where(ok, n[1] / ln, f32(0)), np.where(ok, n[2] / ln, f32(1))]
    else:
        n = [np.zeros((H, W), f32), np.zeros((H, W), f32), np.ones((H, W), f32)]
    gn = [k.R[0, 2], k.R[1, 2], k.R[2, 2]]
    n = [np.where(tri == -2, sn[a], np.where(tri == -3, gn[a], n[a])).astype(f32) for a in range(3)]
    lit = _lit(k, n, e)
    mat = np.where(tri >= 0, 0, np.where(tri == -2, 1, 2))
    col = np.stack(k.col)[mat]                                           # [H,W,3] RGB base
    c = np.minimum(np.maximum(col * lit[..., None], f32(0)), f32(1)) * f32(255) + f32(0.5)
    rgb = np.where((tri == -1)[..., None], np.uint8(255), c.astype(np.int32).astype(np.uint8))
    depth = np.where(tri == -1, f32(0), best).astype(f32)
    if unmirrored:
        return rgb, depth, tri
    return np.ascontiguousarray(rgb[:, ::-1, ::-1]), np.ascontiguousarray(depth[:, ::-1]), np.ascontiguousarray(tri[:, ::-1])
