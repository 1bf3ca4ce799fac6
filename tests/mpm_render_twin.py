"""The MPM renderer's specification: the operation order of the ud_mpm_render_* block of include/unidom_hip.h restated in NumPy f32, one
operation per rounding, by brute force: every particle and every primitive is evaluated at every pixel -- no bounding window, no tiles
(particles go through in chunks only to bound memory).  The kernels of csrc/mpm_render.hip are held bit-equal to this in colour, depth
and id (tests/test_mpm_render_gpu.py), which is also what shows that their culling window is conservative; this file is held to f64
geometry and to its stated properties by tests/test_mpm_render_cpu.py.

render(conf, x, prim_pos, prim_rot, prim_sizes) -> (color [H,W,3] u8 RGB, depth [H,W] f32, id [H,W] i32), not mirrored.
Camera, eye and lit are the cloth twin's (the contract says they are the same operations).
"""
import numpy as np

import cloth_render_twin as ct

f32 = np.float32
MARCH_K = 64
MARCH_EPS = f32(1.0e-4)
NORMAL_STEP = f32(1.0e-4)
FLT_MAX = f32(3.4028235e38)


class Conf(ct.Conf):
    """ud_mpm_render_conf with its defaults"""
    particle_color = (0.5, 0.5, 0.5, 1.0)
    prim_color = (0.35, 0.3, 0.05)
    mode = 0
    radius = 0.008
    point_size = 1
    prim_kind = 0


def _qrot(q, v):
    uv = [q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]]
    w = [q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]]
    return [v[a] + f32(2) * (q[0] * uv[a] + w[a]) for a in range(3)]


def prim_frame(k, pos, rot):
    """(A [3,3], o [3]) of one primitive: the sim-to-local matrix and the camera in the local frame"""
    pos, q = np.asarray(pos, f32), np.asarray(rot, f32)
    c = [q[0], -q[1], -q[2], -q[3]]
    nq = np.sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3] * c[3]) + f32(1e-12)
    iq = [c[a] / nq for a in range(4)]
    one, zero = f32(1), f32(0)
    cols = [_qrot(iq, e) for e in ([one, zero, zero], [zero, one, zero], [zero, zero, one])]
    A = np.array([[cols[c_][a] for c_ in range(3)] for a in range(3)], f32)
    o = np.array(_qrot(iq, [k.P[0] - pos[0], k.P[2] - pos[1], k.P[1] - pos[2]]), f32)
    return A, o


def bowl_sdf(s, p0, p1, p2):
    r, h, t = s
    w = np.sqrt(r * r - h * h)
    q0 = np.sqrt((p0 * p0 + p2 * p2) + f32(1e-12))
    q1 = p1
    d0, d1 = q0 - w, q1 - h
    val1 = np.sqrt((d0 * d0 + d1 * d1) + f32(1e-12)) - t
    val2 = np.abs(np.sqrt((q0 * q0 + q1 * q1) + f32(1e-12)) - r) - t
    return np.where(h * q0 < w * q1, val1, val2)


def _box(s, o, dl, znear):
    tnear = np.full(dl[0].shape, -np.inf, f32)
    tfar = np.full(dl[0].shape, np.inf, f32)
    axis = np.zeros(dl[0].shape, np.int32)
    ok = np.ones(dl[0].shape, bool)
    for a in range(3):
        par = dl[a] == 0
        ok &= ~(par & ~(np.abs(o[a]) <= s[a]))
        t1, t2 = (-s[a] - o[a]) / dl[a], (s[a] - o[a]) / dl[a]
        tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
        up = ~par & (tn > tnear)
        tnear = np.where(up, tn, tnear)
        axis = np.where(up, np.int32(a), axis)
        tfar = np.where(par, tfar, np.minimum(tfar, tf))
    hit = ok & (tnear <= tfar) & (tnear >= znear)
    nl = [np.where(axis == a, np.where(dl[a] > 0, f32(-1), f32(1)), f32(0)).astype(f32) for a in range(3)]
    return hit, tnear, nl


def _bowl(s, o, dl, znear):
    r, h, t = s
    aa = (dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2]
    bq = (o[0] * dl[0] + o[1] * dl[1]) + o[2] * dl[2]
    tcb = -bq / aa
    q = [o[a] + tcb * dl[a] for a in range(3)]
    rb = r + t
    h2 = rb * rb - ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    hs = np.sqrt(h2 / aa)
    tout = tcb + hs
    tt = np.maximum(tcb - hs, znear)
    active = (h2 >= 0) & (tt <= tout)
    ln = np.sqrt(aa)
    hit = np.zeros(aa.shape, bool)
    for _ in range(MARCH_K):
        if not active.any():
            break
        v = bowl_sdf(s, o[0] + tt * dl[0], o[1] + tt * dl[1], o[2] + tt * dl[2])
        h_now = active & (v <= MARCH_EPS)
        hit |= h_now
        adv = active & ~h_now
        tn = tt + v / ln
        tt = np.where(adv, tn, tt)
        active = adv & (tn <= tout)
    p = [o[a] + tt * dl[a] for a in range(3)]
    e = NORMAL_STEP
    n = [bowl_sdf(s, p[0] + e, p[1], p[2]) - bowl_sdf(s, p[0] - e, p[1], p[2]),
         bowl_sdf(s, p[0], p[1] + e, p[2]) - bowl_sdf(s, p[0], p[1] - e, p[2]),
         bowl_sdf(s, p[0], p[1], p[2] + e) - bowl_sdf(s, p[0], p[1], p[2] - e)]
    l = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    okl = l > 0
    nl = [np.where(okl, n[0] / l, f32(0)), np.where(okl, n[1] / l, f32(0)), np.where(okl, n[2] / l, f32(1))]
    return hit, tt, nl


def render(conf, x, prim_pos=None, prim_rot=None, prim_sizes=None, chunk=64):
    with np.errstate(all="ignore"):
        return _render(conf, x, prim_pos, prim_rot, prim_sizes, chunk)


def _render(conf, x, prim_pos, prim_rot, prim_sizes, chunk):
    k = ct._K(conf)
    W, H = k.W, k.H
    mode, kind = int(conf.mode), int(conf.prim_kind)
    pc = np.asarray(conf.particle_color, f32)
    alpha = pc[3]
    oma = f32(1) - alpha
    rad = f32(conf.radius)
    half = f32(int(conf.point_size)) * f32(0.5)
    thresh = (k.znear + rad) if mode == 0 else k.znear

    x = np.asarray(x, f32).reshape(-1, 3)
    N = x.shape[0]
    xe, ye, ze = ct._eye(k, x)
    d = -ze
    sx = k.cx + (k.fx * xe) / d
    sy = k.cy - (k.fy * ye) / d
    fin = (np.abs(x[:, 0]) <= FLT_MAX) & (np.abs(x[:, 1]) <= FLT_MAX) & (np.abs(x[:, 2]) <= FLT_MAX)
    keep = fin & (d >= thresh)

    pxs = np.arange(W, dtype=np.int32).astype(f32) + f32(0.5)
    pys = np.arange(H, dtype=np.int32).astype(f32) + f32(0.5)
    rx = np.broadcast_to(((pxs - k.cx) / k.fx)[None, :], (H, W))
    ry = np.broadcast_to(((k.cy - pys) / k.fy)[:, None], (H, W))
    qa = (rx * rx + ry * ry) + f32(1)

    # ---- particles: nearest depth, then lowest index (argmin takes the first minimum; strict < between chunks)
    pdep = np.full((H, W), np.inf, f32)
    pid = np.full((H, W), -1, np.int32)
    idx = np.nonzero(keep)[0]
    for b in range(0, len(idx), chunk):
        ii = idx[b:b + chunk]
        if mode == 0:
            cx_, cy_, cz_ = xe[ii, None, None], ye[ii, None, None], (-d[ii])[:, None, None]
            tc = ((rx * cx_ + ry * cy_) - cz_) / qa
            qx, qy, qz = cx_ - tc * rx, cy_ - tc * ry, cz_ + tc
            h2 = rad * rad - ((qx * qx + qy * qy) + qz * qz)
            ts = tc - np.sqrt(h2 / qa)
            cand = np.where((h2 >= 0) & (ts >= k.znear), ts, f32(np.inf)).astype(f32)
        else:
            lox, hix = sx[ii] - half, sx[ii] + half
            loy, hiy = sy[ii] - half, sy[ii] + half
            cu = (lox[:, None] <= pxs[None, :]) & (pxs[None, :] < hix[:, None])
            cv = (loy[:, None] <= pys[None, :]) & (pys[None, :] < hiy[:, None])
            cand = np.where(cv[:, :, None] & cu[:, None, :], d[ii, None, None], f32(np.inf)).astype(f32)
        j = np.argmin(cand, axis=0)
        best_c = np.take_along_axis(cand, j[None], 0)[0]
        win = best_c < pdep
        pdep = np.where(win, best_c, pdep)
        pid = np.where(win, ii[j].astype(np.int32), pid)

    idimg = np.full((H, W), -1, np.int32)
    best = np.zeros((H, W), f32)
    if mode == 0:
        idimg = pid.copy()
        best = np.where(pid >= 0, pdep, f32(0)).astype(f32)

    # ---- primitives
    D = [(k.R[0, c] * rx + k.R[1, c] * ry) - k.R[2, c] for c in range(3)]
    Ds = [D[0], D[2], D[1]]
    n = [np.zeros((H, W), f32), np.zeros((H, W), f32), np.ones((H, W), f32)]
    sizes = np.zeros((0, 3), f32) if prim_sizes is None else np.asarray(prim_sizes, f32).reshape(-1, 3)
    for j in range(len(sizes)):
        A, o = prim_frame(k, np.asarray(prim_pos, f32).reshape(-1, 3)[j], np.asarray(prim_rot, f32).reshape(-1, 4)[j])
        dl = [(A[a, 0] * Ds[0] + A[a, 1] * Ds[1]) + A[a, 2] * Ds[2] for a in range(3)]
        hit, th, nl = (_box if kind == 0 else _bowl)(sizes[j], o, dl, k.znear)
        take = hit & ((idimg == -1) | (th < best))
        ns = [(A[0, c] * nl[0] + A[1, c] * nl[1]) + A[2, c] * nl[2] for c in range(3)]
        ne = [(k.R[r, 0] * ns[0] + k.R[r, 1] * ns[2]) + k.R[r, 2] * ns[1] for r in range(3)]
        idimg = np.where(take, np.int32(-4 - j), idimg)
        best = np.where(take, th, best).astype(f32)
        n = [np.where(take, ne[a], n[a]).astype(f32) for a in range(3)]

    # ---- ground
    tg = (k.gz - k.P[2]) / D[2]
    hx, hy = k.P[0] + tg * D[0], k.P[1] + tg * D[1]
    take = ((D[2] < 0) & (tg >= k.znear) & (hx >= k.gmin[0]) & (hx <= k.gmax[0]) & (hy >= k.gmin[1]) & (hy <= k.gmax[1])
            & ((idimg == -1) | (tg < best)))
    idimg = np.where(take, np.int32(-3), idimg)
    best = np.where(take, tg, best).astype(f32)

    # ---- shading of the nearest opaque thing
    e = [best * rx, best * ry, -best]
    pj = np.maximum(idimg, 0)
    sn = [(best * rx - xe[pj]) / rad, (best * ry - ye[pj]) / rad, (-best - (-d[pj])) / rad]
    gn = [k.R[0, 2], k.R[1, 2], k.R[2, 2]]
    n = [np.where(idimg >= 0, sn[a], np.where(idimg == -3, gn[a], n[a])).astype(f32) for a in range(3)]
    lit = ct._lit(k, n, e)
    cols = np.stack([pc[:3], np.asarray(conf.prim_color, f32), np.asarray(conf.ground_color, f32)])
    base = cols[np.where(idimg >= 0, 0, np.where(idimg == -3, 2, 1))]
    bc = np.minimum(np.maximum(base * lit[..., None], f32(0)), f32(1))
    bc = np.where((idimg == -1)[..., None], f32(1), bc).astype(f32)

    # ---- point mode: the nearest point, unlit, over what is behind it
    if mode == 1:
        take = (pid >= 0) & ((idimg == -1) | (pdep < best))
        blend = alpha * pc[:3][None, None, :] + oma * bc
        bc = np.where(take[..., None], blend, bc).astype(f32)
        idimg = np.where(take, pid, idimg)
        best = np.where(take, pdep, best).astype(f32)

    c = np.minimum(np.maximum(bc, f32(0)), f32(1)) * f32(255) + f32(0.5)
    rgb = c.astype(np.int32).astype(np.uint8)
    depth = np.where(idimg == -1, f32(0), best).astype(f32)
    return np.ascontiguousarray(rgb), depth, idimg.astype(np.int32)
