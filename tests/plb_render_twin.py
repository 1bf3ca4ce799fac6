"""NumPy f32 restatement of csrc/plb_render.hip -- THE SPECIFICATION of the PLB renderer (include/unidom_hip.h, ud_plb_render_*): the bake,
next_hit, the G-buffer and the image in the operation order the header states, vectorised over pixels.  Written from the text of the
reference's renderer.py / renderer_utils.py; this project's own code.  Every array is float32 and every constant an np.float32, so each
operation rounds once, as the kernels' do (built without FMA contraction, with correctly rounded divide and sqrt).  Primitive distances
and normals are f64 (the shape layer of csrc/plb_prim.h restated below), cast to f32.

`nudge`: cos / sin results moved by that many ulps (np.nextafter) -- the only operations of the image that are not pinned; the CPU test
measures what such a nudge can change."""
import numpy as np

F = np.float32
INF = F(1e10)
LIMIT = F(100.0)
MAX_PRIM = 4


def f32(a):
    return np.asarray(a, dtype=np.float32)


# ---------------------------------------------------------------- the hash
def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def rand(seed, pixel, sample, k):
    """r(pixel, sample, k) of the header; pixel: uint32 array."""
    c = np.uint32((sample * 0x85EBCA6B + k * 0xC2B2AE35) & 0xFFFFFFFF)
    h = lowbias32(np.uint32(seed & 0xFFFFFFFF) ^ (np.asarray(pixel, dtype=np.uint32) * np.uint32(0x9E3779B9) + c))
    return (h >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24)


# ---------------------------------------------------------------- small vector helpers, [.., 3] float32
def norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def normalize(v):
    with np.errstate(all="ignore"):
        il = F(1.0) / norm(v)
        return il[..., None] * v


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


# ---------------------------------------------------------------- f64 shape layer (csrc/plb_prim.h), [M,3] float64
def qrot(q, v):
    qv = np.broadcast_to(np.asarray(q[1:], np.float64), v.shape)
    uv = np.cross(qv, v)
    uuv = np.cross(qv, uv)
    return v + 2 * (q[0] * uv + uuv)


def qinv(q):
    q = np.asarray(q, np.float64)
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([q[0] / n, -q[1] / n, -q[2] / n, -q[3] / n])


def _len(*c):
    s = c[0] * c[0]
    for a in c[1:]:
        s = s + a * a
    return np.sqrt(s + 1e-14)


def _box_sdf(sz, y):
    q = np.abs(y) - np.asarray(sz, np.float64)
    m = np.maximum(q, 0.0)
    return _len(m[:, 0], m[:, 1], m[:, 2]) + np.minimum(np.maximum(q[:, 0], np.maximum(q[:, 1], q[:, 2])), 0.0)


def _chop(gap, ch, pl):
    py = (pl[:, 1] + ch / 2) + ch / 2
    p1 = py - np.minimum(np.maximum(py, 0.0), ch)
    xa, xb = pl[:, 0] - gap / 2, pl[:, 0] + gap / 2
    rest = p1 * p1 + pl[:, 2] * pl[:, 2] + 1e-14
    la, lb = np.sqrt(xa * xa + rest), np.sqrt(xb * xb + rest)
    a = la <= lb
    return np.where(a, la, lb), np.stack([np.where(a, xa, xb), p1, pl[:, 2]], axis=-1)


def shape_sdf(kind, sc, ch, radius, pl):
    if kind == 6:
        return _chop(sc[0], ch, pl)[0] - radius
    if kind == 3:
        return _box_sdf(sc, pl)
    if kind == 4:
        l = _len(pl[:, 0], pl[:, 2])
        d0, d1 = l - sc[0], np.abs(pl[:, 1]) - sc[1]
        m0, m1 = np.maximum(d0, 0.0), np.maximum(d1, 0.0)
        return np.minimum(np.maximum(d0, d1), 0.0) + np.sqrt(m0 * m0 + m1 * m1 + 1e-14)
    if kind == 5:
        q0 = _len(pl[:, 0], pl[:, 2]) - sc[0]
        return np.sqrt(q0 * q0 + pl[:, 1] * pl[:, 1] + 1e-14) - sc[1]
    py = pl[:, 1] + ch / 2
    p1 = py - np.minimum(np.maximum(py, 0.0), ch)
    return np.sqrt(pl[:, 0] * pl[:, 0] + p1 * p1 + pl[:, 2] * pl[:, 2] + 1e-14) - radius


def _normalize64(n):
    il = 1.0 / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2] + 1e-14)
    return n * il[:, None]


def shape_normal(kind, sc, ch, pl):
    if kind == 6:
        l, p = _chop(sc[0], ch, pl)
        return p * (1.0 / l)[:, None]
    if kind == 3:
        n = np.zeros_like(pl)
        for i in range(3):
            inc, dec = pl.copy(), pl.copy()
            inc[:, i] += 1e-4; dec[:, i] -= 1e-4
            n[:, i] = (0.5 / 1e-4) * (_box_sdf(sc, inc) - _box_sdf(sc, dec))
        return _normalize64(n)
    if kind == 4:
        l = _len(pl[:, 0], pl[:, 2])
        d0, d1 = l - sc[0], np.abs(pl[:, 1]) - sc[1]
        f = np.where(d0 > d1, 1.0, 0.0); ins = np.where(np.maximum(d0, d1) <= 0.0, 1.0, 0.0)
        n20, n21 = np.maximum(d0, 0.0) + ins * f, np.maximum(d1, 0.0) + ins * (1 - f)
        l2 = np.sqrt(n20 * n20 + n21 * n21 + 1e-14)
        sy = np.where(pl[:, 1] >= 0.0, 1.0, -1.0)
        return _normalize64(np.stack([pl[:, 0] / l * (n20 / l2), n21 / l2 * sy, pl[:, 2] / l * (n20 / l2)], axis=-1))
    if kind == 5:
        l = _len(pl[:, 0], pl[:, 2])
        q0, q1 = l - sc[0], pl[:, 1]
        lq = np.sqrt(q0 * q0 + q1 * q1 + 1e-14)
        return _normalize64(np.stack([pl[:, 0] / l * (q0 / lq), q1 / lq, pl[:, 2] / l * (q0 / lq)], axis=-1))
    py = pl[:, 1] + ch / 2
    p1 = py - np.minimum(np.maximum(py, 0.0), ch)
    il = 1.0 / np.sqrt(pl[:, 0] * pl[:, 0] + p1 * p1 + pl[:, 2] * pl[:, 2] + 1e-14)
    return np.stack([pl[:, 0] * il, p1 * il, pl[:, 2] * il], axis=-1)


class Prim:
    """One primitive of one env: kind 0..6, constants, f64 state."""
    def __init__(self, kind, radius=0.0, h=0.0, shape=(0.0, 0.0, 0.0), color=(0.3, 0.3, 0.3), pos=(0.0, 0.0, 0.0), rot=(1.0, 0.0, 0.0, 0.0), gap=0.0):
        self.kind, self.radius, self.h, self.shape, self.color = int(kind), float(radius), float(h), tuple(map(float, shape)), f32(color)
        self.pos, self.rot, self.gap = np.asarray(pos, np.float64), np.asarray(rot, np.float64), float(gap)
        self.qi = qinv(self.rot)

    def _local(self, pp):
        return qrot(self.qi, pp.astype(np.float64) - self.pos)

    def sdf(self, pp):
        return shape_sdf(self.kind, (self.gap,) if self.kind == 6 else self.shape, self.h, self.radius, self._local(pp)).astype(np.float32)

    def normal(self, pp):
        nl = shape_normal(self.kind, (self.gap,) if self.kind == 6 else self.shape, self.h, self._local(pp))
        return qrot(self.rot, nl).astype(np.float32)


# ---------------------------------------------------------------- the renderer
class Env:
    """One env's baked state."""
    def __init__(self, bbox, status, vol, sdf):
        self.bbox, self.status, self.vol, self.sdf = bbox, int(status), vol, sdf


class RenderTwin:
    def __init__(self, conf):
        """conf: a RenderConf (unidom_amd.engine.plb_render) or anything with its fields."""
        self.res = tuple(int(r) for r in conf.voxel_res)
        self.bake_size = int(conf.bake_size)
        self.img = tuple(int(r) for r in conf.image_res)
        self.depth, self.spp = int(conf.max_ray_depth), int(conf.spp)
        self.dx, self.inv_dx, self.thr = F(conf.dx), F(1.0 / conf.dx), F(conf.sdf_threshold)
        self.cam = f32(conf.camera_pos)
        self.fov_aspect = F(0.23 * (self.img[0] / self.img[1]))
        r0, r1 = float(conf.camera_rot[0]), float(conf.camera_rot[1])
        c0, s0, c1, s1 = np.cos(r0), np.sin(r0), np.cos(r1), np.sin(r1)
        A = [[c1, 0.0, s1], [0.0, 1.0, 0.0], [-s1, 0.0, c1]]
        Bm = [[1.0, 0.0, 0.0], [0.0, c0, s0], [0.0, -s0, c0]]
        self.mat = f32([[(A[r][0] * Bm[0][q] + A[r][1] * Bm[1][q]) + A[r][2] * Bm[2][q] for q in range(3)] for r in range(3)])

    # ---- bake
    def bake_one(self, x, color):
        res, dx, inv_dx = self.res, self.dx, self.inv_dx
        px = np.asarray(x, np.float64).astype(np.float32)
        v = (np.floor(px * inv_dx) - F(6.0)) * dx
        b0, hi = v.min(0), v.max(0)
        status = int(np.any((hi - b0) / dx >= f32(res)))
        b1 = (b0.astype(np.float64) + np.asarray(res, np.float64) * np.float64(dx)).astype(np.float32)
        vol = np.full(res, 2 ** 32 - 1, dtype=np.int64)
        if not status:
            s = self.bake_size
            o = np.arange(-s - 1, s + 1, dtype=np.int32)
            off = np.stack(np.meshgrid(o, o, o, indexing="ij"), axis=-1).reshape(-1, 3)
            p = (px - b0) * inv_dx
            idx = p.astype(np.int32)[:, None, :] + off[None]
            d = idx.astype(np.float32) - p[:, None, :]
            dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            q = np.minimum(np.maximum(F(0.0), F(51.0) * dist), F(255.0))
            val = (q.astype(np.int64) << 24) + np.asarray(color, np.int64)[:, None]
            ok = np.all((idx >= 0) & (idx < np.asarray(res, np.int32)), axis=-1)
            flat = (idx[..., 0].astype(np.int64) * res[1] + idx[..., 1]) * res[2] + idx[..., 2]
            np.minimum.at(vol.reshape(-1), flat[ok], val[ok])
        sdf = (((vol >> 24) & 255).astype(np.float32)) / F(255.0)
        sdf = self.smooth(self.smooth(sdf))
        return Env(np.stack([b0, b1]), status, vol, sdf)

    @staticmethod
    def smooth(v):
        out = np.ones_like(v)
        a, b, c = v.shape
        s = np.zeros((a - 2, b - 2, c - 2), dtype=np.float32)
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    s = s + v[i:a - 2 + i, j:b - 2 + j, k:c - 2 + k]
        out[1:-1, 1:-1, 1:-1] = s / F(27.0)
        return out

    @staticmethod
    def decode_color(vol):
        """[..., 3] float32: channel j = ((c >> 8 (2 - j)) & 255) / 255."""
        return np.stack([((vol >> (8 * (2 - j))) & 255).astype(np.float32) / F(255.0) for j in range(3)], axis=-1)

    def bake(self, x, color):
        return [self.bake_one(xb, color) for xb in x]

    # ---- sampling
    def _tex(self, e, pos):
        with np.errstate(all="ignore"):
            q = (pos - e.bbox[0]) / (e.bbox[1] - e.bbox[0])
            ok = np.all((q >= 0) & (q <= 1), axis=-1)
        q = np.where(ok[:, None], q, F(0.0))
        res = np.asarray(self.res, np.int32)
        p = q * f32(self.res)
        b = np.minimum(p.astype(np.int32), res - 1)
        f = p - b.astype(np.float32)
        b1 = np.minimum(b + 1, res - 1)
        lin = lambda x, y, z: (x.astype(np.int64) * self.res[1] + y) * self.res[2] + z
        x, y, z, x1, y1, z1 = b[:, 0], b[:, 1], b[:, 2], b1[:, 0], b1[:, 1], b1[:, 2]
        idx = [lin(x, y, z), lin(x1, y, z), lin(x, y, z1), lin(x1, y, z1), lin(x, y1, z), lin(x1, y1, z), lin(x, y1, z1), lin(x1, y1, z1)]
        return ok, idx, f

    @staticmethod
    def _mix(v, f):
        one = F(1.0)
        c00 = v[0] * (one - f[:, 0]) + v[1] * f[:, 0]
        c01 = v[2] * (one - f[:, 0]) + v[3] * f[:, 0]
        c10 = v[4] * (one - f[:, 0]) + v[5] * f[:, 0]
        c11 = v[6] * (one - f[:, 0]) + v[7] * f[:, 0]
        c0 = c00 * (one - f[:, 1]) + c10 * f[:, 1]
        c1 = c01 * (one - f[:, 1]) + c11 * f[:, 1]
        return c0 * (one - f[:, 2]) + c1 * f[:, 2]

    def sample_sdf(self, e, pos):
        ok, idx, f = self._tex(e, pos)
        flat = e.sdf.reshape(-1)
        return np.where(ok, self._mix([flat[i] for i in idx], f) - self.thr, F(0.0))

    def sample_color(self, e, pos):
        ok, idx, f = self._tex(e, pos)
        flat = e.vol.reshape(-1)
        out = np.zeros((pos.shape[0], 3), dtype=np.float32)
        for ch in range(3):
            v = [((flat[i] >> (8 * (2 - ch))) & 255).astype(np.float32) / F(255.0) for i in idx]
            out[:, ch] = np.where(ok, self._mix(v, f), F(0.0))
        return out

    def sample_normal(self, e, p):
        d = F(1e-3)
        n = np.zeros_like(p)
        for i in range(3):
            inc, dec = p.copy(), p.copy()
            inc[:, i] = inc[:, i] + d; dec[:, i] = dec[:, i] - d
            n[:, i] = F(500.0) * (self.sample_sdf(e, inc) - self.sample_sdf(e, dec))
        return normalize(n)

    # ---- next_hit
    def next_hit(self, e, prims, o, d):
        """o, d: [P,3] f32.  Returns dict(t, n, c, rough, kind, exhausted): exhausted = the primitive trace ran out its 200 steps."""
        P = d.shape[0]
        o = np.broadcast_to(f32(o), d.shape)
        t = np.full(P, INF, dtype=np.float32); rough = np.full(P, F(0.05), dtype=np.float32); kind = np.zeros(P, np.int32)
        n = np.zeros((P, 3), np.float32); c = np.zeros((P, 3), np.float32)
        with np.errstate(all="ignore"):
            rc = -(o[:, 2] + F(5.5)) / d[:, 2]
            m = (d[:, 2] != 0) & (rc > 0) & (rc < t)
            t[m] = rc[m]; n[m] = f32([0, 0, 1]); c[m] = f32([0.6, 0.7, 0.7]); rough[m] = 0; kind[m] = 1
            gd = (o[:, 1] + F(0.002)) / (-d[:, 1])
            m = (d[:, 1] < 0) & (gd < LIMIT) & (gd < t)
            p0, p2 = o[:, 0] + d[:, 0] * gd, o[:, 2] + d[:, 2] * gd
            ins = (p0 <= 1) & (p0 >= 0) & (p2 <= 1) & (p2 >= 0)
            chk = (((np.where(ins, p0, 0) / F(0.25)).astype(np.int32) + (np.where(ins, p2, 0) / F(0.25)).astype(np.int32)) % 2).astype(np.float32) * F(0.2) + F(0.35)
            f = np.where(ins, chk, F(0.4)).astype(np.float32)
        t[m] = gd[m]; n[m] = f32([0, 1, 0]); rough[m] = 0; kind[m] = 2
        c[m] = (f32([0.3, 0.5, 0.7])[None] * f[:, None])[m]
        exhausted = np.zeros(P, bool)
        if prims:
            dist = np.zeros(P, np.float32); sv = np.full(P, INF, dtype=np.float32); sid = np.zeros(P, np.int32); steps = np.zeros(P, np.int32)
            for _ in range(200):
                act = (dist < LIMIT) & (sv > F(1e-8))
                if not act.any():
                    break
                pp = o[act] + dist[act, None] * d[act]
                nsv = np.full(pp.shape[0], INF, dtype=np.float32); nid = sid[act].copy()
                for i, pr in enumerate(prims):
                    dd = pr.sdf(pp)
                    mm = dd < nsv
                    nsv = np.where(mm, dd, nsv); nid = np.where(mm, i, nid)
                sv[act] = nsv; sid[act] = nid; dist[act] = dist[act] + nsv; steps[act] += 1
            exhausted = (steps == 200) & (dist < LIMIT) & (sv > F(1e-8))
            m = (dist < t) & (dist < LIMIT)
            if m.any():
                pp = o[m] + dist[m, None] * d[m]
                nn = np.zeros((pp.shape[0], 3), np.float32); cc = np.zeros((pp.shape[0], 3), np.float32)
                for i, pr in enumerate(prims):
                    mi = sid[m] == i
                    if mi.any():
                        nn[mi] = pr.normal(pp[mi]); cc[mi] = pr.color
                t[m] = dist[m]; n[m] = nn; c[m] = cc; rough[m] = 0; kind[m] = 3 + sid[m]
        # the body
        hit = np.ones(P, bool)
        tn = np.full(P, -INF, dtype=np.float32); tf = np.full(P, INF, dtype=np.float32)
        with np.errstate(all="ignore"):
            for i in range(3):
                z = d[:, i] == 0
                hit &= ~(z & ((o[:, i] < e.bbox[0, i]) | (o[:, i] > e.bbox[1, i])))
                i1, i2 = (e.bbox[0, i] - o[:, i]) / d[:, i], (e.bbox[1, i] - o[:, i]) / d[:, i]
                tf = np.where(z, tf, np.minimum(np.maximum(i1, i2), tf))
                tn = np.where(z, tn, np.maximum(np.minimum(i1, i2), tn))
        hit &= ~(tn > tf)
        ids = np.nonzero(hit)[0]
        if ids.size:
            oo, dd = o[ids], d[ids]
            t0 = np.maximum(tn[ids], F(0.0)) + F(1e-4)
            pos = oo + dd * t0[:, None]
            step = np.zeros_like(pos)
            live = np.ones(ids.size, bool)
            for _ in range(500):
                la = np.nonzero(live)[0]
                if la.size == 0:
                    break
                s = self.sample_sdf(e, pos[la])
                neg = s < 0
                if neg.any():
                    g = la[neg]
                    pg, bs = pos[g].copy(), step[g].copy()
                    for _l in range(20):
                        bs = bs * F(0.5)
                        q = pg - bs
                        mv = self.sample_sdf(e, q) < 0
                        pg = np.where(mv[:, None], q, pg)
                    dist = norm(oo[g] - pg)
                    gi = ids[g]
                    tk = dist < t[gi]
                    if tk.any():
                        w = gi[tk]
                        t[w] = dist[tk]; kind[w] = 16
                        n[w] = self.sample_normal(e, pg[tk]); c[w] = self.sample_color(e, pg[tk])
                    live[g] = False
                fw = la[~neg]
                mstep = np.maximum(s[~neg] * F(0.05), F(0.01))
                step[fw] = d[ids[fw]] * mstep[:, None]
                pos[fw] = pos[fw] + step[fw]
        return dict(t=t, n=n, c=c, rough=rough, kind=kind, exhausted=exhausted)

    # ---- camera, G-buffer, image
    def pixels(self):
        u, v = np.meshgrid(np.arange(self.img[0]), np.arange(self.img[1]), indexing="ij")
        return u.reshape(-1), v.reshape(-1)

    def camera_ray(self, u, v, ju, jv):
        r1 = F(self.img[1])
        c = np.stack([((F(0.46) * (u.astype(np.float32) + ju)) / r1 - self.fov_aspect) - F(1e-5),
                      ((F(0.46) * (v.astype(np.float32) + jv)) / r1 - F(0.23)) - F(1e-5), np.full(u.shape, F(-1.0), dtype=np.float32)], axis=-1)
        c = normalize(c)
        m = self.mat
        return np.stack([(m[r, 0] * c[:, 0] + m[r, 1] * c[:, 1]) + m[r, 2] * c[:, 2] for r in range(3)], axis=-1)

    def gbuffer(self, e, prims):
        """dict(kind [W,H], t, normal [W,H,3], albedo, exhausted) of one env."""
        W, H = self.img
        if e.status:
            return dict(kind=np.zeros((W, H), np.int32), t=np.zeros((W, H), np.float32), normal=np.zeros((W, H, 3), np.float32),
                        albedo=np.zeros((W, H, 3), np.float32), exhausted=np.zeros((W, H), bool))
        u, v = self.pixels()
        h = self.next_hit(e, prims, self.cam, self.camera_ray(u, v, F(0.5), F(0.5)))
        return dict(kind=h["kind"].reshape(W, H), t=h["t"].reshape(W, H), normal=h["n"].reshape(W, H, 3), albedo=h["c"].reshape(W, H, 3),
                    exhausted=h["exhausted"].reshape(W, H))

    @staticmethod
    def _trig(fn, a, nudge):
        r = fn(a).astype(np.float32)
        for _ in range(abs(nudge)):
            r = np.nextafter(r, F(np.inf) if nudge > 0 else F(-np.inf))
        return r

    def image(self, e, prims, spp=None, seed=0, nudge=0):
        """The f32 image of one env in render_frame's orientation, [H,W,3]."""
        W, H = self.img
        spp = self.spp if spp is None else int(spp)
        if e.status:
            return np.zeros((H, W, 3), np.float32)
        u, v = self.pixels()
        pixel = (u * H + v).astype(np.uint32)
        acc = np.zeros((W * H, 3), np.float32)
        one = F(1.0)
        for s in range(spp):
            d = self.camera_ray(u, v, rand(seed, pixel, s, 0), rand(seed, pixel, s, 1))
            pos = np.broadcast_to(self.cam, d.shape).copy()
            thr = np.ones((W * H, 3), np.float32)
            alive = np.ones(W * H, bool)
            for b in range(self.depth):
                ia = np.nonzero(alive)[0]
                if ia.size == 0:
                    break
                h = self.next_hit(e, prims, pos[ia], d[ia])
                hp = pos[ia] + h["t"][:, None] * d[ia]
                with np.errstate(all="ignore"):
                    cont = norm(h["n"]) != 0
                alive[ia[~cont]] = False
                if not cont.any():
                    continue
                g = ia[cont]
                nn, rough, px = h["n"][cont], h["rough"][cont], pixel[g]
                kk = 2 + 4 * b
                a = np.broadcast_to(f32([1, 0, 0]), nn.shape).copy()
                mm = np.abs(nn[:, 1]) < F(0.999)
                a[mm] = normalize(cross(nn[mm], np.broadcast_to(f32([0, 1, 0]), nn[mm].shape)))
                w = cross(nn, a)
                phi = F(6.2831855) * rand(seed, px, s, kk)
                r = rand(seed, px, s, kk + 1)
                ay, ax = np.sqrt(r), np.sqrt(one - r)
                cp, sp = self._trig(np.cos, phi, nudge), self._trig(np.sin, phi, nudge)
                su, sv = rand(seed, px, s, kk + 2), rand(seed, px, s, kk + 3)
                sx = su * F(2.0) - one
                sphi = (sv * F(2.0)) * F(3.1415927)
                yz = np.sqrt(one - sx * sx)
                gl = np.stack([sx * rough, (yz * self._trig(np.cos, sphi, nudge)) * rough, (yz * self._trig(np.sin, sphi, nudge)) * rough], axis=-1)
                nd = (ax[:, None] * (cp[:, None] * a + sp[:, None] * w) + ay[:, None] * nn) + gl
                nd = normalize(nd)
                d[g] = nd
                pos[g] = hp[cont] + F(1e-4) * nd
                thr[g] = thr[g] * h["c"][cont]
            c1 = ((d[:, 0] * F(0.8) + d[:, 1] * F(0.65)) + d[:, 2] * F(0.15)) * F(0.5) + F(0.5)
            c1 = np.maximum(np.minimum(c1, one), F(0.0))
            rg = (c1 * F(0.9) + (one - c1) * F(0.7)) * F(1.5)
            bl = (c1 * F(0.9) + (one - c1) * F(0.8)) * F(1.5)
            acc = acc + thr * np.stack([rg, rg, bl], axis=-1)
        fu, fv = u.astype(np.float32) / F(W), v.astype(np.float32) / F(H)
        du, dv = fu - F(0.5), fv - F(0.5)
        darken = one - F(0.9) * np.maximum(np.sqrt(du * du + dv * dv) - F(0.0), F(0.0))
        with np.errstate(all="ignore"):
            img = np.sqrt(((acc * darken[:, None]) * F(1.5)) / F(spp)).reshape(W, H, 3)
        return np.ascontiguousarray(img[:, ::-1].transpose(1, 0, 2))

    @staticmethod
    def to_u8(img):
        return np.uint8(img.clip(0, 1) * 255)


def prims_of(sim_conf, prim_pos, prim_rot=None, prim_gap=None):
    """The Prim list of one env from a PlbConf-like conf and that env's state rows."""
    P = len(sim_conf.prim_radius)
    get = lambda name, i, fill: (list(getattr(sim_conf, name, ())) + [fill] * MAX_PRIM)[i]
    return [Prim(get("prim_kind", i, 0), sim_conf.prim_radius[i], get("prim_h", i, 0.0), get("prim_shape", i, (0.0, 0.0, 0.0)),
                 get("prim_color", i, (0.3, 0.3, 0.3)), prim_pos[i], (1.0, 0.0, 0.0, 0.0) if prim_rot is None else prim_rot[i],
                 0.0 if prim_gap is None else prim_gap[i]) for i in range(P)]
