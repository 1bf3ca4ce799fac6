"""NumPy f32 restatement of the lit / roulette instances of k_render_image (csrc/plb_render.hip) -- THE SPECIFICATION of
ud_plb_render_set_light (include/unidom_hip.h): RenderTwin's image with the two branches of the reference's trace (renderer.py:374-397) in
the operation order the header states.  With both flags off it is RenderTwin.image, bit for bit (tests/test_plb_render_light_cpu.py).

Draws: the hash of plb_render_twin; bounce b takes k = 2 + 4b + 0..3 as before, k = 2^30 + 4b + 0..2 for the light noise and
k = 2^30 + 4b + 3 for the roulette.

`records` (image(..., records=[])): one list per sample, one dict per loop iteration b:
    lanes     the pixels (u * res1 + v) that ran iteration b
    hit       [lanes] the normal was non-zero (the others hit the sky)
    facing    [lanes] hit and dot > 0: a shadow ray was sent
    occluded  [lanes] facing and the shadow ray's next_hit distance <= 100
    lit       [lanes] facing and not occluded: contrib += throughput * dot
    dot       [lanes] f32 (0 where not hit)
    draw, max_c, survived   [lanes] the roulette draw, throughput.max() before it and draw <= max_c (roulette only)
    throughput              [lanes,3] after the iteration
"""
import numpy as np

from plb_render_twin import F, LIMIT, RenderTwin, cross, f32, norm, normalize, rand

LIGHT_K = 1 << 30
NOISE = F(0.03)


class LightTwin(RenderTwin):
    def __init__(self, conf, use_directional_light=None, use_roulette=None, light_direction=None):
        super().__init__(conf)
        pick = lambda given, name: getattr(conf, name) if given is None else given
        self.light = bool(pick(use_directional_light, "use_directional_light"))
        self.roulette = bool(pick(use_roulette, "use_roulette"))
        self.light_direction = f32(np.asarray(pick(light_direction, "light_direction"), np.float64))     # rounded to f32 at set_light

    def image(self, e, prims, spp=None, seed=0, nudge=0, records=None, centre=False):
        """The f32 image of one env in render_frame's orientation, [H,W,3].  centre: both pixel jitters 0.5 (the G-buffer's ray) instead of the
        draws k = 0, 1."""
        W, H = self.img
        spp = self.spp if spp is None else int(spp)
        if e.status:
            return np.zeros((H, W, 3), np.float32)
        u, v = self.pixels()
        pixel = (u * H + v).astype(np.uint32)
        acc = np.zeros((W * H, 3), np.float32)
        one = F(1.0)
        for s in range(spp):
            ju, jv = (F(0.5), F(0.5)) if centre else (rand(seed, pixel, s, 0), rand(seed, pixel, s, 1))
            d = self.camera_ray(u, v, ju, jv)
            pos = np.broadcast_to(self.cam, d.shape).copy()
            thr = np.ones((W * H, 3), np.float32)
            contrib = np.zeros((W * H, 3), np.float32)
            alive = np.ones(W * H, bool)
            rec_s = []
            for b in range(self.depth):
                ia = np.nonzero(alive)[0]
                if ia.size == 0:
                    break
                rec = dict(lanes=ia, hit=np.zeros(ia.size, bool), facing=np.zeros(ia.size, bool), occluded=np.zeros(ia.size, bool),
                           lit=np.zeros(ia.size, bool), dot=np.zeros(ia.size, np.float32))
                h = self.next_hit(e, prims, pos[ia], d[ia])
                hp = pos[ia] + h["t"][:, None] * d[ia]
                with np.errstate(all="ignore"):
                    cont = norm(h["n"]) != 0
                alive[ia[~cont]] = False
                rec["hit"] = cont
                if cont.any():
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
                    if self.light:                                           # renderer.py:374-386
                        kl = LIGHT_K + 4 * b
                        noise = np.stack([(rand(seed, px, s, kl + j) - F(0.5)) * NOISE for j in range(3)], axis=-1)
                        direct = normalize(self.light_direction[None] + noise)
                        dot = (direct[:, 0] * nn[:, 0] + direct[:, 1] * nn[:, 1]) + direct[:, 2] * nn[:, 2]
                        facing = dot > 0
                        occ = np.zeros(g.size, bool)
                        if facing.any():
                            sh = self.next_hit(e, prims, pos[g][facing], direct[facing])
                            occ[facing] = ~(sh["t"] > LIMIT)
                        lit = facing & ~occ
                        contrib[g[lit]] = contrib[g[lit]] + (thr[g[lit]] * one) * dot[lit, None]
                        ci = np.nonzero(cont)[0]
                        rec["facing"][ci] = facing; rec["occluded"][ci] = occ; rec["lit"][ci] = lit; rec["dot"][ci] = dot
                if self.roulette:                                            # :391-397, for every lane of this iteration, the sky's included
                    draw = rand(seed, pixel[ia], s, LIGHT_K + 4 * b + 3)
                    max_c = np.maximum(np.maximum(thr[ia, 0], thr[ia, 1]), thr[ia, 2])
                    stop = draw > max_c
                    with np.errstate(all="ignore"):
                        thr[ia] = np.where(stop[:, None], F(0.0), thr[ia] / max_c[:, None])        # 0 / 0 (max_c == 0, draw == 0) as written
                    alive[ia[stop]] = False
                    rec.update(draw=draw, max_c=max_c, survived=~stop)
                rec["throughput"] = thr[ia].copy()
                rec_s.append(rec)
            if records is not None:
                records.append(rec_s)
            if self.light:                                                   # :408-410: the sample is contrib, the sky term is not added
                acc = acc + contrib
            else:
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
