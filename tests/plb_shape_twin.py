"""Test infrastructure: torch f64 twin of the PLB step with the Box, Cylinder and Torus primitives, the reference of
tests/test_plb_shape_*.py.  On top of tests/plb_prim_twin.py (the base class's contact, constant orientation) and tests/plb_rot_twin.py
(orientation as per-env state) it restates the geometry of GenORM/policy/pbm/plb/engine/primitive/primitives.py: length and normalize
(:8-14), Cylinder._sdf / _normal (:182-202), Torus._sdf / _normal (:217-231), Box._sdf and its finite-difference _normal (:250-269); the
Capsule (:61-73) stays the parents'.  Only the geometry is overridden: the local point, the signed distance, the normal, and the two lines
of `collide` that form `dist` and `D`.  `torch.autograd` is the adjoint, the Box's central difference included: indicators, signs and the
arm abs / min / max took are constants of it, sub-gradients at ties are torch's (the cases stay away from ties: honesty_shape).
Kinds: 0 sticky Sphere, 1 Capsule, 2 RollingPin, 3 Box (shape = size), 4 Cylinder (shape = (h, r): h radial, r axial), 5 Torus (tx, ty).
PARITY UNPINNED: taichi is absent, the reference ships no recording of this path -- this restatement is the specification."""
from __future__ import annotations

import torch

from oracle.twin.plb_twin_torch import DT
from tests.plb_prim_twin import PlbPrimTwin, honesty
from tests.plb_rot_twin import PlbRotTwin, qinv, qrot

BOX, CYLINDER, TORUS = 3, 4, 5
FD = 1e-4                                                             # Box._normal's d (:261)


def length(x):
    """primitives.py:8-10."""
    return torch.sqrt((x * x).sum(-1) + 1e-14)


def normalize(n):
    """primitives.py:12-14."""
    return n / length(n)[..., None]


def box_sdf(size, pl):
    """:251-256.  q = |p| - size; length(max(q, 0)) + min(max(q0, max(q1, q2)), 0)."""
    q = pl.abs() - size
    return length(torch.clamp(q, min=0.0)) + torch.clamp(q.max(-1).values, max=0.0)


def box_normal(size, pl):
    """:259-269: central differences of _sdf with d = 1e-4, then n / length(n)."""
    n = []
    for i in range(3):
        e = torch.zeros(3, dtype=DT)
        e[i] = FD
        n.append((0.5 / FD) * (box_sdf(size, pl + e) - box_sdf(size, pl - e)))
    n = torch.stack(n, -1)
    return n / length(n)[..., None]


def cylinder_d(hr, pl):
    """The d of :185 and :192 (the same numbers: length(.) > 0, so its abs is itself)."""
    l = length(torch.stack([pl[..., 0], pl[..., 2]], -1))
    return l, torch.stack([l, pl[..., 1].abs()], -1) - hr


def cylinder_sdf(hr, pl):
    """:185-186."""
    _, d = cylinder_d(hr, pl)
    return torch.clamp(d.max(-1).values, max=0.0) + length(torch.clamp(d, min=0.0))


def cylinder_normal(hr, pl):
    """:190-202."""
    l, d = cylinder_d(hr, pl)
    f = (d[..., 0] > d[..., 1]).to(DT)
    inside = (d.max(-1).values <= 0.0).to(DT)
    n2 = torch.clamp(d, min=0.0) + inside[..., None] * torch.stack([f, 1 - f], -1)
    n2_ = n2 / length(n2)[..., None]
    p2 = torch.stack([pl[..., 0], pl[..., 2]], -1) / l[..., None]
    sign = (pl[..., 1] >= 0).to(DT) * 2 - 1
    n3 = torch.stack([p2[..., 0] * n2_[..., 0], n2_[..., 1] * sign, p2[..., 1] * n2_[..., 0]], -1)
    return normalize(n3)


def torus_q(txy, pl):
    l = length(torch.stack([pl[..., 0], pl[..., 2]], -1))
    return l, torch.stack([l - txy[0], pl[..., 1]], -1)


def torus_sdf(txy, pl):
    """:218-220."""
    return length(torus_q(txy, pl)[1]) - txy[1]


def torus_normal(txy, pl):
    """:223-231."""
    l, q = torus_q(txy, pl)
    n2 = q / length(q)[..., None]
    x2 = torch.stack([pl[..., 0], pl[..., 2]], -1) / l[..., None]
    n3 = torch.stack([x2[..., 0] * n2[..., 0], n2[..., 1], x2[..., 1] * n2[..., 0]], -1)
    return normalize(n3)


class PlbShapeTwin(PlbRotTwin):
    """rot_state False: PlbPrimTwin's step and loss (constant orientation `rot`, three action dimensions); True: PlbRotTwin's."""

    def __init__(self, conf, kinds=(BOX,), shape=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), h=(0.0, 0.0), rot=None, mu=(0.0, 0.0),
                 action_scale=(1.0, 1.0, 1.0), action_scale_w=(1.0, 1.0, 1.0), action_dim=3, substeps=None, rot_state=False):
        P = len(kinds)
        rot = ((1, 0, 0, 0),) * P if rot is None else rot
        contact = tuple(0 if k == 0 else 1 for k in kinds)             # every kind but the Sphere goes through Primitive.collide
        # the parents assert their own kinds: constructed with the mapped ones, the real ones kept beside them
        PlbPrimTwin.__init__(self, conf, kinds=contact, h=h, rot=rot, mu=mu, action_scale=action_scale, substeps=substeps)
        assert all(k in (0, 1, 2, BOX, CYLINDER, TORUS) for k in kinds) and action_dim in (3, 6)
        if rot_state:
            assert kinds[0] != 0 and all(k == 0 for k in kinds[1:]) and not (kinds[0] == 2 and action_dim == 6)
        else:
            assert 2 not in kinds and action_dim == 3
        self.kin, self.action_dim, self.rot_state = tuple(kinds), action_dim, bool(rot_state)
        self.action_scale_w = torch.tensor(action_scale_w, dtype=DT)
        self.shape = [torch.tensor((tuple(s) + (0.0,) * 3)[:3], dtype=DT) for s in (tuple(shape) + ((0.0,) * 3,) * 2)[:max(P, 1)]]
        self._q0 = self._q1 = None

    # ---- geometry of the local point -----------------------------------------------------------------------------------------------
    def _sdf(self, pi, pl):
        k, sc = self.kin[pi], self.shape[pi]
        if k == BOX:
            return box_sdf(sc, pl)
        if k == CYLINDER:
            return cylinder_sdf(sc[:2], pl)
        if k == TORUS:
            return torus_sdf(sc[:2], pl)
        py = pl[..., 1] + self.h[pi] / 2                               # Capsule, as PlbPrimTwin.local
        py = py - torch.clamp(py, 0.0, self.h[pi])
        p = torch.stack([pl[..., 0], py, pl[..., 2]], -1)
        return torch.sqrt((p * p).sum(-1) + 1e-14) - self.c.radius[pi]

    def _normal(self, pi, pl):
        k, sc = self.kin[pi], self.shape[pi]
        if k == BOX:
            return box_normal(sc, pl)
        if k == CYLINDER:
            return cylinder_normal(sc[:2], pl)
        if k == TORUS:
            return torus_normal(sc[:2], pl)
        py = pl[..., 1] + self.h[pi] / 2
        py = py - torch.clamp(py, 0.0, self.h[pi])
        p = torch.stack([pl[..., 0], py, pl[..., 2]], -1)
        return p / torch.sqrt((p * p).sum(-1) + 1e-14)[..., None]

    def local_pl(self, d, qi):
        """d [B,...,3] = point - position, qi [B,4] or [4] -> the point in the primitive's frame."""
        if qi.dim() == 1:
            qi = qi[None].expand(d.shape[0], 4)
        return qrot(qi.reshape((qi.shape[0],) + (1,) * (d.dim() - 2) + (4,)), d)

    def sdf(self, pi, pts, pos):
        return self._sdf(pi, self.local_pl(pts - pos, self.qi[pi]))

    def sdf_q(self, pi, pts, pos, q):
        return self._sdf(pi, self.local_pl(pts - pos, qinv(q)))

    def normal(self, pi, pts, pos):
        return qrot(self.q[pi], self._normal(pi, self.local_pl(pts - pos, self.qi[pi])))

    def collide(self, pi, gp, u, pos_f, pos_f1, soft, occ=None, q_f=None, q_f1=None):
        """PlbRotTwin.collide with `dist` and `D` from the kind's own _sdf / _normal; without rot_state q_f = q_f1 = the constant orientation."""
        B = pos_f.shape[0]
        if self.rot_state:
            q_f = self._q0[:, pi] if q_f is None else q_f
            q_f1 = self._q1[:, pi] if q_f1 is None else q_f1
            qi_f = qinv(q_f)
        else:
            q_f = q_f1 = self.q[pi][None].expand(B, 4)
            qi_f = self.qi[pi][None].expand(B, 4)
        dt = self.c.dt
        g = gp if gp.dim() == 3 else gp[None]
        P0, P1, sf = pos_f[:, None, :], pos_f1[:, None, :], soft[:, None]
        pl = self.local_pl(g - P0, qi_f)
        dist = self._sdf(pi, pl)
        D = qrot(q_f[:, None, :], self._normal(pi, pl))
        infl = torch.clamp(torch.exp(-dist * sf), max=1.0)
        active = ((sf > 0) & (infl > 0.1)) | (dist <= 0)
        cv = (qrot(q_f1[:, None, :], pl) + P1 - g) / dt
        w = u - cv
        nc = (w * D).sum(-1)
        t = w - torch.clamp(nc, max=0.0)[..., None] * D
        tt = (t * t).sum(-1)
        tn = torch.sqrt(tt + 1e-8)
        tf = t / tn[..., None] * torch.clamp(tn + nc * self.mu[pi], min=0.0)[..., None]
        flag = (nc < 0) & (torch.sqrt(tt.detach()) > 1e-30)
        t2 = torch.where(flag[..., None], tf, t)
        out = cv + w * (1 - infl[..., None]) + t2 * infl[..., None]
        if occ is not None:
            self.diag.append(dict(pi=pi, occ=occ.detach(), active=active.detach(), flag=flag.detach(), infl=infl.detach(), dist=dist.detach(),
                                  nc=nc.detach(), soft=sf.detach().expand_as(dist), pl=pl.detach(), kind=self.kin[pi], shape=self.shape[pi]))
        return torch.where(active[..., None], out, u)

    def step(self, *args):
        """rot_state: PlbRotTwin.step(x, v, C, F, prim_pos, prim_rot, action, softness, E, nu, ys, fric); else PlbPrimTwin.step (no prim_rot)."""
        return PlbRotTwin.step(self, *args) if self.rot_state else PlbPrimTwin.step(self, *args)

    def loss(self, x, prim_pos, target_density, target_sdf, weights, soft_contact=True, prim_rot=None):
        if self.rot_state:
            return PlbRotTwin.loss(self, x, prim_pos, target_density, target_sdf, weights, soft_contact, prim_rot)
        return PlbPrimTwin.loss(self, x, prim_pos, target_density, target_sdf, weights, soft_contact)


# ---- the cases the shape tests share, and the conditions that keep them honest --------------------------------------------------------
SHAPES = {BOX: (0.06, 0.04, 0.05), CYLINDER: (0.06, 0.04, 0.0), TORUS: (0.07, 0.025, 0.0)}
NAMES = {BOX: "box", CYLINDER: "cylinder", TORUS: "torus"}
TILT = (0.9, 0.1, -0.3, 0.2)                         # as plb_rot_twin.ROT0: normalised, then (rot_state) perturbed per env
SCALE_W = (0.05, 0.05, 0.05)
# Softness per env.  A cell outside the surface is active while exp(-dist softness) > 0.1, a shell ln(10) / softness thick: 0.0035 at the
# reference's default 666, a ninth of a cell at dx = 1 / 32, which leaves the outside regions (face, edge, side, cap, rim) all but empty
# on a rod four cells wide.  120 and 80 make it 0.019 and 0.029, about a cell; env 0 keeps the default.
SOFT = (666.0, 120.0, 80.0)
# where the primitive sits, per kind (found by moving it until honesty_shape held; env offsets are the case's own random 3 mm)
PLACE = {BOX: (0.5093, 0.2931, 0.4968), CYLINDER: (0.508, 0.2658, 0.5172), TORUS: (0.4584, 0.3299, 0.5287)}


def shape_case(kind, B, N, rot, seed=0, two=False):
    """tests/plb_prim_twin.capsule_case (the rod cut from the torus sample, perturbed v, C, F) with a Box, a Cylinder or a Torus a few cells
    across placed off-lattice in the rod, tilted, and an action that pushes it further in.  rot: a rot_state case (a start rotation per env,
    six action dimensions); two: a second primitive on the rod as well, capsule_case's (its kind is the caller's business).  Returns ((x, v, C, F, prim_pos[, prim_rot], action, E, nu, ys), softness [B,P], the twin's keyword arguments for primitive 0)."""
    import numpy as np
    from tests.plb_prim_twin import capsule_case
    x, v, Cm, F, prim, act, E, nu, ys = capsule_case(B, N, seed=seed, two=two)
    prim[:, 0] += np.array(PLACE[kind]) - np.array([0.5093, 0.2931, 0.4968])
    P = prim.shape[1]
    soft = np.array(SOFT)[:B, None].repeat(P, 1)
    q = np.array(TILT) / np.linalg.norm(TILT)
    kw = dict(kinds=(kind,), shape=(SHAPES[kind],))
    if not rot:
        kw.update(rot=(tuple(q),), action_dim=3, rot_state=False)
        return (x, v, Cm, F, prim, act, E, nu, ys), soft, kw
    r = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (B, P, 1))
    r[:, 0] = q[None] + np.random.default_rng(1).normal(size=(B, 4)) * 0.01
    ang = np.array([[0.3, -0.2, 0.25], [-0.4, 0.1, 0.2], [0.2, 0.3, -0.35]])[:B]
    kw.update(action_scale_w=SCALE_W, action_dim=6, rot_state=True)
    return (x, v, Cm, F, prim, r, np.concatenate([act, ang], 1), E, nu, ys), soft, kw


def regions(kind, shape, pl):
    """Which region of its shape each local point lies in: a dict of boolean masks."""
    if kind == BOX:
        q = pl.abs() - shape
        n = (q > 0).sum(-1)
        return dict(inside=n == 0, face=n == 1, edge=n >= 2)
    if kind == CYLINDER:
        _, d = cylinder_d(shape[:2], pl)
        ins = d.max(-1).values <= 0
        f = d[..., 0] > d[..., 1]
        return dict(side=(d[..., 0] > 0) & (d[..., 1] <= 0), cap=(d[..., 1] > 0) & (d[..., 0] <= 0), rim=(d[..., 0] > 0) & (d[..., 1] > 0),
                    inside_f1=ins & f, inside_f0=ins & ~f, y_pos=pl[..., 1] >= 0, y_neg=pl[..., 1] < 0)
    l, q = torus_q(shape[:2], pl)
    tube = length(q) - shape[1] <= 0
    return dict(in_tube=tube, out_tube=~tube, in_ring=q[..., 0] < 0, out_ring=q[..., 0] >= 0)


def honesty_shape(tw, min_flag=20, min_noflag=5):
    """plb_prim_twin.honesty (enough active occupied cells in both arms of the contact, none near influence = 0.1, dist = 0, nc = 0) and, for
    every substep of a Box, Cylinder or Torus: no occupied cell the contact can reach (dist < 0.1: beyond it the cell is inactive whatever
    round-off does) near a kink of its shape -- Box: |q_i| and |pl_i +- d| above 1e-9 at pl and its six sample points, inside the two
    largest q apart by 1e-9; Cylinder: |d0|, |d1|, |pl.y| above 1e-9, inside |d0 - d1| above 1e-9, l > 1e-3; Torus: l > 1e-3 and
    length(q) > 1e-3.  Returns (the least counts of an env, {region: active occupied cells, summed over envs and substeps})."""
    least = honesty(tw, min_flag, min_noflag)
    count = {}
    for d in tw.diag:
        kind = d.get("kind", 1)
        if kind not in (BOX, CYLINDER, TORUS):
            continue
        occ, act, pl, sc = d["occ"], d["occ"] & d["active"], d["pl"], d["shape"]
        near = occ & (d["dist"] < 0.1)
        for name, m in regions(kind, sc, pl).items():
            count[name] = count.get(name, 0) + int((m & act).sum())
        if kind == BOX:
            for i in range(-1, 3):
                for s in ((0.0,) if i < 0 else (FD, -FD)):
                    e = torch.zeros(3, dtype=DT)
                    if i >= 0:
                        e[i] = s
                    y = pl + e
                    q = y.abs() - sc
                    assert not bool((near[..., None] & (q.abs() < 1e-9)).any()), "a Box sample within 1e-9 of q_i = 0"
                    assert not bool((near[..., None] & (y.abs() < 1e-9)).any()), "a Box sample within 1e-9 of pl_i = 0"
                    top = q.sort(-1).values
                    ins = top[..., 2] <= 0
                    assert not bool((near & ins & ((top[..., 2] - top[..., 1]).abs() < 1e-9)).any()), "a Box sample inside within 1e-9 of a tie of q"
        elif kind == CYLINDER:
            l, dd = cylinder_d(sc[:2], pl)
            assert not bool((near[..., None] & (dd.abs() < 1e-9)).any()) and not bool((near & (pl[..., 1].abs() < 1e-9)).any()), "a Cylinder cell at a kink"
            assert not bool((near & (dd.max(-1).values <= 0) & ((dd[..., 0] - dd[..., 1]).abs() < 1e-9)).any()), "a Cylinder cell inside at d0 = d1"
            assert not bool((near & (l <= 1e-3)).any()), "a Cylinder cell on the axis"
        else:
            l, q = torus_q(sc[:2], pl)
            assert not bool((near & (l <= 1e-3)).any()) and not bool((near & (length(q) <= 1e-3)).any()), "a Torus cell on the axis or the ring's centre line"
    return least, count


def assert_regions(kind, counts, least=3):
    """Every region of the kind holds at least `least` active occupied cells, summed over the given honesty_shape counts."""
    total = {}
    for c in counts:
        for k, n in c.items():
            total[k] = total.get(k, 0) + n
    want = {BOX: ("inside", "face", "edge"), CYLINDER: ("side", "cap", "rim", "inside_f1", "inside_f0", "y_pos", "y_neg"),
            TORUS: ("in_tube", "out_tube", "in_ring", "out_ring")}[kind]
    assert all(total.get(k, 0) >= least for k in want), (NAMES[kind], total)
    return total
