"""Test infrastructure: torch f64 twin of the PLB step with ROTATING primitives, the reference of tests/test_plb_rot_*.py.  On top of
tests/plb_prim_twin.py (the Capsule's contact with a constant orientation) it restates GenORM/policy/pbm/plb/engine/primitive/
{primive_base.py:31-38,82-89,117-121,185-193 (rotation state, collider_v with rotation[f + 1], forward_kinematics, set_velocity with
action.dim = 6), primitives.py:83-99 (RollingPin.forward_kinematics), utils.py:19-41 (qmul with its normalisation, w2quat)}: every
primitive carries a per-env quaternion (w, x, y, z) that turns once per substep, the contact at substep f reads q_f for the signed distance
and the normal and q_{f+1} for the collider velocity.  `torch.autograd` is the adjoint: branch decisions are constants, sub-gradients at
ties are torch's.  w2quat returns the identity when |w| <= 1e-9, and |w| is taken under a `where` guard, so that arm sends the cotangent
0 to w (taichi's reverse mode would form 0 * inf there): this is the definition the kernels are held to.
PARITY UNPINNED: taichi is absent, the reference ships no recording of this path -- this restatement is the specification."""
from __future__ import annotations

import torch

from oracle.twin.plb_twin_torch import DT
from tests.plb_prim_twin import PlbPrimTwin


def qrot(rot, v):
    """utils.py:7-13, batched: rot [..., 4] against v [..., 3] (broadcast over the leading dimensions)."""
    qv = rot[..., 1:4].expand(v.shape)
    uv = torch.linalg.cross(qv, v, dim=-1)
    uuv = torch.linalg.cross(qv, uv, dim=-1)
    return v + 2 * (rot[..., 0:1] * uv + uuv)


def qmul(q, r):
    """utils.py:19-27: terms = outer(r, q), the Hamilton product q r, normalised.  q, r [..., 4]."""
    w = r[..., 0] * q[..., 0] - r[..., 1] * q[..., 1] - r[..., 2] * q[..., 2] - r[..., 3] * q[..., 3]
    x = r[..., 0] * q[..., 1] + r[..., 1] * q[..., 0] - r[..., 2] * q[..., 3] + r[..., 3] * q[..., 2]
    y = r[..., 0] * q[..., 2] + r[..., 1] * q[..., 3] + r[..., 2] * q[..., 0] - r[..., 3] * q[..., 1]
    z = r[..., 0] * q[..., 3] - r[..., 1] * q[..., 2] + r[..., 2] * q[..., 1] + r[..., 3] * q[..., 0]
    out = torch.stack([w, x, y, z], -1)
    return out / torch.sqrt((out * out).sum(-1, keepdim=True))


def w2quat(w):
    """utils.py:29-41: axis-angle [..., 3] -> quaternion; the identity when |w| <= 1e-9, where the gradient to w is 0 by definition
    (|w| is formed from a guarded copy, so the dead arm never differentiates sqrt at 0)."""
    n2 = (w * w).sum(-1, keepdim=True)
    big = n2 > 1e-18                                                  # |w| > 1e-9
    ws = torch.where(big, w, torch.ones_like(w))
    n = torch.sqrt((ws * ws).sum(-1, keepdim=True))
    s = torch.sin(n / 2)
    rot = torch.cat([torch.cos(n / 2), ws / n * s], -1)
    ident = torch.cat([torch.ones_like(n), torch.zeros_like(w)], -1)
    return torch.where(big, rot, ident)


def qinv(q):
    """inv_trans (utils.py:43-47): conj(q) / |q|."""
    return torch.cat([q[..., :1], -q[..., 1:]], -1) / torch.sqrt((q * q).sum(-1, keepdim=True))


class PlbRotTwin(PlbPrimTwin):
    """kinds: 0 sticky Sphere (primitive 1 only: never moves), 1 Capsule with the base kinematics, 2 RollingPin (the Capsule's geometry
    and contact, its own kinematics, three action dimensions)."""

    def __init__(self, conf, kinds=(1,), h=(0.0, 0.0), mu=(0.0, 0.0), action_scale=(1.0, 1.0, 1.0), action_scale_w=(1.0, 1.0, 1.0),
                 action_dim=3, substeps=None):
        contact = tuple(1 if k == 2 else k for k in kinds)                # the RollingPin collides as a Capsule
        super().__init__(conf, kinds=contact, h=h, rot=((1, 0, 0, 0),) * len(kinds), mu=mu, action_scale=action_scale, substeps=substeps)
        assert kinds[0] in (1, 2) and all(k == 0 for k in kinds[1:]) and action_dim in (3, 6) and not (kinds[0] == 2 and action_dim == 6)
        self.kin, self.action_dim = tuple(kinds), action_dim
        self.action_scale_w = torch.tensor(action_scale_w, dtype=DT)
        self._q0 = self._q1 = None                                        # [B,P,4] of the substep being run

    # ---- geometry in a per-env frame ---------------------------------------------------------------------------------------------
    def local_q(self, pi, d, qi):
        """d [B,...,3] = point - position, qi [B,4] -> (point in the primitive's frame, vector from the axis segment, its length)."""
        pl = qrot(qi.reshape((qi.shape[0],) + (1,) * (d.dim() - 2) + (4,)), d)
        py = pl[..., 1] + self.h[pi] / 2
        py = py - torch.clamp(py, 0.0, self.h[pi])
        p = torch.stack([pl[..., 0], py, pl[..., 2]], -1)
        return pl, p, torch.sqrt((p * p).sum(-1) + 1e-14)

    def sdf_q(self, pi, pts, pos, q):
        return self.local_q(pi, pts - pos, qinv(q))[2] - self.c.radius[pi]

    def collide(self, pi, gp, u, pos_f, pos_f1, soft, occ=None, q_f=None, q_f1=None):
        """Primitive.collide with rotation[f] = q_f [B,4] (distance, normal, the inverse) and rotation[f + 1] = q_f1 (collider velocity)."""
        q_f = self._q0[:, pi] if q_f is None else q_f
        q_f1 = self._q1[:, pi] if q_f1 is None else q_f1
        dt = self.c.dt
        g = gp if gp.dim() == 3 else gp[None]
        P0, P1, sf = pos_f[:, None, :], pos_f1[:, None, :], soft[:, None]
        pl, p, ln = self.local_q(pi, g - P0, qinv(q_f))
        dist = ln - self.c.radius[pi]
        D = qrot(q_f[:, None, :], p / ln[..., None])
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
                                  nc=nc.detach(), soft=sf.detach().expand_as(dist)))
        return torch.where(active[..., None], out, u)

    # ---- kinematics -------------------------------------------------------------------------------------------------------------
    def kinematics(self, pos, rot, a):
        """One substep: pos [B,P,3], rot [B,P,4], a [B,action_dim] = clip(action) -> (pos, rot) of the next substep."""
        c, S = self.c, self.S
        lo, hi = torch.tensor(c.lower_bound, dtype=DT), torch.tensor(c.upper_bound, dtype=DT)
        B, P = pos.shape[0], pos.shape[1]
        zero3 = torch.zeros((B, 3), dtype=DT)
        new_pos, new_rot = [], []
        for pi in range(P):
            if pi == 0 and self.kin[0] == 2:                                                 # RollingPin.forward_kinematics
                vel = a[:, :3] * self.action_scale / S
                dw, dth, dy = vel[:, 0], vel[:, 1], vel[:, 2]
                z = torch.zeros_like(dw)
                y_dir = qrot(rot[:, 0], torch.tensor([0.0, -1.0, 0.0], dtype=DT).expand(B, 3))
                up = torch.tensor([0.0, 1.0, 0.0], dtype=DT).expand(B, 3)
                x_dir = torch.linalg.cross(up, y_dir, dim=-1) * dw[:, None] * 0.03
                x_dir = torch.stack([x_dir[:, 0], dy, x_dir[:, 2]], -1)
                r1 = qmul(w2quat(torch.stack([z, -dth, z], -1)), qmul(rot[:, 0], w2quat(torch.stack([z, dw, z], -1))))
                step = x_dir
            else:                                                                            # Primitive.forward_kinematics
                step = a[:, :3] * self.action_scale / S if pi == 0 else zero3
                w = a[:, 3:6] * self.action_scale_w / S if (pi == 0 and self.action_dim == 6) else zero3
                r1 = qmul(w2quat(w), rot[:, pi])
            new_pos.append(torch.maximum(torch.minimum(pos[:, pi] + step, hi), lo))
            new_rot.append(r1)
        return torch.stack(new_pos, 1), torch.stack(new_rot, 1)

    def step(self, x, v, C, F, prim_pos, prim_rot, action, softness, E, nu, ys, fric):
        """set_action (clip +-1), `substeps` x (forward_kinematics, substep with q_f / q_{f+1}), copy frame cur -> 0."""
        a = torch.clamp(action, -1, 1)
        pos, rot = prim_pos, prim_rot
        for _ in range(self.S):
            pos1, rot1 = self.kinematics(pos, rot, a)
            self._q0, self._q1 = rot, rot1
            x, v, C, F = self.substep(x, v, C, F, pos, pos1, softness, E, nu, ys, fric)
            pos, rot = pos1, rot1
        return x, v, C, F, pos, rot

    def loss(self, x, prim_pos, target_density, target_sdf, weights, soft_contact=True, prim_rot=None):
        """PlbPrimTwin.loss with the Capsule's distance taken in the primitive's current frame prim_rot [B,P,4]."""
        c = self.c
        gm = self.grid_mass(x)
        density = (gm - target_density[None]).abs().sum(-1)
        sdf = (target_sdf[None] * gm).sum(-1)
        contact = torch.zeros_like(density)
        for pi in range(prim_pos.shape[1]):
            if self.kinds[pi] == 1:
                dij = torch.clamp(self.sdf_q(pi, x, prim_pos[:, pi, None, :], prim_rot[:, pi]), min=0.0)
            else:
                d = x - prim_pos[:, pi, None, :]
                dij = torch.clamp(torch.sqrt((d * d).sum(-1) + 1e-14) - c.radius[pi], min=0.0)
            if soft_contact:
                sw = 1 / (1 + dij * dij * 10000)
                md = (dij * sw / sw.sum(-1, keepdim=True)).sum(-1)
            else:
                md = dij.min(-1).values
            contact = contact + md ** 2
        total = contact * weights[0] + density * weights[1] + sdf * weights[2]
        return total, torch.stack([contact, density, sdf], -1)


# ---- the inputs the rotating-primitive tests share ------------------------------------------------------------------------------
RADIUS, HEIGHT, MU = 0.05, 0.12, 0.9
ROT0 = (0.9, 0.1, -0.3, 0.2)                        # normalised below, then perturbed per env: deliberately NOT unit (rot[0] is used as given)
SCALE_W = (0.05, 0.05, 0.05)
ROLL_SCALE = (0.7, 0.05, 1.0)


def rot_case(B, N, rolling=False, two=False):
    """tests/plb_prim_twin.capsule_case (the pressed-in rod) with a start rotation per env and the action of the kinematics under test:
    six-dimensional (the case's linear part, angular part scaled by SCALE_W) or the RollingPin's (dw, dth, dy) scaled by ROLL_SCALE.
    Returns (x, v, C, F, prim_pos, prim_rot, action, E, nu, ys) as numpy arrays and the twin's keyword arguments."""
    import numpy as np
    from tests.plb_prim_twin import capsule_case
    x, v, Cm, F, prim, act, E, nu, ys = capsule_case(B, N, two=two)
    P = prim.shape[1]
    q = np.array(ROT0) / np.linalg.norm(ROT0)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (B, P, 1))
    rot[:, 0] = q[None] + np.random.default_rng(1).normal(size=(B, 4)) * 0.01
    if rolling:
        act = np.array([[0.3, -0.2, -0.004], [-0.25, 0.3, -0.003], [0.2, 0.15, -0.0035]])[:B]
        kw = dict(kinds=(2,) + (0,) * (P - 1), action_scale=ROLL_SCALE, action_dim=3)
    else:
        ang = np.array([[0.3, -0.2, 0.25], [-0.4, 0.1, 0.2], [0.2, 0.3, -0.35]])[:B]
        act = np.concatenate([act, ang], 1)
        kw = dict(kinds=(1,) + (0,) * (P - 1), action_scale_w=SCALE_W, action_dim=6)
    return (x, v, Cm, F, prim, rot, act, E, nu, ys), kw
