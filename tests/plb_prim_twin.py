"""Test infrastructure: torch f64 twin of the PLB substep with the base class's primitive contact model (Capsule), the reference
of tests/test_plb_capsule_*.py.  A restatement of GenORM/policy/pbm/plb/engine/primitive/{primive_base.py:57-115 (sdf, normal,
collider_v, collide), primitives.py:55-73 (Capsule), utils.py (length, qrot, inv_trans)} inside the dense substep of
oracle.twin.plb_twin_torch.PlbTorchTwin; `torch.where` takes the branches, `torch.autograd` is the adjoint (branch decisions are
constants of it, sub-gradients at ties are torch's).  Kind 0 is the sticky Sphere of the base twin, unchanged operation for operation.
PARITY UNPINNED: taichi is absent, the reference ships no recording of this path -- this restatement is the specification."""
from __future__ import annotations

import torch

from oracle.twin.plb_twin_torch import DT, PlbTorchTwin, svd_ref


def qrot(rot, v):
    """utils.py:7-13.  rot [4], v [..., 3]."""
    qv = rot[1:4].expand_as(v)
    uv = torch.linalg.cross(qv, v, dim=-1)
    uuv = torch.linalg.cross(qv, uv, dim=-1)
    return v + 2 * (rot[0] * uv + uuv)


class PlbPrimTwin(PlbTorchTwin):
    def __init__(self, conf, kinds=(0, 0), h=(0.0, 0.0), rot=((1, 0, 0, 0), (1, 0, 0, 0)), mu=(0.0, 0.0), action_scale=(1.0, 1.0, 1.0),
                 substeps=None):
        super().__init__(conf)
        self.kinds, self.h, self.mu = tuple(kinds), tuple(float(a) for a in h), tuple(float(a) for a in mu)
        self.q = [torch.tensor(r, dtype=DT) for r in rot]
        for k, q in zip(self.kinds, self.q):
            assert k in (0, 1) and (k == 0 or float(q.norm()) > 0.9)                        # inv_trans asserts it
        self.qi = [torch.cat([q[:1], -q[1:]]) / torch.sqrt((q * q).sum()) for q in self.q]
        self.action_scale = torch.tensor(action_scale, dtype=DT)
        self.S = conf.substeps if substeps is None else int(substeps)
        self.diag = []          # per substep and primitive of kind 1: what the cells saw (detached), for the tests' honesty conditions

    # ---- Capsule geometry --------------------------------------------------------------------------------
    def local(self, pi, d):
        """d = point - position -> (point in the primitive's frame, vector from the axis segment, its length with 1e-14)."""
        pl = qrot(self.qi[pi], d)
        py = pl[..., 1] + self.h[pi] / 2
        py = py - torch.clamp(py, 0.0, self.h[pi])
        p = torch.stack([pl[..., 0], py, pl[..., 2]], -1)
        return pl, p, torch.sqrt((p * p).sum(-1) + 1e-14)

    def sdf(self, pi, pts, pos):
        return self.local(pi, pts - pos)[2] - self.c.radius[pi]

    def normal(self, pi, pts, pos):
        _, p, ln = self.local(pi, pts - pos)
        return qrot(self.q[pi], p / ln[..., None])

    def collide(self, pi, gp, u, pos_f, pos_f1, soft, occ=None):
        """Primitive.collide for cells gp [G,3] (or [B,G,3]), velocities u [B,G,3], positions [B,3], softness [B]."""
        dt = self.c.dt
        g = gp if gp.dim() == 3 else gp[None]
        P0, P1, sf = pos_f[:, None, :], pos_f1[:, None, :], soft[:, None]
        pl, p, ln = self.local(pi, g - P0)
        dist = ln - self.c.radius[pi]
        D = qrot(self.q[pi], p / ln[..., None])
        infl = torch.clamp(torch.exp(-dist * sf), max=1.0)
        active = ((sf > 0) & (infl > 0.1)) | (dist <= 0)
        cv = (qrot(self.q[pi], pl) + P1 - g) / dt
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

    # ---- one substep for B envs: PlbTorchTwin.substep with the primitive loop generalised ------------------
    def substep(self, x, v, C, F, pos_f, pos_f1, softness, E, nu, ys, fric):
        c = self.c
        n, dt, dx, inv_dx = c.n_grid, c.dt, c.dx, c.inv_dx
        B, N = x.shape[0], x.shape[1]
        I3 = torch.eye(3, dtype=DT)
        F_tmp = (I3 + dt * C) @ F
        U, sig, V = svd_ref(F_tmp)
        Vt = V.transpose(-1, -2)
        mu = (E / (2 * (1 + nu)))[:, None]
        lam = (E * nu / ((1 + nu) * (1 - 2 * nu)))[:, None]
        base = (x.detach() * inv_dx - 0.5).to(torch.int64)
        fx = x * inv_dx - base.to(DT)
        w = [0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1) ** 2, 0.5 * (fx - 0.5) ** 2]
        sg = torch.clamp(sig, min=0.05)
        eps = torch.log(sg)
        eps_hat = eps - eps.sum(-1, keepdim=True) / 3
        eps_hat_norm = torch.sqrt((eps_hat * eps_hat).sum(-1) + 1e-8)
        delta_gamma = eps_hat_norm - ys[:, None] / (2 * mu)
        yields = delta_gamma > 0
        eps_y = eps - (delta_gamma / eps_hat_norm)[..., None] * eps_hat
        F_y = (U * torch.exp(eps_y)[..., None, :]) @ Vt
        new_F = torch.where(yields[..., None, None], F_y, F_tmp)
        J = torch.linalg.det(new_F)
        r = U @ Vt
        stress = 2 * mu[..., None, None] * (new_F - r) @ new_F.transpose(-1, -2) + I3 * (lam * J * (J - 1))[..., None, None]
        stress = (-dt * c.p_vol * 4 * inv_dx * inv_dx) * stress
        affine = stress + c.p_mass * C
        G = n * n * n
        grid_v = torch.zeros((B, G, 3), dtype=DT)
        grid_m = torch.zeros((B, G), dtype=DT)
        lins, weights, dposs = [], [], []
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    off = torch.tensor([i, j, k], dtype=DT)
                    weight = w[i][..., 0] * w[j][..., 1] * w[k][..., 2]
                    idx = base + torch.tensor([i, j, k])
                    lin = (idx[..., 0] * n + idx[..., 1]) * n + idx[..., 2]
                    lins.append(lin); weights.append(weight); dposs.append(off - fx)
                    dpos = (off - fx) * dx
                    contrib = weight[..., None] * (c.p_mass * v + (affine @ dpos[..., None])[..., 0])
                    grid_v = grid_v.scatter_add(1, lin[..., None].expand(-1, -1, 3), contrib)
                    grid_m = grid_m.scatter_add(1, lin, weight * c.p_mass)
        ar = torch.arange(n)
        Ig = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(G, 3)
        gp = Ig.to(DT) * dx
        occ = grid_m > 1e-12
        safe_m = torch.where(occ, grid_m, torch.ones_like(grid_m))
        g30 = torch.tensor(c.gravity, dtype=DT) * dt * 30
        vo = grid_v / safe_m[..., None] + g30
        for pi in range(pos_f.shape[1]):
            if self.kinds[pi] == 1:                                                         # Primitive.collide, primive_base.py:91-115
                vo = self.collide(pi, gp, vo, pos_f[:, pi], pos_f1[:, pi], softness[:, pi], occ)
                continue
            d = gp[None] - pos_f[:, pi, None, :]                                            # Sphere.collide (sticky), as the base twin
            dist = torch.sqrt((d * d).sum(-1) + 1e-14) - c.radius[pi]
            soft = softness[:, pi, None]
            infl = torch.clamp(torch.exp(-dist * soft), max=1.0)
            cond = (((soft > 0) & (infl > 0.1)) | (dist <= 0.001)) & (soft > 0)
            cv = ((pos_f1[:, pi] - pos_f[:, pi]) / dt)[:, None, :]
            vo = torch.where(cond[..., None], cv.expand_as(vo), vo)
        Igf = Ig.to(DT)
        fr = fric[:, None]
        self.bottom_all_zeroed = getattr(self, "bottom_all_zeroed", 0)
        for d in range(3):
            lo = (Ig[None, :, d] < 3) & (vo[..., d] < 0)
            if d != 1:
                vo = torch.cat([torch.where(lo, torch.zeros_like(vo[..., e]), vo[..., e])[..., None] if e == d else vo[..., e:e + 1]
                                for e in range(3)], -1)
            else:
                lin_ = vo[..., 1] + 1e-30
                normal = torch.tensor([0.0, 1.0, 0.0], dtype=DT)
                vit = vo - lin_[..., None] * normal - Igf[None] * 1e-30
                lit = torch.sqrt((vit * vit).sum(-1) + 1e-8)
                sc = torch.clamp(1.0 + fr * lin_ / lit, min=0.0)
                vf = sc[..., None] * (vit + Igf[None] * 1e-30)
                vf = torch.cat([vf[..., 0:1], torch.zeros_like(vf[..., 1:2]), vf[..., 2:3]], -1)
                zero_all = torch.zeros_like(vo)
                only_y = torch.cat([vo[..., 0:1], torch.zeros_like(vo[..., 1:2]), vo[..., 2:3]], -1)
                branch = torch.where((fr == 0)[..., None], only_y, torch.where((fr < 10)[..., None], vf, zero_all))
                self.bottom_all_zeroed += int((lo & occ & (fr >= 10)).sum())                # cells the ground_friction >= 10 branch stopped
                vo = torch.where(lo[..., None], branch, vo)
            hi = (Ig[None, :, d] > n - 3) & (vo[..., d] > 0)
            vo = torch.cat([torch.where(hi, torch.zeros_like(vo[..., e]), vo[..., e])[..., None] if e == d else vo[..., e:e + 1]
                            for e in range(3)], -1)
        out = torch.where(occ[..., None], vo, torch.zeros_like(vo))
        new_v = torch.zeros((B, N, 3), dtype=DT)
        new_C = torch.zeros((B, N, 3, 3), dtype=DT)
        for lin, weight, dpos in zip(lins, weights, dposs):
            g_v = out.gather(1, lin[..., None].expand(-1, -1, 3))
            new_v = new_v + weight[..., None] * g_v
            new_C = new_C + 4 * inv_dx * weight[..., None, None] * (g_v[..., :, None] * dpos[..., None, :])
        new_x = torch.clamp(x + dt * new_v, min=0.0, max=1.0 - 3 * dx)
        return new_x, new_v, new_C, new_F

    def step(self, x, v, C, F, prim_pos, action, softness, E, nu, ys, fric):
        """set_action (clip +-1, v = a * action_scale / substeps for primitive 0), `substeps` substeps, copy frame cur -> 0."""
        c = self.c
        S = self.S
        a = torch.clamp(action, -1, 1)
        pv = torch.zeros_like(prim_pos)
        pv = torch.cat([(a[:, :3] * self.action_scale / S)[:, None, :], pv[:, 1:]], 1)
        lo, hi = torch.tensor(c.lower_bound, dtype=DT), torch.tensor(c.upper_bound, dtype=DT)
        pos = prim_pos
        for _ in range(S):
            pos1 = torch.maximum(torch.minimum(pos + pv, hi), lo)
            x, v, C, F = self.substep(x, v, C, F, pos, pos1, softness, E, nu, ys, fric)
            pos = pos1
        return x, v, C, F, pos

    def loss(self, x, prim_pos, target_density, target_sdf, weights, soft_contact=True):
        """PlbTorchTwin.loss with d_i = max(sdf(x_i), 0) taken from the primitive's own sdf."""
        c = self.c
        gm = self.grid_mass(x)
        density = (gm - target_density[None]).abs().sum(-1)
        sdf = (target_sdf[None] * gm).sum(-1)
        contact = torch.zeros_like(density)
        for pi in range(prim_pos.shape[1]):
            if self.kinds[pi] == 1:
                dij = torch.clamp(self.sdf(pi, x, prim_pos[:, pi, None, :]), min=0.0)
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


# ---- the pressed-in state the Capsule tests share, and the conditions that keep them honest ---------------------------------
def capsule_case(B, N, seed=0, two=False):
    """Particles cut from the torus box (the first N of its sample: a thin vertical rod from the floor up), v, C, F perturbed as
    tests/test_plb.py does, a Capsule placed off-lattice inside the rod, per env a little elsewhere, and an action that moves it
    further in.  two: a sticky Sphere as primitive 1, on the rod as well.  Returns numpy arrays."""
    import numpy as np
    from oracle.twin.plb_twin import torus_particles
    rng = np.random.default_rng(seed)
    x = torus_particles(1000)[:N][None].repeat(B, 0) + rng.normal(size=(B, N, 3)) * 1e-4
    v = rng.normal(size=(B, N, 3)) * 0.01
    Cm = rng.normal(size=(B, N, 3, 3)) * 0.1
    F = np.eye(3)[None, None] + rng.normal(size=(B, N, 3, 3)) * 0.002
    prim = (np.array([[0.5093, 0.2931, 0.4968]]) + rng.normal(size=(B, 1, 3)) * 0.003)
    if two:
        prim = np.concatenate([prim, np.array([[0.4971, 0.1213, 0.5037]])[None].repeat(B, 0) + rng.normal(size=(B, 1, 3)) * 0.003], 1)
    act = np.array([[-0.004, 0.003, 0.002], [-0.003, -0.002, 0.003], [-0.0035, 0.001, -0.002]])[:B]
    E = np.array([5e3, 3e3, 4e3])[:B]
    nu = np.array([0.35, 0.3, 0.25])[:B]
    ys = np.array([1762.2, 30.0, 200.0])[:B]
    return x, v, Cm, F, prim, act, E, nu, ys


def honesty(tw, min_flag=20, min_noflag=5):
    """The conditions under which a comparison against this twin means something, asserted on its own forward (tw.diag: every
    Capsule substep run so far).  Per env, over those substeps: enough occupied cells in each arm of the contact.  In every substep:
    no occupied cell so near a branch point that round-off could take the other arm (a branch flip is an O(1) difference, not
    round-off).  Returns the least counts of an env."""
    assert tw.diag, "no Capsule substep ran"
    n_flag = n_noflag = 0
    for d in tw.diag:
        occ, act = d["occ"], d["occ"] & d["active"]
        n_flag, n_noflag = n_flag + (act & d["flag"]).sum(-1), n_noflag + (act & ~d["flag"]).sum(-1)
        soft = d["soft"] > 0
        assert not bool((occ & soft & ((d["infl"] - 0.1).abs() < 1e-6)).any()), "a cell within 1e-6 of influence = 0.1"
        assert not bool((occ & (d["dist"].abs() < 1e-9)).any()), "a cell within 1e-9 of dist = 0"
        assert not bool((act & (d["nc"].abs() < 1e-12)).any()), "an active cell within 1e-12 of nc = 0"
    least = (int(n_flag.min()), int(n_noflag.min()))
    assert least[0] >= min_flag and least[1] >= min_noflag, least
    return least
