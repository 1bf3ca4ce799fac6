"""Test infrastructure: torch f64 twin of the PLB step with the Chopsticks primitive, the reference of tests/test_plb_chopsticks_*.py.  On
top of tests/plb_shape_twin.py (the base class's contact through a kind's own _sdf / _normal) and tests/plb_rot_twin.py (orientation as
per-env state) it restates GenORM/policy/pbm/plb/engine/primitive/primitives.py:102-173: two Capsules side by side whose opening `gap` is
state.  Geometry (:130-147), for the local point pl: p = pl + (0, h/2, 0), delta = (gap/2, 0, 0), a = capsule_sdf(p - delta), b =
capsule_sdf(p + delta) with capsule_sdf the Capsule's _sdf (:61-66), which shifts y by h/2 AGAIN before it takes off clamp(y, 0, h) -- each
stick's axis segment spans local y in [-h, 0] at x = -+gap/2, the primitive's position is the sticks' TOP END; sdf = min(a, b), the normal
m a_n + (1 - m) b_n with m = [a <= b].  Kinematics (:113-128), once per substep: gap[f+1] = max(gap[f] - gap_vel, minimal_gap), pos[f+1] =
clamp(pos[f] + v), rot[f+1] = qmul(rot[f], w2quat(w)) -- a RIGHT multiplication, where the base class has w2quat(w) on the left -- with
(v, w, gap_vel) = clip(action, -1, 1) * (action_scale, action_scale_w, action_scale_gap) / substeps, seven action dimensions.  World normal,
contact model and collider velocity are the base class's: the closing motion is not part of the collider velocity.
`torch.autograd` is the adjoint: m and the arm of min are constants (min is written as where(a <= b, a, b): a tie takes stick a for both), so
are the arms of clamp / max; sub-gradients at ties are torch's and the cases stay away from them (honesty_chop).
Kinds: primitive 0 is the Chopsticks (6), primitive 1, if any, the unactuated sticky Sphere of every rot_state handle.
PARITY UNPINNED: taichi is absent, the reference ships no chopsticks.yml and no recording of this path -- this restatement is the
specification."""
from __future__ import annotations

import numpy as np
import torch

from oracle.twin.plb_twin_torch import DT
from tests.plb_prim_twin import PlbPrimTwin, honesty
from tests.plb_rot_twin import PlbRotTwin, qmul, w2quat
from tests.plb_shape_twin import PlbShapeTwin, length, normalize

CHOPSTICKS = 6
# margins of honesty_chop: how far an occupied cell within reach of the contact must stay from the a = b plane (in |a - b|) and from the ends
# of a stick's axis segment (in local y), and how far gap - gap_vel must stay from minimal_gap in every substep.  The kernels and the twin
# agree to ~1e-13 on these quantities; a cell nearer than that could take the other arm on the device, an O(1) difference.
MARGIN_AB, MARGIN_Y, MARGIN_GAP = 1e-9, 1e-9, 1e-9


def capsule_p2(h, p):
    """The p2 of Capsule._sdf / _normal (:61-73): p.y += h / 2; p.y -= clamp(p.y, 0, h)."""
    py = p[..., 1] + h / 2
    py = py - torch.clamp(py, 0.0, h)
    return torch.stack([p[..., 0], py, p[..., 2]], -1)


def chop_sticks(h, r, gap, pl):
    """:130-145.  gap broadcasts against pl[..., 0].  Returns (a, b, a_n, b_n): both sticks' signed distance and local normal."""
    up = torch.tensor([0.0, h / 2, 0.0], dtype=DT)
    p = pl + up                                                       # grid_pos - (0, -h/2, 0)
    zero = torch.zeros_like(gap)
    delta = torch.stack([gap / 2, zero, zero], -1)
    pa, pb = capsule_p2(h, p - delta), capsule_p2(h, p + delta)
    return length(pa) - r, length(pb) - r, normalize(pa), normalize(pb)


def chop_sdf(h, r, gap, pl):
    a, b, _, _ = chop_sticks(h, r, gap, pl)
    return torch.where(a <= b, a, b)                                  # ti.min(a, b); the arm is a constant of the adjoint


def chop_normal(h, r, gap, pl):
    a, b, a_n, b_n = chop_sticks(h, r, gap, pl)
    m = (a <= b).to(DT)[..., None]
    return m * a_n + (1 - m) * b_n


def qmul_right_by_hand(q, r):
    """The Hamilton product q r written out from its definition (scalar and vector parts), normalised: what rot[f+1] = qmul(rot[f], w2quat(w))
    must equal.  q, r [4] tensors."""
    w = q[0] * r[0] - (q[1:] * r[1:]).sum()
    vec = q[0] * r[1:] + r[0] * q[1:] + torch.linalg.cross(q[1:], r[1:])
    out = torch.cat([w[None], vec])
    return out / torch.sqrt((out * out).sum())


class PlbChopsticksTwin(PlbShapeTwin):
    def __init__(self, conf, kinds=(CHOPSTICKS,), h=(0.06, 0.0), mu=(0.0, 0.0), min_gap=(0.06, 0.0), action_scale=(1.0, 1.0, 1.0),
                 action_scale_w=(1.0, 1.0, 1.0), action_scale_gap=1.0, substeps=None):
        P = len(kinds)
        assert kinds[0] == CHOPSTICKS and all(k == 0 for k in kinds[1:])
        # the parents assert their own kinds: constructed with the contact kinds (1 = Primitive.collide), the real ones kept beside them
        PlbPrimTwin.__init__(self, conf, kinds=(1,) + (0,) * (P - 1), h=h, rot=((1, 0, 0, 0),) * P, mu=mu, action_scale=action_scale,
                             substeps=substeps)
        self.kin, self.action_dim, self.rot_state = tuple(kinds), 7, True
        self.action_scale_w = torch.tensor(action_scale_w, dtype=DT)
        self.action_scale_gap, self.min_gap = float(action_scale_gap), tuple(float(g) for g in min_gap)
        self.shape = [torch.zeros(3, dtype=DT) for _ in range(max(P, 1))]           # unused by kind 6 (the diagnostics carry it)
        self._q0 = self._q1 = None
        self._gap = None                                                          # [B,P] of the substep (or loss) being run
        self.gap_log = []                                                         # per substep: gap[f] - gap_vel of primitive 0, [B]

    def _gap_of(self, pi, pl):
        g = self._gap[:, pi]
        return g.reshape((g.shape[0],) + (1,) * (pl.dim() - 2))

    def _sdf(self, pi, pl):
        if self.kin[pi] != CHOPSTICKS:
            return super()._sdf(pi, pl)
        return chop_sdf(self.h[pi], self.c.radius[pi], self._gap_of(pi, pl), pl)

    def _normal(self, pi, pl):
        if self.kin[pi] != CHOPSTICKS:
            return super()._normal(pi, pl)
        return chop_normal(self.h[pi], self.c.radius[pi], self._gap_of(pi, pl), pl)

    def kinematics(self, pos, rot, gap, a):
        """One substep (:113-117): pos [B,P,3], rot [B,P,4], gap [B,P], a [B,7] = clip(action) -> (pos, rot, gap) of the next substep."""
        c, S = self.c, self.S
        lo, hi = torch.tensor(c.lower_bound, dtype=DT), torch.tensor(c.upper_bound, dtype=DT)
        B, P = pos.shape[0], pos.shape[1]
        zero3 = torch.zeros((B, 3), dtype=DT)
        new_pos, new_rot, new_gap = [], [], []
        for pi in range(P):
            if pi == 0:                                                           # Chopsticks.forward_kinematics
                step = a[:, :3] * self.action_scale / S
                w = a[:, 3:6] * self.action_scale_w / S
                gv = a[:, 6] * self.action_scale_gap / S
                pre = gap[:, 0] - gv
                self.gap_log.append(pre.detach())
                new_gap.append(torch.clamp(pre, min=self.min_gap[0]))
                new_rot.append(qmul(rot[:, 0], w2quat(w)))                        # rotation[f] on the LEFT
            else:                                                                 # Primitive.forward_kinematics with v = w = 0
                step = zero3
                new_gap.append(gap[:, pi])
                new_rot.append(qmul(w2quat(zero3), rot[:, pi]))
            new_pos.append(torch.maximum(torch.minimum(pos[:, pi] + step, hi), lo))
        return torch.stack(new_pos, 1), torch.stack(new_rot, 1), torch.stack(new_gap, 1)

    def step(self, x, v, C, F, prim_pos, prim_rot, prim_gap, action, softness, E, nu, ys, fric):
        """set_action (clip +-1), `substeps` x (forward_kinematics, substep with q_f / q_{f+1} and gap_f), copy frame cur -> 0."""
        a = torch.clamp(action, -1, 1)
        pos, rot, gap = prim_pos, prim_rot, prim_gap
        for _ in range(self.S):
            pos1, rot1, gap1 = self.kinematics(pos, rot, gap, a)
            self._q0, self._q1, self._gap = rot, rot1, gap
            n0 = len(self.diag)
            x, v, C, F = self.substep(x, v, C, F, pos, pos1, softness, E, nu, ys, fric)
            for d in self.diag[n0:]:
                d["gap"], d["h"] = gap[:, d["pi"]].detach(), self.h[d["pi"]]
            pos, rot, gap = pos1, rot1, gap1
        return x, v, C, F, pos, rot, gap

    def loss(self, x, prim_pos, prim_rot, prim_gap, target_density, target_sdf, weights, soft_contact=True):
        """PlbRotTwin.loss with the Chopsticks' distance at the current gap prim_gap [B,P]."""
        self._gap = prim_gap
        return PlbRotTwin.loss(self, x, prim_pos, target_density, target_sdf, weights, soft_contact, prim_rot)


# ---- the cases the Chopsticks tests share, and the conditions that keep them honest ----------------------------------------------------
H, R, MIN_GAP = 0.06, 0.03, 0.06                    # primitives.py:166-173 (init_gap is per env below)
TILT = (0.9, 0.1, -0.3, 0.2)
SCALE_W, SCALE_GAP = (0.05, 0.05, 0.05), 0.03
SOFT = (666.0, 120.0, 80.0)                         # as tests/plb_shape_twin.py: env 0 the reference's default, a thicker shell in envs 1 and 2
# where the primitive's position (the sticks' top end) sits: found on the CPU by moving it until honesty_chop held at N = 33 and N = 300
PLACE = (0.5122, 0.402, 0.5003)
# The opening per env, with S = 3 substeps and gap_vel = a[6] SCALE_GAP / S:
#   env 0 opens (gap_vel = -0.005: 0.070 -> 0.075 -> 0.080 -> 0.085, never clamped);
#   env 1 closes from above minimal_gap and reaches the clamp in the second substep (gap_vel = 0.006: 0.069 -> 0.063 -> max(0.057, 0.06) -> 0.06);
#   env 2 starts at init_gap = minimal_gap and closes (gap_vel = 0.004: clamped throughout, so g_action[6] and the kinematic part of
#   g_prim_gap0 are exactly 0).
GAP0 = (0.070, 0.069, 0.060)
ACT_GAP = (-0.5, 0.6, 0.4)


def chop_case(B, N, seed=0, two=False, place=PLACE):
    """tests/plb_prim_twin.capsule_case (the rod cut from the torus sample, perturbed v, C, F) with a tilted Chopsticks astride the rod and an
    action that moves it further in, turns it and drives the gap as GAP0 / ACT_GAP say.  two: a sticky Sphere as primitive 1, on the rod as
    well.  Returns ((x, v, C, F, prim_pos, prim_rot, prim_gap, action, E, nu, ys), softness [B,P], the twin's keyword arguments)."""
    from tests.plb_prim_twin import capsule_case
    x, v, Cm, F, prim, act, E, nu, ys = capsule_case(B, N, seed=seed, two=two)
    prim[:, 0] += np.array(place) - np.array([0.5093, 0.2931, 0.4968])
    P = prim.shape[1]
    soft = np.array(SOFT)[:B, None].repeat(P, 1)
    q = np.array(TILT) / np.linalg.norm(TILT)
    r = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (B, P, 1))
    r[:, 0] = q[None] + np.random.default_rng(1).normal(size=(B, 4)) * 0.01
    ang = np.array([[0.3, -0.2, 0.25], [-0.4, 0.1, 0.2], [0.2, 0.3, -0.35]])[:B]
    gap = np.zeros((B, P))
    gap[:, 0] = np.array(GAP0)[:B]
    action = np.concatenate([act, ang, np.array(ACT_GAP)[:B, None]], 1)
    kw = dict(kinds=(CHOPSTICKS,) + (0,) * (P - 1), h=(H, 0.0), min_gap=(MIN_GAP, 0.0), action_scale_w=SCALE_W, action_scale_gap=SCALE_GAP)
    return (x, v, Cm, F, prim, r, gap, action, E, nu, ys), soft, kw


def honesty_chop(tw, min_flag=20, min_noflag=5, least=3):
    """plb_prim_twin.honesty (enough active occupied cells in both arms of the contact per env, none near influence = 0.1, dist = 0, nc = 0) and,
    for every Chopsticks substep run so far: at least `least` active occupied cells on EACH stick in the cap region (local y clamped: beyond an
    end of the axis segment) and in the side region (alongside it), summed over envs and substeps; no occupied cell the contact can reach
    (dist < 0.1) within MARGIN_AB of the a = b plane or within MARGIN_Y of an end of the axis segment; no env with a substep whose
    gap - gap_vel lies within MARGIN_GAP of minimal_gap.  Returns (the least counts of an env, {stick_region: cells})."""
    worst = honesty(tw, min_flag, min_noflag)
    count = dict(a_cap=0, a_side=0, b_cap=0, b_side=0)
    seen = False
    for d in tw.diag:
        if d.get("kind") != CHOPSTICKS:
            continue
        seen = True
        occ, act, pl, h = d["occ"], d["occ"] & d["active"], d["pl"], d["h"]
        near = occ & (d["dist"] < 0.1)
        a, b, _, _ = chop_sticks(h, tw.c.radius[d["pi"]], d["gap"][:, None], pl)
        py = pl[..., 1] + h / 2 + h / 2
        assert not bool((near & ((a - b).abs() < MARGIN_AB)).any()), "a cell within MARGIN_AB of the a = b plane"
        assert not bool((near & ((py.abs() < MARGIN_Y) | ((py - h).abs() < MARGIN_Y))).any()), "a cell within MARGIN_Y of an end of the axis segment"
        on_a, side = a <= b, (py >= 0) & (py <= h)
        for name, m in (("a_cap", on_a & ~side), ("a_side", on_a & side), ("b_cap", ~on_a & ~side), ("b_side", ~on_a & side)):
            count[name] += int((m & act).sum())
    assert seen, "no Chopsticks substep ran"
    assert all(n >= least for n in count.values()), count
    for pre in tw.gap_log:
        assert not bool(((pre - tw.min_gap[0]).abs() < MARGIN_GAP).any()), "gap - gap_vel within MARGIN_GAP of minimal_gap"
    return worst, count
