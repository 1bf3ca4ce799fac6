"""Test infrastructure: torch f64 twins of the PLB step with BOTH primitives actuated, the reference of tests/test_plb_two_hand_*.py.
Thin subclasses of tests/plb_prim_twin.py, plb_rot_twin.py, plb_shape_twin.py and plb_chopsticks_twin.py that restate ONE thing,
GenORM/policy/pbm/plb/engine/primitive/primitives.py:280-319: `Primitives` gives every primitive its own action.dim and slices one flat action
vector by the running offsets `action_dims` (set_action :307-311), get_grad concatenates the per-primitive gradients (:313-319).  Here:
the action row is [A0 + action_dim1], primitive 0 takes columns 0 .. A0 - 1 exactly as the parent twin has it (A0 = 3, 6, or the
Chopsticks' 7), primitive 1 takes columns A0 .. A0 + action_dim1 - 1 and ALWAYS follows the base class (primive_base.py:117-121,185-193),
also beside a RollingPin or a Chopsticks:
    v = a[0:3] action_scale1 / substeps,  w = a[3:6] action_scale_w1 / substeps (0 with action_dim1 = 3),
    pos[f+1] = clamp(pos[f] + v, lower_bound, upper_bound),  rot[f+1] = qmul(w2quat(w), rot[f])   (left multiplication).
The clip to [-1, 1] is the parents', applied to the whole row.  action_dim1 = 0 is the parent twin to the letter.  Everything else --
substep, contact, geometry, losses, primitive 0's kinematics -- is inherited; the constructors are restated only to lift the parents'
`kinds[1:] == 0` asserts (primitive 1 may be kind 0, 1, 3, 4 or 5; RollingPin and Chopsticks stay primitive 0 only).
PARITY UNPINNED: taichi is absent and the reference ships no two-handed task -- this restatement is the specification."""
from __future__ import annotations

import torch

from oracle.twin.plb_twin_torch import DT
from tests.plb_chopsticks_twin import CHOPSTICKS, PlbChopsticksTwin
from tests.plb_prim_twin import PlbPrimTwin
from tests.plb_rot_twin import PlbRotTwin, qmul, w2quat
from tests.plb_shape_twin import BOX, CYLINDER, TORUS, PlbShapeTwin


class _TwoHand:
    """Primitive 1's action block: where it sits in the row and what it does to primitive 1."""

    def _two(self, A0, action_dim1, action_scale1, action_scale_w1):
        assert action_dim1 in (0, 3, 6)
        self.A0, self.action_dim1 = int(A0), int(action_dim1)
        self.action_dims = (0, self.A0, self.A0 + self.action_dim1)      # Primitives.action_dims
        self.action_scale1 = torch.tensor(action_scale1, dtype=DT)
        self.action_scale_w1 = torch.tensor(action_scale_w1, dtype=DT)

    def block1(self, a):
        """a [B,A] = clip(action) -> primitive 1's (v, w) per substep, [B,3] each."""
        zero3 = torch.zeros((a.shape[0], 3), dtype=DT)
        blk = a[:, self.A0:self.A0 + self.action_dim1]
        v = blk[:, :3] * self.action_scale1 / self.S
        w = blk[:, 3:6] * self.action_scale_w1 / self.S if self.action_dim1 == 6 else zero3
        return v, w

    def _bounds(self):
        return torch.tensor(self.c.lower_bound, dtype=DT), torch.tensor(self.c.upper_bound, dtype=DT)

    def step_plain(self, x, v, C, F, prim_pos, action, softness, E, nu, ys, fric):
        """PlbPrimTwin.step with primitive 1's velocity from its block instead of zero."""
        if self.action_dim1 == 0:
            return PlbPrimTwin.step(self, x, v, C, F, prim_pos, action, softness, E, nu, ys, fric)
        S = self.S
        a = torch.clamp(action, -1, 1)
        pv = torch.stack([a[:, :3] * self.action_scale / S, self.block1(a)[0]], 1)
        lo, hi = self._bounds()
        pos = prim_pos
        for _ in range(S):
            pos1 = torch.maximum(torch.minimum(pos + pv, hi), lo)
            x, v, C, F = self.substep(x, v, C, F, pos, pos1, softness, E, nu, ys, fric)
            pos = pos1
        return x, v, C, F, pos

    def move1(self, pos, rot, new_pos, new_rot, a):
        """The parent's kinematics moved primitive 0 (and left primitive 1 where it was): put primitive 1's own step in its place."""
        if self.action_dim1 == 0:
            return new_pos, new_rot
        v, w = self.block1(a)
        lo, hi = self._bounds()
        p1 = torch.maximum(torch.minimum(pos[:, 1] + v, hi), lo)
        r1 = qmul(w2quat(w), rot[:, 1])
        return torch.stack([new_pos[:, 0], p1], 1), torch.stack([new_rot[:, 0], r1], 1)


class PlbTwoHandPrimTwin(_TwoHand, PlbPrimTwin):
    """Constant orientation, Spheres and Capsules (PlbPrimTwin asserts nothing about primitive 1)."""

    def __init__(self, conf, action_dim1=0, action_scale1=(1.0, 1.0, 1.0), **kw):
        PlbPrimTwin.__init__(self, conf, **kw)
        assert action_dim1 in (0, 3)
        self._two(3, action_dim1, action_scale1, (1.0, 1.0, 1.0))

    def step(self, *args):
        return self.step_plain(*args)


class PlbTwoHandRotTwin(_TwoHand, PlbRotTwin):
    """rot_state with Capsules / a RollingPin / Spheres: kinds[0] in (1, 2), kinds[1] in (0, 1)."""

    def __init__(self, conf, kinds=(1,), h=(0.0, 0.0), mu=(0.0, 0.0), action_scale=(1.0, 1.0, 1.0), action_scale_w=(1.0, 1.0, 1.0), action_dim=3,
                 substeps=None, action_dim1=0, action_scale1=(1.0, 1.0, 1.0), action_scale_w1=(1.0, 1.0, 1.0)):
        contact = tuple(1 if k == 2 else k for k in kinds)
        PlbPrimTwin.__init__(self, conf, kinds=contact, h=h, rot=((1, 0, 0, 0),) * len(kinds), mu=mu, action_scale=action_scale, substeps=substeps)
        assert kinds[0] in (1, 2) and all(k in (0, 1) for k in kinds[1:]) and action_dim in (3, 6) and not (kinds[0] == 2 and action_dim == 6)
        assert action_dim1 != 0 or all(k == 0 for k in kinds[1:])         # the parent's own condition where primitive 1 is unactuated
        self.kin, self.action_dim = tuple(kinds), action_dim
        self.action_scale_w = torch.tensor(action_scale_w, dtype=DT)
        self._q0 = self._q1 = None
        self._two(action_dim, action_dim1, action_scale1, action_scale_w1)

    def kinematics(self, pos, rot, a):
        new_pos, new_rot = PlbRotTwin.kinematics(self, pos, rot, a)
        return self.move1(pos, rot, new_pos, new_rot, a)


class PlbTwoHandShapeTwin(_TwoHand, PlbShapeTwin):
    """Every kind of PlbShapeTwin, with or without rot_state; primitive 1 may be kind 0, 1, 3, 4 or 5."""

    def __init__(self, conf, kinds=(BOX,), shape=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), h=(0.0, 0.0), rot=None, mu=(0.0, 0.0),
                 action_scale=(1.0, 1.0, 1.0), action_scale_w=(1.0, 1.0, 1.0), action_dim=3, substeps=None, rot_state=False,
                 action_dim1=0, action_scale1=(1.0, 1.0, 1.0), action_scale_w1=(1.0, 1.0, 1.0)):
        P = len(kinds)
        rot = ((1, 0, 0, 0),) * P if rot is None else rot
        contact = tuple(0 if k == 0 else 1 for k in kinds)
        PlbPrimTwin.__init__(self, conf, kinds=contact, h=h, rot=rot, mu=mu, action_scale=action_scale, substeps=substeps)
        assert all(k in (0, 1, 2, BOX, CYLINDER, TORUS) for k in kinds) and action_dim in (3, 6) and all(k != 2 for k in kinds[1:])
        if rot_state:
            assert kinds[0] != 0 and not (kinds[0] == 2 and action_dim == 6)
            assert action_dim1 != 0 or all(k == 0 for k in kinds[1:])     # the parent's own condition where primitive 1 is unactuated
        else:
            assert 2 not in kinds and action_dim == 3 and action_dim1 in (0, 3)
        self.kin, self.action_dim, self.rot_state = tuple(kinds), action_dim, bool(rot_state)
        self.action_scale_w = torch.tensor(action_scale_w, dtype=DT)
        self.shape = [torch.tensor((tuple(s) + (0.0,) * 3)[:3], dtype=DT) for s in (tuple(shape) + ((0.0,) * 3,) * 2)[:max(P, 1)]]
        self._q0 = self._q1 = None
        self._two(action_dim, action_dim1, action_scale1, action_scale_w1)

    def kinematics(self, pos, rot, a):
        new_pos, new_rot = PlbRotTwin.kinematics(self, pos, rot, a)
        return self.move1(pos, rot, new_pos, new_rot, a)

    def step(self, *args):
        return PlbRotTwin.step(self, *args) if self.rot_state else self.step_plain(*args)


class PlbTwoHandChopsticksTwin(_TwoHand, PlbChopsticksTwin):
    """A Chopsticks (seven action dimensions) beside an actuated primitive 1 of kind 0, 1, 3, 4 or 5: A = 7 + action_dim1.  Primitive 1's gap
    entry is carried.  The constructor is the parent's with its `kinds[1:] == 0` assert lifted (and `shape` for a Box, Cylinder or Torus)."""

    def __init__(self, conf, kinds=(CHOPSTICKS,), h=(0.06, 0.0), mu=(0.0, 0.0), min_gap=(0.06, 0.0), action_scale=(1.0, 1.0, 1.0),
                 action_scale_w=(1.0, 1.0, 1.0), action_scale_gap=1.0, substeps=None, shape=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                 action_dim1=0, action_scale1=(1.0, 1.0, 1.0), action_scale_w1=(1.0, 1.0, 1.0)):
        P = len(kinds)
        assert kinds[0] == CHOPSTICKS and all(k in (0, 1, BOX, CYLINDER, TORUS) for k in kinds[1:])
        assert action_dim1 != 0 or all(k == 0 for k in kinds[1:])         # the parent's own condition where primitive 1 is unactuated
        PlbPrimTwin.__init__(self, conf, kinds=(1,) + tuple(0 if k == 0 else 1 for k in kinds[1:]), h=h, rot=((1, 0, 0, 0),) * P, mu=mu,
                             action_scale=action_scale, substeps=substeps)
        self.kin, self.action_dim, self.rot_state = tuple(kinds), 7, True
        self.action_scale_w = torch.tensor(action_scale_w, dtype=DT)
        self.action_scale_gap, self.min_gap = float(action_scale_gap), tuple(float(g) for g in min_gap)
        self.shape = [torch.tensor((tuple(sc) + (0.0,) * 3)[:3], dtype=DT) for sc in (tuple(shape) + ((0.0,) * 3,) * 2)[:max(P, 1)]]
        self._q0 = self._q1 = None
        self._gap = None
        self.gap_log = []
        self._two(7, action_dim1, action_scale1, action_scale_w1)

    def kinematics(self, pos, rot, gap, a):
        new_pos, new_rot, new_gap = PlbChopsticksTwin.kinematics(self, pos, rot, gap, a)
        new_pos, new_rot = self.move1(pos, rot, new_pos, new_rot, a)
        return new_pos, new_rot, new_gap


def kinematics_numpy(pos, rot, a_blk, scale, scale_w, S, lo, hi):
    """The base class's kinematics of ONE primitive, serially in NumPy, as the device's prologue thread runs it: pos [3], rot [4] (w, x, y, z),
    a_blk [3] or [6] = primitive's block of the RAW action row.  Returns the trajectories P [S+1,3], R [S+1,4]."""
    import numpy as np
    a = np.clip(np.asarray(a_blk, np.float64), -1.0, 1.0)
    v = a[:3] * np.asarray(scale) / S
    w = a[3:6] * np.asarray(scale_w) / S if a.shape[0] == 6 else np.zeros(3)
    n = np.sqrt((w * w).sum())
    dq = np.array([1.0, 0.0, 0.0, 0.0]) if n <= 1e-9 else np.concatenate([[np.cos(n / 2)], w / n * np.sin(n / 2)])
    P, R = [np.asarray(pos, np.float64)], [np.asarray(rot, np.float64)]
    for _ in range(S):
        q, r = dq, R[-1]                                                 # qmul(q, r) = Hamilton product q r, normalised (utils.py:19-27)
        out = np.array([q[0] * r[0] - q[1] * r[1] - q[2] * r[2] - q[3] * r[3],
                        q[0] * r[1] + q[1] * r[0] + q[2] * r[3] - q[3] * r[2],
                        q[0] * r[2] - q[1] * r[3] + q[2] * r[0] + q[3] * r[1],
                        q[0] * r[3] + q[1] * r[2] - q[2] * r[1] + q[3] * r[0]])
        R.append(out / np.sqrt((out * out).sum()))
        P.append(np.maximum(np.minimum(P[-1] + v, hi), lo))
    return np.stack(P), np.stack(R)
