"""Test infrastructure: the inputs tests/test_plb_two_hand_cpu.py and test_plb_two_hand_gpu.py share -- handles with BOTH primitives actuated
-- and the reference runs (torch.autograd through tests/plb_multi_twin.py) with the conditions that keep a comparison honest.

A case is a dict: the handle's description (kinds, radius, h, mu, shape, rot_state, chop, action_dim = A0, action_dim1, the scales, substeps,
upper_bound) and the inputs (x, v, C, F, prim [B,2,3], rot [B,2,4] | None, gap [B,2] | None, act [B,A0 + action_dim1], soft [B,2], E, nu, ys).
Every case is tests/plb_prim_twin.capsule_case(two=True): the rod cut from the torus sample with primitive 0 pressed into it at
y = 0.29 and primitive 1 at y = 0.12, three envs."""
from __future__ import annotations

import numpy as np
import torch

from oracle.twin.plb_twin import PlbConf
from tests.plb_chopsticks_twin import CHOPSTICKS, chop_case, honesty_chop
from tests.plb_multi_twin import PlbTwoHandChopsticksTwin, PlbTwoHandPrimTwin, PlbTwoHandShapeTwin
from tests.plb_prim_twin import capsule_case, honesty
from tests.plb_rot_twin import HEIGHT, MU, RADIUS, ROLL_SCALE
from tests.plb_shape_twin import BOX, SHAPES, honesty_shape

B = 3
TILT0 = np.array([0.9, 0.1, -0.3, 0.2]) / np.linalg.norm([0.9, 0.1, -0.3, 0.2])      # plb_rot_twin.ROT0, normalised
TILT1 = np.array([0.8, -0.3, 0.2, 0.4]) / np.linalg.norm([0.8, -0.3, 0.2, 0.4])      # primitive 1's
# what primitive 1 moves by in one step (its block times its scale), per env, and its angular block
MOVE1 = np.array([[0.003, -0.002, 0.0025], [-0.002, 0.003, -0.003], [0.0025, 0.002, 0.003]])
ANG0 = np.array([[0.3, -0.2, 0.25], [-0.4, 0.1, 0.2], [0.2, 0.3, -0.35]])             # plb_rot_twin.rot_case's
ANG1 = np.array([[-0.25, 0.3, 0.2], [0.35, -0.15, 0.3], [0.15, -0.3, 0.25]])
SCALE_W0, SCALE_W1 = (0.05, 0.05, 0.05), (0.04, 0.06, 0.03)
CAP1 = dict(radius=0.04, h=0.08, mu=0.5)                                              # a Capsule as primitive 1
SOFT3 = (666.0, 120.0, 80.0)                                                          # plb_shape_twin.SOFT: a thicker shell in envs 1 and 2


def _base(N, seed=0):
    x, v, Cm, F, prim, move0, E, nu, ys = capsule_case(B, N, seed=seed, two=True)
    return dict(N=N, x=x, v=v, C=Cm, F=F, prim=prim, E=E, nu=nu, ys=ys, move0=move0, rot=None, gap=None, soft=np.full((B, 2), 666.0),
                upper=(1.0, 1.0, 1.0), substeps=3, rot_state=False, chop=False, action_dim=3, action_dim1=3, scale=(1.0, 1.0, 1.0),
                scale_w=(1.0, 1.0, 1.0), scale1=(1.0, 1.0, 1.0), scale_w1=(1.0, 1.0, 1.0), scale_gap=1.0, min_gap=(0.0, 0.0),
                shape=((0.0,) * 3, (0.0,) * 3), const_rot=((1.0, 0.0, 0.0, 0.0),) * 2)


def _rots(tilts):
    rng = np.random.default_rng(1)
    r = np.stack([np.asarray(t)[None] + rng.normal(size=(B, 4)) * 0.01 for t in tilts], 1)      # deliberately NOT unit: rot[0] is used as given
    return r


def spheres(N):
    """1. Sphere + Sphere, three action dimensions each, unit scales, nine substeps: the one handle that runs both paths."""
    c = _base(N)
    c.update(kinds=(0, 0), radius=(0.025, 0.025), h=(0.0, 0.0), mu=(0.0, 0.0), substeps=9)
    c["act"] = np.concatenate([c["move0"], MOVE1], 1)
    return c


def spheres_clip_clamp(N=33):
    """2a. spheres(N) on both paths: one env's primitive-1 component y at 1.7 (outside the clip) and another env whose primitive 1 reaches
    upper_bound in z mid-step.  With the unit scales the persistent path needs, a clipped component is a move of 1 / substeps per substep, three
    cells: that env's primitive 1 gets softness 0 (a Sphere with softness 0 lets go, primitives.py:46-53) so the move drags nothing along, and
    upper_bound y is 3, so the position clamp NEVER engages in y: the cotangent of prim_pos_out reaches the clipped component through all nine
    substeps and only the clip's indicator makes it 0 (`reference` asserts that the same input just inside the clip has a nonzero cotangent
    there and another prim_pos_out; without the clip the end position would be y + 1.7).  Returns (case, env of the clamp, env of the clip)."""
    c = spheres(N)
    act, prim = c["act"].copy(), c["prim"]
    e = int(np.argmax(prim[:, 1, 2]))                                  # the primitive 1 with the largest z: the bound sits 0.5 mm above it
    k = (e + 1) % B
    act[k, 4] = 1.7
    c["soft"] = c["soft"].copy()
    c["soft"][k, 1] = 0.0
    hi_z = float(prim[e, 1, 2] + 0.0005)
    act[:, 2], act[:, 5] = -np.abs(act[:, 2]), -np.abs(act[:, 5])      # everything else moves away from that bound
    act[e, 5] = 0.004                                                  # 0.00044 per substep: inside in the first, outside from the second
    c.update(act=act, upper=(1.0, 3.0, hi_z))
    # strictly inside or outside, never at equality; and nothing but that primitive meets the bound
    S = c["substeps"]
    for b in range(B):
        for pi in range(2):
            z, step = prim[b, pi, 2], float(np.clip(act[b, 3 * pi + 2], -1, 1)) / S
            hit = False
            for _ in range(S):
                assert z + step != hi_z
                hit |= z + step > hi_z
                z = min(z + step, hi_z)
            assert hit == ((b, pi) == (e, 1)), (b, pi, hit)
    assert prim[k, 1, 1] + 1.0 < 3.0 and (prim[:, :, :2] + 0.01 < 1.0).all()      # no clamp in x or y anywhere
    return c, e, k


CLIP_SCALE1 = (0.004, 0.004, 0.004)


def clipped_of(c):
    """2b. c with primitive 1 on a small action_scale1, so that a clipped component is an ordinary move of 4 mm and the primitive stays IN
    CONTACT (softness as the case has it, the position clamp far away): env 1's first linear component of block 1 at -1.6 and, with six
    dimensions, env 2's second angular one at 1.7.  The other components move primitive 1 as they did.  Returns (case, the clipped (env,
    column) pairs): their cotangent is exactly 0 through the clip's indicator alone, which `reference` checks from the inside."""
    A0, d = c["action_dim"], dict(c)
    act = c["act"].copy()
    act[:, A0:A0 + 3] = c["act"][:, A0:A0 + 3] * np.array(c["scale1"]) / np.array(CLIP_SCALE1)
    assert np.abs(act[:, A0:A0 + 3]).max() < 1.0
    act[1, A0] = -1.6
    clipped = [(1, A0)]
    if c["action_dim1"] == 6:
        act[2, A0 + 4] = 1.7
        clipped.append((2, A0 + 4))
    d.update(scale1=CLIP_SCALE1, act=act)
    return d, tuple(clipped)


def capsule_box(N):
    """3. Constant orientation: a Capsule (scale 0.01) and a Box (another scale), three action dimensions each."""
    c = _base(N)
    c.update(kinds=(1, BOX), radius=(RADIUS, 0.0), h=(HEIGHT, 0.0), mu=(MU, 0.4), shape=((0.0,) * 3, SHAPES[BOX]), scale=(0.01, 0.01, 0.01),
             scale1=(0.008, 0.012, 0.01), const_rot=(tuple(TILT0), tuple(TILT1)), soft=np.array(SOFT3)[:, None].repeat(2, 1))
    c["act"] = np.concatenate([c["move0"] / np.array(c["scale"]), MOVE1 / np.array(c["scale1"])], 1)
    return c


def rot_pair(N, which):
    """4. rot_state: "cap6_cap6", "pin_cap3", "cap6_sph3", "cap6_box6"."""
    c = _base(N)
    c.update(rot_state=True, rot=_rots((TILT0, TILT1)), soft=np.array(SOFT3)[:, None].repeat(2, 1))
    first = np.concatenate([c["move0"], ANG0], 1)
    if which == "cap6_cap6":
        c.update(kinds=(1, 1), radius=(RADIUS, CAP1["radius"]), h=(HEIGHT, CAP1["h"]), mu=(MU, CAP1["mu"]), action_dim=6, action_dim1=6,
                 scale_w=SCALE_W0, scale_w1=SCALE_W1, act=np.concatenate([first, MOVE1, ANG1], 1))
    elif which == "pin_cap3":
        pin = np.array([[0.3, -0.2, -0.004], [-0.25, 0.3, -0.003], [0.2, 0.15, -0.0035]])       # plb_rot_twin.rot_case(rolling=True)
        c.update(kinds=(2, 1), radius=(RADIUS, CAP1["radius"]), h=(HEIGHT, CAP1["h"]), mu=(MU, CAP1["mu"]), action_dim=3, action_dim1=3,
                 scale=ROLL_SCALE, act=np.concatenate([pin, MOVE1], 1))
    elif which == "cap6_sph3":
        c.update(kinds=(1, 0), radius=(RADIUS, 0.025), h=(HEIGHT, 0.0), mu=(MU, 0.0), action_dim=6, action_dim1=3, scale_w=SCALE_W0,
                 act=np.concatenate([first, MOVE1], 1))
    elif which == "cap6_box6":
        c.update(kinds=(1, BOX), radius=(RADIUS, 0.0), h=(HEIGHT, 0.0), mu=(MU, 0.4), shape=((0.0,) * 3, SHAPES[BOX]), action_dim=6,
                 action_dim1=6, scale_w=SCALE_W0, scale_w1=SCALE_W1, act=np.concatenate([first, MOVE1, ANG1], 1))
    else:
        raise KeyError(which)
    return c


def chop_sphere(N):
    """5. Chopsticks (seven action dimensions) + an actuated sticky Sphere (three): A = 10."""
    (x, v, Cm, F, prim, rot, gap, act, E, nu, ys), soft, kw = chop_case(B, N, two=True)
    gap = gap.copy()
    gap[2, 0] = 0.075        # chop_case's env 2 starts AT minimal_gap (its g_action[6] is 0 by design); here every action component has to count:
    c = _base(N)             # gap_vel = 0.004 takes it 0.075 -> 0.071 -> 0.067 -> 0.063, never clamped
    c.update(x=x, v=v, C=Cm, F=F, prim=prim, rot=rot, gap=gap, E=E, nu=nu, ys=ys, soft=soft, rot_state=True, chop=True, kinds=kw["kinds"],
             radius=(0.03, 0.025), h=kw["h"], mu=(0.9, 0.0), min_gap=kw["min_gap"], scale_w=kw["action_scale_w"], scale_gap=kw["action_scale_gap"],
             action_dim=7, act=np.concatenate([act, MOVE1], 1))
    return c


def chop_capsule(N):
    """5b. Chopsticks + a Capsule with six action dimensions (A = 13): a general primitive 1 beside the Chopsticks (the GEN 5 kernels)."""
    c = chop_sphere(N)
    rot = c["rot"].copy()
    rot[:, 1] = _rots((TILT0, TILT1))[:, 1]
    c.update(kinds=(CHOPSTICKS, 1), radius=(0.03, CAP1["radius"]), h=(c["h"][0], CAP1["h"]), mu=(0.9, CAP1["mu"]), rot=rot, action_dim1=6,
             scale_w1=SCALE_W1, act=np.concatenate([c["act"], ANG1], 1))
    return c


def legacy_of(c):
    """The same handle with primitive 1 unactuated (action_dim1 = 0) and primitive 0's block alone: what the parent twins and today's handles take."""
    d = dict(c)
    d.update(action_dim1=0, act=np.ascontiguousarray(c["act"][:, :c["action_dim"]]))
    return d


def zero_block_of(c):
    d = dict(c)
    act = c["act"].copy()
    act[:, c["action_dim"]:] = 0.0
    d["act"] = act
    return d


# ---- the twin of a case, its step, the reference run ---------------------------------------------------------------------------------
def twin_of(c, substeps=None):
    conf = PlbConf(quality=0.5, n_particles=c["N"], radius=tuple(c["radius"]), upper_bound=tuple(c["upper"]))
    S = c["substeps"] if substeps is None else substeps
    two = dict(action_dim1=c["action_dim1"], action_scale1=c["scale1"])
    if c["chop"]:
        return PlbTwoHandChopsticksTwin(conf, kinds=c["kinds"], h=c["h"], mu=c["mu"], min_gap=c["min_gap"], action_scale=c["scale"],
                                        action_scale_w=c["scale_w"], action_scale_gap=c["scale_gap"], substeps=S, shape=c["shape"], action_scale_w1=c["scale_w1"], **two)
    if all(k in (0, 1) for k in c["kinds"]) and not c["rot_state"]:
        return PlbTwoHandPrimTwin(conf, kinds=c["kinds"], h=c["h"], rot=c["const_rot"], mu=c["mu"], action_scale=c["scale"], substeps=S, **two)
    return PlbTwoHandShapeTwin(conf, kinds=c["kinds"], shape=c["shape"], h=c["h"], rot=c["const_rot"], mu=c["mu"], action_scale=c["scale"],
                               action_scale_w=c["scale_w"], action_dim=c["action_dim"], substeps=S, rot_state=c["rot_state"],
                               action_scale_w1=c["scale_w1"], **two)


def state_names(c):
    return ("x", "v", "C", "F", "prim") + (("rot",) if c["rot_state"] else ()) + (("gap",) if c["chop"] else ())


def T(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def twin_step(tw, c, leaves):
    """tw.step on a dict of tensors (the case's names); returns the outputs in state_names order."""
    st = [leaves[k] for k in state_names(c)]
    fric = leaves.get("fric", T(np.full(B, tw.c.ground_friction)))
    return tw.step(*st, leaves["act"], T(c["soft"]), leaves["E"], leaves["nu"], leaves["ys"], fric)


def check_honesty(tw, c):
    """plb_prim_twin.honesty or its shape / chop variant wherever a general primitive is in contact (a Sphere-only handle has no such arm)."""
    if c["chop"]:
        return honesty_chop(tw)
    if any(k >= BOX for k in c["kinds"]):
        return honesty_shape(tw)
    if any(k != 0 for k in c["kinds"]):
        return honesty(tw)
    return None


def reference(c, seed=9, zero_ok=()):
    """autograd through the twin with random cotangents on every output.  Asserts honesty and that the gradient of BOTH action blocks has no
    zero component in any env (zero_ok: the (env, column) pairs the case puts outside the clip on purpose: those must be exactly 0).
    Returns (values, outputs, cotangents, grads, twin)."""
    torch.set_num_threads(8)
    names = state_names(c)
    rng = np.random.default_rng(seed)
    w = [rng.normal(size=np.shape(c[k])) for k in names]
    tw = twin_of(c)
    values = {k: c[k] for k in names + ("act", "E", "nu", "ys")}
    leaves = {k: T(a, True) for k, a in values.items()}
    leaves["fric"] = T(np.full(B, tw.c.ground_friction), True)
    out = twin_step(tw, c, leaves)
    check_honesty(tw, c)
    sum((o * T(wi)).sum() for o, wi in zip(out, w)).backward()
    grads = {k: (t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
    ga = grads["act"].copy()
    assert ga.shape == (B, c["action_dim"] + c["action_dim1"]) and np.isfinite(ga).all()
    for b, col in zero_ok:
        assert ga[b, col] == 0.0
        ga[b, col] = 1.0
    assert np.abs(ga).min() > 0, ga
    if zero_ok:
        # the zeros above are the clip's doing and nothing else's: the same input with those components just INSIDE the clip sends a nonzero
        # cotangent to each of them and moves primitive 1 elsewhere (so a kernel that ignored the clip would miss both the forward and the bar)
        inside = c["act"].copy()
        for b, col in zero_ok:
            assert abs(c["act"][b, col]) > 1.0
            inside[b, col] = 0.999 * np.sign(c["act"][b, col])
        c2 = dict(c, act=inside)
        l2 = {k: T(c2[k], k == "act") for k in names + ("act", "E", "nu", "ys")}
        out2 = twin_step(twin_of(c2), c2, l2)
        sum((o * T(wi)).sum() for o, wi in zip(out2, w)).backward()
        moved = sum(float((a.detach() - T(b_)).abs().max()) for a, b_ in zip(out2[4:], [o.detach().numpy() for o in out[4:]]))
        assert all(l2["act"].grad[b, col] != 0.0 for b, col in zero_ok) and moved > 0, (l2["act"].grad, moved)
    return values, [o.detach().numpy() for o in out], w, grads, tw
