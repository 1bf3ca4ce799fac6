"""Both primitives actuated on the PLB f64 path, on the GPU: ud_plb_conf.action_dim1 / action_scale1 / action_scale_w1 and the [B, A] action row
(A = A0 + action_dim1, primitive 1's block in columns A0 .. A - 1) through ud_plb_step_fwd / _bwd and their _rot / _gap siblings, on both
kernel paths, against tests/plb_multi_twin.py and torch.autograd through it.  PARITY UNPINNED by reference data (taichi is absent, the
reference ships no two-handed task): the twin is the specification.  Bars, the project's own: forward 1e-9 relative on x, v, C, F; prim_pos /
prim_rot / prim_gap 1e-14 absolute; every gradient 1e-6 relative (the action row also block by block); losses 1e-11 / 1e-9.  Three envs,
n_grid 32, N in {33, 300}, 3 substeps (9 on the Sphere-only handles).  Every reference run (tests/plb_two_hand_cases.reference) asserts the
honesty conditions of the primitive twins where a general primitive is in contact and that the gradient of BOTH action blocks has no zero
component in any env."""
import ctypes as C
import functools
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf
from tests import plb_two_hand_cases as K
from tests.plb_multi_twin import PlbTwoHandPrimTwin, PlbTwoHandRotTwin, PlbTwoHandShapeTwin
from tests.plb_shape_twin import BOX, SHAPES

pytestmark = pytest.mark.gpu
B = K.B


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _sim(c, path=0, nb=B, action_dim1=None):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles, cfg.path, cfg.upper_bound = 0.5, c["substeps"], c["N"], path, tuple(c["upper"])
    cfg.prim_radius, cfg.prim_kind, cfg.prim_h, cfg.prim_friction = tuple(c["radius"]), tuple(c["kinds"]), tuple(c["h"]), tuple(c["mu"])
    cfg.prim_rot, cfg.prim_shape = tuple(tuple(q) for q in c["const_rot"]), tuple(tuple(s) for s in c["shape"])
    cfg.prim_init_pos = ((0.5, 0.3, 0.5), (0.5, 0.12, 0.5))
    cfg.rot_state, cfg.action_dim = c["rot_state"], c["action_dim"]
    cfg.action_scale, cfg.action_scale_w, cfg.action_scale_gap, cfg.prim_min_gap = c["scale"], c["scale_w"], c["scale_gap"], tuple(c["min_gap"])
    cfg.action_dim1 = c["action_dim1"] if action_dim1 is None else action_dim1
    cfg.action_scale1, cfg.action_scale_w1 = c["scale1"], c["scale_w1"]
    sim = PlbSimulator(cfg, batch_size=nb)
    assert sim.n_grid == 32 and sim.substeps == c["substeps"] and sim.action_dim == c["action_dim"] + cfg.action_dim1
    assert sim.action_dims == (0, c["action_dim"], sim.action_dim)
    return sim


def _dev(sim, a, r=False):
    return torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)


def _state(sim, c, hl):
    return sim.reset()._replace(x=hl["x"], v=hl["v"], C=hl["C"], F=hl["F"], prim_pos=hl["prim"], prim_rot=hl.get("rot"), prim_gap=hl.get("gap"),
                                softness=_dev(sim, c["soft"]), E=hl["E"], nu=hl["nu"], yield_stress=hl["ys"])


def _outputs(c, s1):
    return (s1.x, s1.v, s1.C, s1.F, s1.prim_pos) + ((s1.prim_rot,) if c["rot_state"] else ()) + ((s1.prim_gap,) if c["chop"] else ())


def _check_forward(c, res, out):
    for name, t, o in zip(K.state_names(c), res, out):
        got = t.detach().cpu().numpy()
        if name in "xvCF":
            print(name, _rel(got, o))
            assert np.isfinite(got).all() and _rel(got, o) < 1e-9, (name, _rel(got, o))
        else:
            print(name, np.abs(got - o).max())
            np.testing.assert_allclose(got, o, rtol=0, atol=1e-14, err_msg=name)


def _check(sim, c, ref, bar=1e-6):
    """Forward and full adjoint of one step against the reference run: every leaf, the action row also block by block, the start rotation
    also primitive by primitive, the ground friction."""
    values, out, w, grads, _ = ref
    hl = {k: _dev(sim, a, True) for k, a in values.items()}
    s1 = sim.step(_state(sim, c, hl), hl["act"])
    res = _outputs(c, s1)
    _check_forward(c, res, out)
    sim.ground_friction_grad = None
    sum((t * _dev(sim, wi)).sum() for t, wi in zip(res, w)).backward()
    sim.check_status()
    A0 = c["action_dim"]
    for name in values:
        got = hl[name].grad.cpu().numpy()
        print(name, _rel(got, grads[name]))
        assert got.shape == grads[name].shape and np.isfinite(got).all() and _rel(got, grads[name]) < bar, (name, _rel(got, grads[name]))
    ga = hl["act"].grad.cpu().numpy()
    for blk, sl in (("block 0", slice(0, A0)), ("block 1", slice(A0, None))):
        print(blk, _rel(ga[:, sl], grads["act"][:, sl]))
        assert _rel(ga[:, sl], grads["act"][:, sl]) < bar, (blk, _rel(ga[:, sl], grads["act"][:, sl]))
    for pi in range(2):
        for name in ("prim",) + (("rot",) if c["rot_state"] else ()):
            got = hl[name].grad.cpu().numpy()[:, pi]
            assert np.abs(grads[name][:, pi]).max() > 0 and _rel(got, grads[name][:, pi]) < bar, (name, pi, _rel(got, grads[name][:, pi]))
    gfr = sim.ground_friction_grad.cpu().numpy()
    assert np.abs(grads["fric"]).max() > 0 and _rel(gfr, grads["fric"]) < bar, (gfr, grads["fric"])
    return hl


# ---- 1. Sphere + Sphere on both paths ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_spheres(N):
    c = K.spheres(N)
    return c, K.reference(c)


@pytest.mark.parametrize("path", [2, 1])
@pytest.mark.parametrize("N", [33, 300])
def test_two_spheres_forward_and_adjoint(N, path):
    """Both Spheres on the rod, three action dimensions each, unit scales: the persistent launch (path 2) and the multi-kernel path."""
    c, ref = _ref_spheres(N)
    sim = _sim(c, path=path)
    assert sim.launch_plan() == path
    _check(sim, c, ref)


# ---- 2. clip and clamp arms of primitive 1 ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_clip_clamp():
    c, e, k = K.spheres_clip_clamp(33)
    ref = K.reference(c, zero_ok=((k, 4),))
    assert ref[1][4][e, 1, 2] == c["upper"][2]                          # primitive 1 of env e reached the bound
    return c, e, k, ref


@pytest.mark.parametrize("path", [2, 1])
def test_primitive_1_clip_and_clamp(path):
    """Both paths, unit scales.  One env with the y component of primitive 1's block at 1.7: prim_pos_out is y + 1 (y + 1.7 without the
    clip) and its g_action is exactly 0.0 through the clip's indicator ALONE -- upper_bound y is 3, so no position clamp stands between
    prim_pos_out's cotangent and that component, and the reference run asserts that just inside the clip the cotangent is not 0.  That
    primitive has softness 0 (a clipped unit-scale move is three cells per substep), so the other two components of its block get their
    nonzero cotangents from prim_pos_out through nine unclamped substeps.  Another env whose primitive 1 reaches upper_bound in z in the
    second of nine substeps (strictly inside before, strictly outside after: asserted by the case): its cotangent counts the first substep
    only.  The clip with the primitive IN CONTACT: test_primitive_1_clip_in_contact below."""
    c, e, k, ref = _ref_clip_clamp()
    sim = _sim(c, path=path)
    assert sim.launch_plan() == path
    hl = _check(sim, c, ref)
    ga = hl["act"].grad.cpu().numpy()
    assert ga[k, 4] == 0.0 and np.abs(np.delete(ga[k], 4)).min() > 0
    assert float(hl["act"].grad[e, 5]) != 0.0                            # the substep before the clamp still counts


CLIPPED = {"spheres": lambda: K.spheres(33), "cap6_cap6": lambda: K.rot_pair(33, "cap6_cap6"), "pin_cap3": lambda: K.rot_pair(33, "pin_cap3"),
           "chop_sphere": lambda: K.chop_sphere(33), "chop_capsule": lambda: K.chop_capsule(33)}


@functools.lru_cache(maxsize=None)
def _ref_clipped(name):
    c, clipped = K.clipped_of(CLIPPED[name]())
    return c, clipped, K.reference(c, zero_ok=clipped)


@pytest.mark.parametrize("name", sorted(CLIPPED))
def test_primitive_1_clip_in_contact(name):
    """The clip of primitive 1's block on the plain, _rot and _gap families with the primitive in contact (multi-kernel path: action_scale1 =
    0.004, so a clipped component is a 4 mm move): a linear component at -1.6 and, with six dimensions, an angular one at 1.7.  Forward at
    the bars (a kernel that did not clip would move or turn the primitive 1.6 / 1.7 times as far), those components' g_action exactly 0.0,
    every other component nonzero and at the bar; the reference run asserts that just inside the clip they are not 0."""
    c, clipped, ref = _ref_clipped(name)
    sim = _sim(c)
    assert sim.launch_plan() == 1
    hl = _check(sim, c, ref)
    ga = hl["act"].grad.cpu().numpy()
    for b, col in clipped:
        assert ga[b, col] == 0.0, (b, col, ga[b, col])
        ga[b, col] = 1.0
    assert np.abs(ga).min() > 0


# ---- 3. constant orientation: Capsule + Box ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_capsule_box(N):
    c = K.capsule_box(N)
    return c, K.reference(c)


@pytest.mark.parametrize("N", [33, 300])
def test_capsule_and_box_constant_orientation(N):
    c, ref = _ref_capsule_box(N)
    sim = _sim(c)
    assert sim.launch_plan() == 1
    _check(sim, c, ref)


# ---- 4. rot_state -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_rot(N, which):
    c = K.rot_pair(N, which)
    ref = K.reference(c)
    if c["kinds"][1] != 0:
        assert np.abs(ref[3]["rot"][:, 1]).min() > 0                    # the start rotation of a general primitive 1 counts in every component
    return c, ref


@pytest.mark.parametrize("which", ["cap6_cap6", "pin_cap3", "cap6_sph3", "cap6_box6"])
@pytest.mark.parametrize("N", [33, 300])
def test_rot_state_pairs(N, which):
    """Capsule 6 + Capsule 6 (different action_scale_w1; g_prim_rot0 of both), RollingPin + Capsule 3, Capsule 6 + Sphere 3, Capsule 6 + Box 6:
    kind, rotation and rotation cotangent of primitive 1 through the grid op and its adjoint."""
    c, ref = _ref_rot(N, which)
    sim = _sim(c)
    assert sim.launch_plan() == 1
    _check(sim, c, ref)


# ---- 5. Chopsticks + Sphere -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref_chop(N):
    c = K.chop_sphere(N)
    ref = K.reference(c)
    assert np.abs(ref[3]["gap"][:, 0]).min() > 0
    return c, ref


@pytest.mark.parametrize("N", [33, 300])
def test_chopsticks_and_sphere(N):
    """A = 10: the Chopsticks' seven, then the Sphere's three.  The gap leaf and both blocks."""
    c, ref = _ref_chop(N)
    sim = _sim(c)
    assert sim.action_dim == 10 and sim.launch_plan() == 1
    hl = _check(sim, c, ref)
    assert _rel(hl["gap"].grad.cpu().numpy()[:, 0], ref[3]["gap"][:, 0]) < 1e-6


@functools.lru_cache(maxsize=None)
def _ref_chop_capsule(N):
    c = K.chop_capsule(N)
    ref = K.reference(c)
    assert np.abs(ref[3]["gap"][:, 0]).min() > 0 and np.abs(ref[3]["rot"][:, 1]).min() > 0
    return c, ref


@pytest.mark.parametrize("N", [33, 300])
def test_chopsticks_and_capsule(N):
    """A = 13: a general primitive 1 (a Capsule with six action dimensions) beside the Chopsticks, through the GEN 5 grid op and its adjoint."""
    c, ref = _ref_chop_capsule(N)
    sim = _sim(c)
    assert sim.action_dim == 13 and sim.launch_plan() == 1
    _check(sim, c, ref)


# ---- 6. losses on a rot_state handle with a general primitive 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("soft_contact", [True, False])
@pytest.mark.parametrize("second", ["capsule", "box"])
def test_rot_state_loss_with_a_general_primitive_1(second, soft_contact):
    """tests/test_plb_rot_gpu.py's contact-loss case with a Capsule (or a Box) in place of primitive 1's Sphere: loss, parts (1e-11), g_x,
    g_prim_pos, g_prim_rot of BOTH primitives (1e-9)."""
    from oracle.twin.plb_twin import torus_particles
    nb, N = 2, 300
    radius, h = (0.03, 0.035), (0.06, 0.07)
    conf = PlbConf(quality=0.5, n_particles=N, radius=radius)
    if second == "capsule":
        kinds, shape = (1, 1), ((0.0,) * 3,) * 2
        tw = PlbTwoHandRotTwin(conf, kinds=kinds, h=h, action_dim=6, action_dim1=3)
    else:
        kinds, shape = (1, BOX), ((0.0,) * 3, SHAPES[BOX])
        tw = PlbTwoHandShapeTwin(conf, kinds=kinds, shape=shape, h=h, action_dim=6, rot_state=True, action_dim1=3)
    rng = np.random.default_rng(2)
    x = np.stack([torus_particles(1000)[:N], torus_particles(1000)[:N] + rng.normal(size=(N, 3)) * 0.003])
    prim = np.array([[[0.44, 0.28, 0.5], [0.60, 0.42, 0.45]], [[0.5, 0.35, 0.56], [0.40, 0.12, 0.58]]])
    rot = np.array([[[0.9, 0.1, -0.3, 0.2], [0.8, -0.3, 0.2, 0.4]], [[0.7, -0.4, 0.2, 0.5], [0.6, 0.5, -0.4, 0.3]]]) * np.array([[[1.03], [0.97]], [[0.96], [1.02]]])
    td = tw.grid_mass(torch.tensor((torus_particles(1000)[:N] + np.array([0.004, -0.01, 0.0]))[None]))[0]
    ts = torch.tensor(rng.normal(size=tw.c.n_grid ** 3))
    wts = (3.0, 0.7, 1.3)
    tx, tp, tr = K.T(x, True), K.T(prim, True), K.T(rot, True)
    total, parts = tw.loss(tx, tp, td, ts, wts, soft_contact=soft_contact, prim_rot=tr)
    gl = np.array([1.0, -2.5])
    (total * K.T(gl)).sum().backward()
    for pi in range(2):
        assert np.abs(tp.grad.numpy()[:, pi]).max() > 0 and np.abs(tr.grad.numpy()[:, pi]).min() > 0, pi
        d = tw.sdf_q(pi, K.T(x), K.T(prim)[:, pi, None, :], K.T(rot)[:, pi])
        assert int((d > 0).sum()) > 100 and float(d.abs().min()) > 1e-9   # nearly every particle's max(sdf, 0) is in its open arm, none at the kink
        assert pi == 0 or bool((d > 0).all())                              # primitive 1 stands clear of the rod: the hard minimum is not the clamped 0
    c = dict(K._base(N), kinds=kinds, radius=radius, h=h, mu=(0.0, 0.0), shape=shape, rot_state=True, action_dim=6, action_dim1=3)
    sim = _sim(c, nb=nb)
    hx, hp, hr = _dev(sim, x, True), _dev(sim, prim, True), _dev(sim, rot, True)
    st = sim.reset()._replace(x=hx, prim_pos=hp, prim_rot=hr)
    hloss, hparts = sim.compute_loss(st, td.numpy(), ts.numpy(), wts, soft_contact)
    assert _rel(hloss.detach().cpu().numpy(), total.detach().numpy()) < 1e-11
    assert _rel(hparts.cpu().numpy(), parts.detach().numpy()) < 1e-11
    (hloss * _dev(sim, gl)).sum().backward()
    for name, got, want in (("x", hx, tx), ("prim", hp, tp), ("rot", hr, tr)):
        print(name, _rel(got.grad.cpu().numpy(), want.grad.numpy()))
        assert _rel(got.grad.cpu().numpy(), want.grad.numpy()) < 1e-9, name
    assert _rel(hr.grad.cpu().numpy()[:, 1], tr.grad.numpy()[:, 1]) < 1e-9


# ---- 7. a zero block is the legacy handle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,path", [("spheres", 2), ("spheres", 1), ("cap6_sph3", 1), ("chop", 1)])
def test_zero_block_is_the_legacy_handle(which, path):
    """The same inputs on a handle with action_dim1 = 0 (action [B, A0]) and on one with action_dim1 = 3 and a zero block: prim_pos out
    (prim_rot, prim_gap) bit-equal; the particle state within 1e-9 of the legacy twin on both (summation order forbids bit equality)."""
    torch.set_num_threads(8)
    c = {"spheres": K.spheres, "chop": K.chop_sphere}.get(which, lambda N: K.rot_pair(N, which))(33)
    zero, legacy = K.zero_block_of(c), K.legacy_of(c)
    tw = K.twin_of(legacy)
    with torch.no_grad():
        ref = K.twin_step(tw, legacy, {k: K.T(legacy[k]) for k in K.state_names(c) + ("act", "E", "nu", "ys")})
    ref = [o.numpy() for o in ref]
    outs = []
    for case in (legacy, zero):
        sim = _sim(case, path=path)
        assert sim.launch_plan() == path and sim.action_dim == case["act"].shape[1]
        hl = {k: _dev(sim, case[k]) for k in K.state_names(c) + ("act", "E", "nu", "ys")}
        res = _outputs(c, sim.step(_state(sim, case, hl), hl["act"]))
        sim.check_status()
        _check_forward(c, res, ref)
        outs.append([t.cpu().numpy() for t in res])
    for name, a, b in list(zip(K.state_names(c), *outs))[4:]:
        assert np.array_equal(a, b), name
    assert np.abs(outs[0][4] - c["prim"]).max() > 0


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def _header_codes():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidom_hip.h")).read()
    return {k: int(val) for k, val in re.findall(r"UD_ERR_(\w+)\s*=\s*(-?\d+)", src)}


UD_ERR = _header_codes()


def _create(**over):
    """ud_plb_create on a conf of two Capsule-sized primitives with `over` on top; *out starts as a sentinel.  Returns (code, *out, message)."""
    from unidom_amd import _lib
    L = _lib.lib()
    d3 = lambda *a: (C.c_double * 3)(*a)
    kw = dict(n_particles=33, n_grid=32, substeps=3, dt=2e-4, gravity=d3(0.0, -0.4, 0.0), ground_friction=0.5, n_primitives=2,
              radius=(C.c_double * 2)(0.05, 0.04), lower_bound=d3(0.0, 0.0, 0.0), upper_bound=d3(1.0, 1.0, 1.0), max_envs=1, path=1,
              prim_kind=(C.c_int * 2)(1, 0), capsule_h=(C.c_double * 2)(0.12, 0.08), min_gap=(C.c_double * 2)(0.06, 0.0))
    kw.update(over)
    conf = _lib.ud_plb_conf(**kw)
    out = C.c_void_p(0x5EED)
    code = int(L.ud_plb_create(C.byref(conf), C.byref(out)))
    msg = L.ud_last_error().decode() if code != 0 else ""
    if code == 0:
        L.ud_plb_destroy(out)
    return code, out.value, msg


def test_refusals_name_their_field_and_leave_no_handle():
    kinds = lambda a, b: (C.c_int * 2)(a, b)
    INVALID, UNSUPPORTED = UD_ERR["INVALID"], UD_ERR["UNSUPPORTED"]
    cases = [
        (dict(action_dim1=6), INVALID, "action_dim1"),                                                   # (v, w) without rot_state
        (dict(action_dim1=3, n_primitives=1), INVALID, "action_dim1"),
        (dict(action_dim1=4), INVALID, "action_dim1"),
        (dict(action_dim1=-3), INVALID, "action_dim1"),
        (dict(action_dim1=3, rot_state=1, action_dim=6, prim_kind=kinds(1, 2)), UNSUPPORTED, "prim_kind[1]"),   # a RollingPin stays primitive 0
        (dict(action_dim1=3, rot_state=1, action_dim=6, prim_kind=kinds(1, 6)), UNSUPPORTED, "prim_kind[1]"),   # so does a Chopsticks
        (dict(action_dim1=3, prim_kind=kinds(1, 2)), INVALID, "prim_kind[1]"),                            # ... and without rot_state neither exists
        (dict(action_dim1=0, rot_state=1, action_dim=6, prim_kind=kinds(1, 1)), UNSUPPORTED, "primitive 1 is unactuated"),   # today's refusal, unchanged
        (dict(action_dim1=3, rot_state=1, action_dim=6, prim_kind=kinds(1, 1), path=2), UNSUPPORTED, "path"),
    ]
    for over, code, word in cases:
        got, out, msg = _create(**over)
        assert got == code and out == 0x5EED and word in msg, (over, got, out, msg)
    # what the refusals stand next to is accepted
    for over in (dict(action_dim1=3), dict(action_dim1=6, rot_state=1, action_dim=6, prim_kind=kinds(1, 1)),
                 dict(action_dim1=3, rot_state=1, action_dim=3, prim_kind=kinds(2, 1))):
        got, out, msg = _create(**over)
        assert got == 0 and out not in (None, 0x5EED), (over, got, msg)


# ---- 9. top of the stack ----------------------------------------------------------------------------------------------------------------
def _bimanual(nb=2):
    from unidom_amd.engine.plb_simulator import BimanualConf, PlbSimulator
    cfg = BimanualConf()
    cfg.n_particles, cfg.quality = 300, 0.5
    sim = PlbSimulator(cfg, batch_size=nb)
    assert (sim.n_grid, sim.substeps, sim.action_dim, sim.action_dims) == (32, 9, 6, (0, 3, 6)) and sim.launch_plan() == 2
    return cfg, sim


def test_solver_gradient_on_the_bimanual_task():
    """Solver.forward on BimanualConf cut to N = 300, n_grid 32: the action gradient [H = 2, B, 6] through two chained steps plus compute_loss
    against autograd through the twin (which applies the 0.005 scales itself, where the simulator applies them on the host), 1e-6."""
    from unidom_amd.algorithms.plb_solver import Solver, make_goal
    from unidom_amd.engine.plb_losses import PlbLoss
    torch.set_num_threads(8)
    nb, H, wts = 2, 2, (1.0, 1.0, 1.0)
    cfg, sim = _bimanual(nb)
    push = torch.tensor([[-0.6, 0.0, 0.0, 0.6, 0.0, 0.0]] * 3, dtype=torch.float64, device=sim.device)
    loss = PlbLoss(sim, weights=wts, soft_contact=True).load_target_density(make_goal(sim, push))
    solver = Solver(sim, loss, horizon=H, n_iters=1, softness=666.0)
    actions = np.random.default_rng(3).uniform(-1, 1, size=(H, nb, 6)) * 0.6
    state0 = solver.start_state()
    total, grad, _ = solver.forward(state0, _dev(sim, actions))
    sim.check_status()
    tw = PlbTwoHandPrimTwin(PlbConf(quality=0.5, n_particles=300, radius=cfg.prim_radius), kinds=(0, 0), action_scale=cfg.action_scale,
                            action_dim1=3, action_scale1=cfg.action_scale1)
    assert tw.S == 9
    td, ts = loss.target_density.detach().cpu().reshape(-1), loss.target_sdf.detach().cpu().reshape(-1)
    cpu = lambda t: t.detach().cpu()
    x, v, Cm, F, p = (cpu(t) for t in (state0.x, state0.v, state0.C, state0.F, state0.prim_pos))
    a = K.T(actions, True)
    ref = 0.0
    for t in range(H):
        x, v, Cm, F, p = tw.step(x, v, Cm, F, p, a[t], cpu(state0.softness), cpu(state0.E), cpu(state0.nu), cpu(state0.yield_stress),
                                 torch.full((nb,), float(cfg.ground_friction), dtype=torch.float64))
        ref = ref + tw.loss(x, p, td, ts, wts, soft_contact=True)[0].sum()
    ref.backward()
    want, got = a.grad.numpy(), grad.cpu().numpy()
    assert got.shape == (H, nb, 6) and np.abs(want).min() > 0             # both blocks, every env, every step
    assert abs(float(total) - float(ref.detach())) < 1e-9 * abs(float(ref.detach()))
    for name, sl in (("all", slice(None)), ("block 0", slice(0, 3)), ("block 1", slice(3, 6))):
        print(name, _rel(got[..., sl], want[..., sl]))
        assert _rel(got[..., sl], want[..., sl]) < 1e-6, (name, _rel(got[..., sl], want[..., sl]))


def test_policy_acts_on_both_primitives():
    """PlbPolicy sizes its last layer from sim.action_dim = A: act returns [B, 6] and agrees with tests/plb_policy_twin.py inside the
    forward bound tests/test_plb_policy_gpu.py derives (no relu pre-activation and no clamp input within its bound of the kink)."""
    from tests import plb_policy_twin as ptw
    from tests.test_plb_policy_gpu import forward_bounds, kink_margins
    from unidom_amd.engine.plb_policy import PlbPolicy, policy_dims
    nb = 2
    cfg, sim = _bimanual(nb)
    pol = PlbPolicy(sim, hidden_dims=(16,), activation="relu", n_observed_particles=7).init_params(3)
    assert pol.dims[-1] == 6 == policy_dims(sim.n_particles, sim.n_primitive, sim.action_dim, (16,), 7)[2][-1]
    st = sim.reset()
    rng = np.random.default_rng(5)
    st = st._replace(v=_dev(sim, rng.normal(size=tuple(st.v.shape)) * 0.1))
    got = pol.act(st)
    assert tuple(got.shape) == (nb, 6)
    params = pol.get_params().cpu()
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * 2, dtype=torch.float64)[None].repeat(nb, 1, 1)
    want, hs = ptw.policy(st.x.cpu(), st.v.cpu(), st.prim_pos.cpu(), rot, params, pol.dims, pol.obs_step, pol.obs_num, "relu", 1.0)
    wb = ptw.split_params(params, pol.dims)
    e = forward_bounds(hs, wb)
    relu, clamp, _, _ = kink_margins(hs, wb, e, "relu")
    assert relu > 0 and clamp > 0, (relu, clamp)
    assert bool(((got.detach().cpu() - want).abs() <= e[-1]).all()), float(((got.detach().cpu() - want).abs() - e[-1]).max())
    assert float(want.abs().min()) > 0


@pytest.mark.parametrize("module", ["plb_solver", "plb_solver_nn"])
def test_solver_command_line_runs_the_bimanual_env(module):
    """python -m unidom_amd.algorithms.plb_solver[_nn] --env bimanual: exit 0, one finite loss per iteration."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "unidom_amd.algorithms." + module, "--env", "bimanual", "--iters", "2", "--horizon", "2",
                        "--num_envs", "2"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(m) for m in re.findall(r"loss (\S+)", r.stdout)]
    assert len(losses) == 2 and np.isfinite(losses).all(), r.stdout
