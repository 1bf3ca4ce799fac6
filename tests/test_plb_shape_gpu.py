"""Box, Cylinder and Torus primitives of the PLB f64 path on the GPU (prim_kind 3 / 4 / 5: the GEN = 3 / 4 instantiations behind the shape
layer of csrc/plb_prim.h) against the torch restatement tests/plb_shape_twin.py and its autograd, with a constant tilted orientation and
on rot_state with six action dimensions.  PARITY UNPINNED by reference data (taichi is absent): the restatement is the specification.
Bars: forward 1e-9 relative on x, v, C, F, prim_pos, prim_rot; every adjoint leaf 1e-6 of its max-norm; the contact loss 1e-11 / its
gradient 1e-9 (tests/test_plb_rot_gpu.py's); the kinematics alone 1e-12.  Every reference run asserts plb_shape_twin.honesty_shape: enough
occupied cells in both arms of the contact, none near a branch point of the contact or a kink of the shape, every region of the shape hit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf, torus_particles
from tests import plb_shape_twin as T

S, B = 3, 3                                   # n_grid 32: dx = 0.03125, the shapes span a few cells in every direction
KINDS = [T.BOX, T.CYLINDER, T.TORUS]
IDS = [T.NAMES[k] for k in KINDS]
MODES = ["const", "rot"]
R2 = (0.03, 0.03)                             # PlbConf.radius / prim_radius: what a Sphere or Capsule beside the shape takes, ignored by kinds 3 to 5


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _T(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def _twin(N, kw, mu=(0.7,), upper=(1.0, 1.0, 1.0), radius=R2, **more):
    P = len(kw["kinds"])
    return T.PlbShapeTwin(PlbConf(quality=0.5, n_particles=N, radius=radius[:P], upper_bound=upper), mu=mu, substeps=S, **{**kw, **more})


def _sim(N, nb, kw, mu=(0.7,), upper=(1.0, 1.0, 1.0), radius=R2, h=(0.0, 0.0), ckpt=None, lanes=0, path=0, shape=None, rot_state=None, rot=None):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    P = len(kw["kinds"])
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles, cfg.path, cfg.lanes, cfg.upper_bound = 0.5, S, N, path, lanes, upper
    cfg.prim_radius, cfg.prim_kind, cfg.prim_h, cfg.prim_friction = radius[:P], kw["kinds"], h[:P], mu
    cfg.prim_shape = kw.get("shape", ()) if shape is None else shape
    rot_state = kw.get("rot_state", False) if rot_state is None else rot_state
    cfg.prim_rot = ((1.0, 0.0, 0.0, 0.0),) * P if rot_state and rot is None else (kw.get("rot", ((1.0, 0.0, 0.0, 0.0),) * P) if rot is None else rot)
    cfg.rot_state, cfg.action_dim, cfg.action_scale_w = rot_state, kw.get("action_dim", 3), kw.get("action_scale_w", (1.0, 1.0, 1.0))
    cfg.prim_init_pos = ((0.5, 0.3, 0.5),) * P
    if ckpt is not None:
        cfg.grid_ckpt_cells = ckpt
    sim = PlbSimulator(cfg, batch_size=nb)
    assert sim.launch_plan() == 1 and sim.n_grid == 32 and sim.substeps == S          # the multi-kernel path
    return sim


def _dev(sim, a, r=False):
    return torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)


def _split(case, rot):
    """(x, v, C, F, prim, rot or None, act, E, nu, ys)"""
    return case if rot else case[:5] + (None,) + case[5:]


def _twin_step(tw, leaves, soft, rot):
    args = [leaves[k] for k in ("x", "v", "C", "F", "prim")] + ([leaves["rot"]] if rot else []) + [leaves["act"], _T(soft)] + \
        [leaves[k] for k in ("E", "nu", "ys", "fric")]
    return tw.step(*args)


def _state(sim, hl, soft, rot):
    s = sim.reset()._replace(x=hl["x"], v=hl["v"], C=hl["C"], F=hl["F"], prim_pos=hl["prim"], softness=_dev(sim, soft), E=hl["E"], nu=hl["nu"],
                             yield_stress=hl["ys"])
    return s._replace(prim_rot=hl["rot"]) if rot else s


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,mu", [(33, 0.7), (300, 0.0), (300, 0.7)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_hip_shape_forward_matches_the_twin(kind, mode, N, mu):
    """One step, three envs (softness 666, 120, 80).  N = 33 leaves most lanes of a wave idle, N = 300 spreads the touched cells over
    several waves and blocks."""
    torch.set_num_threads(8)
    rot = mode == "rot"
    case, soft, kw = T.shape_case(kind, B, N, rot)
    x, v, Cm, F, prim, q, act, E, nu, ys = _split(case, rot)
    tw = _twin(N, kw, mu=(mu,))
    vals = dict(x=x, v=v, C=Cm, F=F, prim=prim, rot=q, act=act, E=E, nu=nu, ys=ys, fric=np.full(B, tw.c.ground_friction))
    with torch.no_grad():
        ref = _twin_step(tw, {k: _T(a) for k, a in vals.items() if a is not None}, soft, rot)
    T.assert_regions(kind, [T.honesty_shape(tw)[1]])
    sim = _sim(N, B, kw, mu=(mu,))
    s = sim.step(_state(sim, {k: _dev(sim, a) for k, a in vals.items() if a is not None and k != "fric"}, soft, rot), act)
    sim.check_status()
    got = (s.x, s.v, s.C, s.F, s.prim_pos) + ((s.prim_rot,) if rot else ())
    for name, t, r in zip(("x", "v", "C", "F", "prim_pos", "prim_rot"), got, ref):
        g = t.cpu().numpy()
        print(name, _rel(g, r.numpy()))
        assert np.isfinite(g).all() and _rel(g, r.numpy()) < 1e-9, (name, _rel(g, r.numpy()))
    if rot:
        assert np.abs(ref[5].numpy() - q).max() > 1e-3                     # the primitive turned


# ---- adjoint ----------------------------------------------------------------------------------------------------------------------
def _reference_adjoint(N, case, soft, kw, rot, mu=(0.7,), cot=None, need_contact=True, kind=None, **more):
    """autograd through the twin with random output cotangents (cot: which outputs get one; default all)."""
    torch.set_num_threads(8)
    x, v, Cm, F, prim, q, act, E, nu, ys = _split(case, rot)
    P = prim.shape[1]
    rng = np.random.default_rng(9)
    shapes = ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, P, 3)) + (((B, P, 4),) if rot else ())
    w = [rng.normal(size=s) for s in shapes]
    if cot is not None:
        w = [wi if i in cot else np.zeros_like(wi) for i, wi in enumerate(w)]
    tw = _twin(N, kw, mu=mu, **more)
    values = dict(x=x, v=v, C=Cm, F=F, prim=prim, act=act, E=E, nu=nu, ys=ys)
    if rot:
        values["rot"] = q
    leaves = {k: _T(a, True) for k, a in values.items()}
    leaves["fric"] = _T(np.full(B, tw.c.ground_friction), True)
    out = _twin_step(tw, leaves, soft, rot)
    if need_contact:
        counts = T.honesty_shape(tw)[1]
        if kind is not None:
            T.assert_regions(kind, [counts])
    sum((o * _T(wi)).sum() for o, wi in zip(out, w)).backward()
    grads = {k: (t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
    return values, [o.detach().numpy() for o in out], w, grads, tw


def _check_adjoint(sim, ref, soft, rot, bar=1e-6, names=None, fric=True, fwd=1e-9):
    values, out, w, grads, _ = ref
    names = tuple(values) if names is None else names
    hl = {k: _dev(sim, a, True) for k, a in values.items()}
    s1 = sim.step(_state(sim, hl, soft, rot), hl["act"])
    res = (s1.x, s1.v, s1.C, s1.F, s1.prim_pos) + ((s1.prim_rot,) if rot else ())
    for o, t, name in zip(out, res, ("x", "v", "C", "F", "prim_pos", "prim_rot")):
        assert _rel(t.detach().cpu().numpy(), o) < fwd, (name, _rel(t.detach().cpu().numpy(), o))
    sim.ground_friction_grad = None
    sum((t * _dev(sim, wi)).sum() for t, wi in zip(res, w)).backward()
    sim.check_status()
    for name in names:
        got = hl[name].grad.cpu().numpy()
        print(name, _rel(got, grads[name]))
        assert got.shape == grads[name].shape and np.isfinite(got).all() and _rel(got, grads[name]) < bar, (name, _rel(got, grads[name]))
    if fric:
        gfr = sim.ground_friction_grad.cpu().numpy()
        print("fric", _rel(gfr, grads["fric"]))
        assert np.abs(grads["fric"]).max() > 0          # the rod stands on the floor: the friction branch ran
        assert _rel(gfr, grads["fric"]) < 1e-6, (gfr, grads["fric"])
    return hl


@functools.lru_cache(maxsize=None)          # one reference per kind and orientation mode, shared by the cases that differ on the HIP side only
def _ref_single(kind, rot):
    case, soft, kw = T.shape_case(kind, B, 33, rot)
    ref = _reference_adjoint(33, case, soft, kw, rot, kind=kind)
    g = ref[3]
    assert np.abs(g["act"]).min() > 0 and np.isfinite(g["act"]).all() and g["act"].shape == (B, 6 if rot else 3)
    assert not rot or np.abs(g["rot"][:, 0]).min() > 0
    return soft, kw, ref


ADJ = [(k, m, c, l) for k in KINDS for m in MODES for c, l in ([(0, 0), (27, 0)] + ([(27, 1), (27, 4), (27, 8)] if k == T.BOX else []))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode,ckpt,lanes", ADJ, ids=[f"{T.NAMES[k]}-{m}-ckpt{c}-lanes{l}" for k, m, c, l in ADJ])
def test_hip_shape_adjoint_matches_autograd_through_the_twin(kind, mode, ckpt, lanes):
    """ud_plb_step_bwd / _bwd_rot where the grid is recomputed (grid_ckpt_cells 0) and where it is restored, the Box with every lane
    mapping, at N = 33.  Leaves: x, v, C, F, prim_pos, prim_rot (rot_state), every action dimension, E, nu, yield_stress, ground friction."""
    rot = mode == "rot"
    soft, kw, ref = _ref_single(kind, rot)
    sim = _sim(33, B, kw, ckpt=ckpt, lanes=lanes)
    _check_adjoint(sim, ref, soft, rot)


@pytest.mark.gpu
def test_hip_cylinder_and_capsule_on_one_handle():
    """Constant orientation, two general primitives of different kinds, both in the rod at N = 300: the kind is read per primitive at run time."""
    N = 300
    case, soft, kw = T.shape_case(T.CYLINDER, B, N, False, two=True)
    tilt = kw["rot"][0]
    kw = dict(kw, kinds=(T.CYLINDER, 1), shape=(T.SHAPES[T.CYLINDER], (0.0, 0.0, 0.0)), rot=(tilt, (0.8, -0.3, 0.2, 0.4)), h=(0.0, 0.05))
    ref = _reference_adjoint(N, case, soft, kw, False, mu=(0.7, 0.4), kind=T.CYLINDER)
    assert sorted({d["kind"] for d in ref[4].diag}) == [1, T.CYLINDER] and np.abs(ref[3]["prim"][:, 1]).min() > 0
    sim = _sim(N, B, {k: v for k, v in kw.items() if k != "h"}, mu=(0.7, 0.4), h=(0.0, 0.05))
    _check_adjoint(sim, ref, soft, False)


@pytest.mark.gpu
def test_hip_rotating_box_and_sticky_sphere_on_one_handle():
    N = 300
    case, soft, kw = T.shape_case(T.BOX, B, N, True, two=True)
    kw = dict(kw, kinds=(T.BOX, 0), shape=(T.SHAPES[T.BOX], (0.0, 0.0, 0.0)))
    ref = _reference_adjoint(N, case, soft, kw, True, mu=(0.7, 0.0), kind=T.BOX, radius=(0.03, 0.025))
    assert np.abs(ref[3]["prim"][:, 1]).max() > 0        # the sphere touches the cloud too
    sim = _sim(N, B, kw, mu=(0.7, 0.0), radius=(0.03, 0.025))
    _check_adjoint(sim, ref, soft, True)


@pytest.mark.gpu
def test_hip_rotating_box_kinematics_alone():
    """The Box 0.3 along x clear of the rod (0.028 thin): no active occupied cell, so the outputs and, with cotangents on prim_pos and
    prim_rot only, g_action / g_prim_rot0 / g_prim_pos0 are the kinematics chain alone.  Bar 1e-12, as test_hip_rot_kinematics_alone."""
    case, soft, kw = T.shape_case(T.BOX, B, 33, True)
    case = list(case)
    case[4] = case[4] + np.array([0.3, 0.0, 0.0])
    ref = _reference_adjoint(33, tuple(case), soft, kw, True, cot=(4, 5), need_contact=False)
    tw = ref[4]
    assert tw.diag and not any(bool((d["occ"] & d["active"]).any()) for d in tw.diag)
    g = ref[3]
    assert np.abs(g["act"]).min() > 0 and np.abs(g["rot"][:, 0]).min() > 0
    sim = _sim(33, B, kw)
    _check_adjoint(sim, ref, soft, True, bar=1e-12, names=("prim", "rot", "act"), fric=False)


# ---- contact loss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("soft_contact", [True, False], ids=["soft", "hard"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_hip_shape_contact_loss_matches_the_twin(kind, mode, soft_contact):
    """As test_hip_rot_contact_loss_matches_the_twin: primitive 0 the shape with a tilted orientation (per env and not unit on rot_state),
    primitive 1 a Sphere; the contact term takes the shape's own sdf.  loss, parts, g_x, g_prim_pos, g_prim_rot."""
    rot = mode == "rot"
    nb, N = 2, 300
    kw = dict(kinds=(kind, 0), shape=(T.SHAPES[kind], (0.0, 0.0, 0.0)), action_dim=6 if rot else 3, rot_state=rot)
    if not rot:
        kw["rot"] = ((0.9, 0.1, -0.3, 0.2), (1.0, 0.0, 0.0, 0.0))
    tw = _twin(N, kw, mu=(0.0, 0.0), radius=(0.03, 0.025))
    rng = np.random.default_rng(2)
    x = np.stack([torus_particles(1000)[:N], torus_particles(1000)[:N] + rng.normal(size=(N, 3)) * 0.003])
    # the shape beside the rod, clear of it: every particle's max(sdf, 0) in its open arm, so the hard contact's minimum is not 0
    prim = np.array([[[0.40, 0.28, 0.5], [0.55, 0.62, 0.5]], [[0.5, 0.35, 0.62], [0.5, 0.1, 0.5]]])
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (nb, 2, 1))
    q[:, 0] = np.array([[0.9, 0.1, -0.3, 0.2], [0.7, -0.4, 0.2, 0.5]]) * np.array([[1.03], [0.96]])
    td = tw.grid_mass(torch.tensor((torus_particles(1000)[:N] + np.array([0.004, -0.01, 0.0]))[None]))[0]
    ts = torch.tensor(rng.normal(size=tw.c.n_grid ** 3))
    wts = (3.0, 0.7, 1.3)
    tx, tp, tr = _T(x, True), _T(prim, True), _T(q, True)
    total, parts = tw.loss(tx, tp, td, ts, wts, soft_contact=soft_contact, prim_rot=tr if rot else None)
    gl = np.array([1.0, -2.5])
    (total * _T(gl)).sum().backward()
    assert np.abs(tp.grad.numpy()[:, 0]).max() > 0 and float(parts.detach()[:, 0].min()) > 0
    d0 = tw.sdf_q(0, _T(x), _T(prim)[:, 0, None, :], _T(q)[:, 0]) if rot else tw.sdf(0, _T(x), _T(prim)[:, 0, None, :])
    assert float(d0.min()) > 1e-9
    if rot:
        assert np.abs(tr.grad.numpy()[:, 0]).min() > 0 and np.abs(tr.grad.numpy()[:, 1]).max() == 0.0
    sim = _sim(N, nb, kw, mu=(0.0, 0.0), radius=(0.03, 0.025))
    hx, hp, hr = _dev(sim, x, True), _dev(sim, prim, True), _dev(sim, q, True)
    st = sim.reset()._replace(x=hx, prim_pos=hp)
    st = st._replace(prim_rot=hr) if rot else st
    hloss, hparts = sim.compute_loss(st, td.numpy(), ts.numpy(), wts, soft_contact)
    print("loss", _rel(hloss.detach().cpu().numpy(), total.detach().numpy()), "parts", _rel(hparts.cpu().numpy(), parts.detach().numpy()))
    assert _rel(hloss.detach().cpu().numpy(), total.detach().numpy()) < 1e-11
    assert _rel(hparts.cpu().numpy(), parts.detach().numpy()) < 1e-11
    (hloss * _dev(sim, gl)).sum().backward()
    for name, got, want in (("x", hx, tx), ("prim", hp, tp)) + ((("rot", hr, tr),) if rot else ()):
        print(name, _rel(got.grad.cpu().numpy(), want.grad.numpy()))
        assert _rel(got.grad.cpu().numpy(), want.grad.numpy()) < 1e-9, name


# ---- the raw entry points -----------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _raw_step(sim, nb, x, v, Cm, F, pp, pr, so, act, E, nu, ys, cots, pad=0, canary=777.0):
    """ud_plb_step_fwd_rot + ud_plb_step_bwd_rot for the first nb envs; g_action and g_prim_rot0 carry `pad` canary doubles behind them."""
    from unidom_amd import _lib
    L = _lib.lib()
    N, P, A, dev = sim.n_particles, sim.n_primitive, sim.action_dim, sim.device
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    xo, vo, Co, Fo, po, ro = mk(nb, N, 3), mk(nb, N, 3), mk(nb, N, 3, 3), mk(nb, N, 3, 3), mk(nb, P, 3), mk(nb, P, 4)
    ckpt = torch.empty((L.ud_plb_ckpt_bytes(sim._h, C.c_int(nb)) // 8,), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(L.ud_plb_step_fwd_rot(sim._h, C.c_int(nb), _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(pr), _p(so), _p(act), _p(E), _p(nu), _p(ys),
                                     _p(xo), _p(vo), _p(Co), _p(Fo), _p(po), _p(ro), _p(ckpt), st), "ud_plb_step_fwd_rot")
    ox, ov, oC, oF, op = mk(nb, N, 3), mk(nb, N, 3), mk(nb, N, 3, 3), mk(nb, N, 3, 3), mk(nb, P, 3)
    oa = torch.full((nb * A + pad,), canary, dtype=torch.float64, device=dev)
    orot = torch.full((nb * P * 4 + pad,), canary, dtype=torch.float64, device=dev)
    oE, onu, oys, ofr = mk(nb), mk(nb), mk(nb), mk(nb)
    _lib.check(L.ud_plb_step_bwd_rot(sim._h, C.c_int(nb), _p(ckpt), _p(so), _p(act), _p(E), _p(nu), _p(ys), *[_p(c) for c in cots], _p(ox),
                                     _p(ov), _p(oC), _p(oF), _p(op), _p(orot), _p(oa), _p(oE), _p(onu), _p(oys), _p(ofr), st), "ud_plb_step_bwd_rot")
    torch.cuda.synchronize()
    return oa, orot


@pytest.mark.gpu
def test_hip_shape_batch_size_canaries():
    """A B = 1 call after a B = 3 call on a max_envs = 3 rotating-Box handle writes g_action [1,6] and g_prim_rot0 [1,1,4] and not a word
    behind them, and gives env 0 of the B = 3 call."""
    N = 33
    case, soft, kw = T.shape_case(T.BOX, B, N, True)
    sim = _sim(N, B, kw)
    x, v, Cm, F, prim, q, act, E, nu, ys = (_dev(sim, a) for a in case)
    so = _dev(sim, soft)
    rng = np.random.default_rng(4)
    cots = [_dev(sim, rng.normal(size=s)) for s in ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, 1, 3), (B, 1, 4))]
    oa3, or3 = _raw_step(sim, 3, x, v, Cm, F, prim, q, so, act, E, nu, ys, cots)
    first = lambda t: t[:1].contiguous()
    oa1, or1 = _raw_step(sim, 1, *(first(t) for t in (x, v, Cm, F, prim, q, so, act, E, nu, ys)), [first(c) for c in cots], pad=24)
    oa1, or1, oa3, or3 = (t.cpu().numpy() for t in (oa1, or1, oa3, or3))
    assert (oa1[6:] == 777.0).all() and (or1[4:] == 777.0).all(), (oa1, or1)
    assert np.isfinite(oa1[:6]).all() and np.abs(oa1[:6]).min() > 0 and (oa1[:6] != 777.0).all() and (or1[:4] != 777.0).all()
    assert _rel(oa1[:6], oa3[:6]) < 1e-9 and _rel(or1[:4], or3[:4]) < 1e-9


@pytest.mark.gpu
def test_hip_shape_contract():
    """Create-time refusals return their code and name the field; the entry points without _rot refuse a rot_state Box handle and leave
    the outputs as they were."""
    from unidom_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = UD_ERR["INVALID"], UD_ERR["UNSUPPORTED"]
    tilt = ((0.9, 0.1, -0.3, 0.2),)
    box = dict(kinds=(T.BOX,), shape=(T.SHAPES[T.BOX],), rot=tilt)
    rbox = dict(kinds=(T.BOX,), shape=(T.SHAPES[T.BOX],), action_dim=6, rot_state=True)
    refused = [(dict(kw=dict(box, shape=((0.06, 0.0, 0.05),))), INVALID, "prim_shape[0][1]"),
               (dict(kw=dict(box, shape=((0.06, 0.04, -1.0),))), INVALID, "prim_shape[0][2]"),
               (dict(kw=dict(box, kinds=(T.CYLINDER,), shape=((0.06, 0.0, 0.0),))), INVALID, "prim_shape[0][1]"),
               (dict(kw=dict(box, kinds=(T.TORUS,), shape=((-0.07, 0.025, 0.0),))), INVALID, "prim_shape[0][0]"),
               (dict(kw=dict(box, kinds=(6,))), INVALID, "prim_kind[0] = 6"),
               (dict(kw=dict(box, kinds=(-1,))), INVALID, "prim_kind[0] = -1"),
               (dict(kw=dict(box, rot=((0.5, 0.1, 0.1, 0.1),))), INVALID, "prim_rot[0]"),
               (dict(kw=box, path=2), UNSUPPORTED, "path = 2"),
               (dict(kw=rbox, path=2), UNSUPPORTED, "path = 2"),
               (dict(kw=dict(rbox, action_dim=6, rot_state=False)), INVALID, "rot_state"),
               (dict(kw=dict(rbox, kinds=(T.BOX, T.TORUS), shape=(T.SHAPES[T.BOX], T.SHAPES[T.TORUS])), mu=(0.0, 0.0)), UNSUPPORTED, "primitive 1")]
    for kwargs, code, word in refused:
        with pytest.raises(_lib.UnidomError) as e:
            _sim(33, 1, kwargs.pop("kw"), **kwargs)
        assert f"status {code})" in str(e.value) and word in str(e.value), str(e.value)
    for kind in KINDS:                                 # a Cylinder and a Torus ignore the third constant; action_dim 3 and 6 both create
        _sim(33, 1, dict(rbox, kinds=(kind,), shape=(T.SHAPES[kind][:2] + (-5.0,) if kind != T.BOX else T.SHAPES[kind],), action_dim=3))
    N = 33
    sim = _sim(N, 1, rbox)
    mk = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=sim.device)
    x, v, Cm, F, pp, so, act, E = mk(1, N, 3), mk(1, N, 3), mk(1, N, 3, 3), mk(1, N, 3, 3), mk(1, 1, 3), mk(1, 1), mk(1, 6), mk(1)
    out = torch.full((1 << 16,), 777.0, dtype=torch.float64, device=sim.device)   # stands in for every output / checkpoint / grid-sized array
    st = C.c_void_p(torch.cuda.current_stream(sim.device).cuda_stream)
    one = C.c_int(1)
    calls = {
        "ud_plb_step_fwd": lambda: L.ud_plb_step_fwd(sim._h, one, _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(so), _p(act), _p(E), _p(E), _p(E), _p(out),
                                                     _p(out), _p(out), _p(out), _p(out), _p(None), st),
        "ud_plb_step_bwd": lambda: L.ud_plb_step_bwd(sim._h, one, _p(out), _p(so), _p(act), _p(E), _p(E), _p(E), *([_p(None)] * 5), _p(out), _p(out),
                                                     _p(out), _p(out), *([_p(None)] * 6), st),
        "ud_plb_loss_fwd": lambda: L.ud_plb_loss_fwd(sim._h, one, _p(x), _p(pp), _p(out), _p(out), _p(out), one, _p(out), _p(None), st),
        "ud_plb_loss_bwd": lambda: L.ud_plb_loss_bwd(sim._h, one, _p(x), _p(pp), _p(out), _p(out), _p(out), one, _p(out), _p(out), _p(None), st),
    }
    for name, call in calls.items():
        assert call() == INVALID, name
        assert "rot_state" in L.ud_last_error().decode(), (name, L.ud_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())


@pytest.mark.gpu
def test_hip_capsule_handle_ignores_prim_shape():
    """Kinds 0 to 2 ignore prim_shape: a Capsule handle created with nonsense in it runs the kernels it always ran and gives the outputs of
    one created with zeros, bit for bit.  N = 33 with one lane per particle: one wave of one block does all the scattering, so the order of
    the f64 atomic sums, and with it every bit of the result, is fixed from run to run."""
    N = 33
    case, soft, _ = T.shape_case(T.BOX, B, N, False)
    kw = dict(kinds=(1,), rot=((0.9, 0.1, -0.3, 0.2),))
    outs = []
    for shape in (((0.0, 0.0, 0.0),), ((-3.0, float("nan"), 1e300),), ((0.0, 0.0, 0.0),)):
        sim = _sim(N, B, kw, h=(0.05, 0.0), lanes=1, shape=shape)
        x, v, Cm, F, prim, act, E, nu, ys = case
        hl = dict(x=x, v=v, C=Cm, F=F, prim=prim, E=E, nu=nu, ys=ys)
        s = sim.step(_state(sim, {k: _dev(sim, a) for k, a in hl.items()}, np.full((B, 1), 666.0), False), act)
        sim.check_status()
        outs.append([t.cpu() for t in (s.x, s.v, s.C, s.F, s.prim_pos)])
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))     # the premise: two handles with the same conf agree bit for bit
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert float((outs[0][0] - torch.tensor(case[0])).abs().max()) > 0


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plb_simulator_rotating_box_step_loss_backward():
    """PlbSimulator with a rotating Box: step -> compute_loss -> backward.  The loss (1e-9) and all six g_action components and g_E (1e-6)
    against autograd through the twin's step and loss."""
    torch.set_num_threads(8)
    N = 33
    case, soft, kw = T.shape_case(T.BOX, B, N, True)
    x, v, Cm, F, prim, q, act, E, nu, ys = case
    tw = _twin(N, kw)
    rng = np.random.default_rng(3)
    td, ts = np.abs(rng.normal(size=32 ** 3)) * 1e-5, rng.normal(size=32 ** 3)
    wts, gl = (3.0, 0.7, 1.3), np.array([1.0, -2.5, 0.5])
    ta, tE = _T(act, True), _T(E, True)
    out = tw.step(*map(_T, (x, v, Cm, F, prim, q)), ta, _T(soft), tE, _T(nu), _T(ys), _T(np.full(B, tw.c.ground_friction)))
    T.honesty_shape(tw)
    total, _ = tw.loss(out[0], out[4], _T(td), _T(ts), wts, True, prim_rot=out[5])
    (total * _T(gl)).sum().backward()
    assert np.abs(ta.grad.numpy()).min() > 0 and np.abs(tE.grad.numpy()).min() > 0
    sim = _sim(N, B, kw)
    ha, hE = _dev(sim, act, True), _dev(sim, E, True)
    hl = dict(x=x, v=v, C=Cm, F=F, prim=prim, rot=q, nu=nu, ys=ys)
    s1 = sim.step(_state(sim, {**{k: _dev(sim, a) for k, a in hl.items()}, "E": hE}, soft, True), ha)
    loss, _ = sim.compute_loss(s1, _dev(sim, td), _dev(sim, ts), wts, True)
    (loss * _dev(sim, gl)).sum().backward()
    sim.check_status()
    print("loss", _rel(loss.detach().cpu().numpy(), total.detach().numpy()), "act", _rel(ha.grad.cpu().numpy(), ta.grad.numpy()),
          "E", _rel(hE.grad.cpu().numpy(), tE.grad.numpy()))
    assert _rel(loss.detach().cpu().numpy(), total.detach().numpy()) < 1e-9
    assert ha.grad.shape == (B, 6) and _rel(ha.grad.cpu().numpy(), ta.grad.numpy()) < 1e-6
    assert _rel(hE.grad.cpu().numpy(), tE.grad.numpy()) < 1e-6


def _header_codes():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidom_hip.h")).read()
    return {k: int(val) for k, val in re.findall(r"UD_ERR_(\w+)\s*=\s*(-?\d+)", src)}


UD_ERR = _header_codes()
