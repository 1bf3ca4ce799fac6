"""Rotating primitives of the PLB f64 path on the GPU: ud_plb_step_fwd_rot / _bwd_rot / ud_plb_loss_*_rot (rot_state handles: a Capsule
with six action dimensions, the RollingPin) against the torch restatement tests/plb_rot_twin.py and its autograd.  PARITY UNPINNED by
reference data (taichi is absent): the restatement is the specification.  Bars: those of tests/test_plb.py and test_plb_capsule_gpu.py
(forward 1e-9 relative on x, v, C, F; prim_pos and prim_rot 1e-14 absolute; adjoint 1e-6 relative; losses 1e-11 / 1e-9; the
kinematics alone 1e-14 absolute / 1e-12 relative).  Every reference run asserts the conditions that keep the comparison honest
(plb_prim_twin.honesty): enough occupied cells in both arms of the contact, none near a branch point."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf, torus_particles
from tests.plb_prim_twin import honesty
from tests.plb_rot_twin import HEIGHT, MU, RADIUS, ROLL_SCALE, SCALE_W, PlbRotTwin, rot_case

S, B = 3, 3                                   # n_grid 32: dx = 0.03125, the capsule spans a few cells in every direction
KINS = ["sixdim", "rolling"]


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _T(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def _twin(N, kw, mu=(MU,), radius=(RADIUS,), h=(HEIGHT,), upper=(1.0, 1.0, 1.0), substeps=S, quality=0.5):
    return PlbRotTwin(PlbConf(quality=quality, n_particles=N, radius=radius, upper_bound=upper), h=h, mu=mu, substeps=substeps, **kw)


def _sim(N, nb, kw, mu=(MU,), radius=(RADIUS,), h=(HEIGHT,), upper=(1.0, 1.0, 1.0), substeps=S, ckpt=None, lanes=0, path=0, quality=0.5,
         rot_state=True):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles, cfg.path, cfg.lanes, cfg.upper_bound = quality, substeps, N, path, lanes, upper
    cfg.prim_radius, cfg.prim_kind, cfg.prim_h, cfg.prim_friction = radius, kw["kinds"], h, mu
    cfg.prim_rot = ((1.0, 0.0, 0.0, 0.0),) * len(radius)
    cfg.action_scale = kw.get("action_scale", (1.0, 1.0, 1.0))
    cfg.rot_state, cfg.action_dim, cfg.action_scale_w = rot_state, kw["action_dim"], kw.get("action_scale_w", (1.0, 1.0, 1.0))
    cfg.prim_init_pos = ((0.5, 0.3, 0.5),) * len(radius)
    if ckpt is not None:
        cfg.grid_ckpt_cells = ckpt
    sim = PlbSimulator(cfg, batch_size=nb)
    assert sim.launch_plan() == 1 and sim.n_grid == 32 * int(quality / 0.5) and sim.substeps == substeps
    return sim


def _dev(sim, a, r=False):
    return torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)


def _soft(P=1):
    return np.full((B, P), 666.0)


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kin", KINS)
@pytest.mark.parametrize("mu", [0.0, 0.9])
@pytest.mark.parametrize("N", [33, 300])
def test_hip_rot_forward_matches_the_twin(N, mu, kin):
    """One step, three envs.  N = 33 leaves most lanes of a wave idle, N = 300 spreads the touched cells over several waves and blocks."""
    torch.set_num_threads(8)
    case, kw = rot_case(B, N, rolling=kin == "rolling")
    x, v, Cm, F, prim, rot, act, E, nu, ys = case
    tw = _twin(N, kw, mu=(mu,))
    with torch.no_grad():
        ref = tw.step(*map(_T, (x, v, Cm, F, prim, rot, act)), _T(_soft()), _T(E), _T(nu), _T(ys), _T(np.full(B, tw.c.ground_friction)))
    honesty(tw)
    sim = _sim(N, B, kw, mu=(mu,))
    D = lambda a: _dev(sim, a)
    s = sim.reset()._replace(x=D(x), v=D(v), C=D(Cm), F=D(F), prim_pos=D(prim), prim_rot=D(rot), softness=D(_soft()), E=D(E), nu=D(nu),
                             yield_stress=D(ys))
    s = sim.step(s, act)
    sim.check_status()
    for name, t, r in zip("xvCF", (s.x, s.v, s.C, s.F), ref):
        got = t.cpu().numpy()
        print(name, _rel(got, r.numpy()))
        assert np.isfinite(got).all() and _rel(got, r.numpy()) < 1e-9, (name, _rel(got, r.numpy()))
    np.testing.assert_allclose(s.prim_pos.cpu().numpy(), ref[4].numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(s.prim_rot.cpu().numpy(), ref[5].numpy(), rtol=0, atol=1e-14)
    assert np.abs(ref[5].numpy() - rot).max() > 1e-3                     # the primitive turned


# ---- adjoint ----------------------------------------------------------------------------------------------------------------------
OUT_SHAPES = lambda N, P: ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, P, 3), (B, P, 4))
LEAVES = ("x", "v", "C", "F", "prim", "rot", "act", "E", "nu", "ys")


def _reference_adjoint(N, case, kw, soft, mu=(MU,), radius=(RADIUS,), h=(HEIGHT,), upper=(1.0, 1.0, 1.0), cot=None, need_contact=True):
    """autograd through the twin with random output cotangents (cot: which outputs get one; default all six)."""
    torch.set_num_threads(8)
    x, v, Cm, F, prim, rot, act, E, nu, ys = case
    P = prim.shape[1]
    rng = np.random.default_rng(9)
    w = [rng.normal(size=s) for s in OUT_SHAPES(N, P)]
    if cot is not None:
        w = [wi if i in cot else np.zeros_like(wi) for i, wi in enumerate(w)]
    tw = _twin(N, kw, mu=mu, radius=radius, h=h, upper=upper)
    leaves = dict(x=_T(x, True), v=_T(v, True), C=_T(Cm, True), F=_T(F, True), prim=_T(prim, True), rot=_T(rot, True), act=_T(act, True),
                  E=_T(E, True), nu=_T(nu, True), ys=_T(ys, True), fric=_T(np.full(B, tw.c.ground_friction), True))
    out = tw.step(leaves["x"], leaves["v"], leaves["C"], leaves["F"], leaves["prim"], leaves["rot"], leaves["act"], _T(soft), leaves["E"],
                  leaves["nu"], leaves["ys"], leaves["fric"])
    if need_contact:
        honesty(tw)
    sum((o * _T(wi)).sum() for o, wi in zip(out, w)).backward()
    grads = {k: (t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
    values = dict(x=x, v=v, C=Cm, F=F, prim=prim, rot=rot, act=act, E=E, nu=nu, ys=ys)
    return values, [o.detach().numpy() for o in out], w, grads, tw


@functools.lru_cache(maxsize=None)          # one reference per kinematics, shared by the cases that differ on the HIP side only
def _ref_single(kin):
    case, kw = rot_case(B, 33, rolling=kin == "rolling")
    ref = _reference_adjoint(33, case, kw, _soft())
    g = ref[3]
    assert np.abs(g["rot"][:, 0]).min() > 0 and np.abs(g["act"]).min() > 0 and np.isfinite(g["act"]).all()
    return kw, ref


def _check_adjoint(sim, ref, soft, bar=1e-6, names=LEAVES, fric=True):
    values, out, w, grads, _ = ref
    hl = {k: _dev(sim, a, True) for k, a in values.items()}
    s = sim.reset()._replace(x=hl["x"], v=hl["v"], C=hl["C"], F=hl["F"], prim_pos=hl["prim"], prim_rot=hl["rot"], softness=_dev(sim, soft),
                             E=hl["E"], nu=hl["nu"], yield_stress=hl["ys"])
    s1 = sim.step(s, hl["act"])
    res = (s1.x, s1.v, s1.C, s1.F, s1.prim_pos, s1.prim_rot)
    for o, t, name in zip(out[:4], res, "xvCF"):
        assert _rel(t.detach().cpu().numpy(), o) < 1e-9, (name, _rel(t.detach().cpu().numpy(), o))
    np.testing.assert_allclose(s1.prim_pos.detach().cpu().numpy(), out[4], rtol=0, atol=1e-14)
    np.testing.assert_allclose(s1.prim_rot.detach().cpu().numpy(), out[5], rtol=0, atol=1e-14)
    sim.ground_friction_grad = None
    sum((t * _dev(sim, wi)).sum() for t, wi in zip(res, w)).backward()
    sim.check_status()
    for name in names:
        got = hl[name].grad.cpu().numpy()
        print(name, _rel(got, grads[name]))
        assert got.shape == grads[name].shape and np.isfinite(got).all() and _rel(got, grads[name]) < bar, (name, _rel(got, grads[name]))
    if fric:
        gfr = sim.ground_friction_grad.cpu().numpy()
        print("fric", gfr, grads["fric"])
        assert np.abs(grads["fric"]).max() > 0          # the rod stands on the floor: the friction branch ran
        assert _rel(gfr, grads["fric"]) < 1e-6, (gfr, grads["fric"])
    return hl


@pytest.mark.gpu
@pytest.mark.parametrize("kin", KINS)
@pytest.mark.parametrize("ckpt,lanes", [(0, 0), (27, 0), (27, 1), (27, 4), (27, 8)])
def test_hip_rot_adjoint_matches_autograd_through_the_twin(ckpt, lanes, kin):
    """ud_plb_step_bwd_rot where the grid is recomputed (grid_ckpt_cells 0) and where it is restored, with every lane mapping, for both
    kinematics at N = 33.  Leaves: x, v, C, F, prim_pos, prim_rot, action (all action_dim entries), E, nu, yield_stress, ground friction."""
    kw, ref = _ref_single(kin)
    sim = _sim(33, B, kw, ckpt=ckpt, lanes=lanes)
    _check_adjoint(sim, ref, _soft())


@pytest.mark.gpu
@pytest.mark.parametrize("kin", KINS)
def test_hip_rot_kinematics_alone(kin):
    """The primitive far from the particles: no active occupied cell, so prim_pos_out / prim_rot_out (1e-14) and, with cotangents on
    prim_pos and prim_rot only, g_action / g_prim_rot0 / g_prim_pos0 (1e-12 relative) are the kinematics chain of the epilogue alone.
    Moved 0.3 along x, not y: the rod stands from y = 0.05 to 0.55 and 0.3 up the tilted capsule still reaches its top, sideways the
    rod is 0.028 thin."""
    case, kw = rot_case(B, 33, rolling=kin == "rolling")
    case = list(case)
    case[4] = case[4] + np.array([0.3, 0.0, 0.0])
    ref = _reference_adjoint(33, tuple(case), kw, _soft(), cot=(4, 5), need_contact=False)
    tw = ref[4]
    assert tw.diag and not any(bool((d["occ"] & d["active"]).any()) for d in tw.diag)
    g = ref[3]
    assert np.abs(g["act"]).min() > 0 and np.abs(g["rot"][:, 0]).min() > 0
    sim = _sim(33, B, kw)
    _check_adjoint(sim, ref, _soft(), bar=1e-12, names=("prim", "rot", "act"), fric=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kin", KINS)
def test_hip_rot_clamps(kin):
    """One env with an action entry outside [-1, 1] (its cotangent is zero), one whose position reaches upper_bound (the clamp stops
    the cotangent): forward and adjoint."""
    rolling = kin == "rolling"
    case, kw = rot_case(B, 33, rolling=rolling)
    x, v, Cm, F, prim, rot, act, E, nu, ys = case
    act = act.copy()
    act[2, 1 if rolling else 4] = 1.7
    e = int(np.argmax(prim[:, 0, 1]))                                   # the highest primitive: the bound sits 0.5 mm above it, and it moves up
    upper = (1.0, float(prim[e, 0, 1] + 0.0005), 1.0)
    if rolling:
        act[e, 2] = 0.004                                               # dy, scale 1
    else:
        act[e, 1] = 0.004
    ref = _reference_adjoint(33, (x, v, Cm, F, prim, rot, act, E, nu, ys), kw, _soft(), upper=upper)
    assert abs(ref[1][4][e, 0, 1] - upper[1]) == 0.0                    # it reached the bound
    assert ref[3]["act"][2, 1 if rolling else 4] == 0.0
    sim = _sim(33, B, kw, upper=upper)
    hl = _check_adjoint(sim, ref, _soft())
    assert float(hl["act"].grad[2, 1 if rolling else 4]) == 0.0


@pytest.mark.gpu
def test_hip_rotating_capsule_and_sticky_sphere_on_one_handle():
    """Primitive 0 a rotating Capsule (six action dimensions), primitive 1 a sticky Sphere, both in the rod: forward and adjoint."""
    N = 300
    case, kw = rot_case(B, N, two=True)
    soft = _soft(2)
    mu, radius, h = (MU, 0.0), (RADIUS, 0.025), (HEIGHT, 0.0)
    ref = _reference_adjoint(N, case, kw, soft, mu=mu, radius=radius, h=h)
    assert np.abs(ref[3]["prim"][:, 1]).max() > 0        # the sphere touches the cloud too
    sim = _sim(N, B, kw, mu=mu, radius=radius, h=h)
    _check_adjoint(sim, ref, soft)


# ---- contact loss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("soft_contact", [True, False])
def test_hip_rot_contact_loss_matches_the_twin(soft_contact):
    """As test_hip_capsule_contact_loss_matches_the_twin at N = 300, n_grid 32: primitive 0 a Capsule with a tilted rotation per env
    (not unit), primitive 1 a Sphere.  loss, parts, g_x, g_prim_pos, g_prim_rot."""
    nb, N = 2, 300
    kw = dict(kinds=(1, 0), action_dim=6)
    radius, h = (0.03, 0.025), (0.06, 0.0)
    tw = _twin(N, kw, mu=(0.0, 0.0), radius=radius, h=h)
    rng = np.random.default_rng(2)
    x = np.stack([torus_particles(1000)[:N], torus_particles(1000)[:N] + rng.normal(size=(N, 3)) * 0.003])
    prim = np.array([[[0.44, 0.28, 0.5], [0.55, 0.62, 0.5]], [[0.5, 0.35, 0.56], [0.5, 0.1, 0.5]]])
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (nb, 2, 1))
    rot[:, 0] = np.array([[0.9, 0.1, -0.3, 0.2], [0.7, -0.4, 0.2, 0.5]]) * np.array([[1.03], [0.96]])
    td = tw.grid_mass(torch.tensor((torus_particles(1000)[:N] + np.array([0.004, -0.01, 0.0]))[None]))[0]
    ts = torch.tensor(rng.normal(size=tw.c.n_grid ** 3))
    wts = (3.0, 0.7, 1.3)
    tx, tp, tr = _T(x, True), _T(prim, True), _T(rot, True)
    total, parts = tw.loss(tx, tp, td, ts, wts, soft_contact=soft_contact, prim_rot=tr)
    gl = np.array([1.0, -2.5])
    (total * _T(gl)).sum().backward()
    assert np.abs(tp.grad.numpy()[:, 0]).max() > 0 and np.abs(tr.grad.numpy()[:, 0]).min() > 0 and float(parts.detach()[:, 0].min()) > 0
    assert np.abs(tr.grad.numpy()[:, 1]).max() == 0.0                     # the sphere has no orientation
    d0 = tw.sdf_q(0, _T(x), _T(prim)[:, 0, None, :], _T(rot)[:, 0])
    assert int((d0 > 0).sum()) > 100 and float(d0.abs().min()) > 1e-9      # the max(sdf, 0) of nearly every particle is in its open arm
    sim = _sim(N, nb, kw, mu=(0.0, 0.0), radius=radius, h=h)
    hx, hp, hr = _dev(sim, x, True), _dev(sim, prim, True), _dev(sim, rot, True)
    st = sim.reset()._replace(x=hx, prim_pos=hp, prim_rot=hr)
    hloss, hparts = sim.compute_loss(st, td.numpy(), ts.numpy(), wts, soft_contact)
    assert _rel(hloss.detach().cpu().numpy(), total.detach().numpy()) < 1e-11
    assert _rel(hparts.cpu().numpy(), parts.detach().numpy()) < 1e-11
    (hloss * _dev(sim, gl)).sum().backward()
    for name, got, want in (("x", hx, tx), ("prim", hp, tp), ("rot", hr, tr)):
        print(name, _rel(got.grad.cpu().numpy(), want.grad.numpy()))
        assert _rel(got.grad.cpu().numpy(), want.grad.numpy()) < 1e-9, name


# ---- the raw entry points -----------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _raw_step(sim, nb, x, v, Cm, F, pp, pr, so, act, E, nu, ys, cots, pad=0, canary=777.0):
    """ud_plb_step_fwd_rot + ud_plb_step_bwd_rot for the first nb envs.  g_action and g_prim_rot0 are allocated with `pad` canary
    doubles behind them.  Returns (outputs, gradients dict, the two padded buffers)."""
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
    return (xo, vo, Co, Fo, po, ro), dict(x=ox, prim=op, E=oE), oa, orot


@pytest.mark.gpu
def test_hip_rot_batch_size_canaries():
    """A B = 1 call after a B = 3 call on a max_envs = 3 handle writes g_action [1,6] and g_prim_rot0 [1,1,4] and not a word behind them
    (the per-env bounds PlbArgs::Bcall exists for), and gives env 0 of the B = 3 call."""
    N = 33
    case, kw = rot_case(B, N)
    sim = _sim(N, B, kw)
    x, v, Cm, F, prim, rot, act, E, nu, ys = (_dev(sim, a) for a in case)
    so = _dev(sim, _soft())
    rng = np.random.default_rng(4)
    cots = [_dev(sim, rng.normal(size=s)) for s in OUT_SHAPES(N, 1)]
    _, _, oa3, or3 = _raw_step(sim, 3, x, v, Cm, F, prim, rot, so, act, E, nu, ys, cots)
    first = lambda t: t[:1].contiguous()
    _, _, oa1, or1 = _raw_step(sim, 1, *(first(t) for t in (x, v, Cm, F, prim, rot, so, act, E, nu, ys)), [first(c) for c in cots], pad=24)
    oa1, or1, oa3, or3 = (t.cpu().numpy() for t in (oa1, or1, oa3, or3))
    assert (oa1[6:] == 777.0).all() and (or1[4:] == 777.0).all(), (oa1, or1)
    assert np.isfinite(oa1[:6]).all() and np.abs(oa1[:6]).min() > 0 and (oa1[:6] != 777.0).all() and (or1[:4] != 777.0).all()
    assert _rel(oa1[:6], oa3[:6]) < 1e-9 and _rel(or1[:4], or3[:4]) < 1e-9


@pytest.mark.gpu
def test_hip_rot_contract():
    """Old entry points refuse a rot_state handle and the new ones a plain handle (UD_ERR_INVALID); the configurations the issue rules out
    are refused with their code and a reason; a rot_state handle runs the multi-kernel path."""
    from unidom_amd import _lib
    L = _lib.lib()
    INVALID, UNSUPPORTED = UD_ERR["INVALID"], UD_ERR["UNSUPPORTED"]
    six, roll = dict(kinds=(1,), action_dim=6), dict(kinds=(2,), action_dim=3)
    refused = [(dict(kw=six, path=2), UNSUPPORTED, "rot_state"),
               (dict(kw=roll, rot_state=False), INVALID, "rot_state"),
               (dict(kw=six, rot_state=False), INVALID, "rot_state"),
               (dict(kw=dict(kinds=(0,), action_dim=3)), UNSUPPORTED, "primitive 0"),
               (dict(kw=dict(kinds=(2,), action_dim=6)), UNSUPPORTED, "three action dimensions"),
               (dict(kw=dict(kinds=(1, 1), action_dim=6), radius=(RADIUS, RADIUS), h=(HEIGHT, HEIGHT), mu=(0.0, 0.0)), UNSUPPORTED, "primitive 1")]
    for kwargs, code, word in refused:
        with pytest.raises(_lib.UnidomError) as e:
            _sim(33, 1, kwargs.pop("kw"), **kwargs)
        assert f"status {code})" in str(e.value) and word in str(e.value), str(e.value)
    N = 33
    mk = lambda sim, *shape: torch.zeros(shape, dtype=torch.float64, device=sim.device)
    for rot_state in (True, False):
        kw = six if rot_state else dict(kinds=(1,), action_dim=3)
        sim = _sim(N, 1, kw, rot_state=rot_state)
        assert sim.launch_plan() == 1
        A = sim.action_dim
        x, v, Cm, F, pp, pr, so, act, E = mk(sim, 1, N, 3), mk(sim, 1, N, 3), mk(sim, 1, N, 3, 3), mk(sim, 1, N, 3, 3), mk(sim, 1, 1, 3), mk(sim, 1, 1, 4), \
            mk(sim, 1, 1), mk(sim, 1, 6), mk(sim, 1)
        big = mk(sim, 1 << 16)                  # stands in for every output / checkpoint / grid-sized array: the refusal comes before any launch
        st = C.c_void_p(torch.cuda.current_stream(sim.device).cuda_stream)
        one = C.c_int(1)
        calls = {
            "ud_plb_step_fwd": lambda: L.ud_plb_step_fwd(sim._h, one, _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(so), _p(act), _p(E), _p(E), _p(E), _p(big),
                                                         _p(big), _p(big), _p(big), _p(big), _p(None), st),
            "ud_plb_step_bwd": lambda: L.ud_plb_step_bwd(sim._h, one, _p(big), _p(so), _p(act), _p(E), _p(E), _p(E), *([_p(None)] * 5), _p(big), _p(big),
                                                         _p(big), _p(big), *([_p(None)] * 6), st),
            "ud_plb_loss_fwd": lambda: L.ud_plb_loss_fwd(sim._h, one, _p(x), _p(pp), _p(big), _p(big), _p(big), one, _p(big), _p(None), st),
            "ud_plb_loss_bwd": lambda: L.ud_plb_loss_bwd(sim._h, one, _p(x), _p(pp), _p(big), _p(big), _p(big), one, _p(big), _p(big), _p(None), st),
            "ud_plb_step_fwd_rot": lambda: L.ud_plb_step_fwd_rot(sim._h, one, _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(pr), _p(so), _p(act), _p(E), _p(E),
                                                                 _p(E), _p(big), _p(big), _p(big), _p(big), _p(big), _p(big), _p(None), st),
            "ud_plb_step_bwd_rot": lambda: L.ud_plb_step_bwd_rot(sim._h, one, _p(big), _p(so), _p(act), _p(E), _p(E), _p(E), *([_p(None)] * 6), _p(big),
                                                                 _p(big), _p(big), _p(big), *([_p(None)] * 7), st),
            "ud_plb_loss_fwd_rot": lambda: L.ud_plb_loss_fwd_rot(sim._h, one, _p(x), _p(pp), _p(pr), _p(big), _p(big), _p(big), one, _p(big), _p(None), st),
            "ud_plb_loss_bwd_rot": lambda: L.ud_plb_loss_bwd_rot(sim._h, one, _p(x), _p(pp), _p(pr), _p(big), _p(big), _p(big), one, _p(big), _p(big),
                                                                 _p(None), _p(None), st),
        }
        for name, call in calls.items():
            if name.endswith("_rot") == rot_state:
                continue                                                # the handle's own entry points: the other tests run them
            assert call() == INVALID, name
            assert "rot_state" in L.ud_last_error().decode(), (name, L.ud_last_error().decode())
        torch.cuda.synchronize()


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plb_simulator_rot_state_is_the_raw_entry_points():
    """PlbSimulator with rot_state: reset(), one step() with a [B,6] action, compute_loss(), backward(); the gradients on the action and on
    state.prim_rot are those of the raw entry points chained by hand.  A nine-field PlbState on a plain simulator steps as before."""
    from unidom_amd import _lib
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator, PlbState
    L = _lib.lib()
    N = 33
    case, kw = rot_case(B, N)
    sim = _sim(N, B, kw)
    s0 = sim.reset()
    assert s0.prim_rot.shape == (B, 1, 4) and torch.equal(s0.prim_rot.cpu(), torch.tensor([1.0, 0, 0, 0], dtype=torch.float64).expand(B, 1, 4))
    x, v, Cm, F, prim, rot, act, E, nu, ys = (_dev(sim, a) for a in case)
    so = _dev(sim, _soft())
    rng = np.random.default_rng(3)
    td, ts = _dev(sim, np.abs(rng.normal(size=32 ** 3)) * 1e-5), _dev(sim, rng.normal(size=32 ** 3))
    wts, gl = (3.0, 0.7, 1.3), _dev(sim, [1.0, -2.5, 0.5])
    la, lr = act.clone().requires_grad_(True), rot.clone().requires_grad_(True)
    st = s0._replace(x=x, v=v, C=Cm, F=F, prim_pos=prim, prim_rot=lr, softness=so, E=E, nu=nu, yield_stress=ys)
    s1 = sim.step(st, la)
    loss, _ = sim.compute_loss(s1, td, ts, wts, True)
    (loss * gl).sum().backward()
    # the same by hand: loss_bwd_rot -> step_bwd_rot
    wt = _dev(sim, wts)
    stream = C.c_void_p(torch.cuda.current_stream(sim.device).cuda_stream)
    outs, _, _, _ = _raw_step(sim, B, x, v, Cm, F, prim, rot, so, act, E, nu, ys, [None] * 6)
    gx, gpp, gpr = torch.empty_like(outs[0]), torch.empty_like(outs[4]), torch.empty_like(outs[5])
    _lib.check(L.ud_plb_loss_bwd_rot(sim._h, C.c_int(B), _p(outs[0]), _p(outs[4]), _p(outs[5]), _p(td), _p(ts), _p(wt), C.c_int(1), _p(gl), _p(gx),
                                     _p(gpp), _p(gpr), stream), "ud_plb_loss_bwd_rot")
    _, _, oa, orot = _raw_step(sim, B, x, v, Cm, F, prim, rot, so, act, E, nu, ys, [gx, None, None, None, gpp, gpr])
    ga, gr = la.grad.cpu().numpy(), lr.grad.cpu().numpy()
    assert np.abs(ga).min() > 0 and np.abs(gr).min() > 0
    assert _rel(ga, oa.cpu().numpy().reshape(B, 6)) < 1e-9 and _rel(gr, orot.cpu().numpy().reshape(B, 1, 4)) < 1e-9
    # a plain simulator and a nine-field state
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles, cfg.path = 0.5, S, N, 1
    plain = PlbSimulator(cfg, batch_size=1)
    r = plain.reset()
    assert r.prim_rot is None
    nine = PlbState(r.x, r.v, r.C, r.F, r.prim_pos, r.softness, r.E, r.nu, r.yield_stress)
    a3 = np.array([[0.3, -0.2, 0.1]])
    o1, o2 = plain.step(nine, a3), plain.step(r, a3)
    assert o1.prim_rot is None and _rel(o1.x.cpu().numpy(), o2.x.cpu().numpy()) < 1e-12 and torch.equal(o1.prim_pos, o2.prim_pos)
    assert float((o1.prim_pos - r.prim_pos).abs().max()) > 0


def _header_codes():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidom_hip.h")).read()
    return {k: int(val) for k, val in re.findall(r"UD_ERR_(\w+)\s*=\s*(-?\d+)", src)}


UD_ERR = _header_codes()
