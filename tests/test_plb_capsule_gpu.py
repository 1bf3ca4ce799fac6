"""The Capsule primitive of the PLB f64 path on the GPU: ud_plb_step_fwd / _bwd / ud_plb_loss_* with prim_kind = 1 (multi-kernel
path, the only one such a handle runs) against the torch restatement tests/plb_prim_twin.py and its autograd.  PARITY UNPINNED by
reference data (taichi is absent): the restatement is the specification.  Bars: those of tests/test_plb.py (forward 1e-9 relative,
primitive positions 1e-14 absolute, adjoint 1e-6 relative, losses 1e-11 / 1e-9).  Every reference run asserts the conditions that
keep the comparison honest (plb_prim_twin.honesty): enough occupied cells in both arms of the contact, none near a branch point."""
import functools

import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf, torus_particles
from tests.plb_prim_twin import PlbPrimTwin, capsule_case, honesty

ROT = {"identity": (1.0, 0.0, 0.0, 0.0), "tilted": tuple(np.array([0.9, 0.1, -0.3, 0.2]) / np.linalg.norm([0.9, 0.1, -0.3, 0.2]))}
RADIUS, HEIGHT, S = 0.05, 0.12, 3            # n_grid 32: dx = 0.03125, the capsule spans a few cells in every direction
SOFT1 = np.array([[666.0], [0.0], [666.0]])  # row 1: softness 0, the `dist <= 0` arm of the active test alone
W_SHAPES = lambda B, N, P: ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, P, 3))


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _T(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def _twin(N, kinds, rot, mu, radius=(RADIUS,), h=(HEIGHT,), scale=(1.0, 1.0, 1.0), substeps=S):
    return PlbPrimTwin(PlbConf(quality=0.5, n_particles=N, radius=radius), kinds=kinds, h=h, rot=rot, mu=mu, action_scale=scale, substeps=substeps)


def _sim(N, B, kinds, rot, mu, radius=(RADIUS,), h=(HEIGHT,), scale=(1.0, 1.0, 1.0), substeps=S, ckpt=None, lanes=0, path=0, quality=0.5):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles, cfg.path, cfg.lanes = quality, substeps, N, path, lanes
    cfg.prim_radius, cfg.prim_kind, cfg.prim_h, cfg.prim_rot, cfg.prim_friction, cfg.action_scale = radius, kinds, h, rot, mu, scale
    cfg.prim_init_pos = ((0.5, 0.3, 0.5),) * len(radius)
    if ckpt is not None:
        cfg.grid_ckpt_cells = ckpt
    sim = PlbSimulator(cfg, batch_size=B)
    assert sim.launch_plan() == 1 and sim.n_grid == 32 * int(quality / 0.5) and sim.substeps == substeps
    return sim


def _dev(sim, a, r=False):
    return torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)


# ---- a. forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("q", ["identity", "tilted"])
@pytest.mark.parametrize("mu", [0.0, 0.9])
@pytest.mark.parametrize("N", [33, 300])
def test_hip_capsule_forward_matches_the_twin(N, mu, q):
    """Two chained steps on one handle, three envs (softness 666 / 0 / 666)."""
    torch.set_num_threads(8)
    B = 3
    x, v, Cm, F, prim, act, E, nu, ys = capsule_case(B, N)
    tw = _twin(N, (1,), (ROT[q],), (mu,))
    ref = tuple(map(_T, (x, v, Cm, F, prim)))
    with torch.no_grad():
        for _ in range(2):
            ref = tw.step(*ref, _T(act), _T(SOFT1), _T(E), _T(nu), _T(ys), _T(np.full(B, tw.c.ground_friction)))
    honesty(tw)
    sim = _sim(N, B, (1,), (ROT[q],), (mu,))
    D = lambda a: _dev(sim, a)
    s = sim.reset()._replace(x=D(x), v=D(v), C=D(Cm), F=D(F), prim_pos=D(prim), softness=D(SOFT1), E=D(E), nu=D(nu), yield_stress=D(ys))
    for _ in range(2):
        s = sim.step(s, act)
    sim.check_status()
    for name, t, r in zip("xvCF", (s.x, s.v, s.C, s.F), ref):
        got = t.cpu().numpy()
        print(name, _rel(got, r.numpy()))
        assert np.isfinite(got).all() and _rel(got, r.numpy()) < 1e-9, (name, _rel(got, r.numpy()))
    np.testing.assert_allclose(s.prim_pos.cpu().numpy(), ref[4].numpy(), rtol=0, atol=1e-14)


# ---- b, c. adjoint ----------------------------------------------------------------------------------------------------------------
def _reference_adjoint(N, kinds, rot, mu, radius, h, scale, soft, two):
    torch.set_num_threads(8)
    B, P = 3, len(kinds)
    case = capsule_case(B, N, two=two)
    x, v, Cm, F, prim, act, E, nu, ys = case
    act = act / np.array(scale)                       # the same displacement whatever the scale
    rng = np.random.default_rng(9)
    w = [rng.normal(size=s) for s in W_SHAPES(B, N, P)]
    tw = _twin(N, kinds, rot, mu, radius, h, scale)
    leaves = dict(x=_T(x, True), v=_T(v, True), C=_T(Cm, True), F=_T(F, True), prim=_T(prim, True), act=_T(act, True), E=_T(E, True),
                  nu=_T(nu, True), ys=_T(ys, True), fric=_T(np.full(B, tw.c.ground_friction), True))
    out = tw.step(leaves["x"], leaves["v"], leaves["C"], leaves["F"], leaves["prim"], leaves["act"], _T(soft), leaves["E"], leaves["nu"],
                  leaves["ys"], leaves["fric"])
    honesty(tw)
    sum((o * _T(wi)).sum() for o, wi in zip(out, w)).backward()
    grads = {k: t.grad.numpy().copy() for k, t in leaves.items()}
    assert np.abs(grads["prim"][:, 0]).max() > 0 and np.abs(grads["act"]).max() > 0
    values = dict(x=x, v=v, C=Cm, F=F, prim=prim, act=act, E=E, nu=nu, ys=ys)
    return values, [o.detach().numpy() for o in out], w, grads


@functools.lru_cache(maxsize=None)          # one reference per configuration, shared by the cases that differ on the HIP side only
def _ref_single(scale):
    return _reference_adjoint(300, (1,), (ROT["tilted"],), (0.9,), (RADIUS,), (HEIGHT,), scale, SOFT1, False)


def _check_adjoint(sim, ref, soft):
    values, out, w, grads = ref
    hl = {k: _dev(sim, a, True) for k, a in values.items()}
    s = sim.reset()._replace(x=hl["x"], v=hl["v"], C=hl["C"], F=hl["F"], prim_pos=hl["prim"], softness=_dev(sim, soft), E=hl["E"], nu=hl["nu"],
                             yield_stress=hl["ys"])
    s1 = sim.step(s, hl["act"])
    res = (s1.x, s1.v, s1.C, s1.F, s1.prim_pos)
    for o, t, name in zip(out, res, "xvCFp"):
        assert _rel(t.detach().cpu().numpy(), o) < 1e-9, (name, _rel(t.detach().cpu().numpy(), o))
    sim.ground_friction_grad = None
    sum((t * _dev(sim, wi)).sum() for t, wi in zip(res, w)).backward()
    sim.check_status()
    for name in ("x", "v", "C", "F", "prim", "act", "E", "nu", "ys"):
        got = hl[name].grad.cpu().numpy()
        print(name, _rel(got, grads[name]))
        assert np.isfinite(got).all() and _rel(got, grads[name]) < 1e-6, (name, _rel(got, grads[name]))
    gfr = sim.ground_friction_grad.cpu().numpy()
    print("fric", gfr, grads["fric"])
    assert np.abs(grads["fric"]).max() > 0          # the rod stands on the floor: the friction branch ran
    assert _rel(gfr, grads["fric"]) < 1e-6, (gfr, grads["fric"])


@pytest.mark.gpu
@pytest.mark.parametrize("ckpt,lanes,scale", [(0, 0, 1.0), (27, 0, 1.0), (27, 1, 1.0), (27, 4, 1.0), (27, 8, 1.0), (27, 0, 0.01)])
def test_hip_capsule_adjoint_matches_autograd_through_the_twin(ckpt, lanes, scale):
    """ud_plb_step_bwd on a Capsule handle where the grid is recomputed (grid_ckpt_cells 0) and where it is restored, with every lane
    mapping, and with writer.yml's action scale.  Leaves: x, v, C, F, prim_pos, action, E, nu, yield_stress, ground friction."""
    scale3 = (scale,) * 3
    sim = _sim(300, 3, (1,), (ROT["tilted"],), (0.9,), scale=scale3, ckpt=ckpt, lanes=lanes)
    _check_adjoint(sim, _ref_single(scale3), SOFT1)


@pytest.mark.gpu
def test_hip_capsule_and_sticky_sphere_on_one_handle():
    """Primitive 0 a Capsule, primitive 1 a sticky Sphere, both in the rod: forward 1e-9, adjoint 1e-6."""
    soft = np.array([[666.0, 666.0], [0.0, 666.0], [666.0, 666.0]])
    kinds, rot, mu, radius, h = (1, 0), (ROT["tilted"], ROT["identity"]), (0.9, 0.0), (RADIUS, 0.025), (HEIGHT, 0.0)
    ref = _reference_adjoint(300, kinds, rot, mu, radius, h, (1.0, 1.0, 1.0), soft, True)
    assert np.abs(ref[3]["prim"][:, 1]).max() > 0        # the sphere touches the cloud too
    sim = _sim(300, 3, kinds, rot, mu, radius, h)
    _check_adjoint(sim, ref, soft)


# ---- d. contact loss --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("soft_contact", [True, False])
def test_hip_capsule_contact_loss_matches_the_twin(soft_contact):
    """As test_hip_losses_match_torch_twin (N = 1000, n_grid 64), primitive 0 a tilted Capsule beside the body, primitive 1 a Sphere."""
    B, N = 2, 1000
    kinds, rot, mu, radius, h = (1, 0), (ROT["tilted"], ROT["identity"]), (0.0, 0.0), (0.03, 0.025), (0.06, 0.0)
    tw = PlbPrimTwin(PlbConf(n_particles=N, radius=radius), kinds=kinds, h=h, rot=rot, mu=mu)
    rng = np.random.default_rng(2)
    x = np.stack([torus_particles(1000), torus_particles(1000) + rng.normal(size=(1000, 3)) * 0.003])
    prim = np.array([[[0.44, 0.28, 0.5], [0.55, 0.62, 0.5]], [[0.5, 0.35, 0.56], [0.5, 0.1, 0.5]]])
    td = tw.grid_mass(torch.tensor((torus_particles(1000) + np.array([0.004, -0.01, 0.0]))[None]))[0]
    ts = torch.tensor(rng.normal(size=tw.c.n_grid ** 3))
    wts = (3.0, 0.7, 1.3)
    tx, tp = _T(x, True), _T(prim, True)
    total, parts = tw.loss(tx, tp, td, ts, wts, soft_contact=soft_contact)
    gl = np.array([1.0, -2.5])
    (total * _T(gl)).sum().backward()
    assert np.abs(tp.grad.numpy()[:, 0]).max() > 0 and float(parts.detach()[:, 0].min()) > 0
    d0 = tw.sdf(0, _T(x), _T(prim)[:, 0, None, :])
    assert int((d0 > 0).sum()) > 100 and float(d0.abs().min()) > 1e-9      # the max(sdf, 0) of nearly every particle is in its open arm
    sim = _sim(N, B, kinds, rot, mu, radius, h, substeps=19, quality=1.0)
    hx, hp = _dev(sim, x, True), _dev(sim, prim, True)
    st = sim.reset()._replace(x=hx, prim_pos=hp)
    hloss, hparts = sim.compute_loss(st, td.numpy(), ts.numpy(), wts, soft_contact)
    assert _rel(hloss.detach().cpu().numpy(), total.detach().numpy()) < 1e-11
    assert _rel(hparts.cpu().numpy(), parts.detach().numpy()) < 1e-11
    (hloss * _dev(sim, gl)).sum().backward()
    assert _rel(hx.grad.cpu().numpy(), tx.grad.numpy()) < 1e-9 and _rel(hp.grad.cpu().numpy(), tp.grad.numpy()) < 1e-9


# ---- e. the Writer task's own shape ------------------------------------------------------------------------------------------------
def _writer_reference(act):
    from unidom_amd.engine.plb_simulator import WriterConf
    torch.set_num_threads(8)
    w = WriterConf()
    conf = PlbConf(quality=w.quality, n_particles=w.n_particles, E=w.E, nu=w.nu, yield_stress=w.yield_stress, gravity=w.gravity,
                   ground_friction=w.ground_friction, radius=w.prim_radius, lower_bound=w.lower_bound, upper_bound=w.upper_bound)
    tw = PlbPrimTwin(conf, kinds=w.prim_kind, h=w.prim_h, rot=w.prim_rot, mu=w.prim_friction, action_scale=w.action_scale, substeps=2)
    return w, tw


@pytest.mark.gpu
def test_hip_writer_shape_forward_matches_the_twin():
    """WriterConf: 10 000 particles, n_grid 64, ground_friction 100 (the floor's all-zeroed branch), one frictionless Capsule turned by
    init_rot, action scale 0.01; two substeps, one env, forward only, from reset() -- with the Capsule nudged off the lattice: at
    writer.yml's init_pos (0.5, 0.13, 0.5) the grid nodes x = z = 0.5 lie exactly on its axis, where the normal is the zero vector and
    w . D = 0 exactly, the one place where a last-bit difference could pick the other arm."""
    from unidom_amd.engine.plb_simulator import PlbSimulator
    act = np.array([[0.3, -1.0, 0.2]])
    w, tw = _writer_reference(act)
    w.substeps = 2
    sim = PlbSimulator(w, batch_size=1)
    assert sim.launch_plan() == 1 and (sim.n_particles, sim.n_grid, sim.substeps) == (10000, 64, 2) and w.ground_friction == 100.0
    s0 = sim.reset()
    assert s0.x.shape == (1, 10000, 3) and s0.prim_pos.shape == (1, 1, 3)
    np.testing.assert_array_equal(s0.prim_pos.cpu().numpy(), [[w.prim_init_pos[0]]])
    s0 = s0._replace(prim_pos=s0.prim_pos + _dev(sim, [0.0007, 0.0, -0.0004]))
    C = lambda t: t.cpu()
    with torch.no_grad():
        ref = tw.step(C(s0.x), C(s0.v), C(s0.C), C(s0.F), C(s0.prim_pos), _T(act), C(s0.softness), C(s0.E), C(s0.nu), C(s0.yield_stress),
                      _T([w.ground_friction]))
    honesty(tw)
    assert tw.bottom_all_zeroed > 100                 # the ground_friction >= 10 branch stopped occupied bottom cells
    s1 = sim.step(s0, act)
    sim.check_status()
    for name, t, r in zip("xvCF", (s1.x, s1.v, s1.C, s1.F), ref):
        print(name, _rel(t.cpu().numpy(), r.numpy()))
        assert _rel(t.cpu().numpy(), r.numpy()) < 1e-9, (name, _rel(t.cpu().numpy(), r.numpy()))
    np.testing.assert_allclose(s1.prim_pos.cpu().numpy(), ref[4].numpy(), rtol=0, atol=1e-14)
    assert abs(float(s1.prim_pos[0, 0, 1]) - (0.13 - 0.01)) < 1e-14        # clip(-1) * 0.01 over the two substeps, above lower_bound 0.05


# ---- f. contract -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_capsule_contract():
    from unidom_amd import _lib
    with pytest.raises(_lib.UnidomError, match=r"status -?\d+.*multi-kernel") as e:
        _sim(33, 1, (1,), (ROT["identity"],), (0.0,), path=2)
    assert f"status {UD_ERR['UNSUPPORTED']})" in str(e.value)
    for kinds, rot in (((1,), ((0.5, 0.0, 0.0, 0.0),)), ((2,), (ROT["identity"],))):
        with pytest.raises(_lib.UnidomError) as e:
            _sim(33, 1, kinds, rot, (0.0,))
        assert f"status {UD_ERR['INVALID']})" in str(e.value), str(e.value)
    # A conf whose new fields are all zero is the handle of before: bit for bit an explicitly Sphere-configured one.  Bit for bit is
    # only defined where no grid cell sums two particles (the p2g atomics add in whatever order the lanes arrive: two runs of ONE
    # handle differ in the last bits otherwise), so: three particles more than four cells apart, the sticky sphere on the first.
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    _, v, Cm, F, _, act, E, nu, ys = capsule_case(2, 3)
    x = np.array([[0.503, 0.301, 0.497], [0.21, 0.61, 0.33], [0.71, 0.45, 0.76]])[None].repeat(2, 0)
    prim = np.array([[0.51, 0.305, 0.49], [0.9, 0.9, 0.9]])[None].repeat(2, 0)
    assert PlbSimulator(HipConf(), batch_size=1).launch_plan() == 2     # a spelled-out Sphere conf (scale (1, 1, 1)) keeps the persistent path
    outs = []
    for explicit in (False, True):
        cfg = HipConf()
        cfg.quality, cfg.substeps, cfg.n_particles, cfg.path = 0.5, S, 3, 1
        if not explicit:
            cfg.prim_kind, cfg.prim_h, cfg.prim_rot, cfg.prim_friction, cfg.action_scale = (0, 0), (0.0, 0.0), ((0.0,) * 4,) * 2, (0.0, 0.0), (0.0,) * 3
        sim = PlbSimulator(cfg, batch_size=2)
        D = lambda a: _dev(sim, a)
        s = sim.reset()._replace(x=D(x), v=D(v), C=D(Cm), F=D(F), prim_pos=D(prim), E=D(E[:2]), nu=D(nu[:2]), yield_stress=D(ys[:2]))
        s = sim.step(s, act[:2])
        outs.append([t.cpu() for t in (s.x, s.v, s.C, s.F, s.prim_pos)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float((outs[0][1][:, 0] - torch.tensor(v)[:, 0]).abs().max()) > 1.0      # the sphere took the first particle along


def _header_codes():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidom_hip.h")).read()
    return {k: int(val) for k, val in re.findall(r"UD_ERR_(\w+)\s*=\s*(-?\d+)", src)}


UD_ERR = _header_codes()
