"""The Capsule primitive of the PLB f64 path (frictional soft contact, primive_base.py:57-115): the torch restatement the HIP
kernels are held to (tests/plb_prim_twin.py) against the base twin, known answers and central differences.  No GPU."""
import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf, torus_particles
from oracle.twin.plb_twin_torch import PlbTorchTwin
from tests.plb_prim_twin import PlbPrimTwin, capsule_case, honesty, qrot

T = lambda a, r=False: torch.tensor(np.asarray(a, np.float64), requires_grad=r)
Z90 = (np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5))          # 90 degrees about z: the capsule's axis (local y) lies along world -x


def test_two_sticky_spheres_are_the_base_twin_bit_for_bit():
    """Guards the copied substep: kind 0 everywhere must be PlbTorchTwin operation for operation."""
    N = 150
    rng = np.random.default_rng(0)
    x = torus_particles(1000)[:N].copy()
    v = rng.normal(size=(N, 3)) * 0.01
    Cm = rng.normal(size=(N, 3, 3)) * 0.1
    F = np.eye(3)[None] + rng.normal(size=(N, 3, 3)) * 0.002
    prim = np.array([x[3], [0.5, 0.55, 0.5]])
    conf = PlbConf(quality=0.5, n_particles=N)
    assert conf.n_grid == 32
    args = [T(a[None]) for a in (x, v, Cm, F, prim)] + [T([[0.3, -0.2, 0.1]]), T([[666.0, 666.0]]), T([5e3]), T([0.35]), T([1762.2]), T([0.5])]
    ref = PlbTorchTwin(conf).step(*args)
    got = PlbPrimTwin(conf).step(*args)
    for a, b, name in zip(got, ref, ("x", "v", "C", "F", "prim_pos")):
        assert torch.equal(a, b), name
    assert float((got[1] - args[1]).abs().max()) > 0


def _tw(q=(1.0, 0.0, 0.0, 0.0), mu=0.0):
    return PlbPrimTwin(PlbConf(quality=0.5, n_particles=1, radius=(0.03,)), kinds=(1,), h=(0.06,), rot=(q,), mu=(mu,))


@pytest.mark.parametrize("q,off,want", [((1.0, 0, 0, 0), (0.05, 0, 0), 0.02), ((1.0, 0, 0, 0), (0, 0.07, 0), 0.01),
                                        ((1.0, 0, 0, 0), (0, 0, 0), 1e-7 - 0.03), (Z90, (0.07, 0, 0), 0.01)])
def test_capsule_distance_known_answers_and_normal_is_its_gradient(q, off, want):
    tw = _tw(q)
    P = T([[0.5, 0.5, 0.5]])
    pt = np.array([0.5, 0.5, 0.5]) + np.array(off)
    f = lambda a: float(tw.sdf(0, T(a)[None], P)[0])
    assert abs(f(pt) - want) < 1e-12
    nrm = tw.normal(0, T(pt)[None], P)[0].numpy()
    h = 1e-6
    fd = np.array([(f(pt + h * e) - f(pt - h * e)) / (2 * h) for e in np.eye(3)])
    assert np.abs(fd - nrm).max() < 1e-6, (fd, nrm)


def _collide_inside(mu, u_rel):
    """one cell inside the capsule, 2 mm under its surface (softness 0: the dist <= 0 arm, influence 1); returns (u_out - cv, D, u - cv).
    Near the surface on purpose: the normal is p / sqrt(p.p + 1e-14), short of unit length by 1e-14 / (2 p.p) = 6e-12 here."""
    tw = _tw(Z90, mu)
    P0, P1 = T([[0.5, 0.5, 0.5]]), T([[0.5003, 0.4998, 0.5001]])
    g = T([[0.51, 0.52, 0.4804]])
    assert -0.0021 < float(tw.sdf(0, g, P0)) < -0.0019
    pl = tw.local(0, g - P0)[0]
    cv = (qrot(tw.q[0], pl) + P1 - g) / tw.c.dt
    u = cv[None] + T(u_rel)[None, None]
    out = tw.collide(0, g, u, P0, P1, T([0.0]))
    return (out - cv)[0, 0].numpy(), tw.normal(0, g, P0)[0].numpy(), np.asarray(u_rel, np.float64)


def test_collide_known_answers():
    rel, D, _ = _collide_inside(0.0, [0.0, 0.0, 0.0])
    assert np.abs(rel).max() < 1e-9                                            # u = cv stays cv (|t| = sqrt(1e-8) scales a zero vector)
    w = -0.02 * D + np.cross(D, [0.3, -0.1, 0.2])                              # pushes into the capsule: w . D < 0, and slides along it
    rel, D, _ = _collide_inside(0.0, w)
    assert w @ D < 0
    tang = w - (w @ D) * D
    assert abs(rel @ D) < 1e-12                                                # frictionless: the normal part is removed ...
    assert np.abs(rel - tang).max() < 1e-12 and np.linalg.norm(tang) > 0.1     # ... the tangential part kept: t / |t| * max(0, |t| + 0)
    rel, D, _ = _collide_inside(1e6, w)
    assert np.abs(rel).max() == 0.0                                            # large friction: the cell takes the collider's velocity


def test_capsule_twin_autograd_is_the_derivative():
    """Central differences through two substeps of the pressed-in state the GPU tests use (one env of it), the rule of
    test_torch_twin_is_the_numpy_twin_and_its_autograd_is_the_derivative: h = 1e-6, |fd - an| < 1e-5 max(1, |an|)."""
    torch.set_num_threads(4)
    N = 33
    conf = PlbConf(quality=0.5, n_particles=N, radius=(0.05,))
    q = tuple(np.array([0.9, 0.1, -0.3, 0.2]) / np.linalg.norm([0.9, 0.1, -0.3, 0.2]))
    case = capsule_case(1, N)
    rng = np.random.default_rng(5)
    w = [rng.normal(size=s) for s in ((1, N, 3), (1, N, 3), (1, N, 3, 3), (1, N, 3, 3), (1, 1, 3))]

    def run(case, grad=False):
        tw = PlbPrimTwin(conf, kinds=(1,), h=(0.12,), rot=(q,), mu=(0.9,), substeps=2)
        x, v, Cm, F, prim, act, E, nu, ys = case
        leaves = dict(x=T(x, grad), prim=T(prim, grad), act=T(act, grad))
        out = tw.step(leaves["x"], T(v), T(Cm), T(F), leaves["prim"], leaves["act"], T([[666.0]]), T(E), T(nu), T(ys), T([0.5]))
        return tw, leaves, sum((o * T(wi)).sum() for o, wi in zip(out, w))

    tw, leaves, loss = run(case, True)
    honesty(tw)
    loss.backward()
    names = ["x", "v", "C", "F", "prim", "act"]
    h = 1e-6
    for name, idx in (("act", (0, 0)), ("act", (0, 1)), ("prim", (0, 0, 0)), ("prim", (0, 0, 2)), ("x", (0, 7, 1))):
        up, dn = list(case), list(case)
        k = names.index(name)
        up[k], dn[k] = case[k].copy(), case[k].copy()
        up[k][idx] += h; dn[k][idx] -= h
        fd = (float(run(tuple(up))[2]) - float(run(tuple(dn))[2])) / (2 * h)
        an = float(leaves[name].grad[idx])
        assert an != 0.0
        assert abs(fd - an) < 1e-5 * max(1.0, abs(an)), (name, idx, fd, an)
