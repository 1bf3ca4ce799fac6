"""The Box / Cylinder / Torus twin (tests/plb_shape_twin.py) on its own, no GPU: known answers of the signed distances, the analytic
normals against the autograd gradient of the distance, the Box's finite-difference normal against it where no sample crosses a kink,
agreement with the existing twins where the geometry coincides, and the case builders with the conditions that keep the GPU
comparisons honest."""
import math

import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf
from tests import plb_shape_twin as T
from tests.plb_prim_twin import PlbPrimTwin, capsule_case
from tests.plb_rot_twin import HEIGHT, MU, RADIUS, PlbRotTwin, rot_case

DT = torch.float64
BOX_SIZE = torch.tensor([0.05, 0.03, 0.06], dtype=DT)
HR = torch.tensor([0.06, 0.04], dtype=DT)
TXY = torch.tensor([0.07, 0.025], dtype=DT)


def _T(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def _points():
    torch.manual_seed(0)
    return (torch.rand(20000, 3, dtype=DT) - 0.5) * 0.3


def _unit_gradient(f, pts):
    p = pts.clone().requires_grad_(True)
    g, = torch.autograd.grad(f(p).sum(), p)
    return g / torch.sqrt((g * g).sum(-1, keepdim=True))


def test_sdf_known_answers():
    pt = lambda *a: torch.tensor(a, dtype=DT)
    sx, sy, sz = (float(s) for s in BOX_SIZE)
    assert abs(float(T.box_sdf(BOX_SIZE, pt(sx + 0.03, -(sy + 0.04), sz + 0.12))) - math.sqrt(0.03 ** 2 + 0.04 ** 2 + 0.12 ** 2 + 1e-14)) < 1e-15   # corner
    assert abs(float(T.box_sdf(BOX_SIZE, pt(-(sx + 0.03), sy + 0.04, 0.01))) - math.sqrt(0.03 ** 2 + 0.04 ** 2 + 1e-14)) < 1e-15                   # edge
    assert abs(float(T.box_sdf(BOX_SIZE, pt(0.01, 0.0, sz + 0.02))) - math.sqrt(0.02 ** 2 + 1e-14)) < 1e-15                                          # face
    assert abs(float(T.box_sdf(BOX_SIZE, pt(0.0, 0.0, 0.0))) - (-sy + 1e-7)) < 1e-16                                                                  # centre: -min(size) + 1e-7
    # cylinder rim: 0.03 beyond the side, 0.04 beyond the cap
    l = math.sqrt(0.09 ** 2 + 1e-14)
    assert abs(float(T.cylinder_sdf(HR, pt(0.09, -0.08, 0.0))) - math.sqrt((l - 0.06) ** 2 + 0.04 ** 2 + 1e-14)) < 1e-15
    assert abs(float(T.cylinder_sdf(HR, pt(0.09, -0.08, 0.0))) - 0.05) < 1e-12
    # torus: a point on the ring's circle
    assert abs(float(T.torus_sdf(TXY, pt(0.0, 0.0, -0.07))) - (1e-7 - 0.025)) < 1e-14


@pytest.mark.parametrize("name", ["cylinder", "torus"])
def test_analytic_normal_is_the_gradient_of_the_sdf(name):
    sdf, normal, sc = (T.cylinder_sdf, T.cylinder_normal, HR) if name == "cylinder" else (T.torus_sdf, T.torus_normal, TXY)
    pts = _points()
    err = (normal(sc, pts) - _unit_gradient(lambda p: sdf(sc, p), pts)).abs().max()
    print(name, float(err))
    assert float(err) < 1e-12


def test_box_finite_difference_normal_against_the_gradient():
    pts = _points()

    def side(y):                                                     # which side of every kink a point lies on
        q = y.abs() - BOX_SIZE
        return torch.cat([torch.sign(y), torch.sign(q), q.argmax(-1, keepdim=True).to(DT)], -1)
    keep = torch.ones(len(pts), dtype=torch.bool)
    for i in range(3):
        for s in (T.FD, -T.FD):
            e = torch.zeros(3, dtype=DT)
            e[i] = s
            keep &= (side(pts + e) == side(pts)).all(-1)
    dropped = 1 - float(keep.to(DT).mean())
    n, g = T.box_normal(BOX_SIZE, pts)[keep], _unit_gradient(lambda p: T.box_sdf(BOX_SIZE, p), pts)[keep]
    err = (n - g).abs().max(-1).values
    print("dropped", dropped, "worst", float(err.max()), "median", float(err.median()))
    assert dropped <= 0.02
    assert float(err.max()) < 1e-3
    # face regions, at least 1e-3 from every edge (and from the centre planes): +-e_i
    q = pts.abs() - BOX_SIZE
    top = q.sort(-1, descending=True)
    i = top.indices[:, 0]
    face = (top.values[:, 1] < -1e-3) & (top.values[:, 0] - top.values[:, 1] > 1e-3) & (pts.gather(1, i[:, None])[:, 0].abs() > 1e-3)
    assert int(face.sum()) > 1000
    want = torch.zeros_like(pts).scatter(1, i[:, None], torch.sign(pts.gather(1, i[:, None])))
    assert float((T.box_normal(BOX_SIZE, pts) - want)[face].abs().max()) < 1e-9


def _run(tw, case, soft, rot):
    x, v, Cm, F, prim = case[:5]
    rest = case[5:]
    with torch.no_grad():
        if rot:
            return tw.step(*map(_T, (x, v, Cm, F, prim, rest[0], rest[1])), _T(soft), *map(_T, rest[2:]), _T(np.full(len(x), tw.c.ground_friction)))
        return tw.step(*map(_T, (x, v, Cm, F, prim, rest[0])), _T(soft), *map(_T, rest[1:]), _T(np.full(len(x), tw.c.ground_friction)))


def test_capsule_through_the_shape_twin_is_the_existing_twins_bit_for_bit():
    B, N = 3, 33
    soft = np.full((B, 1), 666.0)
    conf = PlbConf(quality=0.5, n_particles=N, radius=(RADIUS,))
    case, kw = rot_case(B, N)
    old = _run(PlbRotTwin(conf, h=(HEIGHT,), mu=(MU,), substeps=3, **kw), case, soft, True)
    new = _run(T.PlbShapeTwin(conf, kinds=(1,), h=(HEIGHT,), mu=(MU,), substeps=3, action_scale_w=kw["action_scale_w"], action_dim=6, rot_state=True),
               case, soft, True)
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    case = capsule_case(B, N)
    q = (0.9, 0.1, -0.3, 0.2)
    old = _run(PlbPrimTwin(conf, kinds=(1,), h=(HEIGHT,), rot=(q,), mu=(MU,), substeps=3), case, soft, False)
    new = _run(T.PlbShapeTwin(conf, kinds=(1,), h=(HEIGHT,), rot=(q,), mu=(MU,), substeps=3), case, soft, False)
    assert all(torch.equal(a, b) for a, b in zip(old, new))


def test_thin_torus_is_nearly_a_sphere():
    """tx = 1e-3 ty: the ring has all but collapsed to a point, the Torus is a sphere of radius ty up to tx.  A sanity check of the
    restatement against the Capsule twin with h = 0, not a tolerance test."""
    ty = 0.05
    conf = PlbConf(quality=0.5, n_particles=33, radius=(ty,))
    torus = T.PlbShapeTwin(conf, kinds=(T.TORUS,), shape=((1e-3 * ty, ty, 0.0),), rot=((0.9, 0.1, -0.3, 0.2),))
    ball = PlbPrimTwin(conf, kinds=(1,), h=(0.0,), rot=((0.9, 0.1, -0.3, 0.2),))
    ar = torch.arange(32, dtype=DT) / 32
    gp = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(1, -1, 3)
    pos = torch.tensor([[[0.5093, 0.2931, 0.4968]]], dtype=DT)
    far = ((gp - pos) ** 2).sum(-1).sqrt() > ty / 2
    assert float((torus.sdf(0, gp, pos) - ball.sdf(0, gp, pos))[far].abs().max()) <= 2e-3 * ty
    assert float((torus.normal(0, gp, pos) - ball.normal(0, gp, pos))[far].abs().max()) <= 1e-2


@pytest.mark.parametrize("kind", [T.BOX, T.CYLINDER, T.TORUS])
def test_shape_cases_are_honest(kind):
    """Every case the GPU tests run: the contact's own conditions, no cell near a kink of the shape, and every region of the shape
    reached by active occupied cells."""
    torch.set_num_threads(8)
    B = 3
    counts = []
    for rot in (False, True):
        for N, mu in ((33, 0.7), (300, 0.0), (300, 0.7)):
            case, soft, kw = T.shape_case(kind, B, N, rot)
            tw = T.PlbShapeTwin(PlbConf(quality=0.5, n_particles=N, radius=(0.03,)), mu=(mu,), substeps=3, **kw)
            out = _run(tw, case, soft, rot)
            assert all(bool(torch.isfinite(o).all()) for o in out)
            least, count = T.honesty_shape(tw)
            print(T.NAMES[kind], rot, N, mu, least, count)
            T.assert_regions(kind, [count])
            counts.append(count)
    T.assert_regions(kind, counts)
