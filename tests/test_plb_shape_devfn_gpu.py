"""The shape layer of csrc/plb_prim.h on its own on the GPU -- plb_shape_sdf, plb_shape_normal, plb_shape_adj behind the test-only launcher
tests/devfn/plb_shape.hip (libdevfn.so, compiled with the flags of plb.o / plb_adj.o) -- against tests/plb_shape_twin.py's geometry and its
autograd, point by point.  This is the guard of the Box normal's adjoint: through a whole step the derivative of the finite-difference
formula and the derivative of an analytic normal differ by 1e-6 of a leaf at the most (few cells lie on edges, docs/HISTORY.md); here
every point is its own case and the two differ by orders more than the bar.

20 000 uniform points of a 0.3-cube (torch.manual_seed(0)) with the sizes of tests/test_plb_shape_cpu.py, random cotangents of distance and
normal.  Points within 1e-9 of a kink (honesty_shape's list: for the Box at pl and its six samples) or within 1e-3 of the Cylinder's / Torus's
axis or the ring's centre line are dropped; points whose samples STRADDLE a kink of the Box stay: both sides take the same arms.

Bars, per point, relative to 1 + the point's own max-norm, from the formats and not from the code: the distance is a handful of f64
operations on numbers below 1: 1e-14.  The Box normal divides a difference of two such distances by 2 d = 2e-4, so each side carries
eps * 0.3 / 2e-4 = 2e-13 before the normalisation: 1e-11, taken for all kinds.  The cotangent: the Box forms (0.5 / d) = 5e3 times a
difference of two gradients with unit components, each a few eps off, on both sides: 1e-11 absolute per unit cotangent, and the
normalisation's adjoint carries the normal's 2e-13 through a second division; Cylinder and Torus divide by l >= 1e-3 twice where the value
itself grows as 1 / l.  1e-9 leaves two orders above those estimates and is three below the 1e-6 the step's leaves are held to.
Measured on an MI355X: see docs/HISTORY.md."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import plb_shape_twin as T

pytestmark = pytest.mark.gpu

SO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devfn", "libdevfn.so")
SHAPE = {T.BOX: (0.05, 0.03, 0.06), T.CYLINDER: (0.06, 0.04, 0.0), T.TORUS: (0.07, 0.025, 0.0)}
SDF = {T.BOX: T.box_sdf, T.CYLINDER: T.cylinder_sdf, T.TORUS: T.torus_sdf}
NORMAL = {T.BOX: T.box_normal, T.CYLINDER: T.cylinder_normal, T.TORUS: T.torus_normal}
N = 20000


@functools.lru_cache(maxsize=None)
def _lib():
    assert os.path.exists(SO), f"{SO} is missing: __graft_entry__.build() (make -C unidom_amd/csrc devfn) builds it"
    return C.CDLL(SO)


def _device(kind, pl, gdist, gnl, pad=7):
    """-> dist [n], nl [n, 3], g [n, 3] of the launcher, and the rows past n, which it must leave untouched"""
    n = pl.shape[0]
    dev = [t.contiguous().cuda() for t in (pl, gdist, gnl)]
    outs = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((n + pad,), (n + pad, 3), (n + pad, 3))]
    consts = (C.c_double * 5)(*SHAPE[kind], 0.0, 0.0)
    fn = _lib().devfn_plb_shape
    fn.restype = C.c_int
    rc = fn(C.c_int(kind), consts, *[C.c_void_p(t.data_ptr()) for t in dev + outs], C.c_long(n))
    assert rc == 0, f"devfn_plb_shape: hipError {rc}"
    torch.cuda.synchronize()
    outs = [o.cpu() for o in outs]
    assert all(bool(torch.isnan(o[n:]).all()) for o in outs), "rows past n were written"
    return [o[:n] for o in outs]


def _away_from_kinks(kind, pl):
    sc = torch.tensor(SHAPE[kind], dtype=T.DT)
    if kind == T.BOX:
        ok = torch.ones(pl.shape[0], dtype=torch.bool)
        for i in range(-1, 3):
            for s in ((0.0,) if i < 0 else (T.FD, -T.FD)):
                e = torch.zeros(3, dtype=T.DT)
                if i >= 0:
                    e[i] = s
                y = pl + e
                q = y.abs() - sc
                top = q.sort(-1).values
                ok &= (q.abs() > 1e-9).all(-1) & (y.abs() > 1e-9).all(-1) & ((top[:, 2] > 0) | ((top[:, 2] - top[:, 1]).abs() > 1e-9))
        return ok
    if kind == T.CYLINDER:
        l, d = T.cylinder_d(sc[:2], pl)
        return (d.abs() > 1e-9).all(-1) & (pl[:, 1].abs() > 1e-9) & ((d.max(-1).values > 0) | ((d[:, 0] - d[:, 1]).abs() > 1e-9)) & (l > 1e-3)
    l, q = T.torus_q(sc[:2], pl)
    return (l > 1e-3) & (T.length(q) > 1e-3)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """points, cotangents, the twin's distance / normal / cotangent of pl, and the device's"""
    torch.manual_seed(0)
    pl = (torch.rand(N, 3, dtype=T.DT) - 0.5) * 0.3
    gdist, gnl = torch.randn(N, dtype=T.DT), torch.randn(N, 3, dtype=T.DT)
    keep = _away_from_kinks(kind, pl)
    assert int(keep.sum()) > 0.99 * N
    pl, gdist, gnl = pl[keep], gdist[keep], gnl[keep]
    sc = torch.tensor(SHAPE[kind], dtype=T.DT)
    sc = sc if kind == T.BOX else sc[:2]
    p = pl.clone().requires_grad_(True)
    dist, nl = SDF[kind](sc, p), NORMAL[kind](sc, p)
    g, = torch.autograd.grad((gdist * dist).sum() + (gnl * nl).sum(), p)
    return pl, gdist, gnl, dist.detach(), nl.detach(), g, _device(kind, pl, gdist, gnl)


def _err(got, ref):
    """per point, relative to 1 + the point's own max-norm"""
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return (got - ref).abs().max(-1).values / (1 + ref.abs().max(-1).values)


@pytest.mark.parametrize("kind", [T.BOX, T.CYLINDER, T.TORUS], ids=["Box", "Cylinder", "Torus"])
def test_shape_layer_matches_the_twin_point_by_point(kind):
    pl, gdist, gnl, dist, nl, g, (ddist, dnl, dg) = _case(kind)
    worst = [float(_err(a, b).max()) for a, b in ((ddist, dist), (dnl, nl), (dg, g))]
    print(T.NAMES[kind], "points", pl.shape[0], "dist %.2e  normal %.2e  g_pl %.2e" % tuple(worst))
    assert all(bool(torch.isfinite(t).all()) for t in (ddist, dnl, dg))
    assert worst[0] < 1e-14 and worst[1] < 1e-11 and worst[2] < 1e-9, worst


def test_box_adjoint_is_the_finite_difference_formulas_own():
    """The adjoint built on the analytic normal (the normalised gradient of _sdf) misses the bar that the kernel's holds on nearly every
    edge or corner point, and on every point with a sample across a kink of q, by orders: the bar tells the two apart."""
    pl, gdist, gnl, dist, nl, g, (_, _, dg) = _case(T.BOX)
    sc = torch.tensor(SHAPE[T.BOX], dtype=T.DT)
    p = pl.clone().requires_grad_(True)
    sdf = T.box_sdf(sc, p)
    grad, = torch.autograd.grad(sdf.sum(), p, create_graph=True)
    ga, = torch.autograd.grad((gdist * sdf).sum() + (gnl * T.normalize(grad)).sum(), p)
    q = pl.abs() - sc
    edge = (q > 0).sum(-1) >= 2
    straddle = torch.zeros(pl.shape[0], dtype=torch.bool)
    for i in range(3):
        for s in (T.FD, -T.FD):
            e = torch.zeros(3, dtype=T.DT)
            e[i] = s
            straddle |= (((pl + e).abs() - sc > 0) != (q > 0)).any(-1)
    miss = _err(dg, ga)
    print("edge or corner points", int(edge.sum()), "of them past 1e-9 against the analytic-normal adjoint %.3f, median %.2e;" %
          (float((miss[edge] > 1e-9).double().mean()), float(miss[edge].median())),
          "points with a sample across q_i = 0:", int(straddle.sum()), "least %.2e" % float(miss[straddle & edge].min()))
    assert int(edge.sum()) > 1000 and int((straddle & edge).sum()) > 10
    assert float(_err(dg, g).max()) < 1e-9
    assert float((miss[edge] > 1e-9).double().mean()) > 0.9
    assert float(miss[straddle & edge].min()) > 1e-6          # a second derivative that jumps between the samples: off by its own size
