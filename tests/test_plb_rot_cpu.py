"""Rotating primitives of the PLB f64 path (six-dimensional actions, RollingPin): the torch restatement the HIP kernels are held to
(tests/plb_rot_twin.py) against the constant-orientation twin, known answers and central differences.  No GPU."""
import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf
from tests.plb_prim_twin import PlbPrimTwin, capsule_case, honesty
from tests.plb_rot_twin import HEIGHT, MU, RADIUS, PlbRotTwin, qmul, qrot, rot_case, w2quat

T = lambda a, r=False: torch.tensor(np.asarray(a, np.float64), requires_grad=r)
IDENT = (1.0, 0.0, 0.0, 0.0)
X90 = (np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0)          # a quarter turn about x: the pin's axis (local y) lies along world z


def _conf(N):
    conf = PlbConf(quality=0.5, n_particles=N, radius=(RADIUS,))
    assert conf.n_grid == 32
    return conf


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def test_identity_rotation_and_zero_spin_is_the_constant_orientation_twin():
    """(a) identity start rotation, zero angular action, six action dimensions: PlbPrimTwin with rot = identity to 1e-13 relative (not
    bit for bit: qmul renormalises)."""
    torch.set_num_threads(4)
    N = 33
    x, v, Cm, F, prim, act, E, nu, ys = capsule_case(1, N)
    common = [T([[666.0]]), T(E), T(nu), T(ys), T([0.5])]
    base = PlbPrimTwin(_conf(N), kinds=(1,), h=(HEIGHT,), rot=(IDENT,), mu=(MU,), substeps=2)
    ref = base.step(T(x), T(v), T(Cm), T(F), T(prim), T(act), *common)
    honesty(base)
    tw = PlbRotTwin(_conf(N), kinds=(1,), h=(HEIGHT,), mu=(MU,), action_dim=6, substeps=2)
    got = tw.step(T(x), T(v), T(Cm), T(F), T(prim), T([[IDENT]]), T(np.concatenate([act, np.zeros((1, 3))], 1)), *common)
    honesty(tw)
    for a, b, name in zip(got[:5], ref, ("x", "v", "C", "F", "prim_pos")):
        assert _rel(a, b) < 1e-13, (name, _rel(a, b))
    assert float((got[1] - T(v)).abs().max()) > 0
    assert torch.equal(got[5], T([[IDENT]]))


def test_quaternion_known_answers():
    """(b) qmul(w2quat((0, 0, theta)), identity) turns (1, 0, 0) to (cos theta, sin theta, 0); w2quat's identity arm."""
    for theta in (0.3, -1.1, 2.5):
        q = qmul(w2quat(T([0.0, 0.0, theta])), T(IDENT))
        got = qrot(q, T([1.0, 0.0, 0.0])).numpy()
        assert np.abs(got - [np.cos(theta), np.sin(theta), 0.0]).max() < 1e-15, (theta, got)
        assert abs(float((q * q).sum()) - 1) < 1e-15
    assert torch.equal(w2quat(T([0.0, 5e-10, 0.0])), T(IDENT)) and not torch.equal(w2quat(T([0.0, 2e-9, 0.0])), T(IDENT))


@pytest.mark.parametrize("dw", [0.4, -0.7])
def test_rolling_pin_rolls_along_minus_x(dw):
    """(b) init_rot a quarter turn about x: y_dir = qrot(q, (0, -1, 0)) = (0, 0, -1), cross((0, 1, 0), y_dir) = (-1, 0, 0), so a positive
    dw moves the pin along -x by 0.03 dw per substep; the turn about the object's own y leaves y_dir where it is, every substep the same."""
    S, scale = 3, (0.7, 0.05, 1.0)
    tw = PlbRotTwin(_conf(1), kinds=(2,), h=(HEIGHT,), mu=(0.0,), action_scale=scale, action_dim=3, substeps=S)
    pos, rot = T([[[0.5, 0.3, 0.5]]]), T([[X90]])
    a = T([[dw, 0.0, -0.2]])
    per = dw * scale[0] / S
    for f in range(S):
        pos1, rot = tw.kinematics(pos, rot, a)
        step = (pos1 - pos)[0, 0].numpy()
        assert np.abs(step - [-0.03 * per, -0.2 * scale[2] / S, 0.0]).max() < 1e-15, (f, step)
        assert abs(float(torch.sqrt((rot * rot).sum())) - 1) < 1e-15
        pos = pos1
    assert np.sign(float(pos[0, 0, 0]) - 0.5) == -np.sign(dw)


def _fd_case(rolling):
    N = 33
    case, kw = rot_case(1, N, rolling=rolling)
    rng = np.random.default_rng(5)
    w = [rng.normal(size=s) for s in ((1, N, 3), (1, N, 3), (1, N, 3, 3), (1, N, 3, 3), (1, 1, 3), (1, 1, 4))]

    def run(case, grad=False):
        tw = PlbRotTwin(_conf(N), h=(HEIGHT,), mu=(MU,), substeps=2, **kw)
        x, v, Cm, F, prim, rot, act, E, nu, ys = case
        leaves = dict(x=T(x, grad), prim=T(prim, grad), rot=T(rot, grad), act=T(act, grad))
        out = tw.step(leaves["x"], T(v), T(Cm), T(F), leaves["prim"], leaves["rot"], leaves["act"], T([[666.0]]), T(E), T(nu), T(ys), T([0.5]))
        return tw, leaves, sum((o * T(wi)).sum() for o, wi in zip(out, w))
    return case, run


@pytest.mark.parametrize("rolling", [False, True])
def test_rot_twin_autograd_is_the_derivative(rolling):
    """(c) central differences through two substeps of the pressed-in state the GPU tests use (one env of it), the rule of
    test_capsule_twin_autograd_is_the_derivative: h = 1e-6, |fd - an| < 1e-5 max(1, |an|).  Both kinematics; entries of the angular
    action (the RollingPin: of all three), the start rotation, the position, the linear action and one particle."""
    torch.set_num_threads(4)
    case, run = _fd_case(rolling)
    tw, leaves, loss = run(case, True)
    honesty(tw)
    loss.backward()
    names = ["x", "v", "C", "F", "prim", "rot", "act"]
    entries = [("rot", (0, 0, 0)), ("rot", (0, 0, 2)), ("prim", (0, 0, 0)), ("prim", (0, 0, 2)), ("act", (0, 0)), ("act", (0, 1)), ("act", (0, 2)),
               ("x", (0, 7, 1))]
    if not rolling:
        entries += [("act", (0, 3)), ("act", (0, 4)), ("act", (0, 5))]
    h = 1e-6
    for name, idx in entries:
        up, dn = list(case), list(case)
        k = names.index(name)
        up[k], dn[k] = case[k].copy(), case[k].copy()
        up[k][idx] += h; dn[k][idx] -= h
        fd = (float(run(tuple(up))[2]) - float(run(tuple(dn))[2])) / (2 * h)
        an = float(leaves[name].grad[idx])
        assert an != 0.0
        assert abs(fd - an) < 1e-5 * max(1.0, abs(an)), (name, idx, fd, an)


def test_zero_angular_action_sends_a_finite_zero_to_the_action():
    """(d) w = 0 takes w2quat's identity arm: the cotangent of act[3:6] is 0 and finite (no 0 * inf), that of the start rotation finite."""
    torch.set_num_threads(4)
    N = 33
    case, kw = rot_case(1, N)
    x, v, Cm, F, prim, rot, act, E, nu, ys = case
    act = act.copy()
    act[:, 3:] = 0.0
    tw = PlbRotTwin(_conf(N), h=(HEIGHT,), mu=(MU,), substeps=2, **kw)
    la, lr = T(act, True), T(rot, True)
    out = tw.step(T(x), T(v), T(Cm), T(F), T(prim), lr, la, T([[666.0]]), T(E), T(nu), T(ys), T([0.5]))
    rng = np.random.default_rng(6)
    sum((o * T(rng.normal(size=tuple(o.shape)))).sum() for o in out).backward()
    assert torch.isfinite(la.grad).all() and torch.equal(la.grad[:, 3:], torch.zeros(1, 3)) and float(la.grad[:, :3].abs().min()) > 0
    assert torch.isfinite(lr.grad).all() and float(lr.grad.abs().max()) > 0
