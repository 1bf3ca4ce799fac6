"""The Chopsticks twin (tests/plb_chopsticks_twin.py) checked by itself, without a GPU: known answers of its signed distance (which a reading
with the sticks centred on the primitive's position fails), the right-multiplied rotation step against a hand-written Hamilton product,
a reduction of a whole step to the Capsule twin's, the gap clamp's zero gradient, and the shared cases against honesty_chop.  PARITY
UNPINNED by reference data (taichi is absent, no chopsticks.yml, no recording): the twin is the specification the kernels are held to."""
import numpy as np
import torch

from oracle.twin.plb_twin import PlbConf
from oracle.twin.plb_twin_torch import DT
from tests import plb_chopsticks_twin as T
from tests.plb_rot_twin import PlbRotTwin, qmul, qrot, w2quat

S, B = 3, 3
H, R = T.H, T.R


def _t(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def _twin(N, kw, mu=(0.7,), radius=(R, 0.025), **more):
    P = len(kw["kinds"])
    return T.PlbChopsticksTwin(PlbConf(quality=0.5, n_particles=N, radius=radius[:P]), mu=mu, substeps=S, **{**kw, **more})


def test_sdf_known_answers_put_the_position_at_the_top_end():
    """Local (gap/2, 0, 0) lies on stick a's axis, at its top end: -r.  (gap/2, h/2, 0) lies h/2 above that end: h/2 - r (0 at the reference's
    defaults).  A reading with the sticks centred on the position would give -r for both.  length() carries its 1e-14: sqrt(1e-14) = 1e-7."""
    for gap in (0.06, 0.1):
        g = _t(gap)
        top = T.chop_sdf(H, R, g, _t([gap / 2, 0.0, 0.0]))
        above = T.chop_sdf(H, R, g, _t([gap / 2, H / 2, 0.0]))
        bottom = T.chop_sdf(H, R, g, _t([-gap / 2, -H, 0.0]))
        below = T.chop_sdf(H, R, g, _t([-gap / 2, -H - 0.05, 0.0]))
        assert abs(float(top) + R) < 2e-7 and abs(float(bottom) + R) < 2e-7
        assert abs(float(above) - (H / 2 - R)) < 1e-12 and abs(float(below) - (0.05 - R)) < 1e-12
        assert abs(float(above) - float(top)) > 0.02
    # the normal is the selected stick's: on the +x side stick a's, pointing away from its axis
    n = T.chop_normal(H, R, _t(0.1), _t([0.05 + 0.04, -0.03, 0.0]))
    assert np.allclose(n.numpy(), [1.0, 0.0, 0.0], atol=1e-12)
    n = T.chop_normal(H, R, _t(0.1), _t([-0.05 - 0.04, -0.03, 0.0]))
    assert np.allclose(n.numpy(), [-1.0, 0.0, 0.0], atol=1e-12)
    # through the twin, behind inv_trans with the identity: the same numbers
    tw = _twin(33, dict(kinds=(T.CHOPSTICKS,), h=(H, 0.0)))
    tw._gap = _t([[0.1]])
    d = tw.sdf_q(0, _t([[[0.55, 0.3 + H / 2, 0.5]]]), _t([[[0.5, 0.3, 0.5]]]), _t([[1.0, 0.0, 0.0, 0.0]]))
    assert abs(float(d) - (H / 2 - R)) < 1e-12


def test_rotation_step_multiplies_on_the_right():
    q = _t(T.TILT) / np.linalg.norm(T.TILT)
    w = _t([0.3, -0.2, 0.25])
    right, left = qmul(q, w2quat(w)), qmul(w2quat(w), q)
    assert float((right - left).abs().max()) > 1e-3                                   # the pair does not commute
    by_hand = T.qmul_right_by_hand(q, w2quat(w))
    assert float((right - by_hand).abs().max()) < 1e-15
    # ... and the twin's kinematics take that one
    tw = _twin(33, dict(kinds=(T.CHOPSTICKS,), h=(H, 0.0), action_scale_w=(1.0, 1.0, 1.0)))
    a = torch.cat([torch.zeros(3, dtype=DT), w * S, torch.zeros(1, dtype=DT)])[None]
    _, r1, g1 = tw.kinematics(_t([[[0.5, 0.3, 0.5]]]), q[None, None], _t([[0.1]]), a)
    assert float((r1[0, 0] - by_hand).abs().max()) < 1e-15 and float((r1[0, 0] - left).abs().max()) > 1e-3
    assert float(g1[0, 0]) == 0.1


def test_gap_clamp_sends_no_gradient_on_the_clamped_arm():
    tw = _twin(33, dict(kinds=(T.CHOPSTICKS,), h=(H, 0.0), min_gap=(0.06, 0.0), action_scale_gap=0.03))
    pos, rot = _t([[[0.5, 0.3, 0.5]]] * 2), _t([[[1.0, 0.0, 0.0, 0.0]]] * 2)
    gap = _t([[0.069], [0.061]], True)                                                # gap_vel = 0.006: env 0 stays open, env 1 hits the floor
    a = _t([[0, 0, 0, 0, 0, 0, 0.6]] * 2, True)
    _, _, g1 = tw.kinematics(pos, rot, gap, a)
    assert np.allclose(g1.detach().numpy()[:, 0], [0.063, 0.06], atol=1e-15)
    g1.sum().backward()
    assert gap.grad[0, 0] == 1.0 and gap.grad[1, 0] == 0.0
    assert abs(float(a.grad[0, 6]) + 0.03 / S) < 1e-15 and a.grad[1, 6] == 0.0


def test_one_stick_alone_is_the_capsule_twin():
    """With stick b out of reach of every occupied cell, w = 0 and gap_vel = 0 a whole step is the Capsule twin's step with the Capsule at
    P + qrot(q, (gap/2, -h/2, 0)), to 1e-12.  The rotation is unit here: rot[0] is used as given, and with |q| != 1 the Capsule's own frame
    and the stick's would differ in how the offset is carried from substep to substep."""
    torch.set_num_threads(8)
    N, gap = 33, 0.5
    case, soft, kw = T.chop_case(B, N)
    x, v, Cm, F, prim, r, g, act, E, nu, ys = case
    q = np.array(T.TILT) / np.linalg.norm(T.TILT)
    r[:, 0] = q
    off = qrot(_t(q), _t([gap / 2, -H / 2, 0.0])).numpy()
    target = prim[:, 0] + np.array([0.03, -0.03, 0.0])                                # where stick a's Capsule is to sit: in the rod
    prim[:, 0] = target - off
    g[:, 0] = gap
    act[:, 3:] = 0.0
    tw = _twin(N, kw)
    fr = _t(np.full(B, tw.c.ground_friction))
    with torch.no_grad():
        got = tw.step(*map(_t, (x, v, Cm, F, prim, r, g, act)), _t(soft), _t(E), _t(nu), _t(ys), fr)
    seen = 0
    for d in tw.diag:                                                                 # stick a is the nearer one at every occupied cell, b acts nowhere
        a_, b_, _, _ = T.chop_sticks(H, R, d["gap"][:, None], d["pl"])
        assert bool((a_ <= b_)[d["occ"]].all()) and float((b_ - R)[d["occ"]].min()) > 0.1
        seen += int((d["occ"] & d["active"]).sum())
    assert seen > 50
    cap = PlbRotTwin(PlbConf(quality=0.5, n_particles=N, radius=(R,)), kinds=(1,), h=(H,), mu=(0.7,), action_dim=6, substeps=S)
    prim_c = prim.copy()
    prim_c[:, 0] = target
    with torch.no_grad():
        ref = cap.step(*map(_t, (x, v, Cm, F, prim_c, r, act[:, :6])), _t(soft), _t(E), _t(nu), _t(ys), fr)
    for name, a, b in zip(("x", "v", "C", "F"), got[:4], ref[:4]):
        err = float((a - b).abs().max() / b.abs().max())
        assert err < 1e-12, (name, err)
    assert float((got[4][:, 0] + _t(off) - ref[4][:, 0]).abs().max()) < 1e-15
    assert float((got[0] - _t(x)).abs().max()) > 1e-6 and float((got[6] - _t(g)).abs().max()) == 0.0


def test_shared_cases_pass_honesty_on_the_twin_alone():
    """The cases of tests/test_plb_chopsticks_gpu.py, chosen here on the CPU: both sticks act on occupied cells in the cap and the side region,
    nothing sits near a branch point, the a = b plane or the gap clamp, and the three envs take the three arms of the gap kinematics."""
    torch.set_num_threads(8)
    for N, two in ((33, False), (300, False), (300, True)):
        case, soft, kw = T.chop_case(B, N, two=two)
        P = case[4].shape[1]
        tw = _twin(N, kw, mu=(0.7, 0.0)[:P])
        with torch.no_grad():
            out = tw.step(*map(_t, case[:8]), _t(soft), *map(_t, case[8:]), _t(np.full(B, tw.c.ground_friction)))
        worst, count = T.honesty_chop(tw)
        assert min(count.values()) >= 20, count
        pre = torch.stack(tw.gap_log[-S:]).numpy()                                    # [S,B]: gap[f] - gap_vel
        assert (pre[:, 0] > T.MIN_GAP).all()                                          # env 0 opens, never clamped
        assert pre[0, 1] > T.MIN_GAP and (pre[1:, 1] < T.MIN_GAP).all()               # env 1 reaches the clamp in the second substep
        assert (pre[:, 2] < T.MIN_GAP).all()                                          # env 2 clamped throughout
        gap1 = out[6].numpy()
        assert abs(gap1[0, 0] - 0.085) < 1e-12 and gap1[1, 0] == T.MIN_GAP and gap1[2, 0] == T.MIN_GAP
        assert float((out[5][:, 0] - _t(case[5])[:, 0]).abs().max()) > 1e-3           # the sticks turned
