"""The Chopsticks primitive of the PLB f64 path on the GPU (prim_kind 6: the GEN = 5 instantiations, the gap kinematics and the *_gap entry
points) against the torch restatement tests/plb_chopsticks_twin.py and its autograd.  PARITY UNPINNED by reference data (taichi is absent,
the reference ships no chopsticks.yml and no recording): the restatement is the specification.
quality 0.5 (n_grid 32), 3 substeps, 3 envs with softness 666 / 120 / 80; env 0 opens and is never clamped, env 1 closes from above
minimal_gap and reaches the clamp in the second substep, env 2 starts at minimal_gap and closes (clamped throughout).
Bars (tests/test_plb_shape_gpu.py's): forward 1e-9 relative on x, v, C, F, prim_pos, prim_rot, prim_gap; every adjoint leaf 1e-6 of its
max-norm; the contact loss 1e-11 / its gradients 1e-9; the kinematics alone 1e-12.  Every reference run asserts
plb_chopsticks_twin.honesty_chop."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle.twin.plb_twin import PlbConf
from tests import plb_chopsticks_twin as T

S, B = 3, 3
R2 = (T.R, 0.025)                            # the Chopsticks' r, and the Sphere's radius where there is one
NAMES = ("x", "v", "C", "F", "prim_pos", "prim_rot", "prim_gap")


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _T(a, r=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=r)


def _twin(N, kw, mu=(0.7, 0.0), radius=R2):
    P = len(kw["kinds"])
    return T.PlbChopsticksTwin(PlbConf(quality=0.5, n_particles=N, radius=radius[:P]), mu=mu[:P], substeps=S, **kw)


def _cfg(N, kw, mu=(0.7, 0.0), radius=R2, ckpt=None, lanes=0, path=0, **over):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf
    P = len(kw["kinds"])
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles, cfg.path, cfg.lanes = 0.5, S, N, path, lanes
    cfg.prim_radius, cfg.prim_kind, cfg.prim_h, cfg.prim_friction = radius[:P], kw["kinds"], kw.get("h", (T.H, 0.0))[:P], mu[:P]
    cfg.prim_min_gap, cfg.action_scale_gap = kw.get("min_gap", (T.MIN_GAP, 0.0))[:P], kw.get("action_scale_gap", 1.0)
    cfg.prim_init_gap = (0.08, 0.0)[:P]
    cfg.prim_rot = ((1.0, 0.0, 0.0, 0.0),) * P
    cfg.rot_state, cfg.action_dim, cfg.action_scale_w = True, 7, kw.get("action_scale_w", (1.0, 1.0, 1.0))
    cfg.prim_init_pos = ((0.5, 0.3, 0.5),) * P
    if ckpt is not None:
        cfg.grid_ckpt_cells = ckpt
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _sim(N, nb, kw, **more):
    from unidom_amd.engine.plb_simulator import PlbSimulator
    sim = PlbSimulator(_cfg(N, kw, **more), batch_size=nb)
    assert sim.launch_plan() == 1 and sim.n_grid == 32 and sim.substeps == S and sim.chopsticks      # the multi-kernel path
    return sim


def _dev(sim, a, r=False):
    return torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)


def _values(case):
    x, v, Cm, F, prim, q, gap, act, E, nu, ys = case
    return dict(x=x, v=v, C=Cm, F=F, prim=prim, rot=q, gap=gap, act=act, E=E, nu=nu, ys=ys)


def _twin_step(tw, leaves, soft):
    return tw.step(*[leaves[k] for k in ("x", "v", "C", "F", "prim", "rot", "gap", "act")], _T(soft), *[leaves[k] for k in ("E", "nu", "ys", "fric")])


def _state(sim, hl, soft):
    return sim.reset()._replace(x=hl["x"], v=hl["v"], C=hl["C"], F=hl["F"], prim_pos=hl["prim"], prim_rot=hl["rot"], prim_gap=hl["gap"],
                                softness=_dev(sim, soft), E=hl["E"], nu=hl["nu"], yield_stress=hl["ys"])


def _outputs(s):
    return (s.x, s.v, s.C, s.F, s.prim_pos, s.prim_rot, s.prim_gap)


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [33, 300])
def test_hip_chopsticks_forward_matches_the_twin(N):
    """One step, three envs.  N = 33 leaves most lanes of a wave idle, N = 300 spreads the touched cells over several waves and blocks."""
    torch.set_num_threads(8)
    case, soft, kw = T.chop_case(B, N)
    tw = _twin(N, kw)
    vals = dict(_values(case), fric=np.full(B, tw.c.ground_friction))
    with torch.no_grad():
        ref = _twin_step(tw, {k: _T(a) for k, a in vals.items()}, soft)
    T.honesty_chop(tw)
    sim = _sim(N, B, kw)
    s = sim.step(_state(sim, {k: _dev(sim, a) for k, a in vals.items() if k != "fric"}, soft), case[7])
    sim.check_status()
    for name, t, r in zip(NAMES, _outputs(s), ref):
        g = t.cpu().numpy()
        print(name, _rel(g, r.numpy()))
        assert g.shape == tuple(r.shape) and np.isfinite(g).all() and _rel(g, r.numpy()) < 1e-9, (name, _rel(g, r.numpy()))
    gap1 = s.prim_gap.cpu().numpy()[:, 0]
    assert gap1[0] > T.GAP0[0] and gap1[1] == T.MIN_GAP and gap1[2] == T.MIN_GAP                    # opened; clamped; clamped
    assert np.abs(ref[5].numpy() - case[5]).max() > 1e-3                                             # the sticks turned


# ---- adjoint ----------------------------------------------------------------------------------------------------------------------
def _reference_adjoint(N, case, soft, kw, cot=None, need_contact=True, mu=(0.7, 0.0)):
    """autograd through the twin with random output cotangents (cot: which outputs get one; default all)."""
    torch.set_num_threads(8)
    P = case[4].shape[1]
    rng = np.random.default_rng(9)
    w = [rng.normal(size=s) for s in ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, P, 3), (B, P, 4), (B, P))]
    if cot is not None:
        w = [wi if i in cot else np.zeros_like(wi) for i, wi in enumerate(w)]
    tw = _twin(N, kw, mu=mu)
    values = _values(case)
    leaves = {k: _T(a, True) for k, a in values.items()}
    leaves["fric"] = _T(np.full(B, tw.c.ground_friction), True)
    out = _twin_step(tw, leaves, soft)
    if need_contact:
        T.honesty_chop(tw)
    sum((o * _T(wi)).sum() for o, wi in zip(out, w)).backward()
    grads = {k: (t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
    return values, [o.detach().numpy() for o in out], w, grads, tw


def _check_adjoint(sim, ref, soft, bar=1e-6, names=None, fric=True, fwd=1e-9):
    values, out, w, grads, _ = ref
    names = tuple(values) if names is None else names
    hl = {k: _dev(sim, a, True) for k, a in values.items()}
    s1 = sim.step(_state(sim, hl, soft), hl["act"])
    res = _outputs(s1)
    for o, t, name in zip(out, res, NAMES):
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


@functools.lru_cache(maxsize=None)          # one reference, shared by the cases that differ on the HIP side only
def _ref_single():
    case, soft, kw = T.chop_case(B, 33)
    ref = _reference_adjoint(33, case, soft, kw)
    g = ref[3]
    assert g["act"].shape == (B, 7) and np.isfinite(g["act"]).all() and np.abs(g["act"][:, :6]).min() > 0
    assert np.abs(g["act"][:2, 6]).min() > 0 and g["act"][2, 6] == 0.0          # env 2 is clamped throughout: no gradient reaches gap_vel
    assert np.abs(g["gap"][:, 0]).min() > 0 and np.abs(g["rot"][:, 0]).min() > 0
    return soft, kw, ref


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 4, 8])
@pytest.mark.parametrize("ckpt", [0, 27])
def test_hip_chopsticks_adjoint_matches_autograd_through_the_twin(ckpt, lanes):
    """ud_plb_step_bwd_gap where the grid is recomputed (grid_ckpt_cells 0) and where it is restored, with every lane mapping, at N = 33.
    Leaves: x, v, C, F, prim_pos, prim_rot, prim_gap, all seven action dimensions, E, nu, yield_stress, ground friction."""
    soft, kw, ref = _ref_single()
    sim = _sim(33, B, kw, ckpt=ckpt, lanes=lanes)
    hl = _check_adjoint(sim, ref, soft)
    assert float(hl["act"].grad[2, 6]) == 0.0


@pytest.mark.gpu
def test_hip_chopsticks_and_sticky_sphere_on_one_handle():
    N = 300
    case, soft, kw = T.chop_case(B, N, two=True)
    ref = _reference_adjoint(N, case, soft, kw)
    assert np.abs(ref[3]["prim"][:, 1]).max() > 0        # the sphere touches the cloud too
    assert np.abs(ref[3]["gap"][:, 1] - ref[2][6][:, 1]).max() == 0.0     # primitive 1's gap entry is carried through, and so is its cotangent
    sim = _sim(N, B, kw)
    _check_adjoint(sim, ref, soft)


def _far_case():
    """The Chopsticks 0.3 along x clear of the rod (0.028 thin): no active occupied cell."""
    case, soft, kw = T.chop_case(B, 33)
    case = list(case)
    case[4] = case[4] + np.array([0.3, 0.0, 0.0])
    return tuple(case), soft, kw


@pytest.mark.gpu
def test_hip_chopsticks_kinematics_alone():
    """No particle near: the outputs and, with cotangents on prim_pos, prim_rot and prim_gap only, g_action / g_prim_pos0 / g_prim_rot0 /
    g_prim_gap0 are the kinematics chain alone.  Bar 1e-12.  Env 0 is never clamped: gap[S] depends on gap[0] and gap_vel.  Envs 1 and 2 end on
    the clamped arm (env 1 from its second substep on, env 2 throughout): gap[S] = minimal_gap, so g_action[6] and g_prim_gap0 are exactly 0.
    No atomic enters these leaves, so a second backward call gives them again bit for bit."""
    case, soft, kw = _far_case()
    ref = _reference_adjoint(33, case, soft, kw, cot=(4, 5, 6), need_contact=False)
    tw, g = ref[4], ref[3]
    assert tw.diag and not any(bool((d["occ"] & d["active"]).any()) for d in tw.diag)
    assert np.abs(g["act"][:, :6]).min() > 0 and np.abs(g["rot"][:, 0]).min() > 0 and g["gap"][0, 0] == ref[2][6][0, 0] and g["act"][0, 6] != 0.0
    assert (g["act"][1:, 6] == 0.0).all() and (g["gap"][1:, 0] == 0.0).all()
    sim = _sim(33, B, kw)
    hl = _check_adjoint(sim, ref, soft, bar=1e-12, names=("prim", "rot", "gap", "act"), fric=False)
    assert bool((hl["act"].grad[1:, 6] == 0.0).all()) and bool((hl["gap"].grad[1:, 0] == 0.0).all()) and float(hl["act"].grad[0, 6]) != 0.0
    first = {k: hl[k].grad.clone() for k in ("prim", "rot", "gap", "act")}
    hl2 = _check_adjoint(sim, ref, soft, bar=1e-12, names=("prim", "rot", "gap", "act"), fric=False)
    assert all(torch.equal(first[k], hl2[k].grad) for k in first)


@pytest.mark.gpu
def test_hip_chopsticks_two_backward_calls_agree():
    """The contact case twice on one handle: every leaf goes through sums of atomics (cell cotangents, per-wave sums of the primitive's), whose
    order may differ from call to call: 1e-12 of the leaf's max-norm."""
    soft, kw, ref = _ref_single()
    sim = _sim(33, B, kw)
    a = _check_adjoint(sim, ref, soft)
    fr1 = sim.ground_friction_grad.clone()
    b = _check_adjoint(sim, ref, soft)
    for k in a:
        assert _rel(a[k].grad.cpu().numpy(), b[k].grad.cpu().numpy()) < 1e-12, k
    assert _rel(fr1.cpu().numpy(), sim.ground_friction_grad.cpu().numpy()) < 1e-12


# ---- contact loss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("soft_contact", [True, False], ids=["soft", "hard"])
def test_hip_chopsticks_contact_loss_matches_the_twin(soft_contact):
    """Primitive 0 the Chopsticks with a tilted, non-unit orientation per env, beside the rod and clear of it, primitive 1 a Sphere; the
    contact term takes the Chopsticks' distance at the current gap.  loss, parts (1e-11), g_x, g_prim_pos, g_prim_rot, g_prim_gap (1e-9)."""
    from oracle.twin.plb_twin import torus_particles
    nb, N = 2, 300
    kw = dict(kinds=(T.CHOPSTICKS, 0), h=(T.H, 0.0), min_gap=(T.MIN_GAP, 0.0))
    tw = _twin(N, kw, mu=(0.0, 0.0))
    rng = np.random.default_rng(2)
    x = np.stack([torus_particles(1000)[:N], torus_particles(1000)[:N] + rng.normal(size=(N, 3)) * 0.003])
    prim = np.array([[[0.40, 0.28, 0.5], [0.55, 0.62, 0.5]], [[0.5, 0.35, 0.62], [0.5, 0.1, 0.5]]])
    q = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (nb, 2, 1))
    q[:, 0] = np.array([[0.9, 0.1, -0.3, 0.2], [0.7, -0.4, 0.2, 0.5]]) * np.array([[1.03], [0.96]])
    gap = np.array([[0.07, 0.0], [0.1, 0.0]])
    td = tw.grid_mass(torch.tensor((torus_particles(1000)[:N] + np.array([0.004, -0.01, 0.0]))[None]))[0]
    ts = torch.tensor(rng.normal(size=tw.c.n_grid ** 3))
    wts = (3.0, 0.7, 1.3)
    tx, tp, tr, tg = _T(x, True), _T(prim, True), _T(q, True), _T(gap, True)
    total, parts = tw.loss(tx, tp, tr, tg, td, ts, wts, soft_contact=soft_contact)
    gl = np.array([1.0, -2.5])
    (total * _T(gl)).sum().backward()
    assert np.abs(tp.grad.numpy()[:, 0]).max() > 0 and float(parts.detach()[:, 0].min()) > 0
    tw._gap = _T(gap)
    d0 = tw.sdf_q(0, _T(x), _T(prim)[:, 0, None, :], _T(q)[:, 0])
    assert float(d0.min()) > 1e-9                                                  # every particle's max(sdf, 0) in its open arm
    assert np.abs(tr.grad.numpy()[:, 0]).min() > 0 and np.abs(tg.grad.numpy()[:, 0]).min() > 0 and np.abs(tg.grad.numpy()[:, 1]).max() == 0.0
    sim = _sim(N, nb, kw, mu=(0.0, 0.0))
    hx, hp, hr, hg = _dev(sim, x, True), _dev(sim, prim, True), _dev(sim, q, True), _dev(sim, gap, True)
    st = sim.reset()._replace(x=hx, prim_pos=hp, prim_rot=hr, prim_gap=hg)
    hloss, hparts = sim.compute_loss(st, td.numpy(), ts.numpy(), wts, soft_contact)
    print("loss", _rel(hloss.detach().cpu().numpy(), total.detach().numpy()), "parts", _rel(hparts.cpu().numpy(), parts.detach().numpy()))
    assert _rel(hloss.detach().cpu().numpy(), total.detach().numpy()) < 1e-11
    assert _rel(hparts.cpu().numpy(), parts.detach().numpy()) < 1e-11
    (hloss * _dev(sim, gl)).sum().backward()
    for name, got, want in (("x", hx, tx), ("prim", hp, tp), ("rot", hr, tr), ("gap", hg, tg)):
        print(name, _rel(got.grad.cpu().numpy(), want.grad.numpy()))
        assert _rel(got.grad.cpu().numpy(), want.grad.numpy()) < 1e-9, name


# ---- the raw entry points -----------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _raw_step(sim, nb, x, v, Cm, F, pp, pr, pg, so, act, E, nu, ys, cots, pad=0, canary=777.0):
    """ud_plb_step_fwd_gap + ud_plb_step_bwd_gap for the first nb envs; prim_gap_out, g_action, g_prim_rot0 and g_prim_gap0 carry `pad` canary
    doubles behind them."""
    from unidom_amd import _lib
    L = _lib.lib()
    N, P, dev = sim.n_particles, sim.n_primitive, sim.device
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    full = lambda n: torch.full((n + pad,), canary, dtype=torch.float64, device=dev)
    xo, vo, Co, Fo, po, ro = mk(nb, N, 3), mk(nb, N, 3), mk(nb, N, 3, 3), mk(nb, N, 3, 3), mk(nb, P, 3), mk(nb, P, 4)
    go = full(nb * P)
    ckpt = torch.empty((L.ud_plb_ckpt_bytes(sim._h, C.c_int(nb)) // 8,), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(L.ud_plb_step_fwd_gap(sim._h, C.c_int(nb), _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(pr), _p(pg), _p(so), _p(act), _p(E), _p(nu), _p(ys),
                                     _p(xo), _p(vo), _p(Co), _p(Fo), _p(po), _p(ro), _p(go), _p(ckpt), st), "ud_plb_step_fwd_gap")
    ox, ov, oC, oF, op = mk(nb, N, 3), mk(nb, N, 3), mk(nb, N, 3, 3), mk(nb, N, 3, 3), mk(nb, P, 3)
    oa, orot, ogap = full(nb * 7), full(nb * P * 4), full(nb * P)
    oE, onu, oys, ofr = mk(nb), mk(nb), mk(nb), mk(nb)
    _lib.check(L.ud_plb_step_bwd_gap(sim._h, C.c_int(nb), _p(ckpt), _p(so), _p(act), _p(E), _p(nu), _p(ys), *[_p(c) for c in cots], _p(ox),
                                     _p(ov), _p(oC), _p(oF), _p(op), _p(orot), _p(ogap), _p(oa), _p(oE), _p(onu), _p(oys), _p(ofr), st), "ud_plb_step_bwd_gap")
    torch.cuda.synchronize()
    return go, oa, orot, ogap


@pytest.mark.gpu
def test_hip_chopsticks_batch_size_canaries():
    """A B = 1 call after a B = 3 call on a max_envs = 3 handle writes prim_gap_out [1,1], g_action [1,7], g_prim_rot0 [1,1,4] and g_prim_gap0
    [1,1] and not a word behind them, and gives env 0 of the B = 3 call."""
    N = 33
    case, soft, kw = T.chop_case(B, N)
    sim = _sim(N, B, kw)
    x, v, Cm, F, prim, q, gap, act, E, nu, ys = (_dev(sim, a) for a in case)
    so = _dev(sim, soft)
    rng = np.random.default_rng(4)
    cots = [_dev(sim, rng.normal(size=s)) for s in ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, 1, 3), (B, 1, 4), (B, 1))]
    three = _raw_step(sim, 3, x, v, Cm, F, prim, q, gap, so, act, E, nu, ys, cots)
    first = lambda t: t[:1].contiguous()
    one = _raw_step(sim, 1, *(first(t) for t in (x, v, Cm, F, prim, q, gap, so, act, E, nu, ys)), [first(c) for c in cots], pad=24)
    for name, n, t1, t3 in zip(("prim_gap_out", "g_action", "g_prim_rot0", "g_prim_gap0"), (1, 7, 4, 1), one, three):
        t1, t3 = t1.cpu().numpy(), t3.cpu().numpy()
        assert (t1[n:] == 777.0).all(), (name, t1)
        assert np.isfinite(t1[:n]).all() and np.abs(t1[:n]).min() > 0 and (t1[:n] != 777.0).all(), (name, t1)
        assert _rel(t1[:n], t3[:n]) < 1e-9, (name, t1[:n], t3[:n])


@pytest.mark.gpu
def test_hip_chopsticks_contract():
    """Create-time refusals return their code and name the field; on a Chopsticks handle the plain and the _rot entry points return
    UD_ERR_INVALID, name the reason and leave the outputs as they were, and so do the _gap entry points on any other handle; the checkpoint
    grows by the gap trajectory, for a Chopsticks handle only."""
    from unidom_amd import _lib
    from unidom_amd.engine.plb_simulator import PlbSimulator
    L = _lib.lib()
    INVALID, UNSUPPORTED = UD_ERR["INVALID"], UD_ERR["UNSUPPORTED"]
    chop = dict(kinds=(T.CHOPSTICKS,))
    box = dict(prim_kind=(3,), prim_shape=((0.06, 0.04, 0.05),))
    refused = [(dict(rot_state=False), INVALID, "prim_kind[0] = 6"),
               (dict(rot_state=False, action_dim=3), INVALID, "needs rot_state and action_dim = 7"),
               (dict(action_dim=6), INVALID, "needs rot_state and action_dim = 7"),
               (dict(action_dim=3), INVALID, "prim_kind[0] = 6"),
               (dict(action_dim=7, **box), INVALID, "action_dim = 7"),
               (dict(action_dim=7, prim_kind=(1,)), INVALID, "action_dim = 7"),
               (dict(action_dim=8), INVALID, "action_dim = 8"),
               (dict(prim_kind=(7,), action_dim=3, rot_state=False), INVALID, "prim_kind[0] = 7 (0 Sphere"),
               (dict(prim_min_gap=(-0.01,)), INVALID, "min_gap[0]"),
               (dict(prim_radius=(0.0,)), INVALID, "radius > 0"),
               (dict(path=2), UNSUPPORTED, "path = 2"),
               (dict(kw=dict(kinds=(T.CHOPSTICKS, T.CHOPSTICKS))), UNSUPPORTED, "primitive 0"),
               (dict(kw=dict(kinds=(T.CHOPSTICKS, 1))), UNSUPPORTED, "primitive 1")]
    for over, code, word in refused:
        over = dict(over)
        with pytest.raises(_lib.UnidomError) as e:
            PlbSimulator(_cfg(33, over.pop("kw", chop), **over), batch_size=1)
        assert f"status {code})" in str(e.value) and word in str(e.value), (over, str(e.value))
    N = 33
    sim = _sim(N, 2, chop)                                                    # action_scale_gap = 0 is 1, min_gap = 0 is legal
    _sim(N, 1, dict(chop, action_scale_gap=0.0, min_gap=(0.0, 0.0)))
    cap = PlbSimulator(_cfg(N, dict(kinds=(1,)), action_dim=6), batch_size=2)                 # a rotating Capsule of the same sizes
    assert not cap.chopsticks and cap.reset().prim_gap is None
    for nb in (1, 2):                                                         # the checkpoint grows by gap[B][S+1][np], rounded up to 256 B
        grow = L.ud_plb_ckpt_bytes(sim._h, C.c_int(nb)) - L.ud_plb_ckpt_bytes(cap._h, C.c_int(nb))
        assert grow == (nb * (S + 1) * 8 + 255) // 256 * 256, grow
    mk = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=sim.device)
    x, v, Cm, F, pp, pr, pg, so, act, E = mk(1, N, 3), mk(1, N, 3), mk(1, N, 3, 3), mk(1, N, 3, 3), mk(1, 1, 3), mk(1, 1, 4), mk(1, 1), mk(1, 1), mk(1, 7), mk(1)
    out = torch.full((1 << 16,), 777.0, dtype=torch.float64, device=sim.device)   # stands in for every output / checkpoint / grid-sized array
    st = C.c_void_p(torch.cuda.current_stream(sim.device).cuda_stream)
    one, nul, o = C.c_int(1), _p(None), _p(out)
    on_chop = {
        "ud_plb_step_fwd": (lambda h: L.ud_plb_step_fwd(h, one, _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(so), _p(act), _p(E), _p(E), _p(E), o, o, o, o, o, nul, st), "rot_state"),
        "ud_plb_step_bwd": (lambda h: L.ud_plb_step_bwd(h, one, o, _p(so), _p(act), _p(E), _p(E), _p(E), *([nul] * 5), o, o, o, o, *([nul] * 6), st), "rot_state"),
        "ud_plb_loss_fwd": (lambda h: L.ud_plb_loss_fwd(h, one, _p(x), _p(pp), o, o, o, one, o, nul, st), "rot_state"),
        "ud_plb_loss_bwd": (lambda h: L.ud_plb_loss_bwd(h, one, _p(x), _p(pp), o, o, o, one, o, o, nul, st), "rot_state"),
        "ud_plb_step_fwd_rot": (lambda h: L.ud_plb_step_fwd_rot(h, one, _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(pr), _p(so), _p(act), _p(E), _p(E), _p(E), o, o, o, o, o,
                                                                o, nul, st), "Chopsticks"),
        "ud_plb_step_bwd_rot": (lambda h: L.ud_plb_step_bwd_rot(h, one, o, _p(so), _p(act), _p(E), _p(E), _p(E), *([nul] * 6), o, o, o, o, *([nul] * 7), st), "Chopsticks"),
        "ud_plb_loss_fwd_rot": (lambda h: L.ud_plb_loss_fwd_rot(h, one, _p(x), _p(pp), _p(pr), o, o, o, one, o, nul, st), "Chopsticks"),
        "ud_plb_loss_bwd_rot": (lambda h: L.ud_plb_loss_bwd_rot(h, one, _p(x), _p(pp), _p(pr), o, o, o, one, o, o, nul, nul, st), "Chopsticks"),
    }
    on_other = {
        "ud_plb_step_fwd_gap": lambda h: L.ud_plb_step_fwd_gap(h, one, _p(x), _p(v), _p(Cm), _p(F), _p(pp), _p(pr), _p(pg), _p(so), _p(act), _p(E), _p(E), _p(E), o, o, o, o,
                                                               o, o, o, nul, st),
        "ud_plb_step_bwd_gap": lambda h: L.ud_plb_step_bwd_gap(h, one, o, _p(so), _p(act), _p(E), _p(E), _p(E), *([nul] * 7), o, o, o, o, *([nul] * 8), st),
        "ud_plb_loss_fwd_gap": lambda h: L.ud_plb_loss_fwd_gap(h, one, _p(x), _p(pp), _p(pr), _p(pg), o, o, o, one, o, nul, st),
        "ud_plb_loss_bwd_gap": lambda h: L.ud_plb_loss_bwd_gap(h, one, _p(x), _p(pp), _p(pr), _p(pg), o, o, o, one, o, o, nul, nul, nul, st),
    }
    for name, (call, word) in on_chop.items():
        assert call(sim._h) == INVALID, name
        assert word in L.ud_last_error().decode() and name in L.ud_last_error().decode(), (name, L.ud_last_error().decode())
    for name, call in on_other.items():
        assert call(cap._h) == INVALID, name
        assert "no Chopsticks" in L.ud_last_error().decode() and name in L.ud_last_error().decode(), (name, L.ud_last_error().decode())
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plb_simulator_chopsticks_step_loss_backward():
    """PlbSimulator with a Chopsticks: step -> PlbLoss.compute_loss -> backward().  The loss (1e-9) and all seven g_action components, g_prim_gap0
    and g_E (1e-6) against autograd through the twin's step and loss; the policy classes refuse the simulator."""
    from unidom_amd.algorithms.plb_solver_nn import SolverNN
    from unidom_amd.engine.plb_losses import PlbLoss
    from unidom_amd.engine.plb_policy import PlbPolicy
    torch.set_num_threads(8)
    N = 33
    case, soft, kw = T.chop_case(B, N)
    x, v, Cm, F, prim, q, gap, act, E, nu, ys = case
    tw = _twin(N, kw)
    sim = _sim(N, B, kw)
    td = tw.grid_mass(_T(x[:1] + np.array([0.004, -0.01, 0.0])))[0].numpy()
    wts, gl = (3.0, 0.7, 1.3), np.array([1.0, -2.5, 0.5])
    loss = PlbLoss(sim, weights=wts, soft_contact=True).load_target_density(td)
    ts = loss.target_sdf.cpu().numpy().reshape(-1)                          # the device SDF (tests/test_plb_goal_gpu.py holds it to its twin)
    ta, tE, tg = _T(act, True), _T(E, True), _T(gap, True)
    out = tw.step(*map(_T, (x, v, Cm, F, prim, q)), tg, ta, _T(soft), tE, _T(nu), _T(ys), _T(np.full(B, tw.c.ground_friction)))
    T.honesty_chop(tw)
    total, _ = tw.loss(out[0], out[4], out[5], out[6], _T(td.reshape(-1)), _T(ts), wts, True)
    (total * _T(gl)).sum().backward()
    assert np.abs(ta.grad.numpy()[:2]).min() > 0 and np.abs(tE.grad.numpy()).min() > 0 and np.abs(tg.grad.numpy()).min() > 0
    ha, hE, hg = _dev(sim, act, True), _dev(sim, E, True), _dev(sim, gap, True)
    hl = dict(x=x, v=v, C=Cm, F=F, prim=prim, rot=q, nu=nu, ys=ys)
    s0 = _state(sim, {**{k: _dev(sim, a) for k, a in hl.items()}, "E": hE, "gap": hg}, soft)
    loss.reset(s0)
    s1 = sim.step(s0, ha)
    info = loss.compute_loss(s1)
    (info["loss"] * _dev(sim, gl)).sum().backward()
    sim.check_status()
    got = info["loss"].detach().cpu().numpy()
    print("loss", _rel(got, total.detach().numpy()), "act", _rel(ha.grad.cpu().numpy(), ta.grad.numpy()), "E", _rel(hE.grad.cpu().numpy(), tE.grad.numpy()),
          "gap", _rel(hg.grad.cpu().numpy(), tg.grad.numpy()))
    assert _rel(got, total.detach().numpy()) < 1e-9
    assert ha.grad.shape == (B, 7) and _rel(ha.grad.cpu().numpy(), ta.grad.numpy()) < 1e-6
    assert _rel(hE.grad.cpu().numpy(), tE.grad.numpy()) < 1e-6 and _rel(hg.grad.cpu().numpy(), tg.grad.numpy()) < 1e-6
    for make in (lambda: PlbPolicy(sim), lambda: SolverNN(sim, loss, None)):
        with pytest.raises(ValueError, match="Chopsticks"):
            make()


@pytest.mark.gpu
def test_solver_with_momentum_follows_the_twin_loop_on_chopsticks():
    """Three Solver iterations (Momentum) from the reset state of a small ChopsticksConf against the same loop through the twin: the losses
    1e-9, the actions' movement 1e-6 of its max-norm (Momentum is linear in the gradient)."""
    from tests.plb_target_twin import MomentumTwin
    from unidom_amd.algorithms.plb_solver import Solver
    from unidom_amd.engine.plb_losses import PlbLoss
    from unidom_amd.engine.plb_simulator import ChopsticksConf, PlbSimulator
    torch.set_num_threads(8)
    nb, N, H, iters, lr, softness = 2, 120, 2, 3, 0.5, 300.0
    cfg = ChopsticksConf()
    cfg.quality, cfg.substeps, cfg.n_particles = 0.5, S, N
    # off the lattice and a little tilted: at the conf's own (0.5, 0.2, 0.5) with the identity the cells at x = 0.5 lie ON the a = b plane
    cfg.prim_init_pos, cfg.prim_rot = ((0.507, 0.2, 0.503),), ((0.99, 0.05, -0.1, 0.08),)
    sim = PlbSimulator(cfg, batch_size=nb)
    assert sim.chopsticks and sim.action_dim == 7 and sim.launch_plan() == 1
    st0 = sim.reset()
    assert st0.prim_gap.shape == (nb, 1) and float(st0.prim_gap[0, 0]) == cfg.prim_init_gap[0]
    tw = T.PlbChopsticksTwin(PlbConf(quality=0.5, n_particles=N, radius=cfg.prim_radius, gravity=cfg.gravity, ground_friction=cfg.ground_friction,
                                     lower_bound=cfg.lower_bound, upper_bound=cfg.upper_bound), kinds=(T.CHOPSTICKS,), h=cfg.prim_h, mu=cfg.prim_friction,
                             min_gap=cfg.prim_min_gap, action_scale=cfg.action_scale, action_scale_w=cfg.action_scale_w,
                             action_scale_gap=cfg.action_scale_gap, substeps=S)
    cpu = lambda t: torch.tensor(t.cpu().numpy())
    x0, v0, C0, F0, p0, r0, g0 = (cpu(t) for t in (st0.x, st0.v, st0.C, st0.F, st0.prim_pos, st0.prim_rot, st0.prim_gap))
    td = tw.grid_mass(x0[:1] + torch.tensor([0.01, -0.005, 0.0], dtype=torch.float64))[0]
    wts = (1.0, 1.0, 1.0)
    loss = PlbLoss(sim, weights=wts, soft_contact=True).load_target_density(td.numpy())
    ts = cpu(loss.target_sdf).reshape(-1)
    full = lambda val: torch.full((nb,), float(val), dtype=torch.float64)
    soft, E, nu, ys, fr = torch.full((nb, 1), softness, dtype=torch.float64), full(cfg.E), full(cfg.nu), full(cfg.yield_stress), full(cfg.ground_friction)
    init = np.random.default_rng(4).uniform(-1, 1, size=(H, nb, 7)) * 0.5
    init[..., 1] = -np.abs(init[..., 1]) - 0.3                              # press down, into the block
    opt = MomentumTwin(init, lr=lr)
    actions, ref_losses = np.array(init), []
    for _ in range(iters):
        a = _T(actions, True)
        x, v, Cm, F, p, r, g = x0, v0, C0, F0, p0, r0, g0
        total = 0.0
        for t in range(H):
            x, v, Cm, F, p, r, g = tw.step(x, v, Cm, F, p, r, g, a[t], soft, E, nu, ys, fr)
            total = total + tw.loss(x, p, r, g, td, ts, wts, True)[0].sum()
        total.backward()
        ref_losses.append(float(total.detach()))
        grad = a.grad.numpy()
        actions = opt.step(grad)
    T.honesty_chop(tw, min_flag=0, min_noflag=0, least=0)                   # nothing near a branch point in any substep of any iteration
    assert sum(int((d["occ"] & d["active"]).sum()) for d in tw.diag) > 100 and np.abs(grad).min() > 0     # the sticks act on the block
    assert np.abs(actions - init).max() > 1e-4                               # and the optimiser really moved the actions
    seen = []
    solver = Solver(sim, loss, horizon=H, n_iters=iters, softness=softness, optim="Momentum", lr=lr)
    got = solver.solve(init_actions=init, callbacks=(lambda s, o, l, g: seen.append(float(l)),))
    sim.check_status()
    assert got.shape == (H, nb, 7) and solver.total_steps == H * iters
    print("losses", _rel(np.array(seen), np.array(ref_losses)), "actions", _rel(got.cpu().numpy() - init, actions - init))
    assert _rel(np.array(seen), np.array(ref_losses)) < 1e-9, (seen, ref_losses)
    assert _rel(got.cpu().numpy() - init, actions - init) < 1e-6, _rel(got.cpu().numpy() - init, actions - init)      # of what the optimiser moved


def _header_codes():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "unidom_hip.h")).read()
    return {k: int(val) for k, val in re.findall(r"UD_ERR_(\w+)\s*=\s*(-?\d+)", src)}


UD_ERR = _header_codes()
