"""GPU: the goal side of the PLB path at the smallest configuration (quality 0.25 -> n_grid 16, 60 particles, B = 2, 2 substeps):
PlbSimulator.get_grid_mass, ud_plb_density_iou, PlbLoss and the Solver, against the torch twin (oracle/twin/plb_twin_torch.py), its
autograd and the NumPy twin tests/plb_target_twin.py.

Bars: 1e-9 forward and 1e-6 gradient, the project's own for this path (tests/test_plb.py: f64 on both sides; what differs is the
summation order of the atomics and the SVD).  Momentum is linear in the gradient, so the Solver's actions carry the 1e-6 bar."""
import numpy as np
import pytest

from oracle.twin.plb_twin import PlbConf, torus_particles
from tests import plb_target_twin as tw

pytestmark = pytest.mark.gpu

B, N, S = 2, 60, 2
WEIGHTS = (1.0, 1.0, 1.0)             # (contact, density, sdf)


class _Conf(PlbConf):
    substeps = S


CONF = _Conf(quality=0.25, n_particles=N)


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _sim():
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    cfg = HipConf()
    cfg.quality, cfg.n_particles, cfg.substeps = 0.25, N, S
    sim = PlbSimulator(cfg, batch_size=B)
    assert (sim.n_grid, sim.substeps, sim.action_dim) == (16, S, 3) == (CONF.n_grid, CONF.substeps, 3)
    return sim


_GOAL = {}


def _goal():
    """Computed once, shared, never written: the grid mass of the start body displaced by less than a cell, its twin SDF and twin IoU."""
    if not _GOAL:
        import torch
        from oracle.twin.plb_twin_torch import PlbTorchTwin
        x = torus_particles(N) + np.array([0.02, 0.0, 0.012])
        td = PlbTorchTwin(CONF).grid_mass(torch.tensor(x[None]))[0].numpy().reshape(16, 16, 16)
        _GOAL.update(td=td, ts=tw.target_sdf(td, stop_at_fixed_point=True)[0], tiou=tw.iou(td, td))
        for a in _GOAL.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _GOAL


def _states(rng):
    """Two different envs: the start body, jittered, with sphere 0 inside it."""
    x = np.stack([torus_particles(N), torus_particles(N) + rng.normal(size=(N, 3)) * 0.004])
    prim = np.array([[[0.49, 0.2, 0.5], [0.5, 0.9, 0.5]], [[0.505, 0.32, 0.49], [0.5, 0.9, 0.5]]])
    return x, prim


def test_get_grid_mass_matches_the_twin():
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    sim = _sim()
    x, prim = _states(np.random.default_rng(0))
    st = sim.reset()._replace(x=torch.tensor(x, device=sim.device))
    gm = sim.get_grid_mass(st)
    assert gm.shape == (B, 16, 16, 16) and gm.dtype == torch.float64
    ref = PlbTorchTwin(CONF).grid_mass(torch.tensor(x)).numpy().reshape(B, 16, 16, 16)
    assert _rel(gm.cpu().numpy(), ref) < 1e-9
    assert abs(float(gm[0].sum()) - N * CONF.p_mass) < 1e-12


def test_density_iou_matches_the_twin_and_is_deterministic():
    import torch
    from unidom_amd.engine.plb_losses import density_iou
    rng = np.random.default_rng(1)
    G = 16 ** 3 + 37                                           # no multiple of the block: the strided loop's tail
    a = rng.uniform(size=(3, G)) * (rng.uniform(size=(3, G)) < 0.1)
    b = rng.uniform(size=(3, G)) * (rng.uniform(size=(3, G)) < 0.2)
    A, Bt = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    per = density_iou(A, Bt)                                   # b_batched = 1
    shared = density_iou(A, Bt[1])                             # b_batched = 0
    again = density_iou(A, Bt)
    assert torch.equal(per, again) and per.shape == (3,)
    for t in range(3):
        assert abs(float(per[t]) - tw.iou(a[t], b[t])) <= 1e-12 * abs(tw.iou(a[t], b[t]))
        assert abs(float(shared[t]) - tw.iou(a[t], b[1])) <= 1e-12 * abs(tw.iou(a[t], b[1]))
    big = torch.tensor(rng.uniform(size=(1, 64 ** 3)), device="cuda")        # every block of the first stage loops more than once
    assert abs(float(density_iou(big, big[0])) - tw.iou(big.cpu().numpy(), big.cpu().numpy())) <= 1e-12
    assert torch.isnan(density_iou(torch.zeros((1, 64), dtype=torch.float64, device="cuda"), A[0, :64])).all()   # max = 0: IEEE's 0 / 0, documented


def test_plb_loss_compute_loss():
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    from unidom_amd.engine.plb_losses import PlbLoss
    sim, g = _sim(), _goal()
    loss = PlbLoss(sim, weights=WEIGHTS, soft_contact=True).load_target_density(g["td"])
    assert np.array_equal(loss.target_sdf.cpu().numpy(), g["ts"])              # the device SDF is the twin's, bit for bit
    assert abs(float(loss.target_iou) - g["tiou"]) <= 1e-12 * g["tiou"]
    x, prim = _states(np.random.default_rng(2))
    T = lambda a, r=True: torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)
    st0 = sim.reset()
    loss.reset(st0)
    hx, hp = T(x), T(prim)
    st = st0._replace(x=hx, prim_pos=hp)
    seen = []
    inner = sim.compute_loss
    sim.compute_loss = lambda *a, **k: seen.append(inner(*a, **k)) or seen[-1]
    out = loss.compute_loss(st)
    sim.compute_loss = inner
    # loss and parts are sim.compute_loss's, bit for bit: it is the same call
    assert len(seen) == 1 and torch.equal(out["loss"], seen[0][0]) and out["loss"] is seen[0][0]
    assert torch.equal(torch.stack([out["contact_loss"], out["density_loss"], out["sdf_loss"]], -1), seen[0][1])
    # ... and a second, separate call with the same fields gives the same values up to the order of its atomic sums
    l2, p2 = sim.compute_loss(st, loss.target_density, loss.target_sdf, WEIGHTS, True)
    assert _rel(l2.detach().cpu().numpy(), out["loss"].detach().cpu().numpy()) < 1e-13 and _rel(p2.cpu().numpy(), seen[0][1].cpu().numpy()) < 1e-13
    # against the twin
    twin = PlbTorchTwin(CONF)
    td, ts = torch.tensor(g["td"].reshape(-1)), torch.tensor(g["ts"].reshape(-1))
    tx, tp = torch.tensor(x, requires_grad=True), torch.tensor(prim, requires_grad=True)
    total, parts = twin.loss(tx, tp, td, ts, WEIGHTS, soft_contact=True)
    assert _rel(out["loss"].detach().cpu().numpy(), total.detach().numpy()) < 1e-9
    x0 = torch.tensor(st0.x.cpu().numpy())
    start, _ = twin.loss(x0, torch.tensor(st0.prim_pos.cpu().numpy()), td, ts, WEIGHTS, soft_contact=True)
    assert _rel(out["reward"].cpu().numpy(), (start - total).detach().numpy()) < 1e-9
    iou = np.array([tw.iou(m, g["td"]) for m in twin.grid_mass(tx.detach()).numpy()])
    init = np.array([tw.iou(m, g["td"]) for m in twin.grid_mass(x0).numpy()])
    assert _rel(out["iou"].cpu().numpy(), iou) < 1e-9 and _rel(out["target_iou"].cpu().numpy(), np.full(B, g["tiou"])) < 1e-9
    inc = np.clip((iou - init) / (g["tiou"] - init), 0, 1)
    assert np.abs(out["incremental_iou"].cpu().numpy() - inc).max() < 1e-9 and out["incremental_iou"].shape == (B,)
    assert all(v.is_cuda for v in out.values())
    gl = np.array([1.0, -2.5])
    (total * torch.tensor(gl)).sum().backward()
    (out["loss"] * T(gl, False)).sum().backward()
    assert _rel(hx.grad.cpu().numpy(), tx.grad.numpy()) < 1e-6 and _rel(hp.grad.cpu().numpy(), tp.grad.numpy()) < 1e-6
    assert np.abs(tp.grad.numpy()).max() > 0 and np.abs(tx.grad.numpy()).max() > 0


def _twin_solve(init, n_iters, lr):
    """The Solver's loop driven through the torch twin and autograd, with the NumPy Momentum.  Returns (actions, total loss per iteration)."""
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    g = _goal()
    twin = PlbTorchTwin(CONF)
    td, ts = torch.tensor(g["td"].reshape(-1)), torch.tensor(g["ts"].reshape(-1))
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    rep = lambda a: f64(a)[None].repeat((B,) + (1,) * np.ndim(a))
    x0 = rep(torus_particles(N))
    v0, C0, F0 = torch.zeros((B, N, 3), dtype=torch.float64), torch.zeros((B, N, 3, 3), dtype=torch.float64), rep(np.eye(3)[None].repeat(N, 0))
    p0 = rep(np.array([[0.475, 0.05, 0.5], [0.5, 0.55, 0.5]]))
    soft = torch.full((B, 2), 666.0, dtype=torch.float64)
    E, nu, ys, fr = (torch.full((B,), v, dtype=torch.float64) for v in (CONF.E, CONF.nu, CONF.yield_stress, CONF.ground_friction))
    opt = tw.MomentumTwin(init, lr=lr)
    actions, losses = np.array(init, np.float64), []
    for _ in range(n_iters):
        a = f64(actions).requires_grad_(True)
        x, v, Cm, F, p = x0, v0, C0, F0, p0
        total = 0.0
        for t in range(a.shape[0]):
            x, v, Cm, F, p = twin.step(x, v, Cm, F, p, a[t], soft, E, nu, ys, fr)
            total = total + twin.loss(x, p, td, ts, WEIGHTS, soft_contact=True)[0].sum()
        total.backward()
        losses.append(float(total.detach()))
        actions = opt.step(a.grad.numpy())
    return actions, losses


def test_solver_with_momentum_follows_the_twin_loop():
    import torch
    from unidom_amd.algorithms.plb_solver import Solver
    from unidom_amd.engine.plb_losses import PlbLoss
    torch.set_num_threads(8)
    rng = np.random.default_rng(4)
    H, iters, lr = 2, 3, 0.02
    init = rng.uniform(-1, 1, size=(H, B, 3)) * 0.004
    ref_actions, ref_losses = _twin_solve(init, iters, lr)
    assert ref_losses[2] < ref_losses[0], ref_losses          # first: the reference loop itself descends on this input
    assert np.abs(ref_actions - init).max() > 1e-4            # and the optimiser really moved the actions
    sim = _sim()
    loss = PlbLoss(sim, weights=WEIGHTS, soft_contact=True).load_target_density(_goal()["td"])
    seen = []
    solver = Solver(sim, loss, horizon=H, n_iters=iters, softness=666.0, optim="Momentum", lr=lr)
    got = solver.solve(init_actions=init, callbacks=(lambda s, o, l, g: seen.append(float(l)),))
    sim.check_status()
    assert got.shape == (H, B, 3) and solver.total_steps == H * iters
    assert _rel(got.cpu().numpy(), ref_actions) < 1e-6, (_rel(got.cpu().numpy(), ref_actions), seen, ref_losses)
    assert _rel(np.array(seen), np.array(ref_losses)) < 1e-9 and seen[2] < seen[0]
