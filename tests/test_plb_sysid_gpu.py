"""GPU: PLB system identification at the smallest configuration of tests/test_plb_goal_gpu.py (quality 0.25 -> n_grid 16, G = 4096, 60
particles, 2 substeps): ud_plb_density_seq_fwd / _bwd, ud_plb_chamfer, PlbTrajectoryLoss, the Identifier and action_scale_on_host, against
the torch twin (oracle/twin/plb_twin_torch.py), its autograd and the NumPy twin tests/plb_sysid_twin.py.

Bars: 1e-9 forward and 1e-6 gradient in _rel = max|a - b| / max|b|, the project's own for this path (tests/test_plb.py: f64 on both sides;
what differs is the order of the atomic sums and the SVD).  Adam's step g / (|g| + eps) is less sensitive to g than Momentum's, so the
Identifier's parameters carry the 1e-6 bar per column; the losses after iteration 0 inherit it."""
import ctypes as C

import numpy as np
import pytest

from oracle.twin.plb_twin import PlbConf, torus_particles
from tests import plb_sysid_twin as tw

pytestmark = pytest.mark.gpu

B, N, S = 2, 60, 2
NG, G = 16, 16 ** 3
OFFSETS = ((0.02, 0.0, 0.012), (-0.015, 0.01, 0.0), (0.005, -0.02, 0.017))     # all below a cell (1 / 16)
INDEX = (2, 0, 1, 1, 2)
PRIM0 = np.array([[0.475, 0.05, 0.5], [0.5, 0.55, 0.5]])


class _Conf(PlbConf):
    substeps = S


CONF = _Conf(quality=0.25, n_particles=N)


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _sim(batch=B, **over):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    cfg = HipConf()
    cfg.quality, cfg.n_particles, cfg.substeps = 0.25, N, S
    for k, v in over.items():
        setattr(cfg, k, v)
    sim = PlbSimulator(cfg, batch_size=batch)
    assert (sim.n_grid, sim.substeps, sim.action_dim) == (NG, S, 3) == (CONF.n_grid, CONF.substeps, 3)
    return sim


_SEQ = {}


def _seq_case():
    """Computed once, shared, never written: M = 5 jittered clouds, T = 3 targets (the grid mass of the start body displaced by less than a
    cell: never the mass of a scored cloud, where exact ties outside empty cells would make the sign a coin toss), the twin's losses and
    its autograd gradient for unequal g_loss."""
    if not _SEQ:
        import torch
        from oracle.twin.plb_twin_torch import PlbTorchTwin
        rng = np.random.default_rng(11)
        twin = PlbTorchTwin(CONF)
        x = np.stack([torus_particles(N) + rng.normal(size=(N, 3)) * 0.004 for _ in INDEX])
        targets = np.stack([twin.grid_mass(torch.tensor((torus_particles(N) + np.array(o))[None]))[0].numpy() for o in OFFSETS])
        gl = np.array([1.0, -2.5, 0.75, 3.0, -0.5])
        tx = torch.tensor(x, requires_grad=True)
        loss = (twin.grid_mass(tx) - torch.tensor(targets)[list(INDEX)]).abs().sum(-1)
        (loss * torch.tensor(gl)).sum().backward()
        _SEQ.update(x=x, targets=targets.reshape(3, NG, NG, NG), gl=gl, loss=loss.detach().numpy(), gx=tx.grad.numpy())
        for a in _SEQ.values():
            a.setflags(write=False)
    return _SEQ


CANARY = -7.25e77


def _guarded(n, dtype, pad=64):
    """(whole, middle): a device buffer of n elements with `pad` canary elements either side."""
    import torch
    whole = torch.full((n + 2 * pad,), CANARY if dtype.is_floating_point else 0x5A5A5A5A5A5A5A5, dtype=dtype, device="cuda")
    return whole, whole[pad:pad + n]


def _intact(whole, n, pad=64):
    fill = whole[0].item()
    return bool((whole[:pad] == fill).all()) and bool((whole[pad + n:] == fill).all())


def _raw(sim, x, targets, index, gl, work_items=None):
    """The C entry points with canaries either side of every output and of the scratch.  Returns (loss, sign, g_x) as device tensors."""
    import torch
    from unidom_amd import _lib
    L = _lib.lib()
    dev = "cuda"
    M, T = x.shape[0], targets.shape[0]
    X, TD = torch.tensor(x, device=dev), torch.tensor(targets.reshape(T, -1), device=dev)
    IDX = None if index is None else torch.tensor(index, dtype=torch.int32, device=dev)
    GL = torch.tensor(gl, device=dev)
    nwork = int(L.ud_plb_density_seq_work_bytes(sim._h, M)) if work_items is None else work_items * 8 * G
    assert L.ud_plb_density_seq_work_bytes(sim._h, M) == 8 * G * M and L.ud_plb_density_seq_sign_bytes(sim._h, M) == M * (G // 64) * 16
    nsign = int(L.ud_plb_density_seq_sign_bytes(sim._h, M)) // 8
    lw, loss = _guarded(M, torch.float64)
    sw, sign = _guarded(nsign, torch.int64)
    ww, work = _guarded(nwork // 8, torch.float64)
    gw, gx = _guarded(M * N * 3, torch.float64)
    p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.ud_plb_density_seq_fwd(sim._h, M, p(X), p(TD), T, p(IDX), p(loss), p(sign), p(work), nwork, st), "ud_plb_density_seq_fwd")
    _lib.check(L.ud_plb_density_seq_bwd(sim._h, M, p(X), p(sign), p(GL), p(gx), st), "ud_plb_density_seq_bwd")
    torch.cuda.synchronize()
    assert _intact(lw, M) and _intact(sw, nsign) and _intact(ww, nwork // 8) and _intact(gw, M * N * 3), "a canary was overwritten"
    assert bool((work == 0).all()), "the sweep leaves the scratch zero"
    return loss.clone(), sign.clone(), gx.clone().reshape(M, N, 3)


def test_sequence_loss_matches_the_twin():
    import torch
    sim, c = _sim(), _seq_case()
    x = torch.tensor(c["x"], device=sim.device, requires_grad=True)
    loss = sim.density_seq_loss(x, torch.tensor(c["targets"], device=sim.device), torch.tensor(INDEX))
    assert loss.shape == (5,) and loss.dtype == torch.float64
    print("loss rel", _rel(loss.detach().cpu().numpy(), c["loss"]))
    assert _rel(loss.detach().cpu().numpy(), c["loss"]) < 1e-9
    (loss * torch.tensor(c["gl"], device=sim.device)).sum().backward()
    print("g_x rel", _rel(x.grad.cpu().numpy(), c["gx"]))
    assert np.abs(c["gx"]).max() > 0 and _rel(x.grad.cpu().numpy(), c["gx"]) < 1e-6
    for m in range(5):                                           # per item as well: a small g_loss must not hide behind a large one
        assert _rel(x.grad[m].cpu().numpy(), c["gx"][m]) < 1e-6, m
    # leading shape [2, 2] and index None (target 0 for every item)
    x4 = torch.tensor(c["x"][:4].reshape(2, 2, N, 3), device=sim.device)
    l4 = sim.density_seq_loss(x4, torch.tensor(c["targets"], device=sim.device))
    l0 = sim.density_seq_loss(torch.tensor(c["x"][:4], device=sim.device), torch.tensor(c["targets"], device=sim.device), [0, 0, 0, 0])
    assert l4.shape == (2, 2) and _rel(l4.reshape(-1).cpu().numpy(), l0.cpu().numpy()) < 1e-13


def test_chunking():
    import torch
    from unidom_amd import _lib
    sim, c = _sim(), _seq_case()
    assert sim.batch_size == 2                                   # M = 5 on a handle with max_envs = 2 is accepted
    one = _raw(sim, c["x"], c["targets"], INDEX, c["gl"])
    two = _raw(sim, c["x"], c["targets"], INDEX, c["gl"], work_items=2)     # 3 chunks, the last one partial
    assert _rel(one[0].cpu().numpy(), c["loss"]) < 1e-9
    assert _rel(two[0].cpu().numpy(), one[0].cpu().numpy()) < 1e-12
    assert torch.equal(two[1], one[1]) and torch.equal(two[2], one[2])
    x = torch.tensor(c["x"], device=sim.device)
    with pytest.raises(_lib.UnidomError, match="ud_plb_density_seq_fwd"):
        sim.density_seq_loss(x, torch.tensor(c["targets"], device=sim.device), torch.tensor(INDEX), work_bytes=8 * G - 1)
    assert b"ud_plb_density_seq_fwd" in _lib.lib().ud_last_error()
    L = _lib.lib()
    z = C.c_void_p(0)
    p = C.c_void_p(x.data_ptr())
    assert L.ud_plb_density_seq_fwd(sim._h, 0, p, p, 1, z, p, z, p, 8 * G, z) != 0 and b"ud_plb_density_seq_fwd" in L.ud_last_error()
    assert L.ud_plb_density_seq_fwd(sim._h, 1, p, p, 0, z, p, z, p, 8 * G, z) != 0
    for k in (2, 3, 6, 8):                                       # a null x / targets / loss / work
        args = [sim._h, 1, p, p, 1, z, p, z, p, 8 * G, z]
        args[k] = z
        assert L.ud_plb_density_seq_fwd(*args) != 0 and b"ud_plb_density_seq_fwd" in L.ud_last_error(), k
    assert L.ud_plb_density_seq_bwd(sim._h, 1, p, z, p, p, z) != 0 and b"ud_plb_density_seq_bwd" in L.ud_last_error()


def test_out_of_range_index():
    import torch
    sim, c = _sim(), _seq_case()
    good = _raw(sim, c["x"], c["targets"], INDEX, c["gl"])
    bad_index = (2, -1, 1, 3, 2)                                 # -1 and T
    bad = _raw(sim, c["x"], c["targets"], bad_index, c["gl"])
    for m in range(5):
        if bad_index[m] == INDEX[m]:
            assert abs(float(bad[0][m]) - float(good[0][m])) <= 1e-12 * abs(float(good[0][m])) and torch.equal(bad[2][m], good[2][m]), m
        else:
            assert torch.isnan(bad[0][m]) and bool((bad[2][m] == 0).all()), m
    W = G // 64 * 2
    assert bool((bad[1].reshape(5, W)[[1, 3]] == 0).all()) and torch.equal(bad[1].reshape(5, W)[[0, 2, 4]], good[1].reshape(5, W)[[0, 2, 4]])


def test_backward_is_reproducible():
    import torch
    from unidom_amd import _lib
    sim, c = _sim(), _seq_case()
    _, sign, gx = _raw(sim, c["x"], c["targets"], INDEX, c["gl"])
    X, GL = torch.tensor(c["x"], device="cuda"), torch.tensor(c["gl"], device="cuda")
    again = torch.empty_like(gx)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().ud_plb_density_seq_bwd(sim._h, 5, p(X), p(sign), p(GL), p(again), C.c_void_p(0)), "ud_plb_density_seq_bwd")
    torch.cuda.synchronize()
    assert torch.equal(again, gx) and float(gx.abs().max()) > 0


def test_chamfer():
    import torch
    from unidom_amd import _lib
    sim = _sim()
    rng = np.random.default_rng(5)
    Na, Nb, M, Tb = 130, 67, 3, 2
    a, b = rng.uniform(size=(M, Na, 3)), rng.uniform(size=(Tb, Nb, 3))
    idx = [1, 0, 1]
    out, mab, mba = sim.chamfer(torch.tensor(a), torch.tensor(b), idx, return_mins=True)
    assert out.shape == (M,) and mab.shape == (M, Na) and mba.shape == (M, Nb)
    ref = [tw.chamfer(a[m], b[idx[m]]) for m in range(M)]
    for m in range(M):
        assert np.array_equal(mab[m].cpu().numpy(), ref[m][1]) and np.array_equal(mba[m].cpu().numpy(), ref[m][2]), m
        assert abs(float(out[m]) - ref[m][0]) <= 1e-13 * ref[m][0], m      # <= 130 positive terms: 130 * 2^-52 between any two orders
    # without the min arrays (one workgroup per item): the same bits
    A, Bt, I = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"), torch.tensor(idx, dtype=torch.int32, device="cuda")
    lone = torch.empty((M,), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    z = C.c_void_p(0)
    _lib.check(_lib.lib().ud_plb_chamfer(M, Na, p(A), Tb, Nb, p(Bt), p(I), p(lone), z, z, z), "ud_plb_chamfer")
    torch.cuda.synchronize()
    assert torch.equal(lone, out) and torch.equal(sim.chamfer(A, Bt, idx), out)
    # one point each; b without a leading axis, no index
    o1 = sim.chamfer(torch.tensor(a[:, :1]), torch.tensor(b[0, :1]))
    assert np.array_equal(o1.cpu().numpy(), np.array([tw.chamfer(a[m, :1], b[0, :1])[0] for m in range(M)]))
    # one NaN coordinate: that item's result is NaN, the others' are unchanged
    an = a.copy()
    an[1, 77, 2] = np.nan
    on, nab, nba = sim.chamfer(torch.tensor(an), torch.tensor(b), idx, return_mins=True)
    assert torch.isnan(on[1]) and torch.equal(on[[0, 2]], out[[0, 2]])
    assert torch.isnan(nab[1, 77]) and torch.isnan(nba[1]).all() and int(torch.isnan(nab[1]).sum()) == 1      # np.min over the NaN column
    _lib.check(_lib.lib().ud_plb_chamfer(M, Na, p(torch.tensor(an, device="cuda")), Tb, Nb, p(Bt), p(I), p(lone), z, z, z), "ud_plb_chamfer")
    torch.cuda.synchronize()
    assert torch.isnan(lone[1]) and torch.equal(lone[[0, 2]], out[[0, 2]])
    assert _lib.lib().ud_plb_chamfer(0, Na, p(A), Tb, Nb, p(Bt), z, p(lone), z, z, z) != 0 and b"ud_plb_chamfer" in _lib.lib().ud_last_error()


# ---- the identification loop ---------------------------------------------------------------------------------------------------------
H = 3
ACTION = (0.6, 0.0, 0.0)
TRUTH = (6500.0, 0.3)
CAND = np.array([[3000.0, 0.38, CONF.yield_stress], [9000.0, 0.22, CONF.yield_stress]])
_IDENT = {}


def _twin_rollout(twin, params):
    """x_0 .. x_H of the twin for params [b,3] (a tensor: leaves stay attached)."""
    import torch
    b = params.shape[0]
    f64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    rep = lambda a: f64(a)[None].repeat((b,) + (1,) * np.ndim(a))
    x, v, Cm, F, p = rep(torus_particles(N)), torch.zeros((b, N, 3), dtype=torch.float64), torch.zeros((b, N, 3, 3), dtype=torch.float64), \
        rep(np.eye(3)[None].repeat(N, 0)), rep(PRIM0)
    soft = torch.full((b, 2), 666.0, dtype=torch.float64)
    fr = torch.full((b,), CONF.ground_friction, dtype=torch.float64)
    act = f64(ACTION)[None].repeat(b, 1)
    xs = [x]
    for _ in range(H):
        x, v, Cm, F, p = twin.step(x, v, Cm, F, p, act, soft, params[:, 0], params[:, 1], params[:, 2], fr)
        xs.append(x)
    return xs


def _twin_forward(twin, targets, params):
    """(per-frame losses [H+1,B], gradient [B,3]) of the twin at params [B,3] (NumPy)."""
    import torch
    leaf = torch.tensor(params, requires_grad=True)
    xs = _twin_rollout(twin, leaf)
    per = torch.stack([(twin.grid_mass(xs[f]) - targets[f][None]).abs().sum(-1) for f in range(H + 1)])
    per.sum().backward()
    return per.detach().numpy(), leaf.grad.numpy()


def _ident_case(n_iters=4):
    """The twin side of the last three tests, computed once: the truth's four target densities, and the reference's loop (tests/plb_sysid_twin.py)
    over the twin's losses and autograd gradients from the two candidates."""
    if not _IDENT:
        import torch
        from oracle.twin.plb_twin_torch import PlbTorchTwin
        torch.set_num_threads(8)
        twin = PlbTorchTwin(CONF)
        with torch.no_grad():
            xs = _twin_rollout(twin, torch.tensor([[TRUTH[0], TRUTH[1], CONF.yield_stress]]))
            targets = torch.stack([twin.grid_mass(x)[0] for x in xs])          # [H+1,G]
        opt = tw.AdamTwin(CAND, lr=100.0)
        params, per0, grad0, plist, losses = CAND.copy(), None, None, [], []
        for it in range(n_iters):
            per, grad = _twin_forward(twin, targets, params)
            if it == 0:
                per0, grad0 = per, grad
            losses.append(per.sum(0))
            params = tw.constrain(opt.step(grad), pin=(None, None, CONF.yield_stress))
            plist.append(params.copy())
        _IDENT.update(targets=targets.numpy().reshape(H + 1, NG, NG, NG), per0=per0, grad0=grad0, params=np.array(plist), losses=np.array(losses))
        for a in _IDENT.values():
            a.setflags(write=False)
    return _IDENT


def test_trajectory_loss_and_parameter_gradients():
    import torch
    from unidom_amd.algorithms.plb_identify import Identifier
    from unidom_amd.engine.plb_losses import PlbTrajectoryLoss
    c = _ident_case()
    assert np.all(c["grad0"] != 0), c["grad0"]                  # first, on the twin: every one of the gradients is there
    assert c["grad0"][0, 0] < 0 < c["grad0"][1, 0]              # g_E points towards the truth for both candidates
    assert np.all(c["per0"][0] == 0) and np.all(c["per0"][1:] > 0)
    sim = _sim()
    loss = PlbTrajectoryLoss(sim).update_target_density(c["targets"])
    ident = Identifier(sim, loss, [ACTION] * H, frames=range(H + 1), softness=666.0, pin=(None, None, CONF.yield_stress))
    per, grad = ident.forward(ident.start_state(), torch.tensor(CAND, device=sim.device))
    sim.check_status()
    per, grad = per.cpu().numpy(), grad.cpu().numpy()
    print("per-frame", per, c["per0"], "grad", grad, c["grad0"])
    assert per.shape == (H + 1, B) and grad.shape == (B, 3)
    # frame 0 scores the reset state against its own grid mass: 0 on the twin, round-off on the device
    assert np.abs(per[0]).max() < 1e-9 * np.abs(c["per0"]).max()
    assert _rel(per, c["per0"]) < 1e-9
    for f in range(1, H + 1):
        assert _rel(per[f], c["per0"][f]) < 1e-9, f
    for k, name in enumerate(("g_E", "g_nu", "g_yield_stress")):
        assert _rel(grad[:, k], c["grad0"][:, k]) < 1e-6, (name, grad[:, k], c["grad0"][:, k])
    # one recording per env [B,K,n,n,n] is the shared one when both envs hold the same
    both = PlbTrajectoryLoss(sim).update_target_density(np.stack([c["targets"]] * B))
    with torch.no_grad():
        states = ident.rollout(ident.start_state(), torch.tensor(CAND, device=sim.device))
        l_shared, l_both = loss.loss_of(states[1:], range(1, H + 1)), both.loss_of(states[1:], range(1, H + 1))
    assert l_shared.shape == (H, B) and _rel(l_both.cpu().numpy(), l_shared.cpu().numpy()) < 1e-13


def test_identifier_follows_the_twin_loop():
    import torch
    from unidom_amd.algorithms.plb_identify import Identifier
    from unidom_amd.engine.plb_losses import PlbTrajectoryLoss
    c = _ident_case()
    ref_l, ref_p = c["losses"], c["params"]
    assert np.all(np.diff(ref_l, axis=0) < 0), ref_l            # first, on the twin: the loss falls in both envs, at every iteration
    assert np.all(np.diff(ref_p[:, 0, 0]) > 50) and np.all(np.diff(ref_p[:, 1, 0]) < -50) and ref_p[0, 0, 0] > 3050 and ref_p[0, 1, 0] < 8950
    sim = _sim()
    loss = PlbTrajectoryLoss(sim).update_target_density(c["targets"])
    ident = Identifier(sim, loss, [ACTION] * H, frames=range(H + 1), softness=666.0, lr=100.0, pin=(None, None, CONF.yield_stress))
    best, plist, losses = ident.solve(CAND, 4)
    sim.check_status()
    best, plist, losses = best.cpu().numpy(), plist.cpu().numpy(), losses.cpu().numpy()
    print("params", plist, ref_p, "losses", losses, ref_l)
    assert plist.shape == (4, B, 3) and losses.shape == (4, B) and ident.total_steps == 4 * H
    for k in range(3):
        assert _rel(plist[:, :, k], ref_p[:, :, k]) < 1e-6, k
    assert np.all(plist[:, :, 2] == CONF.yield_stress)
    assert _rel(losses[0], ref_l[0]) < 1e-9 and _rel(losses[1:], ref_l[1:]) < 1e-6
    assert np.array_equal(best, plist[2])                       # the loss fell every time: the best parameters are those the last rollout ran with


def test_action_scale_on_host():
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    torch.set_num_threads(8)
    scale = (0.005, 0.005, 0.005)
    Bs = 3
    actions = np.array([[0.5, -0.3, 0.2], [1.0, -1.0, 0.7], [1.7, -2.0, 0.4]])      # inside, at and outside +-1
    rng = np.random.default_rng(8)
    # the state: the jitter of tests/test_plb.py:167-173, at which the project holds this path to its bars (x 1e-3, v 0.01, C 0.1, F 0.002,
    # E in [3e3, 5e3], nu in [0.3, 0.35], every other env yielding), sphere 0 on a particle of the body
    x0 = torus_particles(N)[None] + rng.normal(size=(Bs, N, 3)) * 1e-3
    v0 = rng.normal(size=(Bs, N, 3)) * 0.01
    C0 = rng.normal(size=(Bs, N, 3, 3)) * 0.1
    F0 = np.eye(3)[None, None] + rng.normal(size=(Bs, N, 3, 3)) * 0.002
    p0 = np.stack([x0[:, 3], np.repeat(PRIM0[1:2], Bs, 0)], 1)
    par = np.stack([rng.uniform(3e3, 5e3, size=Bs), rng.uniform(0.3, 0.35, size=Bs), np.where(np.arange(Bs) % 2 == 0, 1762.2, 5.0)], 1)
    wx, wv, wp = rng.normal(size=(Bs, N, 3)), rng.normal(size=(Bs, N, 3)) * 0.01, rng.normal(size=(Bs, 2, 3))

    def run(step, dev):
        T = lambda a: torch.tensor(a, device=dev, requires_grad=True)
        W = lambda a: torch.tensor(a, device=dev)
        leaves = dict(x=T(x0), v=T(v0), C=T(C0), F=T(F0), prim_pos=T(p0), action=T(actions), E=T(par[:, 0]), nu=T(par[:, 1]), ys=T(par[:, 2]))
        xo, vo, Co, Fo, po = step(leaves)
        ((xo * W(wx)).sum() + (vo * W(wv)).sum() + (po * W(wp)).sum() + 1e-3 * Co.sum() + 1e-2 * (Fo * Fo).sum()).backward()
        out = [t.detach().cpu().numpy() for t in (xo, vo, Co, Fo, po)]
        return out, {k: t.grad.cpu().numpy() for k, t in leaves.items()}

    twin = PlbTorchTwin(CONF)
    soft_t, fr_t = torch.full((Bs, 2), 666.0, dtype=torch.float64), torch.full((Bs,), CONF.ground_friction, dtype=torch.float64)
    ref_out, ref_g = run(lambda l: twin.step(l["x"], l["v"], l["C"], l["F"], l["prim_pos"], l["action"].clamp(-1, 1) * torch.tensor(scale, dtype=torch.float64), soft_t,
                                             l["E"], l["nu"], l["ys"], fr_t), "cpu")
    assert all(np.abs(g).max() > 0 for g in ref_g.values())
    assert np.all(ref_g["action"][2, :2] == 0) and np.all(ref_g["action"][1] != 0) and np.all(ref_g["action"][0] != 0)

    for on_host, plan in ((False, 1), (True, 2)):
        sim = _sim(batch=Bs, action_scale=scale, action_scale_on_host=on_host)
        assert sim.launch_plan() == plan, (on_host, sim.launch_plan())
        st0 = sim.reset()

        def step(l):
            st = sim.step(st0._replace(x=l["x"], v=l["v"], C=l["C"], F=l["F"], prim_pos=l["prim_pos"], E=l["E"], nu=l["nu"], yield_stress=l["ys"]),
                          l["action"])
            return st.x, st.v, st.C, st.F, st.prim_pos
        out, g = run(step, sim.device)
        sim.check_status()
        fwd = {name: _rel(a, b) for name, a, b in zip("x v C F prim_pos".split(), out, ref_out)}
        bwd = {name: _rel(g[name], ref_g[name]) for name in ref_g}
        print("on_host", on_host, "forward", fwd, "gradient", bwd)
        assert all(r < 1e-9 for r in fwd.values()), (on_host, fwd)
        assert all(r < 1e-6 for r in bwd.values()), (on_host, bwd)
        assert np.all(g["action"][2, :2] == 0) and np.all(g["action"][1] != 0)      # zero outside the clip, passing at equality

    with pytest.raises(ValueError):
        _sim(action_scale=(2.0, 1.0, 1.0), action_scale_on_host=True)
