"""The PLB persistent kernels (csrc/plb_cluster.hip: pcl_fwd_kernel, pcl_bwd_kernel), the multi-kernel path (csrc/plb.hip, csrc/plb_adj.hip)
and the loss kernels against the f64 torch twin at the cases of tests/plb_edge_cases.py -- the part sizes, ring residues, launch cuts, clamps,
clips, absent cotangents and loss shapes no other test reaches.  tests/test_plb_edge_cases.py shows on the CPU that every case reaches its
edge and that the twin's own sensitivity to the summation order is below 1e-8, so the numbers of test_plb.py::test_hip_step_adjoint_matches_
torch_twin apply unchanged: forward 1e-9, every adjoint leaf 1e-6 (max-norm relative, `_rel`), losses 1e-11 / 1e-9.  A leaf the case names
as a structural zero must be exactly 0 on both sides; one that is zero by cancellation is held to plb_edge_cases.CANCEL_BAR.

One line per case: PLBEDGE <tag>: fwd <worst rel>  adj <worst rel> (<leaf>).

What these cases found: the second call of n1000_b19_s2 repeated every output and leaf within 1.6e-14 except g_prim_pos, 1.4e-10 against the
1e-12 asked.  No arena was dirty: pcl_bwd_kernel added each sticky-contact sum G to pos[s + 1] and -G to pos[s] with two atomics per wave, in
two orders, and the start position kept (w + G) - G' of sums near 1e5.  It now keeps G once and the epilogue cancels it against itself where
the bound clamp passes (csrc/plb_cluster.hip), so g_prim_pos along a free axis is the cotangent handed in, bit for bit.  `prim` stays the
worst leaf of most lines below because the twin's autograd still forms (w + G) - G.

As measured on an MI355X (256 CUs), one run:

    PLBEDGE n1_b3_s3/path2: fwd 1.3e-15  adj 3.8e-12 (prim)
    PLBEDGE n1_b3_s3/path1: fwd 1.3e-15  adj 3.3e-11 (prim)
    PLBEDGE n5_b3_s3/path2: fwd 2.1e-15  adj 2.0e-14 (prim)
    PLBEDGE n5_b3_s3/path1: fwd 2.4e-15  adj 4.4e-14 (prim)
    PLBEDGE n32_b3_s3/path2: fwd 3.2e-15  adj 2.4e-11 (prim)
    PLBEDGE n32_b3_s3/path1: fwd 3.2e-15  adj 6.3e-11 (prim)
    PLBEDGE n33_b3_s3/path2: fwd 2.7e-15  adj 9.7e-12 (prim)
    PLBEDGE n33_b3_s3/path1: fwd 2.6e-15  adj 1.2e-11 (prim)
    PLBEDGE n37_b3_s3/path2: fwd 3.3e-15  adj 1.2e-11 (prim)
    PLBEDGE n37_b3_s3/path1: fwd 4.2e-15  adj 1.5e-11 (prim)
    PLBEDGE n64_b3_s3/path2: fwd 2.6e-15  adj 1.3e-11 (prim)
    PLBEDGE n64_b3_s3/path1: fwd 2.6e-15  adj 1.9e-11 (prim)
    PLBEDGE n1_b3_s3/path1/lanes1: fwd 3.3e-15  adj 1.7e-11 (prim)
    PLBEDGE n1_b3_s3/path1/lanes4: fwd 1.8e-15  adj 3.3e-11 (prim)
    PLBEDGE n1_b3_s3/path1/lanes8: fwd 1.3e-15  adj 3.3e-11 (prim)
    PLBEDGE n33_b3_s3/path1/lanes1: fwd 2.6e-15  adj 2.3e-11 (prim)
    PLBEDGE n33_b3_s3/path1/lanes4: fwd 2.7e-15  adj 2.3e-11 (prim)
    PLBEDGE n33_b3_s3/path1/lanes8: fwd 2.6e-15  adj 2.3e-11 (prim)
    PLBEDGE n37_b3_s1/path2: fwd 3.7e-15  adj 5.7e-12 (prim)
    PLBEDGE n37_b3_s2/path2: fwd 3.7e-15  adj 1.7e-11 (prim)
    PLBEDGE n37_b3_s3/path2: fwd 3.3e-15  adj 1.2e-11 (prim)
    PLBEDGE n37_b3_s4/path2: fwd 3.2e-15  adj 9.0e-12 (prim)
    PLBEDGE n33_b2_s128/path2: fwd 2.5e-13  adj 4.8e-11 (v)
    PLBEDGE n33_b2_s129/path1: fwd 2.7e-13  adj 2.4e-11 (ys)
    PLBEDGE n1000_b19_s2/path2: fwd 4.0e-15  adj 3.1e-11 (prim)
    PLBEDGE n1000_b19_s2/path2 second call on the handle: x1 1.6e-16  v1 4.1e-16  C1 9.9e-16  F1 7.4e-16  prim_pos1 0.0e+00  x 5.6e-16  v 2.3e-15
                                                          C 2.9e-15  F 2.7e-15  prim 0.0e+00  act 3.0e-16  E 2.0e-15  nu 1.3e-15  ys 1.4e-14  fric 3.4e-16
    PLBEDGE n1024_b2_s2/path2: fwd 3.6e-15  adj 2.0e-11 (prim)
    PLBEDGE n1025_b2_s2: launch_plan 1 on 256 CUs
    PLBEDGE n1025_b2_s2/path1: fwd 3.5e-15  adj 3.7e-11 (prim)
    PLBEDGE clip/path2: fwd 7.7e-15  adj 4.5e-12 (prim)
    PLBEDGE clip/path1: fwd 8.1e-15  adj 2.1e-11 (prim)
    PLBEDGE bound/path2: fwd 7.0e-15  adj 2.5e-14 (C)
    PLBEDGE bound/path1: fwd 7.1e-15  adj 1.7e-14 (C)
    PLBEDGE xclamp/path2: fwd 3.6e-15  adj 1.1e-11 (prim)
    PLBEDGE xclamp/path1: fwd 3.8e-15  adj 2.8e-11 (prim)
    PLBEDGE only_prim/path2: fwd 3.3e-15  adj 0.0e+00 (prim)  |x| |v| |C| |F| |E| |nu| |ys| |fric| 0.0e+00
    PLBEDGE only_prim/path2/null pointers: fwd 3.1e-15  adj 0.0e+00 (prim)  |x| |v| |C| |F| |E| |nu| |ys| |fric| 0.0e+00
    PLBEDGE only_prim/path1: fwd 4.1e-15  adj 0.0e+00 (prim)  |x| |v| |C| |F| |E| |nu| |ys| |fric| 0.0e+00
    PLBEDGE only_prim/path1/null pointers: fwd 3.8e-15  adj 0.0e+00 (prim)  |x| |v| |C| |F| |E| |nu| |ys| |fric| 0.0e+00
    PLBEDGE only_F/path2: fwd 3.3e-15  adj 2.1e-14 (ys)  |prim| 0.0e+00
    PLBEDGE only_F/path2/null pointers: fwd 3.3e-15  adj 2.4e-14 (ys)  |prim| 0.0e+00
    PLBEDGE only_F/path1: fwd 4.0e-15  adj 9.8e-15 (ys)  |prim| 1.4e-14
    PLBEDGE only_F/path1/null pointers: fwd 3.8e-15  adj 1.7e-14 (ys)  |prim| 1.4e-14
    PLBEDGE loss/n1_soft: fwd 2.0e-17  adj 1.3e-16 (prim)
    PLBEDGE loss/n1_hard: fwd 1.6e-19  adj 1.3e-16 (prim)
    PLBEDGE loss/n255_soft: fwd 4.2e-16  adj 3.6e-16 (prim)
    PLBEDGE loss/n255_hard: fwd 1.2e-16  adj 2.0e-16 (x)
    PLBEDGE loss/n256_soft: fwd 5.1e-16  adj 1.4e-15 (prim)
    PLBEDGE loss/n256_hard: fwd 1.1e-16  adj 1.7e-16 (x)
    PLBEDGE loss/n257_soft: fwd 3.8e-16  adj 1.3e-15 (prim)
    PLBEDGE loss/n257_hard: fwd 2.8e-16  adj 1.7e-16 (prim)
    PLBEDGE loss/inside0_soft: fwd 4.8e-16  adj 7.9e-16 (x)
    PLBEDGE loss/inside0_hard: fwd 3.0e-16  adj 1.2e-16 (x)
    PLBEDGE loss/insideboth_hard: fwd 3.0e-16  adj 3.5e-16 (x)  |prim| 0.0e+00
    PLBEDGE loss/sdfonly_soft: fwd 7.1e-16  adj 5.5e-16 (x)  |prim| 0.0e+00
    PLBEDGE loss/sdfonly_hard: fwd 7.1e-16  adj 5.5e-16 (x)  |prim| 0.0e+00
"""
import ctypes as C

import numpy as np
import pytest

import plb_edge_cases as pc

pytestmark = pytest.mark.gpu

FWD, ADJ = 1e-9, 1e-6
GRAD_LEAVES = ("x", "v", "C", "F", "prim", "act", "E", "nu", "ys", "fric")


def _rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


def _sim(case, path=0, lanes=0):
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    cfg = HipConf()
    cfg.quality, cfg.substeps, cfg.n_particles = pc.QUALITY, case.S, case.N
    cfg.path, cfg.lanes = path, lanes
    for k, val in case.conf_kw.items():
        setattr(cfg, k, val)
    sim = PlbSimulator(cfg, batch_size=case.B)
    assert (sim.n_grid, sim.substeps) == (pc.N_GRID, case.S) and abs(sim.dt - pc.DT) < 1e-18
    return sim


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _hip_step(sim, case):
    """sim.step + backward through autograd -> (outputs [5], {leaf: gradient}) as NumPy"""
    import torch
    x, v, Cm, F, prim, soft, act, E, nu, ys = case.inputs
    T = lambda a, r=True: torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)
    hl = dict(x=T(x), v=T(v), C=T(Cm), F=T(F), prim=T(prim), act=T(act), E=T(E), nu=T(nu), ys=T(ys))
    s = sim.reset()._replace(x=hl["x"], v=hl["v"], C=hl["C"], F=hl["F"], prim_pos=hl["prim"], softness=T(soft, False), E=hl["E"], nu=hl["nu"],
                             yield_stress=hl["ys"])
    s1 = sim.step(s, hl["act"])
    outs = (s1.x, s1.v, s1.C, s1.F, s1.prim_pos)
    sim.ground_friction_grad = None
    sum((t * T(wi, False)).sum() for t, wi in zip(outs, case.w) if wi is not None).backward()
    sim.check_status()
    grads = {k: t.grad.cpu().numpy() for k, t in hl.items()}
    grads["fric"] = sim.ground_friction_grad.cpu().numpy()
    return [t.detach().cpu().numpy() for t in outs], grads


def _raw_step(sim, case):
    """ud_plb_step_fwd / _bwd called directly, a null pointer for every absent output cotangent (autograd would hand the kernels zeros)"""
    import torch
    from unidom_amd import _lib
    L, dev, B = _lib.lib(), sim.device, case.B
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float64), device=dev)
    p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    gi = [T(a) for a in case.inputs]
    fo = [torch.empty_like(t) for t in gi[:5]]
    ck = torch.empty((L.ud_plb_ckpt_bytes(sim._h, C.c_int(B)) // 8,), dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(L.ud_plb_step_fwd(sim._h, C.c_int(B), *(p(t) for t in gi), *(p(t) for t in fo), p(ck), st), "ud_plb_step_fwd")
    gouts = [None if wi is None else T(wi) for wi in case.w]
    og = [torch.empty_like(t) for t in gi[:5]] + [torch.empty((B, 3), dtype=torch.float64, device=dev)] + \
         [torch.empty((B,), dtype=torch.float64, device=dev) for _ in range(4)]
    _lib.check(L.ud_plb_step_bwd(sim._h, C.c_int(B), p(ck), p(gi[5]), p(gi[6]), p(gi[7]), p(gi[8]), p(gi[9]), *(p(t) for t in gouts),
                                 *(p(t) for t in og), st), "ud_plb_step_bwd")
    sim.check_status()
    return [t.cpu().numpy() for t in fo], dict(zip(GRAD_LEAVES, (t.cpu().numpy() for t in og)))


def _hold_to_twin(label, case, outs, grads):
    """prints the PLBEDGE line, then asserts"""
    ref_outs, ref = pc.twin_step(case)
    sel = slice(None) if case.pick is None else list(case.pick)
    assert all(np.isfinite(o).all() for o in outs), label                       # on every env, followed or not
    assert all(np.isfinite(g).all() for g in grads.values()), label
    fwd = {n: _rel(o[sel], r) for n, o, r in zip(("x", "v", "C", "F", "prim_pos"), outs, ref_outs)}
    adj = {k: _rel(grads[k][sel], ref[k]) for k in GRAD_LEAVES if k not in case.zero + case.cancel}
    left = {k: np.abs(grads[k][sel]).max() for k in case.zero + case.cancel}
    wf, wa = max(fwd, key=fwd.get), max(adj, key=adj.get)
    print(f"PLBEDGE {label}: fwd {fwd[wf]:.1e}  adj {adj[wa]:.1e} ({wa})" + "".join(f"  |{k}| {val:.1e}" for k, val in left.items()))
    assert fwd[wf] < FWD, (label, fwd)
    assert adj[wa] < ADJ, (label, adj)
    for k in case.zero:
        assert left[k] == 0.0 and np.abs(ref[k]).max() == 0.0, (label, k, left[k])
    for k in case.cancel:
        assert np.abs(ref[k]).max() == 0.0 and left[k] <= pc.CANCEL_BAR(case, ref), (label, k, left[k], pc.CANCEL_BAR(case, ref))
    return ref_outs, ref


def _run(tag, path, lanes=0, plan=None):
    case = pc.step_case(tag)
    sim = _sim(case, path, lanes)
    assert sim.launch_plan() == (path if plan is None else plan)
    outs, grads = _hip_step(sim, case)
    ref_outs, ref = _hold_to_twin(f"{tag}/path{sim.launch_plan()}" + (f"/lanes{lanes}" if lanes else ""), case, outs, grads)
    return case, sim, outs, grads, ref_outs, ref


@pytest.mark.parametrize("path", [2, 1])
@pytest.mark.parametrize("tag", pc.PART_TAGS)
def test_part_sizes(tag, path):
    """N = 1, 5, 32 (one part: one particle, five, full), 33, 37, 64 (two parts: a last part of one particle, of five, full); B = 3, S = 3.
    In the persistent backward the `live` lanes and the qi == 0 parameter sums see a part with 31 idle octets."""
    _run(tag, path)


@pytest.mark.parametrize("lanes", [1, 4, 8])
@pytest.mark.parametrize("tag", ["n1_b3_s3", "n33_b3_s3"])
def test_part_sizes_multi_kernel_lane_mappings(tag, lanes):
    """the multi-kernel path's 1 / 4 / 8 lanes per particle with one particle in the launch, and with 33 (a block of 256 holds 32 octets)"""
    _run(tag, 1, lanes)


@pytest.mark.parametrize("tag", pc.RING_TAGS)
def test_ring_residues(tag):
    """S = 1, 2 (the ring of three exchange grids has not wrapped: nprev, kprev, gold refer to buffers not yet used), 3, 4; N = 37, B = 3"""
    _run(tag, 2)


@pytest.mark.parametrize("tag,plan", list(zip(pc.SMAX_TAGS, (2, 1))))
def test_pcl_smax_on_both_sides(tag, plan):
    """S = 128 = PCL_SMAX still runs the persistent kernels (the primitive trajectory fills its LDS array), S = 129 falls back to the multi-kernel
    path; N = 33, B = 2.  Forward and adjoint over the whole horizon (the twin takes about 10 s of CPU for each)."""
    _run(tag, 0, plan=plan)


def test_backward_call_cut_into_launches():
    """N = 1000 (32 parts, the last of 8 particles), S = 2, B = 19, every env with its own inputs.  An env of 32 parts fills an XCD at occupancy
    1: 8 envs per launch at occupancy 1, 16 at occupancy 2, and about 115 KB of LDS per backward workgroup allow no more -- on 256 CUs
    plb_cluster_step_bwd cuts the 19 envs into launches either way (the caller's arrays go by b = b0 + bl, the arenas by bl).  The twin follows
    the first and last env of each possible launch; then the same call again on the same handle: the arenas were back in their rest state."""
    if _cus() != 256:
        pytest.skip(f"{_cus()} CUs: the cut of 19 envs into launches of 8 or 16 is that of a 256-CU device")
    case, sim, outs, grads, _, _ = _run(pc.LAUNCH_TAG, 2)
    outs2, grads2 = _hip_step(sim, case)
    again = {n: _rel(b, a) for n, a, b in zip(("x1", "v1", "C1", "F1", "prim_pos1"), outs, outs2)}
    again.update({k: _rel(grads2[k], grads[k]) for k in GRAD_LEAVES})
    print(f"PLBEDGE {pc.LAUNCH_TAG}/path2 second call on the handle: " + "  ".join(f"{k} {val:.1e}" for k, val in again.items()))
    assert max(again.values()) < 1e-12, again


@pytest.mark.parametrize("tag", pc.LARGEST_TAGS)
def test_largest_persistent_body(tag):
    """N = 1024: 32 full parts, the most an XCD of 32 CUs holds at occupancy 1 -- the library picks the persistent path; N = 1025: 33 parts,
    which fit only at occupancy 2.  The library exposes its plan, not the occupancy it queried, so N = 1025's plan is printed (1 on the MI355X:
    two backward workgroups, over 100 KB of LDS each, do not share a CU) and whichever path it names is held to the twin, as N = 1024's is."""
    case = pc.step_case(tag)
    sim = _sim(case, 0)
    plan = sim.launch_plan()
    assert plan in (1, 2)
    if case.N == 1024:
        assert _cus() != 256 or plan == 2
    else:
        print(f"PLBEDGE {tag}: launch_plan {plan} on {_cus()} CUs")
    outs, grads = _hip_step(sim, case)
    _hold_to_twin(f"{tag}/path{plan}", case, outs, grads)


@pytest.mark.parametrize("path", [2, 1])
def test_action_clip(path):
    """raw action 1.7 (env 0, x) and -1.3 (env 1, z), the primitive free to travel: g_action of the clipped components is exactly 0 on both
    sides, every other one nonzero and within 1e-6 of its env's largest"""
    case, sim, outs, grads, _, ref = _run("clip", path)
    clipped = np.abs(case.inputs[6]) > 1
    assert (grads["act"][clipped] == 0.0).all() and (ref["act"][clipped] == 0.0).all()
    assert (np.abs(grads["act"][~clipped]) > 0).all()
    for b in range(case.B):                                                   # env by env: the unclipped env's gradient is 100 times the others'
        assert _rel(grads["act"][b], ref["act"][b]) < ADJ, (b, grads["act"][b], ref["act"][b])


@pytest.mark.parametrize("path", [2, 1])
def test_primitive_pinned_on_its_bound(path):
    """primitive 0 on its upper bound in x, pushed outward in every substep: the bound clamp passes nothing (g_action x exactly 0), the start
    position takes what substep 0's contact books to it"""
    case, sim, outs, grads, ref_outs, ref = _run("bound", path)
    assert (outs[4][:, 0, 0] == case.conf_kw["upper_bound"][0]).all()
    assert (grads["act"][:, 0] == 0.0).all() and (ref["act"][:, 0] == 0.0).all()
    assert _rel(grads["prim"][:, 0, 0], ref["prim"][:, 0, 0]) < ADJ


@pytest.mark.parametrize("path", [2, 1])
def test_particle_on_the_position_clamp(path):
    """one particle of every env ends every substep on x = 1 - 3 dx, bit for bit on both sides; the cotangent of its x passes only through g2p"""
    case, sim, outs, grads, ref_outs, ref = _run("xclamp", path)
    p = pc.XCLAMP_P
    assert (outs[0][:, p, 0] == pc.X_MAX).all() and (ref_outs[0][:, p, 0] == pc.X_MAX).all()
    np.testing.assert_array_equal(outs[0] == pc.X_MAX, ref_outs[0] == pc.X_MAX)
    assert _rel(grads["x"][:, p], ref["x"][:, p]) < ADJ


@pytest.mark.parametrize("path", [2, 1])
@pytest.mark.parametrize("tag", ["only_prim", "only_F"])
def test_absent_output_cotangents(tag, path):
    """a loss on prim_pos alone / on F alone.  Through autograd the kernels get zeros for the other cotangents; called directly they get null
    pointers (their `a.gx ? ... : 0.0` branches).  Both against the twin, and against each other at 1e-12 (the atomics' order)."""
    case, sim, outs, grads, _, _ = _run(tag, path)
    routs, rgrads = _raw_step(sim, case)
    _hold_to_twin(f"{tag}/path{path}/null pointers", case, routs, rgrads)
    for k in GRAD_LEAVES:
        if k not in case.zero + case.cancel:
            assert _rel(rgrads[k], grads[k]) < 1e-12, k


@pytest.mark.parametrize("tag", pc.LOSS_TAGS)
def test_losses(tag):
    """ud_plb_loss_fwd / bwd on the sphere handle against PlbTorchTwin.loss at n_grid 32, B = 3, g_loss = (1, 0, -2.5): N = 1, 255, 256, 257, a
    particle inside sphere 0, one inside each (hard: contact and its gradient exactly 0), weights (0, 0, 1.3).  1e-11 values, 1e-9 gradients."""
    import torch
    from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
    case = pc.loss_case(tag)
    cfg = HipConf()
    cfg.quality, cfg.n_particles = pc.QUALITY, case.N
    sim = PlbSimulator(cfg, batch_size=3)
    assert sim.n_grid == pc.N_GRID
    total, parts, gx, gp = pc.twin_loss(case)
    T = lambda a, r=True: torch.tensor(np.asarray(a, np.float64), device=sim.device, requires_grad=r)
    hx, hp = T(case.x), T(case.prim)
    hloss, hparts = sim.compute_loss(sim.reset()._replace(x=hx, prim_pos=hp), case.target_density, case.target_sdf, case.weights, case.soft)
    (hloss * T(pc.LOSS_GL, False)).sum().backward()
    gotx, gotp = hx.grad.cpu().numpy(), hp.grad.cpu().numpy()
    fwd = max(_rel(hloss.detach().cpu().numpy(), total), _rel(hparts.cpu().numpy(), parts))
    adj = {"x": _rel(gotx, gx)}
    if "prim" not in case.zero:
        adj["prim"] = _rel(gotp, gp)
    wa = max(adj, key=adj.get)
    print(f"PLBEDGE loss/{tag}: fwd {fwd:.1e}  adj {adj[wa]:.1e} ({wa})" + ("" if "prim" not in case.zero else f"  |prim| {np.abs(gotp).max():.1e}"))
    assert np.isfinite(gotx).all() and np.isfinite(gotp).all()
    assert fwd < 1e-11
    assert adj[wa] < 1e-9, adj
    assert (gotx[1] == 0.0).all() and (gotp[1] == 0.0).all()                  # g_loss[1] = 0
    if "prim" in case.zero:
        assert (gotp == 0.0).all() and (gp == 0.0).all()
    if tag == "insideboth_hard":
        assert (hparts.cpu().numpy()[:, 0] == 0.0).all() and (parts[:, 0] == 0.0).all()
    if tag == "inside0_hard":
        assert (gotp[:, 0] == 0.0).all()                                      # sphere 0's minimum is 0: nothing passes
