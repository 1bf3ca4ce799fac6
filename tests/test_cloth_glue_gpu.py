"""GPU: the cloth half of csrc/env_glue.hip -- ud_chamfer_fwd/_bwd and ud_cloth_pnp_fwd/_bwd -- against the restatements of
tests/cloth_glue_cases.py.

Through the C ABI the stored argmins, the contact distance, the macro rows and the chamfer value are compared for EQUALITY with
the f32 NumPy restatement (the file is built without contraction and with correctly rounded divide / sqrt, and no sum in it depends
on arrival order); values are also held to 1e-6 of f64.  Through the autograd functions the gradients are held to f64 with
_glue_compare's bound (tests/test_envs_gpu.py).  Inputs come from the host generator, so tests/test_cloth_glue_cpu.py checks the
same data: no case has a near-tie, and none is left out here.  Output buffers are pre-filled with a sentinel before every call,
so anything left unwritten shows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cloth_glue_cases as cg
from test_envs_gpu import _glue_compare

pytestmark = pytest.mark.gpu

UD_OK, UD_ERR_INVALID, UD_ERR_UNSUPPORTED = 0, -1, -2
SENT_F, SENT_I = np.float32(-777.25), -12345
U = 2.0 ** -24          # unit roundoff of f32


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lib():
    from unidom_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    rc = getattr(L.lib(), name)(*[C.c_int(a) if isinstance(a, int) else L.ptr(a) for a in args], _stream())
    torch.cuda.synchronize()
    return rc


def chamfer_fwd(x, y, B=None, P=None, Q=None, drop=None):
    """-> rc, out [B], idx_xy [B,P], idx_yx [B,Q] (NumPy).  B / P / Q override what is passed as the dimensions; `drop` names an
    argument passed as a null pointer."""
    xd, yd = _dev(x), _dev(y)
    out = torch.full((x.shape[0],), float(SENT_F), device="cuda")
    ixy = torch.full(x.shape[:2], SENT_I, dtype=torch.int32, device="cuda")
    iyx = torch.full((x.shape[0], y.shape[0]), SENT_I, dtype=torch.int32, device="cuda")
    a = {"x": xd, "y": yd, "out": out, "ixy": ixy, "iyx": iyx}
    if drop:
        a[drop] = None
    rc = _call("ud_chamfer_fwd", x.shape[0] if B is None else B, x.shape[1] if P is None else P, y.shape[0] if Q is None else Q,
               a["x"], a["y"], a["out"], a["ixy"], a["iyx"])
    return rc, out.cpu().numpy(), ixy.cpu().numpy(), iyx.cpu().numpy()


def chamfer_bwd(x, y, ixy, iyx, g, B=None, P=None, Q=None, drop=None):
    a = {"x": _dev(x), "y": _dev(y), "ixy": _dev(ixy.astype(np.int32)), "iyx": _dev(iyx.astype(np.int32)), "g": _dev(np.asarray(g, np.float32)),
         "gx": torch.full(x.shape, float(SENT_F), device="cuda")}
    gx = a["gx"]
    if drop:
        a[drop] = None
    rc = _call("ud_chamfer_bwd", x.shape[0] if B is None else B, x.shape[1] if P is None else P, y.shape[0] if Q is None else Q,
               a["x"], a["y"], a["ixy"], a["iyx"], a["g"], a["gx"])
    return rc, gx.cpu().numpy()


def pnp_fwd(actions, prim0, x, B=None, drop=None):
    n = x.shape[0]
    a = {"a": _dev(actions), "p0": _dev(prim0), "x": _dev(x), "macro": torch.full((40, n, 8), float(SENT_F), device="cuda"),
         "contact": torch.full((n,), float(SENT_F), device="cuda"), "idx": torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")}
    outs = a["macro"], a["contact"], a["idx"]
    if drop:
        a[drop] = None
    rc = _call("ud_cloth_pnp_fwd", n if B is None else B, x.shape[1], a["a"], a["p0"], a["x"], a["macro"], a["contact"], a["idx"])
    return (rc,) + tuple(t.cpu().numpy() for t in outs)


@functools.lru_cache(maxsize=None)
def _shape_out_f64(P, Q):
    x, y, _, _ = cg.shape_case(P, Q)
    return cg.chamfer_out_f64(x, y)


def _check_chamfer_fwd(x, y, ixy, iyx, f64, tag):
    rc, out, kxy, kyx = chamfer_fwd(x, y)
    assert rc == UD_OK, _lib().lib().ud_last_error()
    np.testing.assert_array_equal(kxy, ixy, err_msg=f"{tag} idx_xy")
    np.testing.assert_array_equal(kyx, iyx, err_msg=f"{tag} idx_yx")
    e = np.abs(out.astype(np.float64) - f64)
    print(f"GLUE-ABI {tag} out: |kernel-f64| {e.max():.2e}  bound {1e-6 * np.abs(f64).min():.2e}")
    assert (e <= 1e-6 * np.abs(f64)).all(), (tag, e, f64)
    np.testing.assert_array_equal(_bits(out), _bits(cg.chamfer_out_f32(x, y, ixy, iyx)), err_msg=f"{tag} out, f32 restatement bit for bit")


# ---- through the C ABI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Q", cg.SHAPES)
def test_chamfer_fwd_argmins_equal_the_f32_restatement(P, Q):
    """ud_chamfer_fwd at every listed shape, three distinct clouds against one goal cloud, then one env alone: idx_xy and idx_yx
    equal the f32 restatement, `out` is within 1e-6 |f64| of the f64 restatement and bit-equal to the f32 one."""
    x, y, ixy, iyx = cg.shape_case(P, Q)
    f64 = _shape_out_f64(P, Q)
    _check_chamfer_fwd(x, y, ixy, iyx, f64, f"P={P} Q={Q} B=3")
    _check_chamfer_fwd(x[2:], y, ixy[2:], iyx[2:], f64[2:], f"P={P} Q={Q} B=1")


def test_chamfer_fwd_seventy_envs():
    """(65, 63) with B = 70: 70 x 2 x 2 workgroups; every env's indices, env 69's as well as env 0's."""
    x, y = cg.batch(65, 63, 70)
    ixy, iyx = cg.chamfer_argmins(x, y)
    _check_chamfer_fwd(x, y, ixy, iyx, cg.chamfer_out_f64(x, y), "P=65 Q=63 B=70")


@pytest.mark.parametrize("direction,cols", cg.chamfer_plant_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_chamfer_fwd_planted_duplicates_and_single_plants(direction, cols):
    """One identical point at two columns that other quad lanes (and other strides) scan: every row's argmin is the smaller index.
    Both directions' indices and the value equal the restatement."""
    x, y, want = cg.chamfer_plant(direction, cols)
    ixy, iyx = cg.chamfer_argmins(x, y)
    rc, out, kxy, kyx = chamfer_fwd(x, y)
    assert rc == UD_OK
    np.testing.assert_array_equal(kyx if direction else kxy, want)
    np.testing.assert_array_equal(kxy, ixy)
    np.testing.assert_array_equal(kyx, iyx)
    np.testing.assert_array_equal(_bits(out), _bits(cg.chamfer_out_f32(x, y, ixy, iyx)))
    f64 = cg.chamfer_out_f64(x, y)
    assert (np.abs(out - f64) <= 1e-6 * np.abs(f64)).all()


@pytest.mark.parametrize("P", cg.PNP_SIZES)
def test_pnp_fwd_equals_the_f32_restatement(P):
    """ud_cloth_pnp_fwd with B in {1, 3, 5} (the [40, B, 8] stride is not 4): contact_idx equal, contact and all 40 x B x 8 macro
    entries bit-equal to the restatement."""
    for B in cg.PNP_BATCHES:
        a, p0, x = cg.pnp_inputs(P, B)
        macro, contact, idx = cg.pnp_f32(a, p0, x)
        rc, kmacro, kcontact, kidx = pnp_fwd(a, p0, x)
        assert rc == UD_OK
        np.testing.assert_array_equal(kidx, idx, err_msg=f"P={P} B={B} contact_idx")
        np.testing.assert_array_equal(_bits(kcontact), _bits(contact), err_msg=f"P={P} B={B} contact")
        np.testing.assert_array_equal(_bits(kmacro), _bits(macro), err_msg=f"P={P} B={B} macro")


@pytest.mark.parametrize("P,parts", cg.contact_plant_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_pnp_fwd_planted_duplicates_and_single_plants(P, parts):
    """The nearest point sits at two particles held by other waves, other strides, or the later stride of an earlier wave: the
    smaller index is stored."""
    a, p0, x, want = cg.contact_plant(P, parts)
    macro, contact, idx = cg.pnp_f32(a, p0, x)
    rc, kmacro, kcontact, kidx = pnp_fwd(a, p0, x)
    assert rc == UD_OK
    np.testing.assert_array_equal(kidx, want)
    np.testing.assert_array_equal(kidx, idx)
    np.testing.assert_array_equal(_bits(kcontact), _bits(contact))
    np.testing.assert_array_equal(_bits(kmacro), _bits(macro))


def test_refusals_leave_the_outputs_untouched():
    """Above 4096 staged points: UD_ERR_UNSUPPORTED; B = 0 or a null pointer: UD_ERR_INVALID; nothing is written either way."""
    def untouched(*arrs):
        for a in arrs:
            assert (a == (SENT_I if a.dtype == np.int32 else SENT_F)).all()

    big, small = np.full((1, 4097, 3), 0.5, np.float32), np.full((4, 3), 0.25, np.float32)
    for x, y in ((big, small), (small[None], big[0])):                     # P = 4097, then Q = 4097
        rc, *outs = chamfer_fwd(x, y)
        assert rc == UD_ERR_UNSUPPORTED and b"ud_chamfer_fwd" in _lib().lib().ud_last_error()
        untouched(*outs)
    x, y = cg.batch(5, 3, 2)
    ixy, iyx = cg.chamfer_argmins(x, y)
    for kw in ({"B": 0}, {"drop": "out"}, {"drop": "x"}, {"drop": "iyx"}, {"P": 0}, {"Q": -1}):
        rc, *outs = chamfer_fwd(x, y, **kw)
        assert rc == UD_ERR_INVALID, kw
        untouched(*outs)
    rc, gx = chamfer_bwd(big, small, np.zeros((1, 4097), np.int32), np.zeros((1, 4), np.int32), [1.0])
    assert rc == UD_ERR_UNSUPPORTED and b"ud_chamfer_bwd" in _lib().lib().ud_last_error()
    untouched(gx)
    for kw in ({"B": 0}, {"drop": "g"}, {"drop": "iyx"}):
        rc, gx = chamfer_bwd(x, y, ixy, iyx, [1.0, 1.0], **kw)
        assert rc == UD_ERR_INVALID, kw
        untouched(gx)
    a, p0, xx = cg.pnp_inputs(5, 2)
    for kw in ({"B": 0}, {"drop": "contact"}, {"drop": "p0"}):
        rc, *outs = pnp_fwd(a, p0, xx, **kw)
        assert rc == UD_ERR_INVALID, kw
        untouched(*outs)


def _check_chamfer_bwd_bits(x, y, ixy, iyx, tag):
    w = np.array([0.75, -1.25, 2.0], np.float32)[:x.shape[0]]
    rc, gx = chamfer_bwd(x, y, ixy, iyx, w)
    assert rc == UD_OK, _lib().lib().ud_last_error()
    want = cg.chamfer_bwd_f32(x, y, ixy, iyx, w)
    bad = np.argwhere(_bits(gx) != _bits(want))
    assert len(bad) == 0, f"{tag}: {len(bad)} entries differ from the f32 restatement, first at {bad[0]}: {gx[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("P,Q", cg.SHAPES)
def test_chamfer_bwd_equals_the_f32_restatement(P, Q):
    """ud_chamfer_bwd fed the restatement's argmins: g_x bit-equal to the f32 restatement of its fixed summation order (own term,
    then per chunk and wave the sum from the first lane naming the particle, waves in order).  (3756, 64) and (4096, 4096) ask for
    more than 48 KB of dynamic LDS."""
    x, y, ixy, iyx = cg.shape_case(P, Q)
    _check_chamfer_bwd_bits(x, y, ixy, iyx, f"P={P} Q={Q}")


def test_chamfer_bwd_scatter_onto_one_particle_equals_the_f32_restatement():
    x, y = cg.scatter_case()
    ixy, iyx = cg.chamfer_argmins(x, y)
    _check_chamfer_bwd_bits(x, y, ixy, iyx, "scatter P=3 Q=700")


def test_chamfer_bwd_takes_more_goal_points_than_the_forward_stages():
    """ud_chamfer_bwd with Q = 5000 > 4096 and P = 64 is accepted (only P is staged): fed the restatement's argmins, its g_x is no
    worse than f32 torch against f64 -- |kernel - f64|max <= 4 |f32 torch - f64|max + 1e-6 |f64|max -- and within the per-entry
    bound (k + 8) 2^-24 sum|contribution| of the f64 gradient."""
    from unidom_amd.utils.util import calc_chamfer
    P, Q, B = 64, 5000, 3
    x, y = cg.batch(P, Q, B)
    ixy, iyx = cg.chamfer_argmins(x, y)
    w = np.array([0.75, -1.25, 2.0], np.float32)
    rc, gx = chamfer_bwd(x, y, ixy, iyx, w)
    assert rc == UD_OK, _lib().lib().ud_last_error()
    np.testing.assert_array_equal(_bits(gx), _bits(cg.chamfer_bwd_f32(x, y, ixy, iyx, w)))
    ref = {}
    for dt in (torch.float32, torch.float64):
        X = _dev(x).to(dt).requires_grad_(True)
        (g,) = torch.autograd.grad((calc_chamfer(X, _dev(y).to(dt)) * _dev(w).to(dt)).sum(), X)
        ref[dt] = g.double().cpu().numpy()
    e, e32, n = np.abs(gx - ref[torch.float64]).max(), np.abs(ref[torch.float32] - ref[torch.float64]).max(), np.abs(ref[torch.float64]).max()
    print(f"GLUE-ABI bwd P={P} Q={Q}: |kernel-f64| {e:.2e}  |f32-f64| {e32:.2e}  |f64| {n:.2e}  bound {4 * e32 + 1e-6 * n:.2e}")
    assert np.isfinite(gx).all() and e <= 4 * e32 + 1e-6 * n
    grad, mass, k = cg.chamfer_grad_f64(x, y, ixy, iyx, w.astype(np.float64))
    np.testing.assert_allclose(grad, ref[torch.float64], rtol=1e-10, atol=1e-14)
    ratio = np.abs(gx - grad) / ((k[..., None] + 8) * U * mass)
    print(f"GLUE-ABI bwd P={P} Q={Q}: largest |kernel-f64| / ((k+8) u sum|c|) {ratio.max():.3f}  (k up to {k.max()})")
    assert (ratio <= 1).all()


# ---- through the autograd functions ----------------------------------------------------------------------------------
def _chamfer_derived_bound(x, y, tag):
    """Value to 1e-6 |f64|; every gradient entry within (k + 8) 2^-24 sum|contribution| of the f64 gradient, k = the number of goal
    points whose argmin is that particle, the 8 for the roundings inside one contribution, the sum taken in f64."""
    from unidom_amd.envs.basic import _fused
    w = np.array([0.75, -1.25, 2.0])[:x.shape[0]]
    X = _dev(x).requires_grad_(True)
    out = _fused.chamfer(X, _dev(y))
    (g,) = torch.autograd.grad((out * _dev(w.astype(np.float32))).sum(), X)
    out, g = out.detach().double().cpu().numpy(), g.double().cpu().numpy()
    f64 = cg.chamfer_out_f64(x, y)
    e = np.abs(out - f64)
    print(f"GLUE {tag} out: |kernel-f64| {e.max():.2e}  bound {1e-6 * np.abs(f64).min():.2e}")
    assert (e <= 1e-6 * np.abs(f64)).all()
    ixy, iyx = cg.chamfer_argmins(x, y)
    grad, mass, k = cg.chamfer_grad_f64(x, y, ixy, iyx, w)
    bound = (k[..., None] + 8) * U * mass
    err = np.abs(g - grad)
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"GLUE {tag} grad: largest |kernel-f64| / bound {err[i] / bound[i]:.3f} at {i}: |kernel-f64| {err[i]:.2e}  bound {bound[i]:.2e}  k {k[i[:2]]}  "
          f"|f64| {np.abs(grad).max():.2e}")
    assert np.isfinite(g).all() and (err <= bound).all()


@pytest.mark.parametrize("P,Q", cg.SHAPES)
def test_chamfer_autograd_matches_f64(P, Q):
    """_fused.chamfer against calc_chamfer in f32 and f64 torch on the same inputs, one cotangent weight per env.  (3756, 64) and
    (4096, 4096) launch the backward with more than 48 KB of dynamic LDS.
    Bound: _glue_compare's own, |kernel - f64|max <= 4 |f32 torch - f64|max + 1e-6 |f64|max, at every shape but (1, 4096), where
    the one particle sums 4096 terms in another order than torch: there the derived per-entry bound
    (k + 8) 2^-24 sum|contribution| of _chamfer_derived_bound."""
    from unidom_amd.envs.basic import _fused
    from unidom_amd.utils.util import calc_chamfer
    x, y, _, _ = cg.shape_case(P, Q)
    if (P, Q) == (1, 4096):
        return _chamfer_derived_bound(x, y, f"chamfer P={P} Q={Q}")
    yd = _dev(y)
    run = lambda leaves, fusedp: {"out": _fused.chamfer(leaves[0], yd) if fusedp else calc_chamfer(leaves[0], yd.to(leaves[0].dtype))}
    _glue_compare(run, [_dev(x)], ["out"], f"chamfer P={P} Q={Q}")


def test_chamfer_autograd_scatter_onto_one_particle():
    """P = 3, Q = 700, every goal point's argmin particle 1: it receives every chunk and every wave of the backward's scatter.
    Bound: the derived per-entry one, (k + 8) 2^-24 sum|contribution| (k = 700 for particle 1, 0 for the others)."""
    x, y = cg.scatter_case()
    rc, _, _, kyx = chamfer_fwd(x, y)
    assert rc == UD_OK
    np.testing.assert_array_equal(kyx, 1)
    _chamfer_derived_bound(x, y, "chamfer scatter P=3 Q=700")


def _pnp_run(leaves, fusedp):
    from unidom_amd.engine.cloth_simulator import ClothState
    from unidom_amd.envs.basic import _fused
    from unidom_amd.envs.basic.cloth_env import ClothEnv
    a, p0, x = leaves
    if fusedp:
        macro, contact = _fused.pnp_and_contact(a, p0, x)
    else:
        st = ClothState(x=x, v=None, primitive0=p0, primitive1=None, action0=None, action1=None, key=None, cur_step=None,
                        stiffness=None, mu=None)
        macro = ClothEnv.get_pnp_actions(a, st)
        contact = torch.sqrt(((a[..., :3][:, None, :] - x) ** 2).sum(-1)).min(-1).values
    return {"macro": macro, "contact": contact, "release": macro[33:]}


@pytest.mark.parametrize("cots", [("macro",), ("contact",), ("macro", "contact"), ("release",)], ids="+".join)
@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 64, 257, 3573) for B in (1, 5)])
def test_pnp_autograd_matches_f64(P, B, cots):
    """_fused.pnp_and_contact against ClothEnv.get_pnp_actions plus the op-by-op contact distance, f32 and f64 torch, one cotangent set
    at a time: the macro actions', the contact's (the macro cotangent reaches backward as None), both, and the seven release rows'
    alone, where every input gradient is exactly zero.  Bound: _glue_compare's."""
    a, p0, x = cg.pnp_inputs(P, B)
    inputs = [_dev(a), _dev(p0), _dev(x)]
    _glue_compare(_pnp_run, inputs, list(cots), f"pnp P={P} B={B} {'+'.join(cots)}")
    if cots == ("release",):
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        outs = _pnp_run(leaves, True)
        grads = torch.autograd.grad((outs["release"] * torch.rand_like(outs["release"])).sum(), leaves, allow_unused=True)
        for g in grads:
            assert g is not None and bool((g == 0).all())


# ---- the unused contact distance -------------------------------------------------------------------------------------
def _defect_inputs():
    """Env 0: the pick exactly on particle 5 of a 300-particle cloud (contact == 0); env 1: particle 7 is NaN (contact NaN)."""
    a, p0, x = cg.pnp_inputs(300, 2)
    x[0, 5] = a[0, :3]
    x[1, 7] = np.nan
    return a, p0, x


def _pnp_grads(a, p0, x, wm, wc):
    from unidom_amd.envs.basic import _fused
    leaves = [_dev(t).requires_grad_(True) for t in (a, p0, x)]
    macro, contact = _fused.pnp_and_contact(*leaves)
    loss = (macro * wm).sum() + (0.0 if wc is None else (contact * wc).sum())
    return (contact.detach(),) + torch.autograd.grad(loss, leaves, allow_unused=True)


def test_unused_contact_distance_puts_no_nan_into_the_macro_gradient():
    """aux_reward=False: contact_distance is returned but not in the loss.  The kernel must then add no contact term -- 0 * d contact
    is NaN at contact == 0 and at a non-finite nearest particle -- and return the macro-only gradient of the op-by-op form."""
    a, p0, x = _defect_inputs()
    wm = torch.rand((40, 2, 8), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    contact, ga, gp, gx = _pnp_grads(a, p0, x, wm, None)
    assert float(contact[0]) == 0.0 and bool(torch.isnan(contact[1]))
    ref = [_dev(t).requires_grad_(True) for t in (a, p0, x)]
    ra, rp, rx = torch.autograd.grad((_pnp_run(ref, False)["macro"] * wm).sum(), ref, allow_unused=True)
    assert rx is None                                   # contact is not in the graph: nothing flows to x
    for name, got, want in (("g_actions", ga, ra), ("g_prim0", gp, rp), ("g_x", gx, torch.zeros_like(gx))):
        assert bool(torch.isfinite(got).all()), (name, got)
        torch.testing.assert_close(got, want, rtol=2e-5, atol=1e-7, msg=lambda m, name=name: f"{name}: {m}")
    assert bool((gx == 0).all())


def test_contact_in_the_loss_keeps_the_zero_over_zero_where_the_reference_has_it():
    """With the contact in the loss and the pick on a particle, d sqrt at 0 stays the 0/0 it is in the reference: NaN in
    g_actions[0, :3] and g_x[0, 5] and nowhere else in env 0; env 1's rows are what env 1 gives when run alone."""
    a, p0, x = _defect_inputs()
    g = torch.Generator(device="cuda").manual_seed(4)
    wm, wc = torch.rand((40, 2, 8), device="cuda", generator=g), torch.rand((2,), device="cuda", generator=g) + 0.5
    _, ga, gp, gx = _pnp_grads(a, p0, x, wm, wc)
    nan_a, nan_x = torch.zeros_like(ga[0], dtype=torch.bool), torch.zeros_like(gx[0], dtype=torch.bool)
    nan_a[:3] = True
    nan_x[5] = True
    assert torch.equal(torch.isnan(ga[0]), nan_a) and torch.equal(torch.isnan(gx[0]), nan_x)
    assert bool(torch.isfinite(ga[0][~nan_a]).all()) and bool((gx[0][~nan_x] == 0).all()) and bool(torch.isfinite(gp).all())
    _, ga1, gp1, gx1 = _pnp_grads(a[1:], p0[1:], x[1:], wm[:, 1:].contiguous(), wc[1:])
    for got, alone in ((ga[1], ga1[0]), (gp[1], gp1[0]), (gx[1], gx1[0])):
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(alone.cpu().numpy()))
    # env 1 itself: the NaN particle is the argmin, and only it and the pick see the NaN
    assert bool(torch.isnan(ga[1, :3]).all()) and bool(torch.isfinite(ga[1, 3:]).all())
    assert bool(torch.isnan(gx[1, 7]).all()) and bool((gx[1, torch.arange(300, device="cuda") != 7] == 0).all())
