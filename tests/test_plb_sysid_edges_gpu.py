"""GPU: the goal and system-identification kernels -- ud_plb_density_seq_fwd / _bwd and ud_plb_chamfer (csrc/plb_sysid.hip), ud_plb_density_iou
(csrc/plb_target.hip), ud_plb_grid_mass (plb_loss_mass, csrc/plb_adj.hip) -- at the cases of tests/plb_sysid_edge_cases.py, against its
longdouble restatement.  tests/test_plb_sysid_edge_cases.py shows on the CPU that every case reaches its edge, that the restatement is the
torch twin's wherever the twin is defined, and that no cell of any case is within its mass bound of a tie.

Tolerances: derived (tests/plb_sysid_edge_cases.py has the derivations), u = 2^-53, gamma_n = n u / (1 - n u):
    cell mass   |gm_dev - gm_ref|_I <= e_I = gamma_{k_I + 4} A_I;  a cell nobody touches is exactly 0;
                |sum_I gm_dev - N p_mass| <= gamma_{27 N} sum_I A_I
    loss        |loss_dev - loss_ref| <= sum_I e_I + gamma_G sum_I |df_I|
    sign field  the reference's, bit for bit, in every word (the CPU tests hold every cell outside its bound of a tie); bits past G are 0
    gradient    |g_dev - g_ref| <= gamma_{27 + 8} inv_dx sum |term| per component (hence per item and overall); exactly 0 where every term is
    chamfer     min arrays bit-equal (NaN positions included); |out_dev - out_ref| <= (gamma_Na + gamma_Nb + 4 u) out_ref; every route's out and
                min arrays bit-equal to every other route's
    IoU         plb_sysid_edge_cases.iou_ref: iou ((gamma_G + 3 u) (1 + (U + I) / (U - I)) + 2 u); two calls bit-equal

One line per case: PLBSYSID <tag>: <worst error / bound per quantity>.

As measured on an MI355X, one run (docs/HISTORY.md has the table): loss at most 7.0e-3 of its bound (max_chunk; 9.0e-4 elsewhere), g_x 0.17
(low_corner), cell mass 0.40, total mass 2.8e-2, chamfer out 2.7e-3 (0.44 at Na = 2, Nb = 3), IoU 0.14 (G = 1); the exact tie gave loss 0, an
all-zero sign field and g_x 0; every sign field, every min array and every route comparison was bit-equal.  53 tests, 3.5 s."""
import ctypes as C

import numpy as np
import pytest

import plb_sysid_edge_cases as sc

pytestmark = pytest.mark.gpu

LD = sc.LD
CANARY, ICANARY, PAD = -7.25e77, 0x5A5A5A5A5A5A5A5, 64
_SIMS = {}


def _sim(n, N):
    """one handle per (n_grid, N), kept: batch_size 2 at n_grid 16 (the grid-mass tests go past it), 1 elsewhere"""
    if (n, N) not in _SIMS:
        from unidom_amd.engine.plb_simulator import PlbConf as HipConf, PlbSimulator
        cfg = HipConf()
        cfg.quality, cfg.n_particles, cfg.substeps = sc.QUALITY[n], N, 2
        sim = PlbSimulator(cfg, batch_size=2 if n == 16 else 1)
        assert (sim.n_grid, sim.n_particles) == (n, N)
        _SIMS[(n, N)] = sim
    return _SIMS[(n, N)]


def _guarded(n, dtype):
    """(whole, middle): a device buffer of n elements with PAD canary elements either side"""
    import torch
    whole = torch.full((n + 2 * PAD,), CANARY if dtype.is_floating_point else ICANARY, dtype=dtype, device="cuda")
    return whole, whole[PAD:PAD + n]


def _intact(whole, n):
    fill = whole[0].item()
    return bool((whole[:PAD] == fill).all()) and bool((whole[PAD + n:] == fill).all())


def _p(t):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ratio(err, bound):
    """worst err / bound; where the bound is 0 the error has to be"""
    err, bound = np.asarray(err, LD), np.asarray(bound, LD)
    assert (err[bound == 0] == 0).all(), "non-zero where every term is zero"
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _raw(sim, x, targets, index, gl, work_items=None, with_sign=True):
    """The C entry points with canaries either side of every output and of the scratch -> (loss [M], sign words [M, W, 2] uint64 or None,
    g_x [M, N, 3] or None) as NumPy."""
    import torch
    from unidom_amd import _lib
    L = _lib.lib()
    M, N, T = x.shape[0], x.shape[1], targets.shape[0]
    G = sim.n_grid ** 3
    W = (G + 63) // 64
    X, TD, GL = torch.tensor(x, device="cuda"), torch.tensor(targets, device="cuda"), torch.tensor(gl, device="cuda")
    IDX = None if index is None else torch.tensor(index, dtype=torch.int32, device="cuda")
    lib_bytes = int(L.ud_plb_density_seq_work_bytes(sim._h, M))
    assert lib_bytes == sc.library_work_bytes(M, G) and int(L.ud_plb_density_seq_sign_bytes(sim._h, M)) == M * W * 16
    nwork = lib_bytes if work_items is None else work_items * 8 * G
    lw, loss = _guarded(M, torch.float64)
    ww, work = _guarded(nwork // 8, torch.float64)
    sw, sign = _guarded(M * W * 2, torch.int64) if with_sign else (None, None)
    _lib.check(L.ud_plb_density_seq_fwd(sim._h, M, _p(X), _p(TD), T, _p(IDX), _p(loss), _p(sign), _p(work), nwork, _stream()), "ud_plb_density_seq_fwd")
    gw = gx = None
    if with_sign:
        gw, gx = _guarded(M * N * 3, torch.float64)
        _lib.check(L.ud_plb_density_seq_bwd(sim._h, M, _p(X), _p(sign), _p(GL), _p(gx), _stream()), "ud_plb_density_seq_bwd")
    torch.cuda.synchronize()
    assert _intact(lw, M) and _intact(ww, nwork // 8), "a canary was overwritten"
    assert not with_sign or (_intact(sw, M * W * 2) and _intact(gw, M * N * 3)), "a canary was overwritten"
    assert bool((work == 0).all()), "the sweep leaves the scratch zero"
    if not with_sign:
        return loss.cpu().numpy(), None, None
    return loss.cpu().numpy(), sign.cpu().numpy().view(np.uint64).reshape(M, W, 2), gx.cpu().numpy().reshape(M, N, 3)


def _check_seq(label, ref, got, G, items=None):
    """loss, sign and g_x of the items `items` (None = all valid ones) against the reference -> prints and returns the worst ratios"""
    loss, sign, gx = got
    items = np.flatnonzero(~np.isnan(ref.loss.astype(np.float64))) if items is None else np.asarray(items)
    r_loss = _ratio(np.abs(loss[items].astype(LD) - ref.loss[items]), ref.loss_bound[items])
    out = f"PLBSYSID {label}: loss {r_loss:.1e}"
    assert r_loss <= 1.0, (label, r_loss)
    if sign is not None:
        want = sc.sign_words(ref.sign[items], G)
        assert np.array_equal(sign[items], want), (label, "sign field", int((sign[items] != want).sum()))
    if gx is not None:
        per = [_ratio(np.abs(gx[m].astype(LD) - ref.gx[m]), ref.gx_bound[m]) for m in items[:64]]       # per item ...
        r_gx = _ratio(np.abs(gx[items].astype(LD) - ref.gx[items]), ref.gx_bound[items])                # ... and overall
        assert r_gx <= 1.0 and max(per) <= 1.0, (label, r_gx, per)
        assert np.abs(gx[items]).max() > 0
        out += f"  g_x {r_gx:.2f}"
    print(out)
    return r_loss


def _autograd(sim, c):
    """once through PlbSimulator.density_seq_loss and autograd -> (loss, None, g_x)"""
    import torch
    n = sim.n_grid
    x = torch.tensor(c.x, device=sim.device, requires_grad=True)
    loss = sim.density_seq_loss(x, torch.tensor(c.targets.reshape(-1, n, n, n), device=sim.device), None if c.index is None else torch.tensor(c.index))
    assert loss.shape == (c.x.shape[0],) and loss.dtype == torch.float64
    (loss * torch.tensor(c.gl, device=sim.device)).sum().backward()
    return loss.detach().cpu().numpy(), None, x.grad.cpu().numpy()


# ---- the sequence loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sc.GRID_TAGS + sc.BODY_TAGS + sc.CORNER_TAGS + ("max_chunk",))
def test_sequence_loss_at_edge_shapes(tag):
    c, ref = sc.seq_case(tag), sc.seq_ref(tag)
    sim = _sim(c.n, c.x.shape[1])
    G = c.n ** 3
    if tag == "max_chunk":
        from unidom_amd import _lib
        assert int(_lib.lib().ud_plb_density_seq_work_bytes(sim._h, c.x.shape[0])) == 65535 * 8 * G
        assert sc.chunk_sizes(c.x.shape[0], G, 65535 * 8 * G) == [65535, 2]
    _check_seq(tag, ref, _raw(sim, c.x, c.targets, c.index, c.gl), G)
    _check_seq(tag + "/autograd", ref, _autograd(sim, c), G)


@pytest.mark.parametrize("tag", ("chunks", "chunks_noindex"))
def test_every_chunking_gives_the_same_bits(tag):
    c, ref = sc.seq_case(tag), sc.seq_ref(tag)
    sim = _sim(c.n, c.x.shape[1])
    G = c.n ** 3
    first = None
    for k in sc.CHUNK_WORK_ITEMS + (None,):
        got = _raw(sim, c.x, c.targets, c.index, c.gl, work_items=k)
        _check_seq(f"{tag}/work_items {k}", ref, got, G)
        first = first or got
        assert np.array_equal(got[1], first[1]) and np.array_equal(got[2], first[2]), k
    _check_seq(tag + "/autograd", ref, _autograd(sim, c), G)
    # without a sign field: the same forward
    lone = _raw(sim, c.x, c.targets, c.index, c.gl, work_items=3, with_sign=False)
    _check_seq(tag + "/sign NULL", ref, lone, G)


def test_exact_tie_is_an_exact_zero():
    """The target is ud_plb_grid_mass of the scored cloud itself; the stencils are disjoint, so every occupied cell holds ONE term, formed by the
    same expression in plb_loss_mass and plb_seq_scatter: df == 0 exactly -- loss 0, an all-zero sign field, g_x 0."""
    import torch
    c = sc.seq_case("tie")
    sim = _sim(c.n, c.x.shape[1])
    G = c.n ** 3
    gm = sim.get_grid_mass(sim.reset()._replace(x=torch.tensor(c.x, device=sim.device)))
    targets = gm.reshape(2, G).cpu().numpy()
    assert ((targets != 0).sum(-1) == 8 * 27).all()
    loss, sign, gx = _raw(sim, c.x, targets, c.index, c.gl)
    print("PLBSYSID tie: loss", loss, " sign words set", int((sign != 0).sum()), " max |g_x|", np.abs(gx).max())
    assert (loss == 0).all() and not sign.any() and (gx == 0).all()
    # ... and against the OTHER cloud's mass nothing is tied (the kernels are not simply returning zeros)
    loss, sign, gx = _raw(sim, c.x, targets, (1, 0), c.gl)
    assert (loss > 0).all() and sign.any() and np.abs(gx).max() > 0


def test_nan_in_a_target_cell_and_in_a_coordinate():
    c, ref = sc.seq_case("nan"), sc.seq_ref("nan")
    sim = _sim(c.n, c.x.shape[1])
    G = c.n ** 3
    others = [m for m in range(3) if m != sc.NAN_ITEM]
    clean = _raw(sim, c.x, c.targets, c.index, c.gl)
    _check_seq("nan/clean", ref, clean, G)
    t, I = sc.nan_target_cell()
    td = c.targets.copy()
    td[t, I] = np.nan
    loss, sign, gx = _raw(sim, c.x, td, c.index, c.gl)
    assert np.isnan(loss[sc.NAN_ITEM]) and not np.isnan(loss[others]).any()
    word, bit = I >> 6, np.uint64(I & 63)
    assert not ((sign[sc.NAN_ITEM, word] >> bit) & np.uint64(1)).any()                  # the NaN cell: neither ballot
    want = clean[1][sc.NAN_ITEM].copy()
    want[word] &= ~(np.uint64(1) << bit)
    assert np.array_equal(sign[sc.NAN_ITEM], want)                                       # every other cell of that item as before
    assert np.array_equal(sign[others], clean[1][others]) and np.array_equal(gx[others], clean[2][others])
    _check_seq("nan/target cell", ref, (loss, sign, gx), G, items=others)
    x = c.x.copy()
    x[sc.NAN_ITEM, sc.NAN_PARTICLE, sc.NAN_AXIS] = np.nan
    loss, sign, gx = _raw(sim, x, c.targets, c.index, c.gl)
    assert np.isnan(loss[sc.NAN_ITEM]) and not np.isnan(loss[others]).any()
    assert np.array_equal(sign[others], clean[1][others]) and np.array_equal(gx[others], clean[2][others])
    assert np.isnan(gx[sc.NAN_ITEM, sc.NAN_PARTICLE]).any()
    _check_seq("nan/coordinate", ref, (loss, sign, gx), G, items=others)


@pytest.mark.parametrize("bad", ({0: -1, 2: 3}, {3: -1, 4: 3, 5: -1}, {6: 3}), ids=("first_and_last_of_a_chunk", "a_whole_chunk", "a_chunk_of_one"))
def test_index_out_of_range(bad):
    """chunks of 3 items: {0, 1, 2}, {3, 4, 5}, {6}; -1 and T = 3"""
    c, ref = sc.seq_case("chunks"), sc.seq_ref("chunks")
    sim = _sim(c.n, c.x.shape[1])
    G = c.n ** 3
    assert sc.chunk_sizes(7, G, 3 * 8 * G) == [3, 3, 1]
    good = _raw(sim, c.x, c.targets, c.index, c.gl, work_items=3)
    index = tuple(bad.get(m, c.index[m]) for m in range(7))
    loss, sign, gx = _raw(sim, c.x, c.targets, index, c.gl, work_items=3)
    rest = [m for m in range(7) if m not in bad]
    assert np.isnan(loss[list(bad)]).all() and not sign[list(bad)].any() and (gx[list(bad)] == 0).all()
    assert np.array_equal(sign[rest], good[1][rest]) and np.array_equal(gx[rest], good[2][rest])
    _check_seq(f"index {bad}", ref, (loss, sign, gx), G, items=rest)
    lone = _raw(sim, c.x, c.targets, index, c.gl, work_items=3, with_sign=False)
    assert np.isnan(lone[0][list(bad)]).all()
    _check_seq(f"index {bad}/sign NULL", ref, lone, G, items=rest)


# ---- grid mass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sc.MASS_TAGS)
def test_grid_mass_with_the_clamp(tag):
    """B = 1, 2, 3 on a handle made for 2 envs: include/unidom_hip.h says B is not bound by max_envs, and the call accepts 3."""
    import torch
    from unidom_amd import _lib
    c = sc.seq_case(tag)
    sim = _sim(c.n, c.x.shape[1])
    assert sim.batch_size == 2
    G, N = c.n ** 3, c.x.shape[1]
    ref, k, A = sc.grid_mass_ref(c.x, c.n)
    e = sc.mass_bound(k, A)
    worst = 0.0
    for B in (1, 2, 3):
        X = torch.tensor(c.x[:B], device="cuda")
        gw, gm = _guarded(B * G, torch.float64)
        _lib.check(_lib.lib().ud_plb_grid_mass(sim._h, B, _p(X), _p(gm), _stream()), "ud_plb_grid_mass")
        torch.cuda.synchronize()
        assert _intact(gw, B * G)
        got = gm.cpu().numpy().reshape(B, G)
        assert (got[k[:B] == 0] == 0).all()
        worst = max(worst, _ratio(np.abs(got.astype(LD) - ref[:B]), e[:B]))
        total = got.astype(LD).sum(-1)
        r_tot = _ratio(np.abs(total - N * LD(sc.p_mass(c.n))), sc.gamma(27 * N) * A[:B].sum(-1))
        assert worst <= 1.0 and r_tot <= 1.0, (tag, B, worst, r_tot)
    wrapped = sim.get_grid_mass(sim.reset()._replace(x=torch.tensor(c.x[:2], device=sim.device)))
    assert wrapped.shape == (2, c.n, c.n, c.n)
    assert _ratio(np.abs(wrapped.reshape(2, G).cpu().numpy().astype(LD) - ref[:2]), e[:2]) <= 1.0
    print(f"PLBSYSID mass/{tag}: cell {worst:.2f}  total {r_tot:.1e}")


# ---- chamfer -------------------------------------------------------------------------------------------------------------------------
ROUTES = ("both", "neither", "ab", "ba")


def _chamfer(a, b, index, route):
    """ud_plb_chamfer with canaries -> (out [M], min_ab or None, min_ba or None) as NumPy.  both: two kernels (one workgroup per item from
    M = 65 536 on); neither / ab / ba: the one-workgroup kernel with no / one min array."""
    import torch
    from unidom_amd import _lib
    M, Na, Nb, Tb = a.shape[0], a.shape[1], b.shape[1], b.shape[0]
    A, Bt = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    IDX = None if index is None else torch.tensor(index, dtype=torch.int32, device="cuda")
    ow, out = _guarded(M, torch.float64)
    aw, mab = _guarded(M * Na, torch.float64) if route in ("both", "ab") else (None, None)
    bw, mba = _guarded(M * Nb, torch.float64) if route in ("both", "ba") else (None, None)
    _lib.check(_lib.lib().ud_plb_chamfer(M, Na, _p(A), Tb, Nb, _p(Bt), _p(IDX), _p(out), _p(mab), _p(mba), _stream()), "ud_plb_chamfer")
    torch.cuda.synchronize()
    assert _intact(ow, M) and (aw is None or _intact(aw, M * Na)) and (bw is None or _intact(bw, M * Nb)), "a canary was overwritten"
    return out.cpu().numpy(), None if mab is None else mab.cpu().numpy().reshape(M, Na), None if mba is None else mba.cpu().numpy().reshape(M, Nb)


def _check_chamfer(label, a, b, index, routes=ROUTES):
    """every route against the reference and against the first route -> {route: (out, mab, mba)}"""
    ref_out, ref_ab, ref_ba, bound = sc.chamfer_ref(a, b, index)
    got, worst = {}, 0.0
    for route in routes:
        out, mab, mba = got[route] = _chamfer(a, b, index, route)
        assert np.array_equal(np.isnan(out), np.isnan(ref_out)), (label, route)
        ok = ~np.isnan(ref_out)
        worst = max(worst, _ratio(np.abs(out[ok].astype(LD) - ref_out[ok].astype(LD)), bound[ok]))
        assert worst <= 1.0, (label, route, worst)
        assert mab is None or np.array_equal(mab, ref_ab, equal_nan=True), (label, route, "min_ab")
        assert mba is None or np.array_equal(mba, ref_ba, equal_nan=True), (label, route, "min_ba")
        assert np.array_equal(out, got[routes[0]][0], equal_nan=True), (label, route, "out differs between routes")
    print(f"PLBSYSID chamfer/{label}: out {worst:.1e}")
    return got


@pytest.mark.parametrize("tag", sc.TILE_TAGS + ("lattice", "duplicates"))
def test_chamfer_tiles_blocks_and_ties(tag):
    c = sc.chamfer_case(tag)
    _check_chamfer(tag, c.a, c.b, c.index)


def test_chamfer_many_items_take_the_fallback():
    c = sc.chamfer_case("many")
    M = c.a.shape[0]
    assert M == 65536
    full = _check_chamfer("many/65536", c.a, c.b, c.index, routes=("both", "neither"))               # both arrays, M > 65535: one workgroup per item
    part = _check_chamfer("many/65535", c.a[:-1], c.b, c.index[:-1], routes=("both",))               # the two-kernel route
    for i in range(3):
        assert np.array_equal(part["both"][i], full["both"][i][:-1]), i


def test_chamfer_nan_across_a_tile_edge():
    c = sc.chamfer_case("edge257")
    clean = _check_chamfer("edge257", c.a, c.b, c.index)
    for which, m, i, axis in sc.CHAMFER_NANS:
        a, b = c.a.copy(), c.b.copy()
        (a if which == "a" else b)[m, i, axis] = np.nan
        hit = [m] if which == "a" else [j for j in range(3) if c.index[j] == m]
        rest = [j for j in range(3) if j not in hit]
        assert hit and rest
        got = _check_chamfer(f"edge257/NaN in {which}[{m}, {i}]", a, b, c.index)       # np.min / np.mean: the reference is run on the NaN input
        for route in ROUTES:
            assert np.isnan(got[route][0][hit]).all()
            for k in range(3):
                assert got[route][k] is None or np.array_equal(got[route][k][rest], clean[route][k][rest]), (which, route, k)


def test_chamfer_index_out_of_range():
    c = sc.chamfer_case("edge257")
    clean = _check_chamfer("edge257", c.a, c.b, c.index)
    got = _check_chamfer("edge257/index (1, -1, 2)", c.a, c.b, (1, -1, 2))           # -1 and Tb = 2
    for route in ROUTES:
        out, mab, mba = got[route]
        assert np.isnan(out[1:]).all() and out[0] == clean[route][0][0]
        for arr, ref in ((mab, clean[route][1]), (mba, clean[route][2])):
            assert arr is None or (np.isnan(arr[1:]).all() and np.array_equal(arr[0], ref[0])), route


# ---- soft IoU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", sc.IOU_SIZES)
def test_density_iou_at_block_edges(G):
    import torch
    from unidom_amd import _lib
    L = _lib.lib()
    a, b = sc.iou_case(G)
    T = a.shape[0]
    A, Bt = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    nwork = int(L.ud_plb_density_iou_work_bytes(T)) // 8
    worst = 0.0
    for batched in (1, 0):
        other = Bt if batched else Bt[1].contiguous()
        runs = []
        for _ in range(2):
            ow, out = _guarded(T, torch.float64)
            ww, work = _guarded(nwork, torch.float64)
            _lib.check(L.ud_plb_density_iou(G, T, _p(A), _p(other), batched, _p(out), _p(work), _stream()), "ud_plb_density_iou")
            torch.cuda.synchronize()
            assert _intact(ow, T) and _intact(ww, nwork)
            runs.append(out.cpu().numpy())
        assert np.array_equal(runs[0], runs[1])
        for t in range(T):
            ref, bound = sc.iou_ref(a[t], b[t] if batched else b[1])
            worst = max(worst, _ratio(abs(LD(runs[0][t]) - ref), bound))
    print(f"PLBSYSID iou/G {G}: {worst:.1e}")
    assert worst <= 1.0
