"""The cases of tests/plb_sysid_edge_cases.py on the CPU: every case reaches the edge it is named for, the sign-field condition holds with no
exception (no cell within its mass bound of a tie, so the device's sign field must be the reference's bit for bit), no compared gradient is
identically zero, and the longdouble restatement agrees with what the project already trusts: PlbTorchTwin.grid_mass and its autograd within
1e-13 wherever the twin is defined (no clamp), tests/plb_sysid_twin.py::chamfer bit for bit, tests/plb_target_twin.py::iou within its f64
summation error.  The restatement does not depend on the order of the particles beyond 1e-17.

One line per case: PLBSYSID-CPU <tag>: ..."""
import numpy as np
import pytest

import plb_sysid_edge_cases as sc
from tests import plb_sysid_twin as tw

TWIN_BAR = 1e-13
PERM_BAR = 1e-17
REF_TAGS = tuple(t for t in sc.SEQ_TAGS if t != "tie")


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + sc.LD(1e-300)))


def test_longdouble_is_wider_than_double():
    assert np.finfo(sc.LD).eps <= 2.0 ** -63            # x87 extended or better: 2^11 below u


@pytest.mark.parametrize("tag", REF_TAGS)
def test_sequence_case_meets_the_sign_condition_and_is_not_trivial(tag):
    c, r = sc.seq_case(tag), sc.seq_ref(tag)
    M, N = c.x.shape[:2]
    G = c.n ** 3
    assert c.targets.shape[1] == G and c.gl.shape == (M,) and np.isfinite(c.x).all() and (c.gl != 0).all()
    print(f"PLBSYSID-CPU {tag}: violations {r.violations}  smallest |df| / e {r.margin:.2e}")
    assert r.violations == 0 and r.margin > 1.0 and r.occupied_free
    assert np.isfinite(r.loss.astype(np.float64)).all() and (r.loss > 0).all()
    for m in range(M):
        assert np.abs(r.gx[m]).max() > 0 and (r.gx_bound[m] >= 0).all(), m
        assert (r.sign[m] > 0).any() and (r.sign[m] < 0).any(), m
    assert (sc.clamp_count(c.x, c.n) == 0) == c.clamp_free
    # the mass bound is of round-off size and the loss bound far below the 1e-9 the path was held to so far
    assert float((r.loss_bound / r.loss).max()) < 1e-10


def test_grid_cases_reach_their_sweep_shapes():
    trips = {n: sc.sweep_trips(n ** 3) for n in (8, 10, 16, 40, 64)}
    assert trips[8] == [1, 1] and trips[16] == [1] * 16                    # 2 blocks; the one shape the suite had
    assert trips[10] == [1] * 4 and 10 ** 3 % 256 == 232 and 10 ** 3 % 64 == 40        # a partial block, a partial last ballot word
    assert len(trips[40]) == 128 and sorted(set(trips[40])) == [1, 2] and sum(trips[40]) == 250
    assert trips[64] == [8] * 128
    for n in (8, 10, 40, 64):
        c, r = sc.seq_case(f"grid{n}"), sc.seq_ref(f"grid{n}")
        assert c.n == n and sc.QUALITY[n] * 64 == n and c.x.shape == (2, 37, 3)
        G = n ** 3
        # the field is not empty in any part of the loop: cells with df != 0 in the first and the last quarter of the index range, and (n_grid
        # 40, 64) in cells a block reaches only on a later trip
        I = np.flatnonzero(r.sign[0])
        assert I.min() < G // 3 and I.max() > 2 * G // 3, (n, I.min(), I.max())
        if n >= 40:
            assert (I >= 256 * 128).any()
    w = sc.sign_words(sc.seq_ref("grid10").sign, 1000)
    assert w.shape == (2, 16, 2) and not (w[:, 15] >> np.uint64(40)).any()


def test_sign_words_are_the_ballots():
    rng = np.random.default_rng(3)
    s = rng.integers(-1, 2, size=(2, 1000)).astype(np.int8)
    w = sc.sign_words(s, 1000)
    for m, I in ((0, 0), (0, 63), (1, 64), (1, 999), (0, 517)):
        pos, neg = (int(w[m, I >> 6, 0]) >> (I & 63)) & 1, (int(w[m, I >> 6, 1]) >> (I & 63)) & 1
        assert pos - neg == s[m, I] and pos * neg == 0


def test_body_cases_put_item_boundaries_where_they_say():
    for N in sc.BODY_SIZES:
        c = sc.seq_case(f"body{N}")
        assert c.x.shape == (3, N, 3) and c.n == 16 and (c.gl < 0).sum() == 1 and len(set(np.abs(c.gl))) == 3
    # flat threads: item m starts at thread m N
    assert (63 % 64, 64 % 64, 65 % 64, 255 % 256, 256 % 256, 257 % 256) == (63, 0, 1, 255, 0, 1) and 3 * 1000 > 256 * 11


def test_chunk_cases():
    c = sc.seq_case("chunks")
    G = 16 ** 3
    assert c.x.shape == (7, 37, 3) and c.targets.shape[0] == 3 and sorted(set(c.index)) == [0, 1, 2]
    assert [sc.chunk_sizes(7, G, k * 8 * G) for k in sc.CHUNK_WORK_ITEMS] == [[1] * 7, [2, 2, 2, 1], [3, 3, 1], [7]]
    assert sc.library_work_bytes(7, G) == 7 * 8 * G
    assert sc.seq_case("chunks_noindex").index is None and sc.seq_case("chunks_noindex").targets.shape[0] == 1
    m = sc.seq_case("max_chunk")
    G = 8 ** 3
    assert m.x.shape == (65537, 1, 3) and sc.library_work_bytes(65537, G) == 65535 * 8 * G <= sc.SEQ_WORK_CAP
    assert sc.chunk_sizes(65537, G, sc.library_work_bytes(65537, G)) == [65535, 2]
    assert set(m.index) == {0, 1} and (m.gl > 0).any() and (m.gl < 0).any()


def test_low_corner_case():
    c = sc.seq_case("low_corner")
    base, fx, w, _ = sc.stencil(c.x, c.n)
    for m, axes in enumerate(((1,), (0, 2), (0, 1, 2))):
        for a in range(3):
            low = (base[m, :, a] == 0) & (fx[m, :, a] < 0.5)
            assert low.all() == (a in axes) and (a in axes or not low.any()), (m, a)
            if a in axes:
                assert (c.x[m, :, a] >= 0).all() and (w[1, m, :, a] < 0).sum() >= 8          # the middle weight below fx = 0.134
    assert sc.clamp_count(c.x, c.n) == 0 and c.clamp_free
    gm, k, A = sc.grid_mass_ref(c.x, c.n)
    assert (gm < 0).any() and float((A / np.abs(np.where(gm == 0, 1, gm))).max()) > 1.5           # cells where the terms cancel
    print(f"PLBSYSID-CPU low_corner: negative terms in {(w[1] < 0).sum()} weights, worst A / |gm| {float((A[gm != 0] / np.abs(gm[gm != 0])).max()):.1f}")


def test_outside_case():
    c = sc.seq_case("outside")
    n, dx = c.n, 1.0 / c.n
    assert not c.clamp_free and (c.x < -1.5 * dx).any() and (c.x > 1 - 2.5 * dx).any() and (c.x > 1).any()
    assert ((c.x[2] < 0) | (c.x[2] > 1)).all(-1).sum() >= 8                          # outside the box on three axes
    base, _, _, _ = sc.stencil(c.x, n)
    lin, clamped = sc._cells(base, n)
    assert clamped.sum() > 500 and (base.max(axis=(1, 2)) >= n - 2).all() and (base[[0, 2]].min(axis=(1, 2)) <= -2).all()
    assert ((c.x > 1 - 2.5 * dx) & (c.x < 1 - 1.5 * dx)).any() and ((c.x > 1 - 1.5 * dx) & (c.x < 1)).any()
    # >= 8 of one particle's 27 terms land in one cell
    most = max(np.bincount(lin[:, 2, p]).max() for p in range(24))
    assert most == 27
    assert all(np.bincount(lin[:, m, p]).max() >= 8 for m, p in ((2, 0), (2, 8), (2, 16)))
    # trunc, not floor: below -1.5 dx the base is trunc(s - 0.5) > floor(s - 0.5)
    s = c.x[0, :16, 0] * n
    assert (np.trunc(s - 0.5) == np.floor(s - 0.5) + 1).all()
    _, k, _ = sc.grid_mass_ref(c.x, n)
    print(f"PLBSYSID-CPU outside: {clamped.sum()} clamped stencil cells, most terms in one cell {k.max()}")
    assert k.max() >= 4 * 27 + 4 * 8


def test_tie_case_has_disjoint_interior_stencils():
    c = sc.seq_case("tie")
    assert c.targets is None and c.x.shape == (2, 8, 3) and sc.clamp_count(c.x, c.n) == 0
    _, k, _ = sc.grid_mass_ref(c.x, c.n)
    assert set(np.unique(k)) == {0, 1} and (k.sum(-1) == 8 * 27).all()


def test_nan_case_places():
    c = sc.seq_case("nan")
    t, I = sc.nan_target_cell()
    assert [m for m in range(3) if c.index[m] == t] == [sc.NAN_ITEM]                  # nobody else reads that target
    gm, k, _ = sc.grid_mass_ref(c.x, c.n)
    assert k[sc.NAN_ITEM, I] > 0 and c.targets[t, I] != 0
    assert c.x.shape[1] > sc.NAN_PARTICLE


# ---- the restatement against the twin --------------------------------------------------------------------------------------------------
def _twin(n, N):
    from oracle.twin.plb_twin import PlbConf
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    conf = PlbConf(quality=sc.QUALITY[n], n_particles=N)
    assert conf.n_grid == n and conf.p_mass == sc.p_mass(n)
    return PlbTorchTwin(conf)


@pytest.mark.parametrize("tag", tuple(t for t in REF_TAGS if sc.seq_case(t).clamp_free))
def test_restatement_agrees_with_the_torch_twin(tag):
    import torch
    torch.set_num_threads(8)
    c, r = sc.seq_case(tag), sc.seq_ref(tag)
    pick = np.arange(c.x.shape[0]) if c.x.shape[0] <= 8 else np.r_[0:48, c.x.shape[0] - 3:c.x.shape[0]]     # max_chunk: both launches
    twin = _twin(c.n, c.x.shape[1])
    tx = torch.tensor(c.x[pick], requires_grad=True)
    index = np.zeros(c.x.shape[0], np.int64) if c.index is None else np.asarray(c.index)
    gm = twin.grid_mass(tx)
    loss = (gm - torch.tensor(c.targets)[index[pick]]).abs().sum(-1)
    (loss * torch.tensor(c.gl[pick])).sum().backward()
    ref_gm = sc.grid_mass_ref(c.x[pick], c.n)[0]
    worst = {"mass": _rel(gm.detach().numpy(), ref_gm), "loss": float(np.abs((loss.detach().numpy() - r.loss[pick]) / r.loss[pick]).max()),
             "g_x": max(_rel(tx.grad[i].numpy(), r.gx[m]) for i, m in enumerate(pick))}
    print(f"PLBSYSID-CPU {tag}: restatement against the twin  " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v < TWIN_BAR for v in worst.values()), worst


@pytest.mark.parametrize("tag", ("grid10", "body257", "body1000", "low_corner", "outside", "chunks"))
def test_restatement_does_not_depend_on_the_particle_order(tag):
    c, r = sc.seq_case(tag), sc.seq_ref(tag)
    perm = np.random.default_rng(c.x.shape[1]).permutation(c.x.shape[1])
    gm = sc.grid_mass_ref(c.x, c.n)[0]
    gm2 = sc.grid_mass_ref(np.ascontiguousarray(c.x[:, perm]), c.n)[0]
    r2 = sc.density_ref(c.x, c.n, c.targets, c.index, c.gl, perm=perm)
    worst = max(_rel(gm2, gm), float(np.abs((r2.loss - r.loss) / r.loss).max()), _rel(r2.gx, r.gx))
    print(f"PLBSYSID-CPU {tag}: particle order {worst:.1e}")
    assert worst < PERM_BAR and np.array_equal(r2.sign, r.sign)


# ---- chamfer and IoU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sc.CHAMFER_TAGS)
def test_chamfer_reference_is_the_twins(tag):
    c = sc.chamfer_case(tag)
    out, mab, mba, bound = sc.chamfer_ref(c.a, c.b, c.index)
    M = c.a.shape[0]
    for m in (range(M) if M <= 8 else (0, 1, 2, M - 2, M - 1)):
        o, ab, ba = tw.chamfer(c.a[m], c.b[c.index[m]])
        assert np.array_equal(mab[m], ab) and np.array_equal(mba[m], ba), m
        assert abs(out[m] - o) <= bound[m] and 0 < bound[m] < 1e-12 * out[m], m
    Na, Nb = c.a.shape[1], c.b.shape[1]
    if tag in sc.TILE_TAGS and Na > 1 and Nb > 1:
        for m in range(3):
            d = np.linalg.norm(c.a[m][:, None] - c.b[c.index[m]][None], axis=-1)
            assert d[0].argmin() == Nb - 1 and d[:, 0].argmin() == Na - 1, m         # found in the other cloud's LAST tile
            assert d[0].min() < 0.5 * np.partition(d[0], 1)[1] and d[:, 0].min() < 0.5 * np.partition(d[:, 0], 1)[1]
    if tag == "lattice":
        d = np.linalg.norm(c.a[0][:, None] - c.b[c.index[0]][None], axis=-1)
        assert (mab == 0).any() and (mba == 0).any() and ((d == d.min(1, keepdims=True)).sum(1) > 1).sum() > 100      # equal distances
        assert len(np.unique(c.a[0], axis=0)) < 300
    if tag == "duplicates":
        assert np.array_equal(mab[:, :260], mab[:, 260:]) and np.array_equal(mba[:, :300], mba[:, 300:])
    if tag == "many":
        assert M == 65536 and (Na, Nb) == (2, 3) and set(c.index) == {0, 1}


def test_chamfer_reference_with_nan_and_bad_index():
    c = sc.chamfer_case("tiles257x255")
    a = c.a.copy()
    a[1, 256, 1] = np.nan
    out, mab, mba, _ = sc.chamfer_ref(a, c.b, (1, 0, 2))
    assert np.isnan(out[1]) and np.isnan(mab[1, 256]) and np.isnan(mab[1]).sum() == 1 and np.isnan(mba[1]).all()
    assert np.isnan(out[2]) and np.isnan(mab[2]).all() and np.isnan(mba[2]).all() and np.isfinite(out[0])


@pytest.mark.parametrize("G", sc.IOU_SIZES)
def test_iou_cases(G):
    from tests import plb_target_twin as ttw
    a, b = sc.iou_case(G)
    assert a.shape == b.shape == (3, G) and (a >= 0).all() and (b >= 0).all() and a[1].argmax() == G - 1
    if G > 1000:
        assert 0.2 < (a > 0).mean() < 0.4                                             # sparse
    for t in range(3):
        for bb in (b[t], b[1]):
            iou, bound = sc.iou_ref(a[t], bb)
            assert 0 < iou <= 1 + 4 * sc.U and 0 < bound < 8 * sc.gamma(G + 4) * iou
            assert abs(ttw.iou(a[t], bb) - float(iou)) <= 1e-12 * float(iou)
    # plb_iou_partial: 64 blocks of 256 threads stride over G; below 64 x 256 whole blocks own no element
    assert (G < sc.IOU_NB * 256) == (G <= 16383)
