"""Shared by tests/test_plb_sysid_edge_cases.py (CPU) and tests/test_plb_sysid_edges_gpu.py: the inputs that put the goal and system-
identification kernels (csrc/plb_sysid.hip, the IoU half of csrc/plb_target.hip, plb_loss_mass / ud_plb_grid_mass in csrc/plb_adj.hip) at the
shapes and branches the rest of the suite never reaches, and their reference: a plain NumPy restatement in np.longdouble of what
include/unidom_hip.h and the file headers state.  Everything is computed once per process and handed out read-only.

The reference, and what the tolerances of the GPU tests rest on (u = 2^-53, gamma_n = n u / (1 - n u)):

    stencil     s = x inv_dx; base = trunc(s - 0.5) (toward zero, as (int) does); fx = s - base; w = (0.5 (1.5 - fx)^2, 0.75 - (fx - 1)^2,
                0.5 (fx - 0.5)^2), dw = (-(1.5 - fx), -2 (fx - 1), fx - 0.5): IN FLOAT64, every operation written as plb_weights writes it.  The f64
                objects are built without contraction, so these are the device's own bits -- they are inputs of what follows, not part of
                its error.  (A longdouble fx would differ from the device's by u |s|, which 0.5 (fx - 0.5)^2 magnifies without bound near
                fx = 0.5: no bound in gamma could hold.)
    grid mass   27 terms w_i w_j w_k p_mass per particle, formed and added in longdouble into the cell min(max(base + o, 0), n - 1) per axis.
                Per cell also k_I = the number of terms and A_I = sum |term|.  The device forms a term with three rounded products and adds
                the k_I terms of a cell in some order:  |gm_dev - gm_ref|_I <= e_I = gamma_{k_I + 4} A_I.
    loss        df_I = gm_I - target_I, loss = sum_I |df_I| (longdouble).  |loss_dev - loss_ref| <= sum_I e_I + gamma_G sum_I |df_I|.
    sign        sign(df_I), three-valued.  CONDITION (tests/test_plb_sysid_edge_cases.py, no exception): no cell has 0 < |df_I| <= e_I, and
                df_I == 0 only where every term and the target are exactly 0 -- so the device's sign field is the reference's, bit for bit,
                in every cell.
    gradient    g_x[p,d] = inv_dx sum_{27 cells} (g_loss sign_I p_mass) (dw_d w w), plb_seq_bwd_kernel's formula, in longdouble, with
                S[p,d] = sum |term|.  The device rounds g_loss sign p_mass once, each term three more times, adds 27 terms and scales once
                (32 roundings):  |g_dev - g_ref| <= gamma_{27 + 8} inv_dx S.
    chamfer     the two min arrays in f64 exactly as tests/plb_sysid_twin.py::chamfer forms them (minima are order-free: compared bit
                for bit); out_ref = fsum(min_ab) / Na + fsum(min_ba) / Nb.  |out_dev - out_ref| <= (gamma_Na + gamma_Nb + 4 u) out_ref.
    IoU         see `iou_ref`.

Cases (`seq_case(tag)`): see SEQ_TAGS and the builders below; chamfer: `chamfer_case(tag)`; IoU: `iou_case(G)`."""
import math
import zlib
from typing import NamedTuple, Optional

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SEQ_MAX_CHUNK = 65535            # csrc/plb_sysid.hip
SEQ_SWEEP_NB = 128
SEQ_WORK_CAP = 256 << 20
IOU_NB = 64                      # csrc/plb_target.hip

QUALITY = {8: 0.125, 10: 0.15625, 16: 0.25, 40: 0.625, 64: 1.0}     # n_grid = int(64 quality), every one exact in binary


def gamma(n):
    n = np.asarray(n, LD)
    return n * LD(U) / (1 - n * LD(U))


def _rng(tag):
    return np.random.default_rng(zlib.crc32(f"plb_sysid_edges/{tag}".encode()))


def _freeze(obj):
    for a in (obj.values() if isinstance(obj, dict) else obj):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return obj


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def p_mass(n):
    dx = 1.0 / n
    return (dx * 0.5) * (dx * 0.5)               # csrc/plb.hip: p_vol = (dx 0.5)(dx 0.5), p_mass = p_vol * 1


def stencil(x, n):
    """x [..., 3] f64 -> (base int64 [..., 3], fx, w [3 offsets, ..., 3 axes], dw): plb_weights in f64, operation for operation."""
    x = np.asarray(x, np.float64)
    s = x * float(n)
    base = np.trunc(s - 0.5).astype(np.int64)
    fx = s - base.astype(np.float64)
    w = np.stack([0.5 * (1.5 - fx) * (1.5 - fx), 0.75 - (fx - 1) * (fx - 1), 0.5 * (fx - 0.5) * (fx - 0.5)])
    dw = np.stack([-(1.5 - fx), -2 * (fx - 1), fx - 0.5])
    return base, fx, w, dw


def _cells(base, n):
    """-> lin [27, ...] (clamped), clamped [27, ...] bool, in the kernels' order cidx = (i 3 + j) 3 + k"""
    lin, cl = [], []
    for i in range(3):
        for j in range(3):
            for k in range(3):
                raw = base + np.array([i, j, k])
                c = np.clip(raw, 0, n - 1)
                lin.append((c[..., 0] * n + c[..., 1]) * n + c[..., 2])
                cl.append((c != raw).any(-1))
    return np.stack(lin), np.stack(cl)


def clamp_count(x, n):
    """number of (particle, stencil cell) pairs whose index the clamp moves"""
    return int(_cells(stencil(x, n)[0], n)[1].sum())


def grid_mass_ref(x, n):
    """x [M, N, 3] -> (gm [M, G] longdouble, k [M, G] int64, A [M, G] longdouble)"""
    x = np.asarray(x, np.float64)
    M, G = x.shape[0], n ** 3
    base, _, w, _ = stencil(x, n)
    lin, _ = _cells(base, n)
    wl = w.astype(LD)
    pm = LD(p_mass(n))
    gm, A, k = np.zeros(M * G, LD), np.zeros(M * G, LD), np.zeros(M * G, np.int64)
    off = (np.arange(M) * G)[:, None]
    c = 0
    for i in range(3):
        for j in range(3):
            for kk in range(3):
                t = (wl[i, ..., 0] * wl[j, ..., 1] * wl[kk, ..., 2] * pm).reshape(-1)
                idx = (lin[c] + off).reshape(-1)
                np.add.at(gm, idx, t)
                np.add.at(A, idx, np.abs(t))
                np.add.at(k, idx, 1)
                c += 1
    return gm.reshape(M, G), k.reshape(M, G), A.reshape(M, G)


def mass_bound(k, A):
    """e_I = gamma_{k_I + 4} A_I"""
    return gamma(k + 4) * A


class SeqRef(NamedTuple):
    loss: np.ndarray              # [M] longdouble (NaN: index outside [0, T))
    loss_bound: np.ndarray        # [M] longdouble
    sign: np.ndarray              # [M, G] int8
    gx: np.ndarray                # [M, N, 3] longdouble
    gx_bound: np.ndarray          # [M, N, 3] longdouble
    violations: int               # cells with 0 < |df| <= e_I, or df == 0 although a term or the target is not 0
    margin: float                 # min over the cells with df != 0 of |df| / e_I (inf where e_I = 0)
    occupied_free: bool           # every cell that gets a term has |df| > e_I (False only for the exact-tie case)


def density_ref(x, n, targets, index, gl, perm=None):
    """x [M, N, 3]; targets [T, G] f64; index [M] or None; gl [M] -> SeqRef.  Items are taken in blocks of at most 2^22 cells.
    perm: the particles enter in that order; g_x comes back un-permuted."""
    x = np.asarray(x, np.float64)
    M, N, G, T = x.shape[0], x.shape[1], n ** 3, targets.shape[0]
    index = np.zeros(M, np.int64) if index is None else np.asarray(index, np.int64)
    gl = np.asarray(gl, np.float64)
    if perm is not None:
        x = np.ascontiguousarray(x[:, perm])
    loss, lb = np.full(M, np.nan, LD), np.full(M, np.nan, LD)
    sign = np.zeros((M, G), np.int8)
    gx, gb = np.zeros((M, N, 3), LD), np.zeros((M, N, 3), LD)
    viol, margin, occ_free = 0, np.inf, True
    pm, inv_dx = LD(p_mass(n)), LD(n)
    step = max(1, (1 << 22) // G)
    for m0 in range(0, M, step):
        sl = slice(m0, min(M, m0 + step))
        valid = (index[sl] >= 0) & (index[sl] < T)
        rows = np.arange(sl.start, sl.stop)[valid]
        if rows.size == 0:
            continue
        xs = x[rows]
        gm, k, A = grid_mass_ref(xs, n)
        td = targets[index[rows]]
        df = gm - td.astype(LD)
        e = mass_bound(k, A)
        adf = np.abs(df)
        loss[rows] = adf.sum(-1)
        lb[rows] = e.sum(-1) + gamma(G) * adf.sum(-1)
        sg = np.sign(df).astype(np.int8)
        sign[rows] = sg
        nz = adf > 0
        viol += int((nz & (adf <= e)).sum()) + int((~nz & ((A > 0) | (td != 0))).sum())
        with np.errstate(divide="ignore"):
            if nz.any():
                margin = min(margin, float((adf[nz] / e[nz]).min()))
        occ_free = occ_free and bool((adf[k > 0] > e[k > 0]).all())
        # the gather of plb_seq_bwd_kernel
        base, _, w, dw = stencil(xs, n)
        lin, _ = _cells(base, n)
        wl, dwl = w.astype(LD), dw.astype(LD)
        g, S = np.zeros(xs.shape, LD), np.zeros(xs.shape, LD)
        r = np.arange(rows.size)[:, None]
        c = 0
        for i in range(3):
            for j in range(3):
                for kk in range(3):
                    gmI = gl[rows].astype(LD)[:, None] * sg[r, lin[c]].astype(LD) * pm
                    t = np.stack([gmI * dwl[i, ..., 0] * wl[j, ..., 1] * wl[kk, ..., 2],
                                  gmI * wl[i, ..., 0] * dwl[j, ..., 1] * wl[kk, ..., 2],
                                  gmI * wl[i, ..., 0] * wl[j, ..., 1] * dwl[kk, ..., 2]], -1)
                    g += t
                    S += np.abs(t)
                    c += 1
        gx[rows], gb[rows] = inv_dx * g, gamma(27 + 8) * inv_dx * S
    if perm is not None:
        inv = np.argsort(perm)
        gx, gb = gx[:, inv], gb[:, inv]
    return SeqRef(*_freeze([loss, lb, sign, gx, gb]), viol, margin, occ_free)


def sign_words(sign, G):
    """sign [M, G] int8 -> the device's field [M, ceil(G / 64), 2] uint64: ballot pairs (df > 0, df < 0) of 64 consecutive cells"""
    M, W = sign.shape[0], (G + 63) // 64
    out = np.zeros((M, W, 2), np.uint64)
    for which, val in ((0, 1), (1, -1)):
        bits = np.zeros((M, W * 64), np.uint8)
        bits[:, :G] = sign == val
        out[:, :, which] = np.packbits(bits.reshape(M, W, 64), axis=-1, bitorder="little").view("<u8")[..., 0]
    return out


def sweep_trips(G):
    """trips of plb_seq_sweep's loop for every block of one item: b0 = 256 blockIdx.x, b0 += 256 gridDim.x while b0 < G"""
    nbs = (G + 255) // 256
    nb = min(nbs, SEQ_SWEEP_NB)
    return [len(range(256 * b, G, 256 * nb)) for b in range(nb)]


def chunk_sizes(M, G, work_bytes):
    """the launches of ud_plb_density_seq_fwd's loop"""
    chunk = min(work_bytes // (8 * G), M, SEQ_MAX_CHUNK)
    return [min(chunk, M - m0) for m0 in range(0, M, chunk)]


def library_work_bytes(M, G):
    cap = min(max(SEQ_WORK_CAP // (8 * G), 1), SEQ_MAX_CHUNK)
    return 8 * G * min(M, cap)


# ---- sequence-loss cases -------------------------------------------------------------------------------------------------------------
class SeqCase(NamedTuple):
    tag: str
    n: int                        # n_grid
    x: np.ndarray                 # [M, N, 3]
    targets: Optional[np.ndarray]  # [T, G] f64; None: the exact-tie case takes them from the device
    index: Optional[tuple]        # [M] or None
    gl: np.ndarray                # [M]
    clamp_free: bool              # no stencil index is clamped: PlbTorchTwin.grid_mass is defined


GRID_TAGS = tuple(f"grid{n}" for n in (8, 10, 40, 64))
BODY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
BODY_TAGS = tuple(f"body{N}" for N in BODY_SIZES)
CORNER_TAGS = ("low_corner", "outside")
SEQ_TAGS = GRID_TAGS + BODY_TAGS + ("chunks", "chunks_noindex", "max_chunk") + CORNER_TAGS + ("tie", "nan")
MASS_TAGS = CORNER_TAGS + BODY_TAGS                                  # the clouds ud_plb_grid_mass is run on (M = 3 each)
CHUNK_WORK_ITEMS = (1, 2, 3, 7)
OFFSETS = np.array([(0.02, 0.0, 0.012), (-0.015, 0.01, 0.0), (0.005, -0.02, 0.017)])     # in units of a cell of n_grid 16: below 1 / 3
NAN_ITEM, NAN_PARTICLE, NAN_AXIS = 1, 11, 2

_SEQ, _SEQREF, _CHAMFER, _IOU = {}, {}, {}, {}


def _body(rng, N, n, lo=0.25, hi=0.75):
    return rng.uniform(lo, hi, size=(N, 3))


def _targets(body, n, T):
    """the grid mass of the same body displaced by less than a cell (never the mass of a scored cloud), rounded to f64"""
    disp = OFFSETS[:T] * (16.0 / n)
    return grid_mass_ref(body[None] + disp[:, None, :], n)[0].astype(np.float64)


def _plain(tag, n, N, M, T, index, gl, jitter=0.004):
    rng = _rng(tag)
    body = _body(rng, N, n)
    x = body[None] + rng.normal(size=(M, N, 3)) * jitter * (16.0 / n)
    return SeqCase(tag, n, x, _targets(body, n, T), index, np.asarray(gl, np.float64), True)


def seq_case(tag) -> SeqCase:
    """gridN          n_grid N in (8, 10, 40, 64), 37 particles, M = 2, T = 2: 2 sweep blocks; G = 1000 (a partial block and a partial last
                      ballot word); 250 blocks' worth on 128 (two trips and one); 8 trips per block
    bodyN          n_grid 16, M = 3, unequal g_loss with one negative: item boundaries inside a wave, on a wave, on a block
    chunks         n_grid 16, N = 37, M = 7, T = 3, index given; chunks_noindex: the same clouds against target 0
    max_chunk      n_grid 8, N = 1, M = 65 537: two launches of the loop, 65 535 items and 2
    low_corner     n_grid 16, N = 64, M = 3: x in [0, 0.5 dx) on one, two, three axes (base 0, fx < 0.5; negative weights below fx = 0.134);
                   the clamp is not triggered
    outside        n_grid 16, N = 64, M = 3: coordinates below -1.5 dx, above 1 - 2.5 dx (the clamp itself starts at 1 - 1.5 dx), above 1; item 2
                   has particles outside on three axes
    tie            n_grid 16, N = 8 isolated interior particles, M = 2: stencils disjoint; the targets are the device's own grid mass
    nan            n_grid 16, N = 37, M = 3, T = 2, index (0, 1, 0): the clean inputs; the test puts the NaN in (NAN_ITEM, ...)"""
    if tag in _SEQ:
        return _SEQ[tag]
    if tag in GRID_TAGS:
        n = int(tag[4:])
        rng = _rng(tag)
        body = rng.uniform(0.2, 0.8, size=(37, 3))                   # base + 2 <= n - 1 down to n_grid 8
        x = body[None] + rng.normal(size=(2, 37, 3)) * 0.004 * (16.0 / n)
        case = SeqCase(tag, n, x, _targets(body, n, 2), (1, 0), np.array([1.0, -2.5]), True)
    elif tag in BODY_TAGS:
        case = _plain(tag, 16, int(tag[4:]), 3, 2, (1, 0, 1), (1.0, -2.5, 0.75))
    elif tag == "chunks":
        case = _plain(tag, 16, 37, 7, 3, (2, 0, 1, 1, 2, 0, 1), (1.0, -2.5, 0.75, 3.0, -0.5, 0.25, 2.0))
    elif tag == "chunks_noindex":
        c = seq_case("chunks")
        case = c._replace(tag=tag, targets=c.targets[:1], index=None)
    elif tag == "nan":
        case = _plain(tag, 16, 37, 3, 2, (0, 1, 0), (1.0, -2.5, 0.75))
    elif tag == "max_chunk":
        n, M = 8, SEQ_MAX_CHUNK + 2
        rng = _rng(tag)
        body = np.array([[0.47, 0.52, 0.41]])
        x = body[None] + rng.uniform(-0.2, 0.2, size=(M, 1, 3))       # every item another place, all interior
        case = SeqCase(tag, n, x, _targets(body, n, 2), tuple(int(i) for i in rng.integers(0, 2, size=M)), rng.uniform(0.5, 2.0, size=M) *
                       rng.choice([-1.0, 1.0], size=M), True)
    elif tag == "low_corner":
        n, N, dx = 16, 64, 1.0 / 16
        rng = _rng(tag)
        body = _body(rng, N, n, 0.2, 0.6)
        x = np.stack([body.copy() for _ in range(3)])
        for m, axes in enumerate(((1,), (0, 2), (0, 1, 2))):
            for a in axes:
                x[m, :, a] = rng.uniform(0.0, 0.5 * dx, size=N)
                x[m, :8, a] = rng.uniform(0.0, 0.13 * dx, size=8)     # fx < 0.134: the middle weight is negative
        # the target: the same three bodies pushed INTO the box by less than a cell
        td = np.concatenate([grid_mass_ref(x[m][None] + np.array([0.021, 0.017, 0.012]), n)[0].astype(np.float64) for m in range(3)])
        case = SeqCase(tag, n, x, td, (0, 1, 2), np.array([1.0, -2.5, 0.75]), True)
    elif tag == "outside":
        n, N, dx = 16, 64, 1.0 / 16
        rng = _rng(tag)
        body = _body(rng, N, n, 0.3, 0.7)
        x = np.stack([body.copy() for _ in range(3)])
        below, wall, above = (-3.2 * dx, -1.6 * dx), (1 - 2.4 * dx, 1 - 0.6 * dx), (1.02, 1.3)
        # below -1.5 dx: base <= -2, all three offsets in cell 0.  Above 1 - 2.5 dx the stencil reaches the last cell, from 1 - 1.5 dx on
        # (base = n - 2) two offsets share it, above 1 all three
        x[0, :16, 0] = rng.uniform(*below, size=16)
        x[0, 16:32, 2] = rng.uniform(*wall, size=16)
        x[1, :16, 1] = rng.uniform(*above, size=16)
        x[1, 16:32, 0] = rng.uniform(*wall, size=16)
        x[1, 16:32, 2] = rng.uniform(*below, size=16)
        # item 2, outside on three axes.  A particle whose 27 terms all land in one corner cell leaves exactly p_mass there wherever it is --
        # in the displaced target too, an exact tie -- so each corner also gets particles that keep one offset per axis out of it
        x[2, :4] = rng.uniform(*below, size=(4, 3))                                   # 27 terms in cell (0, 0, 0)
        x[2, 4:8] = rng.uniform(-1.45 * dx, -0.6 * dx, size=(4, 3))                   # base -1: 8 terms in it
        x[2, 8:12] = rng.uniform(1 - 0.9 * dx, 1 - 0.55 * dx, size=(4, 3))            # base n - 2: 8 terms in cell (n - 1, n - 1, n - 1)
        x[2, 12:16] = rng.uniform(*above, size=(4, 3))                                # 27 terms in it
        x[2, 16:24] = np.stack([rng.uniform(*below, size=8), rng.uniform(*above, size=8), rng.uniform(1 - 1.4 * dx, 1 - 0.6 * dx, size=8)], -1)
        td = np.concatenate([grid_mass_ref(x[m][None] + np.array([0.021, -0.017, 0.012]), n)[0].astype(np.float64) for m in range(3)])
        case = SeqCase(tag, n, x, td, (0, 1, 2), np.array([1.0, -2.5, 0.75]), False)
    elif tag == "tie":
        n = 16
        rng = _rng(tag)
        corner = np.array([(i, j, k) for i in (3, 9) for j in (3, 9) for k in (3, 9)], np.float64)      # stencils [3, 5] and [9, 11] per axis
        x = (corner[None] + 0.5 + rng.uniform(0.05, 0.95, size=(2, 8, 3))) / n
        case = SeqCase(tag, n, x, None, (0, 1), np.array([1.0, -2.5]), True)
    else:
        raise KeyError(tag)
    _SEQ[tag] = SeqCase(*_freeze(list(case)))
    return _SEQ[tag]


def seq_ref(tag) -> SeqRef:
    """the reference of `seq_case(tag)` (not for "tie": its targets exist on the device only)"""
    if tag not in _SEQREF:
        c = seq_case(tag)
        _SEQREF[tag] = density_ref(c.x, c.n, c.targets, c.index, c.gl)
    return _SEQREF[tag]


def nan_target_cell():
    """(target, cell) of the NaN target cell of the "nan" case: in the one target only NAN_ITEM reads, the cell that item fills most"""
    c = seq_case("nan")
    return c.index[NAN_ITEM], int(np.argmax(grid_mass_ref(c.x[NAN_ITEM:NAN_ITEM + 1], c.n)[0][0]))


# ---- chamfer -------------------------------------------------------------------------------------------------------------------------
class ChamferCase(NamedTuple):
    tag: str
    a: np.ndarray                 # [M, Na, 3]
    b: np.ndarray                 # [Tb, Nb, 3]
    index: tuple                  # [M]


TILE_SHAPES = ((1, 1), (255, 257), (256, 256), (257, 255), (513, 1), (1, 513), (1000, 700))
TILE_TAGS = tuple(f"tiles{Na}x{Nb}" for Na, Nb in TILE_SHAPES)
CHAMFER_INDEX = (1, 0, 1)
CHAMFER_TAGS = TILE_TAGS + ("lattice", "duplicates", "edge257", "many")
MANY_M = 65536
# (array, item or cloud, point, axis) of the NaN across a tile edge, on the "edge257" clouds: b's cloud 1 is read by items 0 and 2
CHAMFER_NANS = (("b", 1, 255, 0), ("b", 1, 256, 2), ("a", 1, 256, 1))


def chamfer_case(tag) -> ChamferCase:
    """tilesAxB     M = 3, Tb = 2, index (1, 0, 1).  Where both clouds have more than one point the LAST point of every b cloud sits 1e-3 from
                 a_0 of the items that use it and the last point of a beside b_0: the nearest neighbour of a first point is found in the
                 other cloud's last tile, and its distance is the cloud's smallest
    lattice      coordinates k / 8, k in 0..4: 125 places for 300 and 270 points -- equal distances, shared points (d = 0), duplicates
    duplicates   random clouds, every point of a and of b present twice (the second copy one tile later)
    edge257      257 points each: the clouds the NaN tests (CHAMFER_NANS) and the index tests write into copies of
    many         M = 65 536, Na = 2, Nb = 3, Tb = 2: with both min arrays the fallback kernel; its first 65 535 items the two-kernel route"""
    if tag in _CHAMFER:
        return _CHAMFER[tag]
    rng = _rng("chamfer/" + tag)
    index = CHAMFER_INDEX
    if tag in TILE_TAGS:
        Na, Nb = TILE_SHAPES[TILE_TAGS.index(tag)]
        a, b = rng.uniform(size=(3, Na, 3)), rng.uniform(size=(2, Nb, 3))
        if Na > 1 and Nb > 1:
            # items 0 and 2 use cloud 1, item 1 cloud 0: a_0 of items 0 and 2 is the same point, so that one b point can sit beside both
            a[2, 0] = a[0, 0]
            b[1, Nb - 1] = a[0, 0] + np.array([1e-3, 0.0, 0.0])
            b[0, Nb - 1] = a[1, 0] + np.array([1e-3, 0.0, 0.0])
            for m in range(3):
                a[m, Na - 1] = b[index[m], 0] + np.array([0.0, 1e-3, 0.0])
    elif tag == "lattice":
        a, b = rng.integers(0, 5, size=(3, 300, 3)) / 8.0, rng.integers(0, 5, size=(2, 270, 3)) / 8.0
    elif tag == "duplicates":
        a, b = rng.uniform(size=(3, 520, 3)), rng.uniform(size=(2, 600, 3))
        a[:, 260:] = a[:, :260]
        b[:, 300:] = b[:, :300]
    elif tag == "edge257":
        a, b = rng.uniform(size=(3, 257, 3)), rng.uniform(size=(2, 257, 3))
    elif tag == "many":
        a, b = rng.uniform(size=(MANY_M, 2, 3)), rng.uniform(size=(2, 3, 3))
        index = tuple(int(i) for i in rng.integers(0, 2, size=MANY_M))
    else:
        raise KeyError(tag)
    _CHAMFER[tag] = ChamferCase(tag, *_freeze([a, b]), index)
    return _CHAMFER[tag]


def chamfer_ref(a, b, index):
    """-> (out [M] f64, min_ab [M, Na], min_ba [M, Nb], bound [M]).  The minima: the expression of plb_sysid_twin.chamfer over all items at once
    (tests/test_plb_sysid_edge_cases.py holds the two to each other bit for bit); the means: math.fsum.  An index outside [0, Tb): NaN."""
    a, b, index = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(index, np.int64)
    M, Na, Nb, Tb = a.shape[0], a.shape[1], b.shape[1], b.shape[0]
    mab, mba, out = np.full((M, Na), np.nan), np.full((M, Nb), np.nan), np.full(M, np.nan)
    ok = np.flatnonzero((index >= 0) & (index < Tb))
    step = max(1, (1 << 21) // (Na * Nb))
    for s in range(0, ok.size, step):
        r = ok[s:s + step]
        d = a[r][:, :, None, :] - b[index[r]][:, None, :, :]
        with np.errstate(invalid="ignore"):
            dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
            mab[r], mba[r] = np.min(dist, axis=2), np.min(dist, axis=1)
    for m in ok:
        out[m] = math.fsum(mab[m]) / Na + math.fsum(mba[m]) / Nb
    bound = np.array((gamma(Na) + gamma(Nb) + 4 * LD(U)) * np.abs(out).astype(LD), np.float64)
    return _freeze([out, mab, mba, bound])


# ---- soft IoU ------------------------------------------------------------------------------------------------------------------------
IOU_SIZES = (1, 63, 255, 256, 257, 16383, 16384, 16385, 64 ** 3)
IOU_T = 3


def iou_case(G):
    """-> (a [3, G], b [3, G]) sparse, non-negative (3 in 10 and 4 in 10 cells occupied), both non-zero in cells 0 and G - 1 so that the product
    sum is never empty; a[1]'s maximum is its last element"""
    if G not in _IOU:
        rng = _rng(f"iou/{G}")
        a = rng.uniform(size=(IOU_T, G)) * (rng.uniform(size=(IOU_T, G)) < 0.3)
        b = rng.uniform(size=(IOU_T, G)) * (rng.uniform(size=(IOU_T, G)) < 0.4)
        for arr in (a, b):
            arr[:, 0] = rng.uniform(0.2, 0.9, size=IOU_T)
            arr[:, G - 1] = rng.uniform(0.2, 0.9, size=IOU_T)
        a[1, G - 1] = 1.25
        _IOU[G] = tuple(_freeze([a, b]))
    return _IOU[G]


def iou_ref(a, b):
    """a, b [G] f64, non-negative -> (iou, bound) in longdouble.

    ma = max(0, max a), mb = max(0, max b): exact.  sab = sum a_I b_I over the f64 products (the device rounds each product once, to the same
    bits), sa = sum a_I, sb = sum b_I: math.fsum, i.e. exact sums rounded once.  I = sab / ma / mb, U = sa / ma + sb / mb, iou = I / (U - I).
    The device adds G non-negative terms in its tree order: each sum is within gamma_G of the exact one, the reference's within u.  To first
    order, with g = gamma_G + u:
        I: two more divisions              dI <= (g + 2 u) I
        U: a division each, one addition   dU <= (g + 2 u) U
        D = U - I: one subtraction         dD <= dU + dI + u D
        iou = I / D: one division          d iou <= iou (dI / I + dD / D + u) = iou ((g + 2 u) (1 + (U + I) / D) + 2 u)
    b / mb <= 1 gives sab / ma / mb <= sa / ma, and likewise for sb: U >= 2 I, D >= U / 2, (U + I) / D <= 3 -- the quotient is never
    ill-conditioned for non-negative densities."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    G = a.size
    ma, mb = LD(max(0.0, a.max())), LD(max(0.0, b.max()))
    sab, sa, sb = LD(math.fsum(a * b)), LD(math.fsum(a)), LD(math.fsum(b))
    I = sab / ma / mb
    Un = sa / ma + sb / mb
    D = Un - I
    iou = I / D
    g = gamma(G) + LD(U)
    return iou, iou * ((g + 2 * LD(U)) * (1 + (Un + I) / D) + 2 * LD(U))
