"""Host side of the cloth env-glue tests (csrc/env_glue.hip: ud_chamfer_fwd/_bwd, ud_cloth_pnp_fwd/_bwd): the inputs, and NumPy
restatements of the kernels' arithmetic.  No GPU import: tests/test_cloth_glue_cpu.py checks on the host the conditions that
tests/test_cloth_glue_gpu.py rests on, with the same data.

env_glue.hip is compiled without FMA contraction and with correctly rounded divide and sqrt, so the f32 restatements below --
one NumPy f32 operation per kernel operation, in the kernel's association -- are exact: argmins, the contact distance, the macro
rows and the chamfer value (whose sums run in a fixed order) are compared for equality.  The f64 versions are the high-precision
reference for values and gradients."""
import functools

import numpy as np

f32 = np.float32
GLUE_T = 256        # threads per workgroup, and goal points per chunk of the chamfer backward
CH_ROWS = 64        # rows per workgroup of the chamfer forward (four lanes share a row)
MAXPTS = 4096       # points per cloud the chamfer kernels stage in LDS

# (P, Q): 64 = rows per workgroup of the forward, 256 = the workgroup and the backward's chunk, 3573 = fold_tshirt,
# 3756 = a P whose backward asks for more than 48 KB of dynamic LDS ((3 P + 1024) * 4 bytes; every P >= 3755 does), 4096 = the limit;
# unequal pairs make the forward's early return for the shorter direction fire
SHAPES = [(1, 1), (1, 4096), (4096, 1), (3, 5), (5, 3), (63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255), (17, 700),
          (700, 17), (3573, 625), (625, 3573), (3756, 64), (4096, 4096)]
PNP_SIZES = [1, 63, 64, 65, 255, 256, 257, 600, 3573]
PNP_BATCHES = [1, 3, 5]


# ---- inputs ----------------------------------------------------------------------------------------------------------
def clouds(P, Q, b):
    """x [P,3], y [Q,3], f32."""
    rs = np.random.RandomState((P * 8191 + Q * 31 + b) % 2 ** 31)
    x = rs.uniform(0.2, 0.8, size=(P, 3)).astype(f32)
    y = rs.uniform(0.2, 0.8, size=(Q, 3)).astype(f32)
    return x, y


def batch(P, Q, B):
    """x [B,P,3]: a distinct cloud per env; y [Q,3]: env 0's goal cloud, shared."""
    return np.stack([clouds(P, Q, b)[0] for b in range(B)]), clouds(P, Q, 0)[1]


def pnp_inputs(P, B):
    """actions [B,6], primitive0 [B,4], x [B,P,3], f32."""
    rs = np.random.RandomState((P * 8191 + B * 127 + 77) % 2 ** 31)
    u = lambda *s: rs.uniform(0.2, 0.8, size=s).astype(f32)
    return u(B, 6), u(B, 4), u(B, P, 3)


# ---- restatements ----------------------------------------------------------------------------------------------------
def mean_sq_f32(a, b):
    """mean_sq3 of the kernels: ((dx*dx + dy*dy) + dz*dz) / 3 in f32, a and b [...,3] broadcast."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((dx * dx + dy * dy) + dz * dz) / f32(3)


def mean_sq_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((dx * dx + dy * dy) + dz * dz) / 3.0


def sq_dist_f32(a, b):
    """The contact scan's (dx*dx + dy*dy) + dz*dz in f32 (no division)."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def sq_dist_f64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def argmin_first(m, axis):
    """The kernels' documented rule (min_takes): a NaN wins over any number, the earliest NaN first; otherwise the first minimum."""
    m = np.asarray(m)
    nan = np.isnan(m)
    first_min = np.argmin(np.where(nan, np.inf, m), axis=axis)
    return np.where(nan.any(axis=axis), nan.argmax(axis=axis), first_min).astype(np.int32)


def chamfer_argmins(x, y, ms=mean_sq_f32):
    """x [B,P,3], y [Q,3] -> idx_xy [B,P] (nearest goal point of every particle), idx_yx [B,Q] (nearest particle of every goal point)."""
    ixy, iyx = [], []
    with np.errstate(all="ignore"):
        for xb in x:
            m = ms(xb[:, None, :], y[None, :, :])           # [P,Q], (x - y) in both directions
            ixy.append(argmin_first(m, 1))
            iyx.append(argmin_first(m, 0))
    return np.stack(ixy), np.stack(iyx)


def _pairwise(v):
    """wave_sum's order: lane ^ 1, lane ^ 2, half-row mirror, row mirror, then (r0 + r1) + (r2 + r3) -- a balanced tree over 64 lanes."""
    v = np.asarray(v, f32)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _block_sum_f32(per_thread):
    """block_sum: wave_sum of each of the four waves, then 0 + w0 + w1 + w2 + w3 in turn."""
    w = _pairwise(np.asarray(per_thread, f32).reshape(GLUE_T // 64, 64))
    t = f32(0)
    for q in range(GLUE_T // 64):
        t = t + w[q]
    return t


def _strided_sum_f32(d):
    """Thread tid adds rows tid, tid + 256, ... in turn, starting from 0; then one block_sum."""
    n = len(d)
    pad = np.zeros(-(-n // GLUE_T) * GLUE_T, f32)
    pad[:n] = d
    acc = np.zeros(GLUE_T, f32)
    for row in pad.reshape(-1, GLUE_T):      # a thread past the end adds nothing: + 0 leaves the (non-negative) sum as it is
        acc = acc + row
    return _block_sum_f32(acc)


def chamfer_out_f32(x, y, ixy, iyx):
    """chamfer_sum_kernel bit for bit: out[b] = sum_p sqrt(m(p, ixy[p])) / P + sum_q sqrt(m(iyx[q], q)) / Q in its fixed order."""
    out = []
    with np.errstate(all="ignore"):
        for xb, jp, jq in zip(x, ixy, iyx):
            P, Q = len(jp), len(jq)
            dp = np.sqrt(mean_sq_f32(xb, y[jp]))
            dq = np.sqrt(mean_sq_f32(xb[jq], y))
            out.append(_strided_sum_f32(dp) / f32(P) + _strided_sum_f32(dq) / f32(Q))
    return np.asarray(out, f32)


def chamfer_out_f64(x, y):
    """calc_chamfer in f64 with the minimum taken over the squared distances (sqrt is monotone)."""
    out = []
    for xb in x:
        m = mean_sq_f64(xb[:, None, :], y[None, :, :])
        out.append(np.sqrt(m.min(1)).mean() + np.sqrt(m.min(0)).mean())
    return np.asarray(out)


def chamfer_grad_f64(x, y, ixy, iyx, g):
    """d (sum_b g[b] out[b]) / dx in f64 for the given argmins -> (grad [B,P,3], sum of |contribution| per entry [B,P,3],
    number of goal points k [B,P] whose argmin is that particle).  One contribution per distance the particle takes part in:
    (g / n) (x_p - y_q) / (3 d)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B, P, Q = x.shape[0], x.shape[1], y.shape[0]
    grad, mass, k = np.zeros((B, P, 3)), np.zeros((B, P, 3)), np.zeros((B, P), np.int64)
    for b in range(B):
        diff = x[b] - y[ixy[b]]
        c = diff * (g[b] / P / (3.0 * np.sqrt(mean_sq_f64(x[b], y[ixy[b]]))))[:, None]
        grad[b] += c
        mass[b] += np.abs(c)
        diff = x[b][iyx[b]] - y
        c = diff * (g[b] / Q / (3.0 * np.sqrt(mean_sq_f64(x[b][iyx[b]], y))))[:, None]
        np.add.at(grad[b], iyx[b], c)
        np.add.at(mass[b], iyx[b], np.abs(c))
        np.add.at(k[b], iyx[b], 1)
    return grad, mass, k


def chamfer_bwd_f32(x, y, ixy, iyx, g):
    """chamfer_bwd_kernel bit for bit -> g_x [B,P,3].  Every particle first takes its own x -> y term.  Then, per chunk of 256 goal
    points and per wave of 64 of them, the contributions naming one particle are summed in goal-point order starting from the first
    of them, and the wave's sums are added to the particle in wave order."""
    x, y, g = np.asarray(x, f32), np.asarray(y, f32), np.asarray(g, f32)
    B, P, Q = x.shape[0], x.shape[1], y.shape[0]
    out = np.empty((B, P, 3), f32)

    def terms(a, b, scale):             # (scale / (3 d)) * (a - b), d = sqrt(((dx*dx + dy*dy) + dz*dz) / 3)
        diff = a - b
        d = np.sqrt(((diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]) / f32(3))
        return (scale / (f32(3) * d))[:, None] * diff

    with np.errstate(all="ignore"):
        for b in range(B):
            gx = terms(x[b], y[ixy[b]], g[b] / f32(P))
            cc = terms(x[b][iyx[b]], y, g[b] / f32(Q))
            for w0 in range(0, Q, 64):             # waves in order: chunk by chunk, wave by wave inside a chunk
                sums = {}
                for q in range(w0, min(w0 + 64, Q)):
                    p = int(iyx[b, q])
                    sums[p] = cc[q] if p not in sums else sums[p] + cc[q]
                for p, s in sums.items():
                    gx[p] = gx[p] + s
            out[b] = gx
    return out


R3, R20 = f32(1) / f32(3), f32(1) / f32(20)


def pnp_f32(actions, prim0, x):
    """pnp_fwd_kernel bit for bit -> macro [40,B,8], contact [B], contact_idx [B]."""
    a, p0, x = np.asarray(actions, f32), np.asarray(prim0, f32), np.asarray(x, f32)
    B = a.shape[0]
    with np.errstate(all="ignore"):
        s = sq_dist_f32(a[:, None, :3], x)                   # pick - x_p
        idx = argmin_first(s, 1)
        contact = np.sqrt(s[np.arange(B), idx])
    macro = np.zeros((40, B, 8), f32)
    zero = np.zeros(B, f32)
    macro[0:3, :, 0] = (a[:, 0] - p0[:, 0]) * R3
    macro[0:3, :, 1] = (zero - p0[:, 1]) * R3
    macro[0:3, :, 2] = (a[:, 2] - p0[:, 2]) * R3
    macro[0:3, :, 3] = 1
    macro[3:13, :, 1] = f32(0.06) / f32(10)                  # constant / constant: a true division
    macro[13:33, :, 0] = (a[:, 3] - a[:, 0]) * R20
    macro[13:33, :, 1] = zero * R20
    macro[13:33, :, 2] = (a[:, 5] - a[:, 2]) * R20
    macro[33:40, :, 3] = 1
    return macro, contact.astype(f32), idx


def contact_argmin_f64(actions, x):
    return argmin_first(sq_dist_f64(np.asarray(actions)[:, None, :3], x), 1)


# ---- planted cases ---------------------------------------------------------------------------------------------------
FAR = np.array([3, 0, 0], f32)                 # the row cloud goes here: every row is then nearest to the plant
PLANT = np.array([2.0, 0.5, 0.5], f32)         # between the two clouds, nearer to every row than any random column
CH_ROWS_N, CH_COLS_N = 70, 300                 # rows: two workgroups, the second partly filled; columns: past one stride of 256
# duplicates: the smaller index must win although a later quad lane (column & 3) finds it
CH_PAIRS = [(3, 4), (2, 5), (1, 64), (7, 256), (0, CH_COLS_N - 1)]
CH_SINGLES = [0, 63, 64, 255, 256, CH_COLS_N - 1]


def chamfer_plant(direction, cols, b=0):
    """direction 0: particles are the rows, goal points the columns (idx_xy must name the plant); direction 1 the other way round
    (idx_yx).  `cols`: the column indices overwritten with one identical point.  -> x [1,P,3], y [Q,3], expected index."""
    if direction == 0:
        x, y = clouds(CH_ROWS_N, CH_COLS_N, 100 + b)
        x = x + FAR
        y[list(cols)] = PLANT
    else:
        x, y = clouds(CH_COLS_N, CH_ROWS_N, 100 + b)
        y = y + FAR
        x[list(cols)] = PLANT
    return x[None].astype(f32), y.astype(f32), min(cols)


def chamfer_plant_cases():
    return [(d, c) for d in (0, 1) for c in CH_PAIRS + [(s,) for s in CH_SINGLES]]


def contact_pairs(P):
    """Other waves, other strides, and the later stride inside an earlier wave (300 is thread 44's second particle, 64 thread 64's first)."""
    return [(63, 64), (5, 256), (255, 256), (0, P - 1)] + ([(300, 64)] if P > 300 else [])


def contact_singles(P):
    return [0, 63, 64, 255, 256, P - 1]


def contact_plant_cases():
    return [(P, c) for P in (257, 600) for c in contact_pairs(P) + [(s,) for s in contact_singles(P)]]


def contact_plant(P, parts, B=2):
    """The cloud far away, the particles `parts` of every env on one point next to that env's pick -> actions, prim0, x, expected index."""
    a, p0, x = pnp_inputs(P, B)
    x = x + FAR
    x[:, list(parts)] = (a[:, :3] + np.array([0.03125, 0, 0], f32))[:, None, :]
    return a, p0, x.astype(f32), min(parts)


SCATTER_P, SCATTER_Q = 3, 700


def scatter_case(B=3):
    """Every goal point's argmin is particle 1 (in the middle of the goal cloud, particles 0 and 2 far away): one particle receives
    every chunk and every wave of the backward's scatter."""
    x, y = batch(SCATTER_P, SCATTER_Q, B)
    x = x.copy()
    x[:, 1] = f32(0.5) + (x[:, 1] - f32(0.5)) * f32(0.125)
    x[:, 0] += FAR
    x[:, 2] -= FAR
    return x.astype(f32), y


@functools.lru_cache(maxsize=None)
def shape_case(P, Q, B=3):
    """(x, y, idx_xy, idx_yx) of batch(P, Q, B) by the f32 restatement; computed once and shared -- treat as read-only."""
    x, y = batch(P, Q, B)
    ixy, iyx = chamfer_argmins(x, y)
    for arr in (x, y, ixy, iyx):
        arr.setflags(write=False)
    return x, y, ixy, iyx
