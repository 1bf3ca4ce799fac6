"""NumPy restatement of the PLB goal arithmetic: the target-SDF map (Loss.update_target / update_target_sdf, engine/losses/loss.py:77-106),
the soft IoU (iou_kernel, :239-254) and the optimisers of optimizer/optim.py.  Written from the formulas, cell-parallel per offset.

The map.  State per cell: S (distance, 1000 = none yet) and P (the occupied cell nearest so far); S_c = 1000 everywhere at the start.
One sweep, every cell I from the copies (S_c, P_c):
    density[I] > threshold:  S = 0, P = I
    otherwise:               S = 1000; for o in {-3..2}^3 without 0, lexicographic with ox slowest, v = I + o inside the grid:
                               if S_c[v] < 1000: d = sqrt(dx^2 + dy^2 + dz^2 + 1e-8) of x_I - x_{P_c[v]}, x_J = J * (1 / n_grid);
                                                 if d < S: S = d, P = P_c[v]
then (S_c, P_c) := (S, P).  The vectorised form visits the offsets in that order and updates with a strict <, which is the same loop.
"""
import numpy as np

INF = 1000.0


def sweep(n, occ, S_c, P_c):
    """One sweep.  occ [n,n,n] bool; S_c [n,n,n] f64; P_c [n,n,n,3] int64 (undefined where S_c = 1000).  Returns (S, P)."""
    h = 1.0 / n
    ar = np.arange(n)
    I = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), -1)                       # [n,n,n,3]
    xI = I * h                                                                     # fl(i * h)
    S = np.full((n, n, n), INF)
    P = np.full((n, n, n, 3), -1, dtype=np.int64)
    for ox in range(-3, 3):
        for oy in range(-3, 3):
            for oz in range(-3, 3):
                if ox == 0 and oy == 0 and oz == 0:
                    continue
                # cells I whose neighbour v = I + o is inside the grid: I in [lo, hi) per axis
                sl_I, sl_v = [], []
                for o in (ox, oy, oz):
                    lo, hi = max(0, -o), min(n, n - o)
                    sl_I.append(slice(lo, hi))
                    sl_v.append(slice(lo + o, hi + o))
                sl_I, sl_v = tuple(sl_I), tuple(sl_v)
                Sv, Pv = S_c[sl_v], P_c[sl_v]
                diff = xI[sl_I] - Pv * h                                           # fl(i h) - fl(p h), per component
                d = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2] + 1e-8)
                take = (Sv < INF) & (d < S[sl_I])
                S[sl_I] = np.where(take, d, S[sl_I])
                P[sl_I] = np.where(take[..., None], Pv, P[sl_I])
    S = np.where(occ, 0.0, S)
    P = np.where(occ[..., None], I, P)
    return S, P


def target_sdf(density, threshold=1e-4, sweeps=0, stop_at_fixed_point=False):
    """density [n,n,n] -> (sdf [n,n,n] f64, nearest [n,n,n] int32 linear index or -1, sweeps_run).
    sweeps = 0: the reference's 2 n.  stop_at_fixed_point: stop after the first sweep that changes nothing (the result is that of all
    the sweeps: the map is deterministic).  sweeps_run = the number of sweeps executed; for the literal loop it is still reported as
    min(sweeps, 1-based number of the first sweep that changed nothing), the device's convention."""
    density = np.asarray(density, np.float64)
    n = density.shape[0]
    assert density.shape == (n, n, n)
    occ = density > threshold
    sweeps = 2 * n if sweeps == 0 else sweeps
    S = np.full((n, n, n), INF)
    P = np.full((n, n, n, 3), -1, dtype=np.int64)
    fixed = None
    for s in range(sweeps):
        S1, P1 = sweep(n, occ, S, P)
        same = np.array_equal(S1, S) and np.array_equal(np.where((S1 < INF)[..., None], P1, -1), np.where((S < INF)[..., None], P, -1))
        S, P = S1, P1
        if same and fixed is None:
            fixed = s + 1
            if stop_at_fixed_point:
                break
    near = np.where(S < INF, (P[..., 0] * n + P[..., 1]) * n + P[..., 2], -1).astype(np.int32)
    return S, near, (fixed if fixed is not None else sweeps)


def brute_force_sdf(density, threshold=1e-4):
    """sqrt(|x_I - x_J|^2 + 1e-8) to the nearest occupied J (0 on occupied cells; 1000 everywhere without any): what the map converges to
    as a VALUE (ties in the argmin are the map's own business)."""
    density = np.asarray(density, np.float64)
    n = density.shape[0]
    occ = density > threshold
    if not occ.any():
        return np.full((n, n, n), INF)
    h = 1.0 / n
    ar = np.arange(n)
    xI = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), -1) * h
    out = np.full((n, n, n), np.inf)
    for J in np.argwhere(occ):
        diff = xI - J * h
        out = np.minimum(out, np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2] + 1e-8))
    return np.where(occ, 0.0, out)


def iou(a, b):
    """iou_kernel: both maxima start at 0."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    ma, mb = max(0.0, a.max()), max(0.0, b.max())
    with np.errstate(divide="ignore", invalid="ignore"):
        I = np.float64(np.sum(a * b)) / ma / mb
        U = np.float64(np.sum(a)) / ma + np.float64(np.sum(b)) / mb
        return I / (U - I)


class MomentumTwin:
    def __init__(self, params, lr=0.1, bounds=(-1.0, 1.0), momentum=0.9):
        self.p, self.lr, self.bounds, self.mu = np.array(params, np.float64), lr, bounds, momentum
        self.buf = np.zeros_like(self.p)

    def step(self, g):
        g = self.buf * self.mu + g * (1 - self.mu)
        self.buf = g
        self.p = np.clip(self.p - self.lr * g, *self.bounds)
        return self.p.copy()


class AdamTwin:
    def __init__(self, params, lr=0.1, bounds=(-1.0, 1.0), beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        self.p, self.lr, self.bounds = np.array(params, np.float64), lr, bounds
        self.b1, self.b2, self.eps, self.iter = beta_1, beta_2, epsilon, 0
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)

    def step(self, g):
        self.m = self.b1 * self.m + (1 - self.b1) * g
        self.v = self.b2 * self.v + (1 - self.b2) * (g * g)
        m_cap = self.m / (1 - self.b1 ** (self.iter + 1))
        v_cap = self.v / (1 - self.b2 ** (self.iter + 1))
        self.iter += 1
        self.p = np.clip(self.p - (self.lr * m_cap) / (np.sqrt(v_cap) + self.eps), *self.bounds)
        return self.p.copy()
