"""CPU: the NumPy twin of the PLB goal arithmetic (tests/plb_target_twin.py) against known answers, the optimisers of
algorithms/plb_solver.py against a restatement of optim.py's formulas, and PlbLoss's reward arithmetic over a stub simulator.

The map starts from S_c = 1000 everywhere, so the FIRST sweep can only mark the occupied cells (no neighbour has a nearest cell yet);
the asymmetric window I - J in {-2..3} shows after the SECOND sweep.  That is what update_target_sdf does (its copies are written at
the end of each call), and what the device is held to in tests/test_plb_target_gpu.py."""
import numpy as np
import pytest

from tests import plb_target_twin as tw


def _one_cell(n, J):
    d = np.zeros((n, n, n))
    d[J] = 1.0
    return d


def _corner_blob_and_far_cell(n):
    d = np.zeros((n, n, n))
    d[:3, :2, :3] = 0.5
    d[n - 2, n - 1, n - 3] = 2e-4
    return d


def test_one_cell_window_after_one_and_two_sweeps_and_full_run():
    n, J = 8, (1, 4, 6)
    d = _one_cell(n, J)
    S1, near1, _ = tw.target_sdf(d, sweeps=1)
    assert S1[J] == 0.0 and (S1 < 1000).sum() == 1 and near1[J] == (J[0] * n + J[1]) * n + J[2] and (near1 >= 0).sum() == 1
    S2, near2, _ = tw.target_sdf(d, sweeps=2)
    I = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1)
    rel = I - np.array(J)
    window = ((rel >= -2) & (rel <= 3)).all(-1)              # I sees v = I + o, o in -3..2: J = I + o  <=>  I - J in -2..3
    assert window.sum() == 5 * 6 * 4                          # clipped by the faces: i in 0..4, j in 2..7, k in 4..7
    assert np.array_equal(S2 < 1000, window) and np.array_equal(near2 >= 0, window)
    S, near, run = tw.target_sdf(d)
    expect = np.sqrt((rel.astype(np.float64) ** 2).sum(-1) / 64 + 1e-8)
    expect[J] = 0.0
    assert np.allclose(S, expect, rtol=1e-15, atol=0) and (near == (J[0] * n + J[1]) * n + J[2]).all()
    assert S[J] == 0.0 and run < 2 * n


@pytest.mark.parametrize("n", [16, 32])
def test_literal_sweeps_equal_the_fixed_point_and_the_brute_force_distance(n):
    d = _corner_blob_and_far_cell(n)
    Ss, ns, runs = tw.target_sdf(d, stop_at_fixed_point=True)
    assert 3 < runs < 2 * n                                   # the fixed point arrives long before 2 n
    if n == 16:                                               # the literal 2 n sweeps: only where they are cheap
        Sl, nl, runl = tw.target_sdf(d)
        assert np.array_equal(Sl, Ss) and np.array_equal(nl, ns) and runl == runs
    bf = tw.brute_force_sdf(d)
    assert np.array_equal(Ss, bf)                             # same formula on the same (I, J) pair: the same bits
    # nearest really is a nearest occupied cell
    occ = d > 1e-4
    assert occ.reshape(-1)[ns.reshape(-1)].all()


def test_empty_full_and_threshold():
    n = 8
    S, near, run = tw.target_sdf(np.zeros((n, n, n)))
    assert (S == 1000).all() and (near == -1).all() and run == 1
    S, near, run = tw.target_sdf(np.ones((n, n, n)))
    assert (S == 0).all() and np.array_equal(near.reshape(-1), np.arange(n ** 3)) and run == 2
    d = np.zeros((n, n, n))
    d[1, 1, 1] = 1e-4                                        # exactly the threshold: not occupied (strict >)
    d[5, 5, 5] = np.nextafter(1e-4, 1.0)
    S, near, _ = tw.target_sdf(d)
    assert S[1, 1, 1] > 0 and S[5, 5, 5] == 0 and (near == (5 * n + 5) * n + 5).all()


def test_strict_less_keeps_the_first_minimal_candidate_in_offset_order():
    """Two occupied cells mirror-symmetric about a plane of cells: every cell of the plane is equidistant from both, so which one it names
    is decided by the offset order (ox slowest, from -3) and the strict <.  Through the first sweeps the plane cell next to the pair hears
    of the LOWER cell first (offset -k comes before +k) and nothing later is strictly nearer."""
    n = 16
    d = np.zeros((n, n, n))
    lo, hi = (5, 8, 8), (9, 8, 8)                            # mirror plane i = 7
    d[lo] = d[hi] = 1.0
    S, near, _ = tw.target_sdf(d)
    lin = lambda J: (J[0] * n + J[1]) * n + J[2]
    assert near[7, 8, 8] == lin(lo)
    plane = near[7]
    assert set(np.unique(plane)) <= {lin(lo), lin(hi)}
    assert np.array_equal(S, tw.brute_force_sdf(d))


def test_iou_twin_by_hand():
    """Two-valued field: k cells at m, l cells at m/2.  iou(a, a): I = sum a^2 / m^2 = k + l/4, U = 2 sum a / m = 2 (k + l/2)."""
    a = np.zeros(64)
    a[:3] = 0.8
    a[3:7] = 0.4
    I, U = 3 + 4 / 4, 2 * (3 + 4 / 2)
    assert abs(tw.iou(a, a) - I / (U - I)) < 1e-15 and abs(tw.iou(a, a) - 4.0 / 6.0) < 1e-15
    sa, sa2, ma = a.sum(), (a * a).sum(), a.max()
    assert abs(tw.iou(a, a) - 1 / (2 * (sa / ma) / (sa2 / ma ** 2) - 1)) < 1e-15
    b = np.zeros(64)
    b[2:5] = 2.0                                             # overlaps one 0.8 cell and two 0.4 cells
    Iab, Uab = (1 * 1.0 + 2 * 0.5), (3 + 2) + 3
    assert abs(tw.iou(a, b) - Iab / (Uab - Iab)) < 1e-15
    assert np.isnan(tw.iou(np.zeros(8), a[:8]))              # max = 0: what IEEE gives, no special case


@pytest.mark.parametrize("kind", ["Momentum", "Adam"])
def test_optimisers_follow_the_formulas(kind):
    import torch
    from unidom_amd.algorithms import plb_solver
    rng = np.random.default_rng(3)
    p0 = rng.uniform(-0.5, 0.5, size=(4, 2, 3))
    for lr in (0.1, 3.0):                                    # 3.0: steps large enough to hit the bounds
        mine = getattr(plb_solver, kind)(torch.tensor(p0), lr=lr)
        ref = (tw.MomentumTwin if kind == "Momentum" else tw.AdamTwin)(p0, lr=lr)
        clipped = 0
        for it in range(5):
            g = rng.normal(size=p0.shape) * (1.0 if it != 2 else 1e-3)
            got, want = mine.step(torch.tensor(g)).numpy(), ref.step(g)
            assert np.allclose(got, want, rtol=1e-12, atol=0), (kind, lr, it)
            assert got.min() >= -1.0 and got.max() <= 1.0
            clipped += int((np.abs(got) == 1.0).sum())
        assert (clipped > 0) == (lr == 3.0)
    assert mine.parameters.dtype == torch.float64


class _StubSim:
    """Just enough of PlbSimulator for PlbLoss: the 'state' is the pair (loss [B], grid mass [B,G])."""
    n_grid = 2
    batch_size = 3

    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def compute_loss(self, state, td, ts, weights, soft):
        import torch
        parts = torch.stack([state[0] * 0.5, state[0] * 0.25, state[0] * 0.25], -1)
        return state[0], parts

    def get_grid_mass(self, state):
        return state[1]


def test_plb_loss_reward_and_incremental_iou_over_a_stub(monkeypatch):
    import torch
    from unidom_amd.engine import plb_losses
    t_iou = lambda a, b: torch.tensor([tw.iou(x.numpy(), (b[i] if b.numel() == a.numel() else b).numpy()) for i, x in enumerate(a)])
    monkeypatch.setattr(plb_losses, "density_iou", lambda a, b: t_iou(a.reshape(a.shape[0], -1), b.reshape(-1) if b.numel() != a.numel() else b.reshape(a.shape[0], -1)))
    monkeypatch.setattr(plb_losses, "target_sdf", lambda d, thr=1e-4: (torch.tensor(tw.target_sdf(d.numpy(), thr)[0]), None, None))
    sim = _StubSim()
    L = plb_losses.PlbLoss(sim, weights=(2.0, 1.0, 0.5), soft_contact=False)
    assert L.weights.tolist() == [2.0, 1.0, 0.5] and L.soft_contact is False
    target = np.zeros((2, 2, 2))
    target[0, 0, 0], target[0, 0, 1] = 1.0, 0.5
    L.load_target_density(target)
    assert abs(float(L.target_iou) - tw.iou(target, target)) < 1e-15 and float(L.target_sdf[0, 0, 0]) == 0.0 and float(L.target_sdf[1, 1, 1]) > 0
    T = lambda a: torch.tensor(np.asarray(a, np.float64))
    start = np.zeros((3, 8))
    start[:, 0], start[:, 2] = 1.0, 1.0                      # overlaps the target in one cell
    L.reset((T([5.0, 6.0, 7.0]), T(start)))
    init = tw.iou(start[0], target)
    assert np.allclose(L._init_iou.numpy(), init) and L._start_loss.tolist() == [5.0, 6.0, 7.0]
    now = np.zeros((3, 8))
    now[0] = target.reshape(-1)                              # env 0 reaches the target: 1
    now[1, 3] = 1.0                                          # env 1 loses all overlap: iou 0 < init: clipped to 0
    now[2] = start[2]
    now[2, 1] = 0.5                                          # env 2 improves part of the way
    out = L.compute_loss((T([1.0, 8.0, 7.0]), T(now)))
    assert out["reward"].tolist() == [4.0, -2.0, 0.0]
    assert out["loss"].tolist() == [1.0, 8.0, 7.0] and out["contact_loss"].tolist() == [0.5, 4.0, 3.5]
    ti = tw.iou(target, target)
    want2 = (tw.iou(now[2], target) - init) / (ti - init)
    inc = out["incremental_iou"].numpy()
    assert inc[0] == 1.0 and inc[1] == 0.0 and 0 < want2 < 1 and abs(inc[2] - want2) < 1e-15
    assert out["target_iou"].shape == (3,) and np.allclose(out["iou"].numpy(), [ti, 0.0, tw.iou(now[2], target)])
    # above the target's own IoU is clipped too: a state whose IoU with the target exceeds iou(target, target) cannot exist for the
    # normalised form, so drive the formula directly
    assert plb_losses.incremental_iou_of(T([2.0, -1.0, 0.5]), T([0.0, 0.0, 0.0]), T([1.0, 1.0, 1.0])).tolist() == [1.0, 0.0, 0.5]
