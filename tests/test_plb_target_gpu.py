"""GPU: ud_plb_target_sdf (csrc/plb_target.hip) against the NumPy twin tests/plb_target_twin.py.  sdf and nearest must be EXACTLY the
twin's in every case: the device takes the same f64 differences, the same left-to-right sum and a correctly rounded square root, and
the strict < in offset order decides every tie.  sweeps_run follows the convention of include/unidom_hip.h, which the twin reports too:
min(sweeps, 1-based number of the first sweep that changed nothing).

The map starts from S_c = 1000 everywhere: the first sweep marks the occupied cells only, the asymmetric window (I - J in -2..3) shows
after the second (tests/test_plb_target_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import plb_target_twin as tw

pytestmark = pytest.mark.gpu


def _dev(density, sweeps=0, threshold=1e-4):
    """density [n,n,n] or [T,n,n,n] (numpy) -> (sdf, nearest, sweeps_run) as numpy arrays."""
    import torch
    from unidom_amd.engine.plb_losses import target_sdf
    d = torch.tensor(np.asarray(density, np.float64), device="cuda")
    sdf, near, run = target_sdf(d, threshold, sweeps, want_nearest=True)
    torch.cuda.synchronize()
    return sdf.cpu().numpy(), near.cpu().numpy(), run.cpu().numpy()


def _same(dev, twin):
    assert np.array_equal(dev[0], twin[0]), ("sdf", int((dev[0] != twin[0]).sum()), float(np.abs(dev[0] - twin[0]).max()))
    assert np.array_equal(dev[1], twin[1]), ("nearest", int((dev[1] != twin[1]).sum()))
    assert int(dev[2].reshape(-1)[0]) == twin[2], ("sweeps_run", dev[2], twin[2])


@pytest.mark.parametrize("sweeps", [1, 2, 0])
def test_n_grid_8_every_face_is_a_boundary(sweeps):
    """Smaller than tile + halo in every direction.  Occupied: one cell near three faces, one in the far corner, so that after two
    sweeps the finite region is the union of two windows that reach 3 cells up and 2 down, both clipped by faces."""
    n = 8
    d = np.zeros((n, n, n))
    d[1, 4, 6] = 1.0
    d[7, 7, 0] = 3e-4
    twin = tw.target_sdf(d, sweeps=sweeps)
    if sweeps == 2:
        I = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1)
        win = np.zeros((n, n, n), bool)
        for J in ((1, 4, 6), (7, 7, 0)):
            rel = I - np.array(J)
            win |= ((rel >= -2) & (rel <= 3)).all(-1)
        assert np.array_equal(twin[0] < 1000, win)
    _same(_dev(d, sweeps), twin)


def test_n_grid_12_not_a_power_of_two_not_a_tile_multiple_two_blobs():
    """h = 1/12 is not a binary fraction: fl(i h) - fl(j h) differs from fl((i - j) h), so the distance depends on the pair, not on the
    offset alone.  12 = 3 tiles of 4 in x, 1.5 tiles of 8 in y and z."""
    n = 12
    d = np.zeros((n, n, n))
    d[1:4, 2:4, 0:3] = 0.01
    d[8:11, 9:12, 7:9] = 0.02
    d[9, 10, 8] = 0.0                                         # a hole inside the second blob
    assert len({i / 12 - j / 12 == (i - j) / 12 for i in range(12) for j in range(12)}) == 2
    twin = tw.target_sdf(d)
    assert np.array_equal(twin[0], tw.brute_force_sdf(d))
    _same(_dev(d), twin)


def test_n_grid_16_mirror_pair_ties_are_decided_by_offset_order():
    n = 16
    d = np.zeros((n, n, n))
    lo, hi = (5, 8, 8), (9, 8, 8)
    d[lo] = d[hi] = 1.0
    twin = tw.target_sdf(d)
    plane = twin[1][7]
    assert set(np.unique(plane)) <= {(5 * n + 8) * n + 8, (9 * n + 8) * n + 8} and plane[8, 8] == (5 * n + 8) * n + 8
    _same(_dev(d), twin)
    for k in (3, 4):                                          # mid-way, where the plane has only heard of some of it
        _same(_dev(d, k), tw.target_sdf(d, sweeps=k))


def test_three_targets_in_one_call_each_equals_the_twin_alone():
    """n_grid 24, T = 3: a corner cell (slowest to converge), an empty target (one sweep), a central blob.  sweeps_run differs per target:
    batch strides and the per-target early return."""
    n = 24
    d = np.zeros((3, n, n, n))
    d[0, 0, 0, 0] = 1.0
    d[2, 9:14, 10:13, 11:15] = 0.3
    twins = [tw.target_sdf(d[t], stop_at_fixed_point=True) for t in range(3)]
    assert twins[1][2] == 1 and len({t[2] for t in twins}) == 3 and (twins[1][0] == 1000).all() and (twins[1][1] == -1).all()
    sdf, near, run = _dev(d)
    for t in range(3):
        _same((sdf[t], near[t], run[t:t + 1]), twins[t])


def test_sweeps_0_is_the_literal_loop_and_k_sweeps_stop_after_k():
    n = 16
    d = np.zeros((n, n, n))
    d[:3, :2, :3] = 0.5
    d[n - 2, n - 1, n - 3] = 2e-4
    literal = tw.target_sdf(d)                                # all 32 sweeps, nothing skipped
    fixed = literal[2]
    assert 3 < fixed < 2 * n
    _same(_dev(d, 0), literal)
    _same(_dev(d, 2 * n), literal)
    for k in (fixed - 3, fixed - 1, fixed):                   # k <= fixed: every one of the k sweeps runs
        part = tw.target_sdf(d, sweeps=k)
        assert part[2] == k
        if k < fixed - 1:
            assert not (np.array_equal(part[0], literal[0]) and np.array_equal(part[1], literal[1]))
        _same(_dev(d, k), part)


def test_full_target_and_cell_at_the_threshold():
    n = 8
    _same(_dev(np.ones((n, n, n))), tw.target_sdf(np.ones((n, n, n))))
    d = np.zeros((n, n, n))
    d[1, 1, 1] = 1e-4
    d[5, 5, 5] = np.nextafter(1e-4, 1.0)
    dev = _dev(d)
    _same(dev, tw.target_sdf(d))
    assert dev[0][1, 1, 1] > 0 and dev[0][5, 5, 5] == 0


def test_captured_in_a_graph_and_replayed_twice():
    import torch
    from unidom_amd.engine.plb_losses import target_sdf
    n = 12
    d_np = np.zeros((2, n, n, n))
    d_np[0, 2, 3, 4] = 1.0
    d_np[1, 8:10, 1:3, 5:9] = 1.0
    twins = [tw.target_sdf(d_np[t]) for t in range(2)]
    d = torch.tensor(d_np, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        target_sdf(d, want_nearest=True)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sdf, near, run = target_sdf(d, want_nearest=True)
    outs = []
    for _ in range(2):
        sdf.fill_(-7.0); near.fill_(-7); run.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        outs.append((sdf.cpu().numpy().copy(), near.cpu().numpy().copy(), run.cpu().numpy().copy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    for t in range(2):
        _same((outs[0][0][t], outs[0][1][t], outs[0][2][t:t + 1]), twins[t])
    # a new density in the same buffer: the replay computes from what is there now
    d.copy_(torch.tensor(d_np[::-1].copy(), device="cuda"))
    g.replay()
    torch.cuda.synchronize()
    _same((sdf[0].cpu().numpy(), near[0].cpu().numpy(), run[:1].cpu().numpy()), twins[1])


def test_bad_arguments():
    import torch
    from unidom_amd import _lib
    L = _lib.lib()
    n = 8
    d = torch.zeros((n, n, n), dtype=torch.float64, device="cuda")
    sdf = torch.empty_like(d)
    assert L.ud_plb_target_work_bytes(n, 1) == 256 + 2 * 4 * n ** 3 and L.ud_plb_target_work_bytes(0, 1) == 0 and L.ud_plb_target_work_bytes(2048, 1) == 0
    work = torch.empty((L.ud_plb_target_work_bytes(n, 1) // 4,), dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    call = lambda n_, T_, d_, s_, sdf_, w_: L.ud_plb_target_sdf(n_, T_, P(d_), 1e-4, s_, P(sdf_), P(None), P(None), P(w_), C.c_void_p(0))
    INVALID, UNSUPPORTED = -1, -2
    for args in ((0, 1, d, 0, sdf, work), (n, 0, d, 0, sdf, work), (n, 1, None, 0, sdf, work), (n, 1, d, 0, None, work), (n, 1, d, 0, sdf, None),
                 (n, 1, d, -1, sdf, work)):
        assert call(*args) == INVALID, args[:2]
        assert b"ud_plb_target_sdf" in L.ud_last_error()
    assert call(1025, 1, d, 0, sdf, work) == UNSUPPORTED and b"1024" in L.ud_last_error()
    assert call(n, 1, d, 0, sdf, work) == 0                   # and the good call, with nearest and sweeps_run left out
    torch.cuda.synchronize()
    assert (sdf == 1000).all()
    iw = torch.empty((L.ud_plb_density_iou_work_bytes(1) // 8,), dtype=torch.float64, device="cuda")
    out = torch.empty((1,), dtype=torch.float64, device="cuda")
    for G_, T_, a_, b_, o_, w_ in ((0, 1, d, d, out, iw), (n ** 3, 0, d, d, out, iw), (n ** 3, 1, None, d, out, iw), (n ** 3, 1, d, None, out, iw),
                                   (n ** 3, 1, d, d, None, iw), (n ** 3, 1, d, d, out, None)):
        assert L.ud_plb_density_iou(G_, T_, P(a_), P(b_), 0, P(o_), P(w_), C.c_void_p(0)) == INVALID
    assert L.ud_plb_grid_mass(C.c_void_p(0), 1, P(d), P(sdf), C.c_void_p(0)) == INVALID
