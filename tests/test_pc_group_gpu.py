"""GPU: the ud_pc_* kernels (csrc/pc_group.hip) against the NumPy specification tests/pc_twin.py, bit for bit.

Every output is integer or a single-rounded / fixed-order float32 result, so the bar is equality of the bits (compared as uint32, so
that -0 and +0 differ).  Every output buffer sits between two pads of sentinels that must stay untouched.  The sizes walk the kernel
paths: FPS n <= 64 / 128 / 256 (one wave, 1 / 2 / 4 points per lane) and n <= 1024 / 2048 / 4096 / 8192 (16 waves, 1 / 2 / 4 / 8 points
per lane); ball query n below and above one LDS chunk of 1024; the group backward's channel tiles of 64 (C = 131 -> three tiles)."""
import numpy as np
import pytest

from tests import pc_twin as tw

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 64
SENT_F, SENT_I = 12345.678, -77777


class _Guarded:
    """A device array of the given shape / dtype between two pads of sentinels."""

    def __init__(self, shape, dtype):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.sent = SENT_I if dtype == torch.int32 else SENT_F
        self.big = torch.full((self.n + 2 * PAD,), self.sent, dtype=dtype, device="cuda")
        self.ref = self.big.clone()

    @property
    def ptr(self):
        return self.big[PAD:].data_ptr()

    def intact(self):
        return bool((self.big[:PAD] == self.ref[:PAD]).all()) and bool((self.big[PAD + self.n:] == self.ref[PAD + self.n:]).all())

    def untouched(self):
        import torch
        return torch.equal(self.big, self.ref)

    def numpy(self):
        return self.big[PAD:PAD + self.n].cpu().numpy().reshape(self.shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _lib():
    import torch
    from unidom_amd import _lib
    return _lib.lib(), torch.cuda.current_stream().cuda_stream


def hip_fps(xyz, m):
    import torch
    L, st = _lib()
    B, n, _ = xyz.shape
    x = _dev(xyz)
    idx, new = _Guarded((B, m), torch.int32), _Guarded((B, m, 3), torch.float32)
    rc = L.ud_pc_fps(B, n, m, x.data_ptr(), idx.ptr, new.ptr, st)
    torch.cuda.synchronize()
    return rc, idx, new


def hip_ball(radius, nsample, xyz, new_xyz):
    import torch
    L, st = _lib()
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    x, q = _dev(xyz), _dev(new_xyz)
    idx, cnt = _Guarded((B, m, nsample), torch.int32), _Guarded((B, m), torch.int32)
    rc = L.ud_pc_ball_query(B, n, m, float(radius), nsample, x.data_ptr(), q.data_ptr(), idx.ptr, cnt.ptr, st)
    torch.cuda.synchronize()
    return rc, idx, cnt


def hip_group_fwd(xyz, feats, new_xyz, idx):
    import torch
    L, st = _lib()
    B, n, _ = xyz.shape
    m, ns = idx.shape[1:]
    Cf = 0 if feats is None else feats.shape[2]
    x, q, i = _dev(xyz), _dev(new_xyz), _dev(idx)
    f = _dev(feats) if Cf else None
    out = _Guarded((B, m, ns, 3 + Cf), torch.float32)
    rc = L.ud_pc_group_fwd(B, n, m, ns, Cf, x.data_ptr(), f.data_ptr() if Cf else None, q.data_ptr(), i.data_ptr(), out.ptr, st)
    torch.cuda.synchronize()
    return rc, out


def hip_group_bwd(n, idx, g_out, centre_idx=None):
    import torch
    L, st = _lib()
    B, m, ns, W = g_out.shape
    i, g = _dev(idx), _dev(g_out)
    c = None if centre_idx is None else _dev(centre_idx)
    gx, gf, gn = _Guarded((B, n, 3), torch.float32), _Guarded((B, n, W - 3), torch.float32), _Guarded((B, m, 3), torch.float32)
    rc = L.ud_pc_group_bwd(B, n, m, ns, W - 3, i.data_ptr(), c.data_ptr() if c is not None else None, g.data_ptr(), gx.ptr,
                           gf.ptr if W > 3 else None, gn.ptr, st)
    torch.cuda.synchronize()
    return rc, gx, gf, gn


# ---- farthest-point sampling ------------------------------------------------------------------------------------------------------
_FPS_REF = {}


def _fps_case(kind, n, B):
    key = (kind, n, B)
    if key not in _FPS_REF:
        rng = np.random.default_rng(1000 * n + 10 * B + len(kind))
        xyz = tw.random_cloud(rng, B, n) if kind == "random" else tw.duplicate_cloud(rng, B, n)
        ms = sorted({1, n, 2 * n + 3})
        idx, new = tw.fps(xyz, ms[-1])                             # a shorter run is a prefix of a longer one
        xyz.setflags(write=False)
        _FPS_REF[key] = (xyz, ms, idx, new)
    return _FPS_REF[key]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 257, 513, 1025])
@pytest.mark.parametrize("kind", ["random", "duplicates"])
def test_fps_is_bit_equal_to_the_twin(kind, n, B):
    xyz, ms, idx, new = _fps_case(kind, n, B)
    if kind == "duplicates" and n > 2:
        assert len(np.unique(xyz[0], axis=0)) < n
    for m in ms:
        rc, gi, gn = hip_fps(xyz, m)
        assert rc == 0
        assert _same(gi.numpy(), idx[:, :m]), (kind, n, B, m)
        assert _same(gn.numpy(), np.ascontiguousarray(new[:, :m])), (kind, n, B, m)
        assert gi.intact() and gn.intact()


@pytest.mark.parametrize("n,m", [(2500, 40), (4097, 24), (8192, 16)])
def test_fps_paths_with_four_and_eight_points_per_lane(n, m):
    xyz = tw.random_cloud(np.random.default_rng(n), 2, n)
    idx, new = tw.fps(xyz, m)
    rc, gi, gn = hip_fps(xyz, m)
    assert rc == 0 and _same(gi.numpy(), idx) and _same(gn.numpy(), new) and gi.intact() and gn.intact()


@pytest.mark.parametrize("side,reps", [(4, 1), (6, 1), (7, 1), (4, 20)])
def test_fps_on_the_exact_lattice_where_every_distance_ties(side, reps):
    """Coordinates i / 64: every squared distance is exact, so whole shells of points tie and only the tie rule decides.  reps > 1
    repeats the lattice (n = 1280: the 16-wave path, ties across waves)."""
    xyz = np.tile(tw.lattice(side), (reps, 1))[None]
    n = xyz.shape[1]
    m = min(n, 64) + 3
    idx, new = tw.fps(xyz, m)
    if side == 4 and reps == 1:
        assert idx[0, :8].tolist() == [0, 63, 7, 28, 49, 14, 35, 56]
    rc, gi, gn = hip_fps(xyz, m)
    assert rc == 0 and _same(gi.numpy(), idx) and _same(gn.numpy(), new) and gi.intact() and gn.intact()


def test_fps_of_200_points_takes_each_once_then_repeats_index_zero():
    xyz, _, idx, _ = _fps_case("random", 200, 1)
    rc, gi, _ = hip_fps(xyz, 512)
    got = gi.numpy()[0]
    assert rc == 0 and sorted(got[:200].tolist()) == list(range(200)) and (got[200:] == 0).all()


# ---- ball query ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [200, 1500])
@pytest.mark.parametrize("nsample", [1, 4, 32, 65])
def test_ball_query_is_bit_equal_to_the_twin(nsample, n):
    xyz, new_xyz, idx, cnt = tw.ball_case(nsample + n, 2, n, 40, nsample)      # asserts empty, partial and full rows and the sqrt point
    rc, gi, gc = hip_ball(0.02, nsample, xyz, new_xyz)
    assert rc == 0
    assert _same(gc.numpy(), cnt) and _same(gi.numpy(), idx)
    assert gi.intact() and gc.intact()


@pytest.mark.parametrize("m", [1, 3, 5])
def test_ball_query_with_fewer_centres_than_waves_in_a_workgroup(m):
    xyz, new_xyz, idx, cnt = tw.ball_case(7, 1, 130, 40, 4)
    rc, gi, gc = hip_ball(0.02, 4, xyz, new_xyz[:, :m])
    assert rc == 0 and _same(gi.numpy(), idx[:, :m]) and _same(gc.numpy(), cnt[:, :m]) and gi.intact() and gc.intact()


@pytest.mark.parametrize("k", [6, 8, 10])
def test_ball_query_excludes_a_point_at_exactly_the_radius(k):
    xyz, centre, radius = tw.boundary_case(k)
    rc, gi, gc = hip_ball(radius, 4, xyz, centre)
    assert rc == 0 and gc.numpy().tolist() == [[1]] and gi.numpy()[0, 0].tolist() == [3, 3, 3, 3]


def test_ball_query_uses_the_sqrt_form():
    p, s = tw.sqrt_disagreement(0, 0.02)
    assert s < F(0.02) * F(0.02)                                   # the squared form would take it
    xyz = np.stack([p, np.zeros(3, F) + F(0.5)])[None]
    rc, gi, gc = hip_ball(0.02, 2, xyz, np.zeros((1, 1, 3), F))
    assert rc == 0 and gc.numpy().tolist() == [[0]] and gi.numpy()[0, 0].tolist() == [0, 0]


# ---- group ----------------------------------------------------------------------------------------------------------------------------
_GROUP_REF = {}


def _group_case(Cf):
    if Cf not in _GROUP_REF:
        rng = np.random.default_rng(50 + Cf)
        B, n, m, ns = 2, 70, 13, 9
        xyz = tw.random_cloud(rng, B, n, 0.06)
        feats = rng.normal(size=(B, n, Cf)).astype(F) if Cf else None
        centre_idx, new_xyz = tw.fps(xyz, m)
        idx, _ = tw.ball_query(0.02, ns, xyz, new_xyz)            # repeated indices inside a row, points nobody selected
        assert len(np.unique(idx[0])) < n
        g_out = rng.normal(size=(B, m, ns, 3 + Cf)).astype(F)
        ref = dict(B=B, n=n, m=m, ns=ns, xyz=xyz, feats=feats, centre_idx=centre_idx, new_xyz=new_xyz, idx=idx, g_out=g_out,
                   out=tw.group_fwd(xyz, feats, new_xyz, idx), plain=tw.group_bwd(n, idx, g_out), centred=tw.group_bwd(n, idx, g_out, centre_idx))
        assert not _same(ref["plain"][0], ref["centred"][0])
        _GROUP_REF[Cf] = ref
    return _GROUP_REF[Cf]


@pytest.mark.parametrize("Cf", [0, 1, 3, 131])
def test_group_forward_is_bit_equal_to_the_twin(Cf):
    r = _group_case(Cf)
    rc, out = hip_group_fwd(r["xyz"], r["feats"], r["new_xyz"], r["idx"])
    assert rc == 0 and _same(out.numpy(), r["out"]) and out.intact()


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("Cf", [0, 1, 3, 131])
def test_group_backward_is_bit_equal_to_the_twin_and_to_itself(Cf, centred):
    r = _group_case(Cf)
    want = r["centred" if centred else "plain"]
    c = r["centre_idx"] if centred else None
    rc, gx, gf, gn = hip_group_bwd(r["n"], r["idx"], r["g_out"], c)
    assert rc == 0
    assert _same(gx.numpy(), want[0]) and _same(gn.numpy(), want[2])
    assert gx.intact() and gn.intact() and gf.intact()
    if Cf:
        assert _same(gf.numpy(), want[1])
    else:
        assert gf.untouched()
    rc2, gx2, gf2, gn2 = hip_group_bwd(r["n"], r["idx"], r["g_out"], c)       # no float atomics: the same bits again
    assert rc2 == 0 and _same(gx2.numpy(), gx.numpy()) and _same(gf2.numpy(), gf.numpy()) and _same(gn2.numpy(), gn.numpy())


def test_group_backward_scans_more_entries_than_one_step_of_256():
    """m nsample = 1000 entries (not a multiple of 256), indices drawn freely: many (j, k) per point, in every position of the scan."""
    rng = np.random.default_rng(9)
    B, n, m, ns, Cf = 1, 11, 125, 8, 2
    idx = rng.integers(0, n, (B, m, ns)).astype(np.int32)
    centre_idx = rng.integers(0, n, (B, m)).astype(np.int32)
    g_out = rng.normal(size=(B, m, ns, 3 + Cf)).astype(F)
    want = tw.group_bwd(n, idx, g_out, centre_idx)
    rc, gx, gf, gn = hip_group_bwd(n, idx, g_out, centre_idx)
    assert rc == 0 and _same(gx.numpy(), want[0]) and _same(gf.numpy(), want[1]) and _same(gn.numpy(), want[2])


# ---- all entry points ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_is_written():
    import torch
    from unidom_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    last = lambda: L.ud_last_error().decode()
    x, q = torch.zeros((2, 8, 3), device="cuda"), torch.zeros((2, 4, 3), device="cuda")
    f, i4 = torch.zeros((2, 8, 2), device="cuda"), torch.zeros((2, 4, 3), dtype=torch.int32, device="cuda")
    g = torch.zeros((2, 4, 3, 5), device="cuda")
    oi, of = _Guarded((4096,), torch.int32), _Guarded((4096,), torch.float32)
    oi2, of2, of3 = _Guarded((4096,), torch.int32), _Guarded((4096,), torch.float32), _Guarded((4096,), torch.float32)
    X, Q, Fp, I, G = x.data_ptr(), q.data_ptr(), f.data_ptr(), i4.data_ptr(), g.data_ptr()
    INVALID, UNSUPPORTED = -1, -2
    calls = [
        ("ud_pc_fps", INVALID, lambda: L.ud_pc_fps(0, 8, 4, X, oi.ptr, of.ptr, st)),
        ("ud_pc_fps", INVALID, lambda: L.ud_pc_fps(2, 0, 4, X, oi.ptr, of.ptr, st)),
        ("ud_pc_fps", INVALID, lambda: L.ud_pc_fps(2, 8, 0, X, oi.ptr, of.ptr, st)),
        ("ud_pc_fps", INVALID, lambda: L.ud_pc_fps(2, 8, 4, None, oi.ptr, of.ptr, st)),
        ("ud_pc_fps", INVALID, lambda: L.ud_pc_fps(2, 8, 4, X, None, of.ptr, st)),
        ("ud_pc_fps", UNSUPPORTED, lambda: L.ud_pc_fps(2, 8193, 4, X, oi.ptr, of.ptr, st)),
        ("ud_pc_fps", UNSUPPORTED, lambda: L.ud_pc_fps(65536, 8, 4, X, oi.ptr, of.ptr, st)),
        ("ud_pc_ball_query", INVALID, lambda: L.ud_pc_ball_query(2, 8, 4, 0.02, 0, X, Q, oi.ptr, oi2.ptr, st)),
        ("ud_pc_ball_query", INVALID, lambda: L.ud_pc_ball_query(2, 8, 0, 0.02, 3, X, Q, oi.ptr, oi2.ptr, st)),
        ("ud_pc_ball_query", INVALID, lambda: L.ud_pc_ball_query(2, 8, 4, 0.02, 3, X, None, oi.ptr, oi2.ptr, st)),
        ("ud_pc_ball_query", INVALID, lambda: L.ud_pc_ball_query(2, 8, 4, 0.02, 3, X, Q, oi.ptr, None, st)),
        ("ud_pc_ball_query", UNSUPPORTED, lambda: L.ud_pc_ball_query(65536, 8, 4, 0.02, 3, X, Q, oi.ptr, oi2.ptr, st)),
        ("ud_pc_group_fwd", INVALID, lambda: L.ud_pc_group_fwd(2, 8, 4, 3, -1, X, Fp, Q, I, of.ptr, st)),
        ("ud_pc_group_fwd", INVALID, lambda: L.ud_pc_group_fwd(2, 8, 4, 3, 2, X, None, Q, I, of.ptr, st)),
        ("ud_pc_group_fwd", INVALID, lambda: L.ud_pc_group_fwd(2, 8, 4, 0, 2, X, Fp, Q, I, of.ptr, st)),
        ("ud_pc_group_fwd", INVALID, lambda: L.ud_pc_group_fwd(2, 8, 4, 3, 2, X, Fp, Q, None, of.ptr, st)),
        ("ud_pc_group_fwd", UNSUPPORTED, lambda: L.ud_pc_group_fwd(2, 8, 1 << 20, 1 << 10, 2, X, Fp, Q, I, of.ptr, st)),
        ("ud_pc_group_bwd", INVALID, lambda: L.ud_pc_group_bwd(2, 8, 4, 3, 2, None, None, G, of.ptr, of2.ptr, of3.ptr, st)),
        ("ud_pc_group_bwd", INVALID, lambda: L.ud_pc_group_bwd(2, 8, 4, 3, 2, I, None, G, of.ptr, None, of3.ptr, st)),
        ("ud_pc_group_bwd", INVALID, lambda: L.ud_pc_group_bwd(2, 8, 4, 3, 2, I, None, G, of.ptr, of2.ptr, None, st)),
        ("ud_pc_group_bwd", INVALID, lambda: L.ud_pc_group_bwd(2, 0, 4, 3, 2, I, None, G, of.ptr, of2.ptr, of3.ptr, st)),
        ("ud_pc_group_bwd", UNSUPPORTED, lambda: L.ud_pc_group_bwd(2, 8, 1 << 20, 1 << 10, 2, I, None, G, of.ptr, of2.ptr, of3.ptr, st)),
    ]
    for name, code, call in calls:
        assert call() == code, name
        assert name in last(), (name, last())
    torch.cuda.synchronize()
    assert all(buf.untouched() for buf in (oi, of, oi2, of2, of3))


def test_one_graph_capture_of_fps_ball_group_replays_the_eager_bits():
    import torch
    from unidom_amd.engine.pointnet import farthest_point_sample, group_points, query_ball_point
    rng = np.random.default_rng(4)
    xyz = torch.tensor(tw.random_cloud(rng, 2, 200, 0.08), device="cuda")
    feats = torch.tensor(rng.normal(size=(2, 200, 3)).astype(F), device="cuda")

    def chain():
        centre_idx, new_xyz = farthest_point_sample(xyz, 64)
        idx, cnt = query_ball_point(0.02, 16, xyz, new_xyz)
        return centre_idx, new_xyz, idx, cnt, group_points(xyz, feats, new_xyz, idx, centre_idx)

    with torch.no_grad():
        eager = [t.clone() for t in chain()]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            chain()                                                # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = chain()
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    for got, want in zip(captured, eager):
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, want.view(torch.int32) if want.dtype == torch.float32 else want)
    # and the eager chain is the twin's
    ci, nx = tw.fps(xyz.cpu().numpy(), 64)
    bi, _ = tw.ball_query(0.02, 16, xyz.cpu().numpy(), nx)
    assert _same(eager[0].cpu().numpy(), ci) and _same(eager[2].cpu().numpy(), bi)
    assert _same(eager[4].cpu().numpy(), tw.group_fwd(xyz.cpu().numpy(), feats.cpu().numpy(), nx, bi))


def test_group_points_autograd_returns_the_kernel_s_adjoint():
    import torch
    from unidom_amd.engine.pointnet import group_points
    r = _group_case(3)
    X = torch.tensor(r["xyz"], device="cuda", requires_grad=True)
    Fe = torch.tensor(r["feats"], device="cuda", requires_grad=True)
    NX = torch.tensor(r["new_xyz"], device="cuda", requires_grad=True)
    idx, cidx, go = _dev(r["idx"]), _dev(r["centre_idx"]), _dev(r["g_out"])
    group_points(X, Fe, NX, idx).backward(go)
    assert _same(X.grad.cpu().numpy(), r["plain"][0]) and _same(Fe.grad.cpu().numpy(), r["plain"][1]) and _same(NX.grad.cpu().numpy(), r["plain"][2])
    X.grad = Fe.grad = NX.grad = None
    group_points(X, Fe, NX, idx, cidx).backward(go)
    assert _same(X.grad.cpu().numpy(), r["centred"][0]) and NX.grad is None
    with pytest.raises(TypeError):
        group_points(X, Fe, NX, idx.long())
