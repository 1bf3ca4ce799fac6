"""CPU: the point-cloud policy's specification twin (tests/pc_twin.py) checked against facts worked out by hand, its case builders, and
the host side of unidom_amd/algorithms/plb_pc_policy.py (model shapes, the per-tensor clip, sample_pc, the command line).  Nothing here
calls a kernel."""
import numpy as np
import pytest

from tests import pc_twin as tw

F = np.float32


def test_twin_fps_takes_every_distinct_point_once_then_repeats_index_zero():
    x = tw.random_cloud(np.random.default_rng(0), 1, 200)
    assert len(np.unique(x[0], axis=0)) == 200
    idx, new_xyz = tw.fps(x, 512)
    assert idx[0, 0] == 0 and sorted(idx[0, :200].tolist()) == list(range(200))
    assert (idx[0, 200:] == 0).all()
    assert np.array_equal(new_xyz[0], x[0][idx[0]])


def test_twin_fps_breaks_the_lattice_ties_towards_the_lowest_index():
    idx, _ = tw.fps(tw.lattice(4, 1.0 / 64)[None], 8)
    assert idx[0].tolist() == [0, 63, 7, 28, 49, 14, 35, 56]


def test_twin_ball_test_is_the_sqrt_form_not_the_squared_one():
    r = F(0.02)
    s = F(0.00039999996)
    assert s < r * r and not (np.sqrt(s) < r)
    p, s_found = tw.sqrt_disagreement(0, 0.02)
    assert s_found < r * r and not tw.ball_pass(p[None], np.zeros(3, F), 0.02)[0]


def test_twin_ball_query_excludes_the_point_at_exactly_the_radius():
    xyz, centre, radius = tw.boundary_case(8)
    d = np.sqrt(tw._d2(xyz[0], centre[0, 0]))
    assert (d[:3] == F(radius)).all() and d[3] < F(radius) < d[4]       # the 3-4-5 triples are exact
    idx, cnt = tw.ball_query(radius, 4, xyz, centre)
    assert cnt[0, 0] == 1 and idx[0, 0].tolist() == [3, 3, 3, 3]


def test_twin_ball_query_fills_with_the_first_hit_and_zeroes_an_empty_row():
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [0.01, 0, 0], [0.015, 0, 0]]], F)
    centres = np.array([[[0.012, 0, 0], [5, 5, 5]]], F)
    idx, cnt = tw.ball_query(0.02, 4, xyz, centres)
    assert idx[0, 0].tolist() == [0, 2, 3, 0] and cnt[0].tolist() == [3, 0] and idx[0, 1].tolist() == [0, 0, 0, 0]
    idx, cnt = tw.ball_query(0.02, 2, xyz, centres)
    assert idx[0, 0].tolist() == [0, 2] and cnt[0].tolist() == [2, 0]


@pytest.mark.parametrize("nsample", [1, 4, 32, 65])
def test_ball_case_builder_covers_empty_partial_and_full_rows(nsample):
    xyz, new_xyz, idx, cnt = tw.ball_case(nsample, 2, 200, 40, nsample)      # the builder asserts the three kinds and the planted point
    assert idx.shape == (2, 40, nsample) and cnt.max() == nsample and cnt.min() == 0


def test_twin_group_adjoint_against_autograd_through_an_index_gather_in_f64():
    """np.add.at in f32 against torch.autograd in f64.  Bound: an output is a sequential f32 sum of T terms, so its error is at most
    (T - 1) u sum |term| with u = 2^-24 (the one rounding of -sum included in T for the centre path)."""
    import torch
    rng = np.random.default_rng(3)
    B, n, m, ns, C = 2, 37, 19, 5, 4
    xyz, feats = tw.random_cloud(rng, B, n), rng.normal(size=(B, n, C)).astype(F)
    centre_idx, new_xyz = tw.fps(xyz, m)
    idx = rng.integers(0, n, (B, m, ns)).astype(np.int32)
    g_out = rng.normal(size=(B, m, ns, 3 + C)).astype(F)
    assert np.array_equal(tw.group_fwd(xyz, feats, new_xyz, idx)[..., 3:], feats[np.arange(B)[:, None, None], idx])
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    li, lc = torch.tensor(idx.astype(np.int64)), torch.tensor(centre_idx.astype(np.int64))

    def autograd(go, with_centres):
        X, Fe = t64(xyz).requires_grad_(True), t64(feats).requires_grad_(True)
        NX = tw._gather(X, lc) if with_centres else t64(new_xyz).requires_grad_(True)
        out = torch.cat([tw._gather(X, li) - NX[:, :, None, :], tw._gather(Fe, li)], -1)
        (out * t64(go)).sum().backward()
        return X.grad.numpy(), Fe.grad.numpy(), (None if with_centres else NX.grad.numpy())

    u = 2.0 ** -24
    ax, af, an = autograd(np.abs(g_out), False)                   # sum |term| per output; an = -(sum_k |g|)
    terms = m * ns + m * (ns + 1)                                 # more additions than any one output sees
    for with_centres in (False, True):
        gx, gf, gn = tw.group_bwd(n, idx, g_out, centre_idx if with_centres else None)
        rx, rf, rn = autograd(g_out, with_centres)
        absx = ax.copy()
        if with_centres:
            for b in range(B):
                np.add.at(absx[b], centre_idx[b], -an[b])
        assert (np.abs(gf - rf) <= terms * u * af).all()
        assert (np.abs(gx - rx) <= terms * u * absx).all(), np.abs(gx - rx).max()
        if not with_centres:
            assert (np.abs(gn - rn) <= ns * u * -an).all()
    # the centre term is visible at f64 scale: dropping it is far outside the f32 bound
    mx, _, _ = tw.group_bwd(n, idx, g_out, centre_idx, drop_centre_term=True)
    rx = autograd(g_out, True)[0]
    assert np.abs(mx - rx).max() > 1e3 * np.abs(tw.group_bwd(n, idx, g_out, centre_idx)[0] - rx).max()


def test_twin_group_adjoint_adds_in_ascending_order_from_plus_zero():
    # 1 + 2^-24 + 2^-24: left to right both small terms are lost, any other order keeps them
    e = F(2.0 ** -24)
    g_out = np.array([[[[1, 0, 0]], [[e, 0, 0]], [[e, 0, 0]]]], F)          # B 1, m 3, nsample 1
    idx = np.zeros((1, 3, 1), np.int32)
    gx, _, gn = tw.group_bwd(2, idx, g_out)
    assert gx[0, 0, 0] == F(1) and gx[0, 1, 0] == 0
    assert np.signbit(gn[0, 0, 1]) and gn[0, 0, 1] == 0                      # -(+0 + 0) = -0


# ---- the host side of the policy ---------------------------------------------------------------------------------------------------
CONVS = 6 * 64 + 64 * 64 + 64 * 128 + 131 * 128 + 128 * 128 + 128 * 256 + 259 * 256 + 256 * 512 + 512 * 1024
HEAD = 1024 * 256 + 256 + 2 * 256 + 128 + 128 * 3 + 3      # dense1, batchnorm1, last_dense1's bias, last_dense2


def test_model_parameter_counts_and_shapes():
    import torch
    from unidom_amd.algorithms.plb_pc_policy import ClsSsgModel, ClsSsgModelPara
    para, plain = ClsSsgModelPara(3), ClsSsgModel(3)
    count = lambda mod: sum(p.numel() for p in mod.parameters())
    assert count(plain) == CONVS + HEAD + 256 * 128 == 1096451
    assert count(para) == CONVS + HEAD + 259 * 128 + 2 * 3 == 1096841
    assert [tuple(w.shape) for w in para.layer1.weights] == [(6, 64), (64, 64), (64, 128)]
    assert [tuple(w.shape) for w in para.layer2.weights] == [(131, 128), (128, 128), (128, 256)]
    assert [tuple(w.shape) for w in para.layer3.weights] == [(259, 256), (256, 512), (512, 1024)]
    assert para.last_dense1.weight.shape == (128, 259) and plain.last_dense1.weight.shape == (128, 256)
    assert para.parameters_process1.gamma.shape == (3,) and not hasattr(plain, "parameters_process1")
    assert all(not n.endswith("bias") for n, _ in para.layer1.named_parameters())       # the convs have no bias
    assert float(para.dense1.bias.detach().abs().max()) == 0 and float(para.batchnorm1.gamma.detach().min()) == 1
    # glorot normal: truncated at two (untruncated) stddev, variance 2 / (fan_in + fan_out)
    w = para.layer3.weights[2].detach()
    std = (2.0 / (512 + 1024)) ** 0.5
    assert float(w.abs().max()) <= 2 * std / 0.87962566103423978 and abs(float(w.std()) / std - 1) < 0.02
    # the same generator state gives the same model
    a = ClsSsgModelPara(3, generator=torch.Generator().manual_seed(5))
    b = ClsSsgModelPara(3, generator=torch.Generator().manual_seed(5))
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))


def test_model_head_is_the_reference_s_inference_form():
    import torch
    from unidom_amd.algorithms.plb_pc_policy import ClsSsgModelPara
    model = ClsSsgModelPara(3, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        model.parameters_process1.gamma.copy_(torch.tensor([1.0, 2.0, -1.0]))
        model.parameters_process1.beta.copy_(torch.tensor([0.5, 0.0, 0.25]))
    p = torch.tensor([[1.0, -2.0, 3.0]])
    s = 1.0 / (1.0 + 1e-3) ** 0.5
    g, b = model.parameters_process1.gamma.detach(), model.parameters_process1.beta.detach()
    once = p * g * s + b
    assert torch.allclose(model.parameters_process1(model.parameters_process1(p)), once * g * s + b, rtol=1e-6, atol=0)   # the same BN twice


def test_bn_is_refused_loudly():
    from unidom_amd.algorithms.plb_pc_policy import ClsSsgModel
    from unidom_amd.engine.pointnet import PointnetSA
    with pytest.raises(NotImplementedError):
        ClsSsgModel(3, bn=True)
    with pytest.raises(NotImplementedError):
        PointnetSA(4, 0.1, 2, [8], in_channels=0, bn=True)


def test_group_all_branch_concatenates_xyz_first_and_centres_on_the_origin():
    import torch
    from unidom_amd.engine.pointnet import PointnetSA
    sa = PointnetSA(None, None, None, [4], in_channels=2, group_all=True)
    xyz, feats = torch.rand(2, 5, 3), torch.rand(2, 5, 2)
    new_xyz, grouped = sa.group(xyz, feats)
    assert new_xyz.shape == (2, 1, 3) and float(new_xyz.abs().max()) == 0
    assert torch.equal(grouped, torch.cat([xyz, feats], 2)[:, None])
    _, out = sa(xyz, feats)
    assert out.shape == (2, 1, 4) and torch.equal(out, torch.matmul(grouped, sa.weights[0]).max(2).values)


def test_clip_is_per_tensor_as_keras_clipnorm():
    import torch
    from unidom_amd.algorithms.plb_pc_policy import clip_per_tensor_
    big, small = torch.tensor([3.0, 4.0]), torch.tensor([0.03, 0.04])
    out = clip_per_tensor_([big.clone(), small.clone(), None], 0.1)
    assert torch.allclose(out[0], big * (0.1 / 5.0)) and torch.equal(out[1], small)       # 5 -> 0.1; 0.05 is left alone
    # a global clip would have scaled both by 0.1 / |(3, 4, 0.03, 0.04)|
    assert not torch.allclose(out[1], small * (0.1 / float(torch.cat([big, small]).norm())))


def test_sample_pc_shapes_and_voxel_means():
    import torch
    from unidom_amd.algorithms.plb_pc_policy import sample_pc
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(1000, 3, dtype=torch.float64, generator=gen) * 0.05
    out = sample_pc(x, 200, gen)
    assert out.shape == (200, 3) and out.dtype == torch.float32
    assert sample_pc(x[None].repeat(3, 1, 1), 17, gen).shape == (3, 17, 3)
    # two points in one voxel and one in another: the draw only ever returns the mean of the pair or the single point
    pts = torch.tensor([[0.0, 0.0, 0.0], [0.001, 0.0, 0.0], [0.02, 0.0, 0.0]], dtype=torch.float64)
    got = sample_pc(pts, 64, gen).double()
    mean, single = torch.tensor([0.0005, 0.0, 0.0], dtype=torch.float64), pts[2]
    is_mean, is_single = (got - mean).abs().max(1).values < 1e-9, (got - single).abs().max(1).values < 1e-9
    assert bool((is_mean | is_single).all()) and bool(is_mean.any()) and bool(is_single.any())
    # seeded: the same generator state, the same draw
    a = sample_pc(x, 50, torch.Generator().manual_seed(3))
    assert torch.equal(a, sample_pc(x, 50, torch.Generator().manual_seed(3)))


def test_parameters_are_normalised_over_the_batch():
    import torch
    from unidom_amd.algorithms.plb_pc_policy import lame, normalise_parameters
    p = torch.tensor([[1.0, 5.0, 2.0], [3.0, 5.0, 6.0]], dtype=torch.float64)
    norm, mean, std = normalise_parameters(p)
    assert norm.tolist() == [[-1.0, 0.0, -1.0], [1.0, 0.0, 1.0]] and mean.tolist() == [2.0, 5.0, 4.0] and std.tolist() == [1.0, 1.0, 2.0]
    again, _, _ = normalise_parameters(p[:1], mean, std)
    assert again.tolist() == [[-1.0, 0.0, -1.0]]
    mu, lam = lame(5e3, 0.35)
    assert abs(mu - 5e3 / 2.7) < 1e-9 and abs(lam - 5e3 * 0.35 / (1.35 * 0.3)) < 1e-9


def test_command_line_parsing():
    from unidom_amd.algorithms.plb_pc_policy import parse_args
    a = parse_args(["--env", "torus", "--num_envs", "4", "--expert_iters", "7", "--epochs", "2", "--seed", "9"])
    assert (a.env, a.num_envs, a.expert_iters, a.epochs, a.seed) == ("torus", 4, 7, 2, 9)
    d = parse_args([])
    assert d.env == "move" and d.lr == 1e-3 and d.num_points == 200 and not d.no_parameters
    with pytest.raises(SystemExit):
        parse_args(["--env", "writer"])
