"""PointNet++ sampling / grouping ops and the set-abstraction layer of the point-cloud policy: the reference's pnet2_layers (layers.py
`Pointnet_SA`, utils.py `sample_and_group` / `sample_and_group_all` / `Conv2d`) over the ud_pc_* kernels of libunidom_hip.so
(csrc/pc_group.hip), which stand in for its CUDA-behind-TensorFlow tf_ops.

float32, batched [B, n, 3] device tensors; indices are int32.  The sampling and grouping run in the library and nowhere else (no torch
restatement on the product path); the 1x1-conv stack, the activation and the max over the sample axis stay in torch.
"""
from __future__ import annotations

import math

import torch

from .. import _lib


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def farthest_point_sample(xyz, npoint):
    """(idx [B,npoint] int32, new_xyz [B,npoint,3]): farthest_point_sample + gather_point (ud_pc_fps).  idx[:,0] = 0; a tie goes to the
    lowest index; npoint > n is legal (index 0 repeats once every point is taken).  No gradient: `group_points` routes new_xyz's
    cotangent back into xyz through `centre_idx`."""
    xyz = _f32(xyz)
    B, n, _ = xyz.shape
    idx = torch.empty((B, int(npoint)), dtype=torch.int32, device=xyz.device)
    new_xyz = torch.empty((B, int(npoint), 3), dtype=torch.float32, device=xyz.device)
    _lib.check(_lib.lib().ud_pc_fps(B, n, int(npoint), _lib.ptr(xyz), _lib.ptr(idx), _lib.ptr(new_xyz), _lib.stream(xyz.device)), "ud_pc_fps")
    return idx, new_xyz


def query_ball_point(radius, nsample, xyz, new_xyz):
    """(idx [B,m,nsample] int32, cnt [B,m] int32): per centre the first nsample points (ascending index) closer than radius, the rest of
    the row repeating the first hit; a centre without a hit gets zeros and cnt 0 (ud_pc_ball_query)."""
    xyz, new_xyz = _f32(xyz), _f32(new_xyz)
    B, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.empty((B, m, int(nsample)), dtype=torch.int32, device=xyz.device)
    cnt = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
    _lib.check(_lib.lib().ud_pc_ball_query(B, n, m, float(radius), int(nsample), *[_lib.ptr(t) for t in (xyz, new_xyz, idx, cnt)], _lib.stream(xyz.device)),
               "ud_pc_ball_query")
    return idx, cnt


class _GroupPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, feats, new_xyz, idx, centre_idx):
        B, n, _ = xyz.shape
        m, nsample = idx.shape[1], idx.shape[2]
        Cf = 0 if feats is None else feats.shape[2]
        x, nx = _f32(xyz), _f32(new_xyz)
        f = None if feats is None else _f32(feats)
        idx = idx.contiguous()
        out = torch.empty((B, m, nsample, 3 + Cf), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().ud_pc_group_fwd(B, n, m, nsample, Cf, *[_lib.ptr(t) for t in (x, f, nx, idx, out)], _lib.stream(x.device)), "ud_pc_group_fwd")
        ctx.shape = (B, n, m, nsample, Cf)
        ctx.save_for_backward(idx, None if centre_idx is None else centre_idx.contiguous())
        return out

    @staticmethod
    def backward(ctx, g_out):
        B, n, m, nsample, Cf = ctx.shape
        idx, centre_idx = ctx.saved_tensors
        g = _f32(g_out)
        mk = lambda *s: torch.empty(s, dtype=torch.float32, device=g.device)
        g_xyz, g_new = mk(B, n, 3), mk(B, m, 3)
        g_feats = mk(B, n, Cf) if Cf else None
        _lib.check(_lib.lib().ud_pc_group_bwd(B, n, m, nsample, Cf, *[_lib.ptr(t) for t in (idx, centre_idx, g, g_xyz, g_feats, g_new)], _lib.stream(g.device)),
                   "ud_pc_group_bwd")
        # with centre_idx the centres' cotangent is already inside g_xyz: new_xyz was a function of xyz, not an input of its own
        return g_xyz, g_feats, (None if centre_idx is not None else g_new), None, None


def group_points(xyz, feats, new_xyz, idx, centre_idx=None):
    """sample_and_group's group, recentre and concat in one kernel: out [B,m,nsample,3+C] = (xyz[idx] - new_xyz[:, :, None], feats[idx]),
    xyz first (utils.py:26-31); feats may be None (C = 0).  Differentiable in xyz, feats and new_xyz (ud_pc_group_fwd / _bwd, no atomics:
    the same bits every time).  centre_idx [B,m]: new_xyz = xyz[centre_idx] (the FPS indices); its cotangent is then added into xyz's and
    new_xyz itself gets none."""
    if idx.dtype != torch.int32 or (centre_idx is not None and centre_idx.dtype != torch.int32):
        raise TypeError("group_points takes int32 indices (farthest_point_sample / query_ball_point return them)")
    return _GroupPoints.apply(xyz, feats, new_xyz, idx, centre_idx)


def glorot_normal_(w, fan_in, fan_out, generator=None):
    """Keras 'glorot_normal': a normal of stddev sqrt(2 / (fan_in + fan_out)) truncated at two stddev, rescaled to that variance."""
    std = math.sqrt(2.0 / (fan_in + fan_out)) / 0.87962566103423978
    return torch.nn.init.trunc_normal_(w, mean=0.0, std=std, a=-2 * std, b=2 * std, generator=generator)


class PointnetSA(torch.nn.Module):
    """layers.py `Pointnet_SA` (knn is forced off there, use_xyz on): sample npoint centres, group nsample neighbours within radius
    around each (or, with group_all, one group holding the whole cloud around the origin), run the bias-free 1x1 convs `mlp` with the
    optional activation, take the max over the sample axis.  forward(xyz [B,n,3], feats [B,n,C] or None) -> (new_xyz [B,m,3],
    new_feats [B,m,mlp[-1]]) with m = 1 for group_all.  in_channels = C.  bn=True (BatchNormalization inside Conv2d) is not built."""

    def __init__(self, npoint, radius, nsample, mlp, in_channels, group_all=False, activation=None, bn=False, generator=None):
        super().__init__()
        if bn:
            raise NotImplementedError("PointnetSA(bn=True): the reference's models are all built with bn=False; only that is implemented")
        self.npoint, self.radius, self.nsample, self.group_all, self.activation = npoint, radius, nsample, bool(group_all), activation
        dims = [3 + int(in_channels)] + [int(f) for f in mlp]
        self.weights = torch.nn.ParameterList()
        for i in range(len(mlp)):       # tf.nn.conv2d filter [1, 1, in, out]: fan_in = in, fan_out = out
            self.weights.append(torch.nn.Parameter(glorot_normal_(torch.empty(dims[i], dims[i + 1]), dims[i], dims[i + 1], generator)))

    def group(self, xyz, feats):
        if self.group_all:                                        # sample_and_group_all: new_xyz = 0, no recentring, xyz first
            new_xyz = torch.zeros((xyz.shape[0], 1, 3), dtype=xyz.dtype, device=xyz.device)
            grouped = xyz if feats is None else torch.cat([xyz, feats], dim=2)
            return new_xyz, grouped[:, None]
        centre_idx, new_xyz = farthest_point_sample(xyz, self.npoint)
        idx, _ = query_ball_point(self.radius, self.nsample, xyz, new_xyz)
        return new_xyz, group_points(xyz, feats, new_xyz, idx, centre_idx)

    def forward(self, xyz, feats):
        new_xyz, h = self.group(xyz, feats)
        for w in self.weights:
            h = torch.matmul(h, w)
            if self.activation is not None:
                h = self.activation(h)
        return new_xyz, h.max(dim=2).values
