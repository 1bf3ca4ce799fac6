"""The specification of the ud_pc_* calls (include/unidom_hip.h, "Point-cloud policy") as plain NumPy float32, written from the contract
and from nothing else: every product and sum below is a separate float32 operation (NumPy never fuses), np.argmax returns the lowest
index among the maxima, np.sqrt is correctly rounded, np.add.at adds one element after the other in the order given.

Also the builders of the test clouds and the torch restatement of the model (indices from here, arithmetic in torch) that
tests/test_pc_policy_gpu.py holds the product against."""
import math

import numpy as np

F = np.float32


def _d2(p, q):
    """(dx dx + dy dy) + dz dz, float32, unfused; p [..,3], q [3]."""
    d = (p - q).astype(F)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F) + d[..., 2] * d[..., 2]).astype(F)


def fps(xyz, m):
    """xyz [B,n,3] f32 -> (idx [B,m] int32, new_xyz [B,m,3])."""
    xyz = np.asarray(xyz, F)
    B, n, _ = xyz.shape
    idx = np.zeros((B, m), np.int32)
    for b in range(B):
        mind = np.full(n, F(1e38), F)
        cur = 0
        for j in range(1, m):
            mind = np.minimum(mind, _d2(xyz[b], xyz[b, cur]))
            cur = int(np.argmax(mind))
            idx[b, j] = cur
    return idx, np.take_along_axis(xyz, idx[:, :, None].astype(np.int64), 1)


def ball_pass(xyz_b, centre, radius):
    return np.maximum(np.sqrt(_d2(xyz_b, centre)), F(1e-20)) < F(radius)


def ball_query(radius, nsample, xyz, new_xyz):
    """-> (idx [B,m,nsample] int32, cnt [B,m] int32)."""
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    B, m = new_xyz.shape[:2]
    idx, cnt = np.zeros((B, m, nsample), np.int32), np.zeros((B, m), np.int32)
    for b in range(B):
        for j in range(m):
            hits = np.nonzero(ball_pass(xyz[b], new_xyz[b, j], radius))[0][:nsample]
            cnt[b, j] = len(hits)
            if len(hits):
                idx[b, j] = hits[0]
                idx[b, j, :len(hits)] = hits
    return idx, cnt


def group_fwd(xyz, feats, new_xyz, idx):
    """-> out [B,m,nsample,3+C]; feats None = C 0."""
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    B = xyz.shape[0]
    rows = np.arange(B)[:, None, None]
    out = (xyz[rows, idx] - new_xyz[:, :, None, :]).astype(F)
    if feats is not None and feats.shape[2]:
        out = np.concatenate([out, np.asarray(feats, F)[rows, idx]], -1)
    return out


def group_bwd(n, idx, g_out, centre_idx=None, drop_centre_term=False):
    """-> (g_xyz [B,n,3], g_feats [B,n,C], g_new_xyz [B,m,3]).  drop_centre_term: the mutation the gradient test must catch."""
    g_out = np.asarray(g_out, F)
    B, m, nsample, W = g_out.shape
    g_xyz, g_feats, g_new = np.zeros((B, n, 3), F), np.zeros((B, n, W - 3), F), np.zeros((B, m, 3), F)
    for b in range(B):
        s = np.zeros((m, 3), F)
        for k in range(nsample):
            s = (s + g_out[b, :, k, :3]).astype(F)
        g_new[b] = -s
        flat = idx[b].reshape(-1)
        np.add.at(g_xyz[b], flat, g_out[b].reshape(-1, W)[:, :3])
        np.add.at(g_feats[b], flat, g_out[b].reshape(-1, W)[:, 3:])
        if centre_idx is not None and not drop_centre_term:
            np.add.at(g_xyz[b], centre_idx[b], g_new[b])
    return g_xyz, g_feats, g_new


# ---- clouds ---------------------------------------------------------------------------------------------------------------------
def lattice(side=4, scale=1.0 / 64):
    """side^3 points (i, j, k) * scale, index (i side + j) side + k: every coordinate and squared distance is exact in f32."""
    g = np.arange(side, dtype=F)
    return (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * F(scale)).astype(F)


def random_cloud(rng, B, n, extent=0.1):
    return (rng.random((B, n, 3)) * extent).astype(F)


def duplicate_cloud(rng, B, n, extent=0.1):
    """n points drawn with replacement from n // 2 + 1 distinct ones: exact duplicates."""
    base = random_cloud(rng, B, n // 2 + 1, extent)
    pick = rng.integers(0, base.shape[1], (B, n))
    return np.take_along_axis(base, pick[:, :, None], 1)


def sqrt_disagreement(seed=0, radius=0.02, tries=200000):
    """A point p with s = |p|^2 (f32, unfused) such that s < r r holds and sqrtf(s) < r does not: seeded search among points at
    distance ~r from the origin.  Returns (p [3] f32, s)."""
    rng = np.random.default_rng(seed)
    r = F(radius)
    v = rng.normal(size=(tries, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (float(r) * (1 + rng.uniform(-3e-7, 3e-7, (tries, 1))))
    p = v.astype(F)
    s = _d2(p, np.zeros(3, F))
    bad = (s < r * r) & ~(np.sqrt(s) < r)
    assert bad.any(), "no point found where s < r*r and sqrtf(s) < r disagree"
    i = int(np.nonzero(bad)[0][0])
    return p[i], s[i]


def ball_case(seed, B, n, m, nsample, radius=0.02):
    """(xyz [B,n,3], new_xyz [B,m,3], idx, cnt): a random cloud dense enough that a ball inside it holds about 1.5 nsample points, centres
    drawn from it, the first m // 8 of them moved far away (empty balls), and next to one centre (put at the origin) the point of
    `sqrt_disagreement`.  Asserts that rows with cnt = 0, 0 < cnt < nsample (nsample > 1) and cnt = nsample all occur and that the
    planted point is the one the two forms of the test disagree on."""
    rng = np.random.default_rng(seed)
    extent = radius * (n * 4 * np.pi / (3 * 1.5 * nsample)) ** (1.0 / 3)     # an inner ball holds ~1.5 nsample points, one at a face fewer
    xyz = random_cloud(rng, B, n, extent)
    pick = rng.integers(0, n, (B, m))
    new_xyz = np.take_along_axis(xyz, pick[:, :, None], 1).copy()
    far = max(1, m // 8)
    new_xyz[:, :far] += F(10.0)
    p, s = sqrt_disagreement(0, radius)
    new_xyz[0, far] = 0
    xyz[0, n // 2] = p
    assert s < F(radius) * F(radius) and not ball_pass(xyz[0, n // 2][None], new_xyz[0, far], radius)[0]
    idx, cnt = ball_query(radius, nsample, xyz, new_xyz)
    hist = np.bincount(cnt.reshape(-1), minlength=nsample + 1)
    assert hist[0] > 0 and hist[nsample] > 0 and (nsample == 1 or hist[1:nsample].sum() > 0), (nsample, hist)
    return xyz, new_xyz, idx, cnt


def boundary_case(k=8):
    """One centre at the origin and the points (3,4,0), (0,3,4), (4,0,3) * 2^-k at exactly d = 5 * 2^-k (every step exact in f32), one
    point just inside and one just outside: (xyz [1,5,3], new_xyz [1,1,3], radius)."""
    u = F(2.0 ** -k)
    pts = np.array([[3, 4, 0], [0, 3, 4], [4, 0, 3]], F) * u
    radius = F(5) * u
    inside = np.array([np.nextafter(F(5) * u, F(0)), 0, 0], F)
    outside = np.array([0, np.nextafter(F(5) * u, F(1)), 0], F)
    xyz = np.concatenate([pts, inside[None], outside[None]])[None]
    return xyz.astype(F), np.zeros((1, 1, 3), F), float(radius)


# ---- the model, restated: indices from the twin, arithmetic in torch -------------------------------------------------------------
def model_indices(point_np):
    """The sampling / grouping indices of ClsSsgModel's layer1 and layer2 for point [B,n,3] (f32 NumPy), all from the twin."""
    c1, x1 = fps(point_np, 512)
    i1, _ = ball_query(0.02, 32, point_np, x1)
    c2, x2 = fps(x1, 128)
    i2, _ = ball_query(0.02, 64, x1, x2)
    return dict(c1=c1, i1=i1, c2=c2, i2=i2)


def _gather(t, idx):
    """t [B,n,C], idx [B,...] (int64 tensor) -> t[b, idx[b,...]]."""
    import torch
    B = t.shape[0]
    rows = torch.arange(B, device=t.device).reshape((B,) + (1,) * (idx.dim() - 1))
    return t[rows, idx]


def restated_model(weights, ind, point, vector, parameters, activation=None, record=None):
    """ClsSsgModel(Para) forward as torch ops on whatever device / dtype `point` has.  weights: the model's state_dict (converted by the
    caller); ind: model_indices() as int64 tensors on that device; parameters None = ClsSsgModel.  The grouping is an index gather, so
    torch.autograd differentiates it (xyz's gradient includes the path through the sampled centres).  record: a list that
    receives the three tensors the maxima over the sample axis are taken of."""
    import torch
    act = (lambda t: t) if activation is None else activation

    def sa(xyz, feats, c, i, ws):
        new_xyz = _gather(xyz, c)
        h = torch.cat([_gather(xyz, i) - new_xyz[:, :, None, :], _gather(feats, i)], -1)
        for w in ws:
            h = act(torch.matmul(h, w))
        if record is not None:
            record.append(h.detach())
        return new_xyz, h.max(dim=2).values

    W = lambda name: [weights[f"{name}.weights.{k}"] for k in range(3)]
    xyz, feats = sa(point, vector, ind["c1"], ind["i1"], W("layer1"))
    xyz, feats = sa(xyz, feats, ind["c2"], ind["i2"], W("layer2"))
    h = torch.cat([xyz, feats], 2)[:, None]
    for w in W("layer3"):
        h = act(torch.matmul(h, w))
    if record is not None:
        record.append(h.detach())
    feats = h.max(dim=2).values
    lin = lambda name, t: torch.nn.functional.linear(t, weights[f"{name}.weight"], weights[f"{name}.bias"])
    bn = lambda name, t: t * (weights[f"{name}.gamma"] * (1.0 / math.sqrt(1.0 + 1e-3))) + weights[f"{name}.beta"]
    net = bn("batchnorm1", act(lin("dense1", feats.reshape(feats.shape[0], -1))))
    if parameters is not None:
        net = torch.cat([net, bn("parameters_process1", bn("parameters_process1", parameters))], 1)
    return act(lin("last_dense2", act(lin("last_dense1", net))))
