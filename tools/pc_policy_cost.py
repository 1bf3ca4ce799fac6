#!/usr/bin/env python
"""What the point-cloud policy's sampling / grouping kernels cost at the reference model's shapes (n = 200 points; layer1 512 centres x 32
samples on 3 feature channels, layer2 128 centres x 64 samples on 128), B = 1 and B = 64, against the op-by-op torch restatement of the
same ops on the device, and the whole ClsSsgModelPara forward + backward both ways.

    python tools/pc_policy_cost.py [--regions 21] [--warmup 3] [--out profiles/pc_policy_cost.txt]

  kernel      one ud_pc_* call through the C ABI on preallocated buffers
  op by op    farthest-point sampling as the loop of torch ops (one dependent arg-max per sample), the ball query as distance matrix ->
              mask -> sort -> first nsample -> fill, grouping as index gathers, the group adjoint as autograd's index_put (atomics)
  model       forward + backward of a scalar loss: the product model, and the same torch conv / max / head ops over the op-by-op
              sampling and grouping
Every figure is the median (min..max) over `--regions` timed regions of `inner` back-to-back calls, device events around a region, after
`--warmup` untimed regions; inner is 20 for the kernels and 1 for whatever takes milliseconds.  The restatement is never the code under
test: its indices are compared with the kernels' before anything is timed.  Then the gradient accuracy of tests/test_pc_policy_gpu.py:
per tensor the GPU's and the f32 CPU restatement's error against the f64 restatement.  Needs a GPU: there is no fallback.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def regions(fn, inner, n, warmup):
    import torch
    us = []
    for r in range(warmup + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            us.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(us), min(us), max(us)


def fmt(t):
    return f"{t[0]:10.2f} us ({t[1]:.2f}..{t[2]:.2f})"


# ---- the op-by-op restatement ------------------------------------------------------------------------------------------------------
def torch_fps(xyz, m):
    import torch
    B, n, _ = xyz.shape
    idx = torch.zeros((B, m), dtype=torch.int64, device=xyz.device)
    mind = torch.full((B, n), 1e38, dtype=xyz.dtype, device=xyz.device)
    cur = torch.zeros((B,), dtype=torch.int64, device=xyz.device)
    rows = torch.arange(B, device=xyz.device)
    for j in range(1, m):
        d = xyz - xyz[rows, cur][:, None, :]
        d = d * d
        mind = torch.minimum(mind, (d[..., 0] + d[..., 1]) + d[..., 2])
        cur = mind.argmax(1)
        idx[:, j] = cur
    return idx, xyz[rows[:, None], idx]


def torch_ball(radius, nsample, xyz, new_xyz):
    import torch
    n = xyz.shape[1]
    d = new_xyz[:, :, None, :] - xyz[:, None, :, :]
    d = d * d
    dist = torch.sqrt((d[..., 0] + d[..., 1]) + d[..., 2]).clamp_min(1e-20)
    cand = torch.arange(n, device=xyz.device).expand(dist.shape).clone()
    cand[~(dist < radius)] = n
    cand = cand.sort(dim=-1).values[..., :nsample]
    if cand.shape[-1] < nsample:
        cand = torch.cat([cand, cand.new_full(cand.shape[:-1] + (nsample - cand.shape[-1],), n)], -1)
    first = cand[..., :1]
    cand = torch.where(cand == n, first.expand_as(cand), cand)
    return torch.where(cand == n, torch.zeros_like(cand), cand)


def gather(t, idx):
    import torch
    rows = torch.arange(t.shape[0], device=t.device).reshape((-1,) + (1,) * (idx.dim() - 1))
    return t[rows, idx]


def torch_group(xyz, feats, new_xyz, idx):
    import torch
    return torch.cat([gather(xyz, idx) - new_xyz[:, :, None, :], gather(feats, idx)], -1)


def torch_model(model, point, vector, parameters):
    import torch

    def sa(layer, xyz, feats):
        c, new_xyz = torch_fps(xyz, layer.npoint)
        h = torch_group(xyz, feats, new_xyz, torch_ball(layer.radius, layer.nsample, xyz, new_xyz))
        for w in layer.weights:
            h = torch.matmul(h, w)
        return new_xyz, h.max(dim=2).values

    xyz, feats = sa(model.layer1, point, vector)
    xyz, feats = sa(model.layer2, xyz, feats)
    _, feats = model.layer3(xyz, feats)
    net = model.batchnorm1(model.dense1(feats.reshape(feats.shape[0], -1)))
    par = model.parameters_process1(model.parameters_process1(parameters))
    return model.head(torch.cat([net, par], 1))


def measure(B, args, say):
    import torch
    from unidom_amd import _lib
    from unidom_amd.algorithms.plb_pc_policy import ClsSsgModelPara
    L = _lib.lib()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(B)
    point = (torch.rand((B, 200, 3), generator=gen) * 0.07).to(dev)
    vector = point - 0.03
    R, W = args.regions, args.warmup
    say(f"B {B}")
    xyz, feats = point, vector
    for name, m, ns, Cf in (("layer1", 512, 32, 3), ("layer2", 128, 64, 128)):
        n = xyz.shape[1]
        f = feats if Cf == feats.shape[2] else torch.randn((B, n, Cf), generator=gen).to(dev)
        ci, nx = torch.empty((B, m), dtype=torch.int32, device=dev), torch.empty((B, m, 3), device=dev)
        bi, bc = torch.empty((B, m, ns), dtype=torch.int32, device=dev), torch.empty((B, m), dtype=torch.int32, device=dev)
        out = torch.empty((B, m, ns, 3 + Cf), device=dev)
        go = torch.randn((B, m, ns, 3 + Cf), generator=gen).to(dev)
        gx, gf, gn = torch.empty((B, n, 3), device=dev), torch.empty((B, n, Cf), device=dev), torch.empty((B, m, 3), device=dev)
        P = lambda t: t.data_ptr()
        k_fps = lambda: _lib.check(L.ud_pc_fps(B, n, m, P(xyz), P(ci), P(nx), st), "fps")
        k_ball = lambda: _lib.check(L.ud_pc_ball_query(B, n, m, 0.02, ns, P(xyz), P(nx), P(bi), P(bc), st), "ball")
        k_fwd = lambda: _lib.check(L.ud_pc_group_fwd(B, n, m, ns, Cf, P(xyz), P(f), P(nx), P(bi), P(out), st), "group_fwd")
        k_bwd = lambda: _lib.check(L.ud_pc_group_bwd(B, n, m, ns, Cf, P(bi), P(ci), P(go), P(gx), P(gf), P(gn), st), "group_bwd")
        for k in (k_fps, k_ball, k_fwd, k_bwd):
            k()
        # the restatement gives the same indices (exact ties aside: it has the same lowest-index rule) before anything is timed
        ti, tnx = torch_fps(xyz, m)
        tb = torch_ball(0.02, ns, xyz, tnx)
        same_fps = float((ti == ci.long()).float().mean())
        same_ball = float((tb == bi.long()).float().mean())
        agree = float((torch_group(xyz, f, tnx, tb) - out).abs().max())
        say(f"  {name}: n {n} -> {m} centres x {ns} samples, {Cf} channels;  indices equal to the restatement's: fps {same_fps:.4f}  ball {same_ball:.4f}  max |group - restatement| {agree:.1e}")

        def t_bwd():
            X, Fe = xyz.detach().requires_grad_(True), f.detach().requires_grad_(True)
            torch_group(X, Fe, gather(X, ti), tb).backward(go)

        rows = [("fps + gather", k_fps, 20, lambda: torch_fps(xyz, m), 1),
                ("ball query", k_ball, 20, lambda: torch_ball(0.02, ns, xyz, tnx), 5),
                ("group forward", k_fwd, 20, lambda: torch_group(xyz, f, tnx, tb), 5),
                ("group backward", k_bwd, 20, t_bwd, 5)]
        for label, kern, ki, op, oi in rows:
            a, b = regions(kern, ki, R, W), regions(op, oi, R, W)
            say(f"    {label:15s} kernel {fmt(a)}   op by op {fmt(b)}   op by op / kernel {b[0] / a[0]:8.1f}")
        xyz, feats = nx.clone(), torch.randn((B, m, 128), generator=gen).to(dev)
    model = ClsSsgModelPara(3, generator=torch.Generator().manual_seed(1)).to(dev)
    par, ga = torch.randn((B, 3), generator=gen).to(dev), torch.randn((B, 3), generator=gen).to(dev)

    def run(forward):
        model.zero_grad(set_to_none=True)
        V = vector.detach().requires_grad_(True)
        (forward(model, point, V, par) * ga).sum().backward()

    product = lambda mod, p, v, q: mod(p, v, q)
    with torch.no_grad():
        diff = float((model(point, vector, par) - torch_model(model, point, vector, par)).abs().max())
    a, b = regions(lambda: run(product), 1, R, W), regions(lambda: run(torch_model), 1, R, W)
    say(f"  model forward + backward: product {fmt(a)}   op by op {fmt(b)}   op by op / product {b[0] / a[0]:6.1f}   (actions differ by {diff:.1e})")


def accuracy(say):
    import torch
    from tests import test_pc_policy_gpu as T
    c = T.model_case()
    model = c["model"].to("cuda")
    dev = lambda x: torch.tensor(x, device="cuda")
    V = dev(c["vector"]).requires_grad_(True)
    model.zero_grad(set_to_none=True)
    (model(dev(c["point"]), V, dev(c["parameters"])) * dev(c["ga"])).sum().backward()
    got = {k: p.grad.double().cpu().numpy() for k, p in model.named_parameters()}
    got["vector"] = V.grad.double().cpu().numpy()
    say("gradient error against the f64 CPU restatement, relative to the tensor's max-abs (tests/test_pc_policy_gpu.py; bar = 8 x f32 cpu)")
    for k in c["names"] + ["vector"]:
        say(f"    {k:28s} gpu {T.rel_err(got[k], c['g64'][k]):.3e}   f32 cpu {T.rel_err(c['g32'][k], c['g64'][k]):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pc_policy_cost.txt"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tools/pc_policy_cost.py measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/pc_policy_cost.py  {torch.cuda.get_device_name(0)}  n 200 points, ClsSsgModelPara shapes")
    say(f"# median (min..max) over {args.regions} regions, device events around a region, {args.warmup} warm-up regions; inner calls per region: kernels 20, op by op 1 (fps, model) or 5")
    for B in args.batches:
        measure(B, args, say)
    accuracy(say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
