#!/usr/bin/env python
"""What the cloth DEPTH observation costs (csrc/env_depth.hip) next to the same map built op by op in torch.

Two shapes: M = 1280 images of P = 512 particles (the 40 x 32 substep observations of one fold_cloth1 step_diff at 32 envs) and
M = 160 of P = 3573 (fold_tshirt, 40 x 4).  Per shape, on one device and one stream:
    fused fwd    ud_cloth_depth_fwd into preallocated buffers (image and owner), one launch
    fused bwd    ud_cloth_depth_bwd, one launch
    op by op     argsort (stable), gathers, two divides, floors, clamps, zeros and index_put_ -- what get_obs(DEPTH) would be
                 without the kernel; its result for contested pixels is whichever write the device lands last
Each figure is the median (min..max) of `--repeats` calls timed one by one with device events after `--warmup` untimed calls.  Next to
the fused times: the bytes the call must write (image + owner, or g_x) over the time, as a fraction of the HBM peak rate.

    python tools/depth_cost.py [--repeats 30] [--warmup 5] [--out profiles/depth_cost.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = W = 320
PIXEL_SIZE, Z_OFFSET = 0.003125, 0.01
HBM_PEAK = 8.0e12   # bytes/s, MI355X specification


def lattice(name):
    """Rest positions of the task's cloth (cloth_simulator.py:339-353), [P,3]."""
    from unidom_amd.envs.basic.cloth_conf import ENVS_DIR
    if name == "fold_tshirt":
        n, mask = 180, np.load(f"{ENVS_DIR}/others/tshirt_mask.npy")
    else:
        n, mask = 80, np.zeros((80, 80), np.float32)
        mask[32:48, 32:64] = 1
    ii, jj = np.nonzero(mask)
    return np.stack([ii / n, np.zeros(len(ii)), (n - jj) / n], -1).astype(np.float32)


def op_by_op(x):
    M, P = x.shape[:2]
    h = x[..., 1] + Z_OFFSET
    iz = torch.argsort(h, dim=1, stable=True)
    hs = torch.gather(h, 1, iz)
    px = torch.clamp(torch.floor(torch.gather(x[..., 0], 1, iz) / PIXEL_SIZE), 0, W - 1).nan_to_num(0.0).long()
    py = torch.clamp(torch.floor(torch.gather(x[..., 2], 1, iz) / PIXEL_SIZE), 0, H - 1).nan_to_num(0.0).long()
    img = torch.zeros((M, H, W), dtype=torch.float32, device=x.device)
    img.index_put_((torch.arange(M, device=x.device)[:, None].expand(M, P), py, px), hs)
    return img


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_cost: needs the GPU")
    if args.repeats < 20:
        sys.exit("depth_cost: at least 20 repeats")
    import ctypes as C

    from unidom_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = [f"# tools/depth_cost.py  {torch.cuda.get_device_name(dev)}  {H} x {W} images, warmup={args.warmup}, median (min..max) of "
             f"{args.repeats} calls, device events around each call; HBM peak taken as {HBM_PEAK / 1e12:.1f} TB/s"]
    for task, M in (("fold_cloth1", 1280), ("fold_tshirt", 160)):
        x0 = lattice(task)
        P = x0.shape[0]
        rng = np.random.default_rng(0)
        x = torch.tensor(np.abs(x0[None] + rng.normal(size=(M, P, 3)) * 2e-3).astype(np.float32), device=dev)
        img = torch.empty((M, H, W), dtype=torch.float32, device=dev)
        owner = torch.empty((M, P), dtype=torch.int32, device=dev)
        g_img = torch.randn((M, H, W), dtype=torch.float32, device=dev)
        g_x = torch.empty((M, P, 3), dtype=torch.float32, device=dev)

        def fwd():
            _lib.check(L.ud_cloth_depth_fwd(M, P, H, W, PIXEL_SIZE, Z_OFFSET, _lib.ptr(x), _lib.ptr(img), _lib.ptr(owner), stream()), "fwd")

        def bwd():
            _lib.check(L.ud_cloth_depth_bwd(M, P, H, W, _lib.ptr(owner), _lib.ptr(g_img), _lib.ptr(g_x), stream()), "bwd")

        t_f = timed(fwd, args.warmup, args.repeats)
        t_b = timed(bwd, args.warmup, args.repeats)
        t_o = timed(lambda: op_by_op(x), args.warmup, args.repeats)
        differ = int((op_by_op(x) != img).sum())
        wf, wb = M * (H * W + P) * 4, M * P * 3 * 4
        lines.append(f"{task:11s} M={M:5d} P={P:5d}")
        lines.append(f"  fused fwd  {t_f[0]:8.3f} ms ({t_f[1]:.3f}..{t_f[2]:.3f})   writes {wf / 1e6:7.1f} MB -> {wf / t_f[0] / 1e9:6.2f} TB/s = "
                     f"{100 * wf / (t_f[0] * 1e-3) / HBM_PEAK:4.1f} % of HBM peak")
        lines.append(f"  fused bwd  {t_b[0]:8.3f} ms ({t_b[1]:.3f}..{t_b[2]:.3f})   writes {wb / 1e6:7.1f} MB -> {wb / t_b[0] / 1e9:6.2f} TB/s = "
                     f"{100 * wb / (t_b[0] * 1e-3) / HBM_PEAK:4.1f} % of HBM peak")
        lines.append(f"  op by op   {t_o[0]:8.3f} ms ({t_o[1]:.3f}..{t_o[2]:.3f})   forward only; {t_o[0] / t_f[0]:.1f} x the fused forward; "
                     f"{differ} of {M * H * W} pixels differ from the fused image")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
