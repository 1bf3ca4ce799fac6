#!/usr/bin/env python
"""What building a goal's target SDF costs (ud_plb_target_sdf, csrc/plb_target.hip) on one MI355X.

Shapes: n_grid 64 and 128 (quality 1 and 2), T = 1 and 8 targets in one call.  Goals: a Torus-like body (the Torus task's upright bar as a grid
mass, see torus_like; T > 1: the same body shifted cell by cell) and a single occupied corner cell, the slowest to converge
(the distance field has to cross the whole grid at 2 cells per sweep towards lower and 3 towards higher indices).  Per shape and goal:
    all 2 n sweeps enqueued   sweeps = 0: every launch after a target's fixed point returns at entry
    exact count               sweeps = max over targets of sweeps_run: no launch is wasted, the early return never fires
The difference of the two is what the launches that return at entry cost.  Each figure is the median (min..max) of `--repeats` calls
timed one by one with device events after `--warmup` untimed calls; outputs and work buffer are preallocated.  No threshold: nobody
has measured this before.

    python tools/plb_target_cost.py [--repeats 20] [--warmup 3] [--out profiles/plb_target_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torus_like(n, T):
    """The Torus task's bar (box 0.028 x 0.5 x 0.028 at (0.5, 0.3, 0.5)), 1000 particles at n_grid 64 and n^3 / 64^3 times as many
    elsewhere (the same particles per cell, so the body stays above the threshold), deposited with the quadratic B-spline weights and
    p_mass = (dx / 2)^2 of the simulator."""
    rng = np.random.default_rng(0)
    N = 1000 * n ** 3 // 64 ** 3
    p = (rng.random((N, 3)) * 2 - 1) * (0.5 * np.array([0.028, 0.5, 0.028])) + np.array([0.5, 0.3, 0.5])
    base = (p * n - 0.5).astype(np.int64)
    fx = p * n - base
    w = [0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1) ** 2, 0.5 * (fx - 0.5) ** 2]
    d = np.zeros((n, n, n))
    p_mass = (0.5 / n) ** 2
    for i, j, k in np.ndindex(3, 3, 3):
        np.add.at(d, (base[:, 0] + i, base[:, 1] + j, base[:, 2] + k), w[i][:, 0] * w[j][:, 1] * w[k][:, 2] * p_mass)
    return np.stack([np.roll(d, (t, 2 * t, -t), (0, 1, 2)) for t in range(T)])


def corner(n, T):
    d = np.zeros((T, n, n, n))
    d[:, 0, 0, 0] = 1.0
    return d


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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_target_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plb_target_cost: needs the GPU")
    from unidom_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = [f"# tools/plb_target_cost.py  {torch.cuda.get_device_name(dev)}  ud_plb_target_sdf, threshold 1e-4, warmup={args.warmup}, median (min..max) "
             f"of {args.repeats} calls, device events around each call"]
    for n in (64, 128):
        for T in (1, 8):
            for name, make in (("torus-like", torus_like), ("corner cell", corner)):
                d = torch.tensor(make(n, T), device=dev)
                sdf = torch.empty_like(d)
                run = torch.zeros((T,), dtype=torch.int32, device=dev)
                work = torch.empty((L.ud_plb_target_work_bytes(n, T) // 4,), dtype=torch.int32, device=dev)

                def call(sweeps):
                    _lib.check(L.ud_plb_target_sdf(n, T, _lib.ptr(d), 1e-4, sweeps, _lib.ptr(sdf), None, _lib.ptr(run), _lib.ptr(work), stream()),
                               "ud_plb_target_sdf")

                call(0)
                torch.cuda.synchronize()
                ran = run.cpu().tolist()
                ref = sdf.clone()
                exact = max(ran)
                t_all = timed(lambda: call(0), args.warmup, args.repeats)
                t_exact = timed(lambda: call(exact), args.warmup, args.repeats)
                torch.cuda.synchronize()
                same = bool(torch.equal(sdf, ref))
                cells = T * n ** 3
                occ = int((d > 1e-4).sum())
                lines.append(f"n_grid {n:3d}  T {T}  {name:11s}  {occ} occupied cells  sweeps_run {ran if T > 1 else ran[0]} of {2 * n}")
                lines.append(f"    all {2 * n:3d} sweeps enqueued  {t_all[0]:9.3f} ms ({t_all[1]:.3f}..{t_all[2]:.3f})")
                lines.append(f"    exact count ({exact:3d})        {t_exact[0]:9.3f} ms ({t_exact[1]:.3f}..{t_exact[2]:.3f})   "
                             f"{t_exact[0] * 1e6 / (exact * cells):.3f} ns per cell and sweep; same sdf bits as the full call: {same}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
