#!/usr/bin/env python
"""What scoring a trajectory for system identification costs on one MI355X (csrc/plb_sysid.hip).

Shapes: Move (1000 particles) and Writer (10 000 particles), n_grid 64, 8 envs, 20 frames = 160 clouds, each frame with a target of its own.
    (a) per frame      one ud_plb_loss_fwd + ud_plb_loss_bwd per frame with weights (0, 1, 0): 20 call pairs, the only way before
    (b) sequence       one ud_plb_density_seq_fwd + _bwd over the 160 items
(a) and (b) alternate; each figure is the median (min..max) of `--repeats` measurements after `--warmup` untimed ones, device events
around the calls of one measurement, every buffer preallocated.  Then one identification iteration of Move (horizon 20, every frame
scored, forward + backward through Identifier.forward) on the multi-kernel handle (the scale in ud_plb_conf) and on the persistent one
(action_scale_on_host), and ud_plb_chamfer at 10 000 x 10 000 points x 8 items.  No threshold: nobody has measured this before.

    python tools/plb_sysid_cost.py [--repeats 20] [--warmup 3] [--out profiles/plb_sysid_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, FRAMES = 8, 20


def measure(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns, warmup, repeats):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ms[k].append(measure(fn))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def fmt(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f}..{t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_sysid_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plb_sysid_cost: needs the GPU")
    from unidom_amd import _lib
    from unidom_amd.algorithms.plb_identify import Identifier
    from unidom_amd.engine.plb_losses import PlbTrajectoryLoss
    from unidom_amd.engine.plb_simulator import MoveConf, PlbSimulator, WriterConf
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lines = [f"# tools/plb_sysid_cost.py  {torch.cuda.get_device_name(dev)}  {B} envs, {FRAMES} frames, warmup={args.warmup}, median (min..max) of "
             f"{args.repeats}, device events around each measurement, (a) and (b) alternating"]
    gen = torch.Generator(device="cpu").manual_seed(0)
    for name, conf in (("Move", MoveConf()), ("Writer", WriterConf())):
        sim = PlbSimulator(conf, batch_size=B)
        N, n = sim.n_particles, sim.n_grid
        G = n ** 3
        st = sim.reset()
        jit = lambda s: (torch.randn((FRAMES, B, N, 3), generator=gen, dtype=torch.float64) * s).to(dev)
        drift = torch.arange(FRAMES, dtype=torch.float64, device=dev)[:, None, None, None] * torch.tensor([0.002, 0.001, 0.0], dtype=torch.float64, device=dev)
        x = (st.x[None] + drift + jit(0.002)).clamp(0.02, 0.9).contiguous()                  # [F,B,N,3]: the body drifting, every cloud its own
        rec = (st.x[None, :1] + 1.3 * drift + jit(0.002)[:, :1]).clamp(0.02, 0.9)
        targets = torch.stack([sim.get_grid_mass(st._replace(x=rec[f]))[0] for f in range(FRAMES)]).reshape(FRAMES, G).contiguous()
        zeros_sdf = torch.zeros((G,), dtype=torch.float64, device=dev)
        wts = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=dev)
        pp = st.prim_pos.contiguous()
        loss_a, gl_a = torch.empty((FRAMES, B), dtype=torch.float64, device=dev), torch.ones((B,), dtype=torch.float64, device=dev)
        gx_a, gpp = torch.empty_like(x), torch.empty_like(pp)

        def per_frame():
            for f in range(FRAMES):
                _lib.check(L.ud_plb_loss_fwd(sim._h, C.c_int(B), p(x[f]), p(pp), p(targets[f]), p(zeros_sdf), p(wts), C.c_int(1), p(loss_a[f]), None, stream()),
                           "ud_plb_loss_fwd")
                _lib.check(L.ud_plb_loss_bwd(sim._h, C.c_int(B), p(x[f]), p(pp), p(targets[f]), p(zeros_sdf), p(wts), C.c_int(1), p(gl_a), p(gx_a[f]), p(gpp),
                                             stream()), "ud_plb_loss_bwd")

        M = FRAMES * B
        xs = x.reshape(M, N, 3)
        idx = torch.arange(FRAMES, dtype=torch.int32, device=dev)[:, None].expand(-1, B).reshape(-1).contiguous()
        nwork, nsign = int(L.ud_plb_density_seq_work_bytes(sim._h, M)), int(L.ud_plb_density_seq_sign_bytes(sim._h, M))
        work = torch.empty((nwork // 8,), dtype=torch.float64, device=dev)
        sign = torch.empty((nsign // 8,), dtype=torch.int64, device=dev)
        loss_b, gl_b, gx_b = torch.empty((M,), dtype=torch.float64, device=dev), torch.ones((M,), dtype=torch.float64, device=dev), torch.empty_like(xs)

        def sequence():
            _lib.check(L.ud_plb_density_seq_fwd(sim._h, M, p(xs), p(targets), FRAMES, p(idx), p(loss_b), p(sign), p(work), nwork, stream()), "ud_plb_density_seq_fwd")
            _lib.check(L.ud_plb_density_seq_bwd(sim._h, M, p(xs), p(sign), p(gl_b), p(gx_b), stream()), "ud_plb_density_seq_bwd")

        ta, tb = alternating([per_frame, sequence], args.warmup, args.repeats)
        torch.cuda.synchronize()
        dl = float((loss_a.reshape(-1) - loss_b).abs().max() / loss_b.abs().max())
        dg = float((gx_a.reshape(M, N, 3) - gx_b).abs().max() / gx_b.abs().max())
        lines.append(f"{name}: {N} particles, n_grid {n}, {M} items, scratch {nwork >> 20} MiB ({nwork // (8 * G)} items per chunk), sign field {nsign >> 20} MiB")
        lines.append(f"    (a) per frame: {FRAMES} x (ud_plb_loss_fwd + _bwd), weights (0, 1, 0)  {fmt(ta)}")
        lines.append(f"    (b) sequence: ud_plb_density_seq_fwd + _bwd                      {fmt(tb)}   (a) / (b) = {ta[0] / tb[0]:.2f}")
        lines.append(f"    (b) against (a): loss rel {dl:.1e}, g_x rel {dg:.1e}")
        del sim
    # one identification iteration of Move: rollout of 20 steps, every frame scored, backward to (E, nu, yield_stress)
    actions = [[0.0, 0.6, 0.0]] * FRAMES
    for label, on_host in (("multi-kernel handle (action scale in ud_plb_conf)", False), ("persistent handle (action_scale_on_host)", True)):
        conf = MoveConf()
        conf.action_scale_on_host = on_host
        sim = PlbSimulator(conf, batch_size=B)
        ident = Identifier(sim, PlbTrajectoryLoss(sim), actions, frames=range(FRAMES))
        params = torch.tensor([[3000.0 + 500 * b, 0.3, 200.0] for b in range(B)], dtype=torch.float64, device=dev)
        with torch.no_grad():
            states = ident.rollout(ident.start_state(), torch.tensor([[6500.0, 0.3, 200.0]] * B, dtype=torch.float64, device=dev))
            ident.loss.update_target_density(torch.stack([sim.get_grid_mass(s)[0] for s in states[:FRAMES]]))
        state0 = ident.start_state()
        (t,) = alternating([lambda: ident.forward(state0, params)], 1, 5)
        sim.check_status()
        lines.append(f"Move identification iteration, horizon {FRAMES}, {sim.substeps} substeps per step, launch_plan {sim.launch_plan()}, {label}: {fmt(t)} of 5")
        del sim, ident
    # chamfer at the design point
    Np = 10000
    a = torch.rand((B, Np, 3), generator=gen, dtype=torch.float64).to(dev)
    b = torch.rand((1, Np, 3), generator=gen, dtype=torch.float64).to(dev)
    out, mab, mba = (torch.empty(s, dtype=torch.float64, device=dev) for s in ((B,), (B, Np), (B, Np)))
    both = lambda: _lib.check(L.ud_plb_chamfer(B, Np, p(a), 1, Np, p(b), None, p(out), p(mab), p(mba), stream()), "ud_plb_chamfer")
    lone = lambda: _lib.check(L.ud_plb_chamfer(B, Np, p(a), 1, Np, p(b), None, p(out), None, None, stream()), "ud_plb_chamfer")
    t2, t1 = alternating([both, lone], args.warmup, args.repeats)
    lines.append(f"ud_plb_chamfer {Np} x {Np} points x {B} items: with both min arrays {fmt(t2)}; without (one workgroup per item) {fmt(t1)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
