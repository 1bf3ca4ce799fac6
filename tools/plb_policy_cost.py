#!/usr/bin/env python
"""What the PLB closed-loop policy costs on the Torus conf (N = 1000, two primitives, hidden (256, 256): d_0 = 1214), fused kernel pair
against the op-by-op torch restatement of the same policy on the device, and the share of a SolverNN iteration each takes.

    python tools/plb_policy_cost.py [--regions 21] [--inner 50] [--warmup 3] [--horizon 10] [--out profiles/plb_policy_cost.txt]

  fused       ud_plb_policy_fwd (taped) and ud_plb_policy_bwd through the C ABI on preallocated buffers
  op by op    gather x 2, scale, cat x 3, one baddbmm + relu per layer, clamp (B independent policies: batched weights), and its
              autograd backward with the parameter gradient accumulated into .grad
  iteration   SolverNN.forward + optimiser step (horizon env steps: act -> step -> compute_loss, backward), host clock around a
              device synchronise
Every figure is the median (min..max) over `--regions` timed regions of `--inner` back-to-back calls each, device events around a
region, after `--warmup` untimed regions.  The backward of the torch restatement needs a graph per call: the `--inner` graphs of a
region are built before its first event.  Needs a GPU: there is no fallback.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def regions(fn, inner, n, warmup, before=None):
    """us per call: median, min, max over n regions of `inner` calls."""
    import torch
    us = []
    for r in range(warmup + n):
        arg = before() if before else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(inner):
            fn(arg[i]) if before else fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            us.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(us), min(us), max(us)


def fmt(t):
    return f"{t[0]:9.2f} us ({t[1]:.2f}..{t[2]:.2f})"


def measure(B, args):
    import torch
    from unidom_amd import _lib
    from unidom_amd.algorithms.plb_solver import make_goal
    from unidom_amd.algorithms.plb_solver_nn import SolverNN
    from unidom_amd.engine.plb_losses import PlbLoss
    from unidom_amd.engine.plb_policy import PlbPolicy
    from unidom_amd.engine.plb_simulator import PlbConf, PlbSimulator
    L = _lib.lib()
    sim = PlbSimulator(PlbConf(), batch_size=B)
    pol = PlbPolicy(sim).init_params(0)
    dev = sim.device
    st = sim.reset()
    N, P, dims = sim.n_particles, sim.n_primitive, pol.dims
    x, pp = st.x.contiguous(), st.prim_pos.contiguous()
    v = torch.randn_like(x) * 0.1
    pr = pol._prim_rot(st)
    params = pol.get_params()
    mk = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    action, tape = mk(B, dims[-1]), mk(L.ud_plb_policy_tape_bytes(B, pol.n_layer, pol._cdims) // 8)
    ga = torch.randn(B, dims[-1], dtype=torch.float64, device=dev)
    gx, gv, gpp, gpr, gp = mk(B, N, 3), mk(B, N, 3), mk(B, P, 3), mk(B, P, 4), torch.zeros(B, pol.n_params, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    shape = pol._shape_args(B)
    p = lambda t: C.c_void_p(t.data_ptr())

    def fused_fwd():
        _lib.check(L.ud_plb_policy_fwd(*shape, p(x), p(v), p(pp), p(pr), p(params), pol._param_stride, p(action), p(tape), stream), "fwd")

    def fused_bwd():
        _lib.check(L.ud_plb_policy_bwd(*shape, p(params), pol._param_stride, p(tape), p(ga), p(gx), p(gv), p(gpp), p(gpr), p(gp), stream), "bwd")

    # the op-by-op restatement: batched weights [B, d_{l+1}, d_l], the same numbers
    Ws, bs, at = [], [], 0
    for l in range(pol.n_layer):
        n = dims[l + 1] * dims[l]
        Ws.append(params[:, at:at + n].reshape(B, dims[l + 1], dims[l]).clone().requires_grad_(True))
        at += n
        bs.append(params[:, at:at + dims[l + 1]].clone().requires_grad_(True))
        at += dims[l + 1]
    idx = torch.arange(pol.obs_num, device=dev) * pol.obs_step
    leaves = [t.clone().requires_grad_(True) for t in (x, v, pp)]

    def torch_fwd():
        X, V, PP = leaves
        h = torch.cat([torch.cat([X[:, idx], V[:, idx] * pol.velocity_weight], -1).reshape(B, -1), torch.cat([PP, pr], -1).reshape(B, -1)], -1)
        for l in range(pol.n_layer):
            h = torch.baddbmm(bs[l][:, :, None], Ws[l], h[:, :, None])[:, :, 0]
            if l != pol.n_layer - 1:
                h = torch.relu(h)
        return torch.clamp(h, -1.0, 1.0)

    def torch_bwd(a):
        a.backward(ga)

    fused_fwd()
    agree = float((torch_fwd().detach() - action).abs().max())
    inner, n, w = args.inner, args.regions, args.warmup
    out = dict(agree=agree, fused_fwd=regions(fused_fwd, inner, n, w), fused_bwd=regions(fused_bwd, inner, n, w),
               torch_fwd=regions(torch_fwd, inner, n, w), torch_bwd=regions(torch_bwd, inner, n, w, before=lambda: [torch_fwd() for _ in range(inner)]))
    # one SolverNN iteration on the fused policy
    goal_actions = torch.tensor([[0.6, 0.0, 0.0]] * 5, dtype=torch.float64, device=dev)
    loss = PlbLoss(sim, weights=(1.0, 1.0, 1.0), soft_contact=True).load_target_density(make_goal(sim, goal_actions))
    solver = SolverNN(sim, loss, pol, horizon=args.horizon, n_iters=1, optim="Adam", lr=0.1)
    optim = solver.optim_cls(params, **solver.optim_kwargs)
    state0, ms = solver.start_state(), []
    for it in range(args.warmup + 9):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, grad, _ = solver.forward(state0, optim.parameters)
        optim.step(grad)
        torch.cuda.synchronize()
        if it >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    sim.check_status()
    out["iter_ms"] = (statistics.median(ms), min(ms), max(ms))
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=21)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_policy_cost.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/plb_policy_cost.py needs a GPU: nothing is measured without one")
    H = args.horizon
    lines = [f"# tools/plb_policy_cost.py  {torch.cuda.get_device_name(0)}  Torus conf: N 1000, P 2, dims (1214, 256, 256, 3), relu, B independent policies",
             f"# median (min..max) over {args.regions} regions of {args.inner} back-to-back calls, device events around a region, {args.warmup} warm-up regions",
             f"# iteration: SolverNN.forward + Adam step, horizon {H}, host clock around a device synchronise, median of 9"]
    for B in (1, 8):
        r = measure(B, args)
        f, t = r["fused_fwd"][0] + r["fused_bwd"][0], r["torch_fwd"][0] + r["torch_bwd"][0]
        it_us = r["iter_ms"][0] * 1e3
        it_torch = it_us - H * f + H * t
        lines += [f"B {B}   fused and op-by-op actions agree to {r['agree']:.1e}",
                  f"    fused     forward {fmt(r['fused_fwd'])}   backward {fmt(r['fused_bwd'])}   sum {f:9.2f} us",
                  f"    op by op  forward {fmt(r['torch_fwd'])}   backward {fmt(r['torch_bwd'])}   sum {t:9.2f} us   op by op / fused {t / f:6.2f}",
                  f"    iteration {r['iter_ms'][0]:9.3f} ms ({r['iter_ms'][1]:.3f}..{r['iter_ms'][2]:.3f});  {H} x fused pair = {100 * H * f / it_us:5.2f} % of it;"
                  f"  with the op-by-op pair in its place the iteration would be {it_torch / 1e3:9.3f} ms, {100 * H * t / it_torch:5.2f} % of it the policy",
                  "    verdict: the fused pair is " + ("FASTER than" if f < t else "NOT faster than") + " the op-by-op restatement at this batch size"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
