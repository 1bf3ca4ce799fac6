#!/usr/bin/env python
"""What the PLB Writer task costs (10 000 particles, n_grid 64, one Capsule: engine/plb_simulator.py WriterConf), and whether the
Sphere handles of the multi-kernel path still run at the speed they ran at before the Capsule existed.

    python tools/plb_writer_cost.py [--parent-lib PATH] [--repeats 25] [--warmup 5] [--rounds 4] [--out profiles/plb_writer_cost.txt]

Every figure is the median (min..max) of `--repeats` calls, each timed with a pair of device events on the call's stream after
`--warmup` untimed calls; one child process per block below, so that every block starts from a fresh runtime and may load its own
library (UNIDOM_HIP_SO).

  writer      WriterConf at B = 1 and 8, the task's own 19 substeps per step: forward (no checkpoint) and forward with checkpoint +
              contact loss + adjoint, in substeps/s; the same handle with a sticky Sphere of the Capsule's radius in its place.
  share       plb_grid's part of a forward substep's kernel time at B = 8 (rocprofv3 kernel trace, a run of its own).
  sphere      with --parent-lib: a Sphere-only handle, path = 1, Torus sizes (1000 particles, n_grid 64, 19 substeps, B = 8), forward
              and forward + loss + adjoint; `--rounds` children per library, the two libraries alternating.  The verdict line says
              whether this library's medians lie within the spread the parent's own children show.
  bench       with --parent-lib: `bench.py --workload torus` and `--plb-grad` once per library (the persistent path, whose code this
              library shares with the parent) as a sanity line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, stream_sync, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    stream_sync()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), lo=min(ms), hi=max(ms), n=len(ms))


def make(cfg, B, grad):
    """(sim, forward-only call, forward + loss + adjoint call) on the state of reset(), the primitive moved a little each call"""
    import torch
    from unidom_amd.engine.plb_simulator import PlbSimulator
    sim = PlbSimulator(cfg, batch_size=B)
    st = sim.reset()
    act = torch.tensor([[0.3, -0.5, 0.2]] * B, dtype=torch.float64, device=sim.device) * (0.004 if cfg.action_scale[0] == 1.0 else 1.0)
    G = sim.n_grid ** 3
    td, ts = torch.zeros(G, dtype=torch.float64, device=sim.device), torch.rand(G, dtype=torch.float64, device=sim.device)

    def fwd():
        with torch.no_grad():
            sim.step(st, act)

    def fwd_bwd():
        s = st._replace(x=st.x.detach().requires_grad_(True), E=st.E.detach().requires_grad_(True))
        a = act.detach().requires_grad_(True)
        s1 = sim.step(s, a)
        loss, _ = sim.compute_loss(s1, td, ts, (1.0, 1.0, 1.0), True)
        loss.sum().backward()

    return sim, fwd, fwd_bwd


def writer_cfg(sphere, substeps=0):
    from unidom_amd.engine.plb_simulator import WriterConf
    cfg = WriterConf()
    if substeps:
        cfg.substeps = substeps
    if sphere:
        cfg.prim_kind, cfg.prim_h, cfg.prim_rot, cfg.prim_friction = (0,), (0.0,), ((1.0, 0.0, 0.0, 0.0),), (0.0,)
    return cfg


def torus_cfg():
    from unidom_amd.engine.plb_simulator import PlbConf
    cfg = PlbConf()
    cfg.path = 1
    return cfg


def child(args):
    import torch
    sync = torch.cuda.synchronize
    out = {}
    if args.child == "writer":
        for B in (1, 8):
            for name, sphere in (("capsule", False), ("sphere", True)):
                sim, fwd, fwd_bwd = make(writer_cfg(sphere), B, True)
                assert sim.launch_plan() == 1
                for kind, fn in (("fwd", fwd), ("fwd_loss_bwd", fwd_bwd)):
                    t = timed(fn, sync, args.warmup, args.repeats)
                    t["substeps_per_s"] = sim.substeps * B / (t["median"] * 1e-3)
                    out[f"B{B}_{name}_{kind}"] = t
                sim.check_status()
    elif args.child == "trace":
        sim, fwd, _ = make(writer_cfg(False), 8, False)
        for _ in range(5):
            fwd()
        sync()
    elif args.child == "sphere":
        sim, fwd, fwd_bwd = make(torus_cfg(), 8, True)
        assert sim.launch_plan() == 1
        for kind, fn in (("fwd", fwd), ("fwd_loss_bwd", fwd_bwd)):
            out[kind] = timed(fn, sync, args.warmup, args.repeats)
        sim.check_status()
    print("RESULT " + json.dumps(out))


def run_child(name, args, lib=None, prefix=()):
    env = dict(os.environ)
    if lib:
        env["UNIDOM_HIP_SO"] = os.path.abspath(lib)
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        raise SystemExit(f"child {name} failed ({p.returncode}); nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    return {}


def fmt(t):
    return f"{t['median']:8.3f} ms ({t['lo']:.3f}..{t['hi']:.3f}, n={t['n']})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_writer_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20
    if args.child:
        return child(args)
    L = ["PLB Writer task (WriterConf: 10 000 particles, n_grid 64, 19 substeps per step, multi-kernel path) on one MI355X",
         f"median (min..max) of {args.repeats} calls after {args.warmup} warm-up calls, device events; tools/plb_writer_cost.py", ""]
    w = run_child("writer", args)
    L.append("primitive  B  call            time per step call                          substeps/s")
    for B in (1, 8):
        for name in ("capsule", "sphere"):
            for kind in ("fwd", "fwd_loss_bwd"):
                t = w[f"B{B}_{name}_{kind}"]
                L.append(f"{name:9s} {B:2d}  {kind:14s}  {fmt(t)}   {t['substeps_per_s']:12.0f}")
    L.append("")
    # plb_grid's share of the forward substep kernels, from a kernel trace of its own
    import csv
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="plb_writer_trace_", dir=os.path.dirname(os.path.abspath(args.out)))
    run_child("trace", args, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "-f", "csv", "--"))
    stats = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
    rows = list(csv.DictReader(open(stats[0])))
    shutil.rmtree(d, ignore_errors=True)
    sub = {k: sum(float(r["TotalDurationNs"]) for r in rows if k in r["Name"]) for k in ("plb_grid<", "plb_p2g<", "plb_g2p_p2g<", "plb_g2p<")}
    tot = sum(sub.values())
    L.append("forward substep kernels at B = 8, Capsule (rocprofv3 kernel trace of 5 step calls, a run of its own), share of their summed time:")
    for k, v in sub.items():
        L.append(f"  {k[:-1]:12s} {100 * v / tot:5.1f} %   {v / 1e3 / (5 * 19):8.2f} us per substep")
    L.append("")
    if args.parent_lib:
        series = {"parent": [], "this": []}
        for _ in range(args.rounds):
            series["parent"].append(run_child("sphere", args, lib=args.parent_lib))
            series["this"].append(run_child("sphere", args))
        L.append(f"Sphere-only handle, path = 1, Torus sizes (1000 particles, n_grid 64, 19 substeps, B = 8): {args.rounds} processes per library, alternating")
        ok = True
        for kind in ("fwd", "fwd_loss_bwd"):
            for who in ("parent", "this"):
                L.append(f"  {kind:13s} {who:6s} medians per process [ms]: " + "  ".join(f"{r[kind]['median']:.3f}" for r in series[who]))
            pm, tm = [r[kind]["median"] for r in series["parent"]], [r[kind]["median"] for r in series["this"]]
            mid = statistics.median(tm)
            where = "within" if min(pm) <= mid <= max(pm) else ("BELOW (faster than)" if mid < min(pm) else "ABOVE (slower than)")
            ok = ok and where == "within"
            L.append(f"  {kind:13s} parent against itself {min(pm):.3f}..{max(pm):.3f}; this library's median of medians {mid:.3f}: {where} that spread")
        L.append("  verdict: " + ("within the parent's own run-to-run spread" if ok else "NOT within the parent's own run-to-run spread"))
        L.append("")
        L.append("bench.py --workload torus (persistent path; its kernels are the parent's instruction for instruction), one run per library:")
        for extra in ((), ("--plb-grad",)):
            for who, lib in (("parent", args.parent_lib), ("this", "")):
                env = dict(os.environ)
                if lib:
                    env["UNIDOM_HIP_SO"] = os.path.abspath(lib)
                p = subprocess.run([sys.executable, "bench.py", "--workload", "torus", "--gpus", "1", "--steps", "20", "--warmup", "3", "--no-cpu-baseline", *extra],
                                   env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
                if p.returncode != 0:
                    raise SystemExit(f"bench.py failed ({p.returncode}); nothing more is started\n{p.stderr[-3000:]}")
                r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                L.append(f"  {' '.join(extra) or 'forward':10s} {who:6s} {r['value']:12.0f} {r['unit']}")
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
