#!/usr/bin/env python
"""What an actuated primitive 1 costs on the PLB f64 path, and whether handles without one (ud_plb_conf.action_dim1 = 0) still run at the
speed they ran at before the field existed.

    python tools/plb_two_hand_cost.py --parent-lib PATH [--repeats 20] [--warmup 5] [--rounds 3] [--out profiles/plb_two_hand_cost.txt]
    python tools/plb_two_hand_cost.py --resources --parent-src DIR [--out ...]      (no GPU: compiles csrc/plb_cluster.hip of both trees)

Every time is the median (min..max) of `--repeats` calls, each timed with a pair of device events on the call's stream after `--warmup`
untimed calls; one child process per block, so that every block starts from a fresh runtime and may load its own library (UNIDOM_HIP_SO).

  (a) legacy   the benched Torus shape (PlbConf: 8 envs x 1000 particles, n_grid 64, 19 substeps; two Spheres, primitive 1 unactuated), forward
               and forward + loss + adjoint, on the persistent path (what bench.py runs) and on the multi-kernel path: `--rounds` processes
               per library, the parent's and this one alternating.  The bar is the parent's own run-to-run spread (the min..max of its
               processes' medians); the verdict says where this library's median of medians lies.
  (b) bimanual BimanualConf (MoveConf's rod, a Sphere at each end, both actuated: action [B,6]) beside MoveConf (the same body, one
               primitive), 1 and 8 envs, forward and forward + loss + adjoint.
  (c) --resources: VGPRs, VGPR / SGPR spills and scratch bytes of pcl_fwd_kernel and pcl_bwd_kernel from the code-object metadata
               (hipcc --offload-arch=gfx950 -save-temps), the parent tree's source against this one's.  Appended to --out.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

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


def make(cfg, B, raw_move):
    """(sim, forward-only call, forward + loss + adjoint call) on the state of reset(); the action moves every actuated primitive a little"""
    import torch
    from unidom_amd.engine.plb_simulator import PlbSimulator
    sim = PlbSimulator(cfg, batch_size=B)
    st = sim.reset()
    row = ([0.3, -0.5, 0.2] * 2)[:sim.action_dim]
    act = torch.tensor([row] * B, dtype=torch.float64, device=sim.device) * raw_move
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


def child(args):
    import torch
    from unidom_amd.engine.plb_simulator import BimanualConf, MoveConf, PlbConf
    sync = torch.cuda.synchronize
    out = {}
    if args.child == "legacy":
        for path in (2, 1):
            cfg = PlbConf()
            cfg.path = path
            sim, fwd, fwd_bwd = make(cfg, 8, 0.004)
            assert sim.launch_plan() == path and (sim.n_particles, sim.n_grid, sim.substeps, sim.action_dim) == (1000, 64, 19, 3)
            for kind, fn in (("fwd", fwd), ("fwd_loss_bwd", fwd_bwd)):
                out[f"path{path}_{kind}"] = timed(fn, sync, args.warmup, args.repeats)
            sim.check_status()
    elif args.child == "bimanual":
        for B in (1, 8):
            for name, conf in (("move", MoveConf), ("bimanual", BimanualConf)):
                sim, fwd, fwd_bwd = make(conf(), B, 0.8)              # 0.8 x action.scale 0.005 = 4 mm per step
                assert sim.launch_plan() == 2 and sim.action_dim == (6 if name == "bimanual" else 3)
                for kind, fn in (("fwd", fwd), ("fwd_loss_bwd", fwd_bwd)):
                    t = timed(fn, sync, args.warmup, args.repeats)
                    t["substeps_per_s"] = sim.substeps * B / (t["median"] * 1e-3)
                    out[f"B{B}_{name}_{kind}"] = t
                sim.check_status()
    print("RESULT " + json.dumps(out))


def run_child(name, args, lib=None):
    env = dict(os.environ)
    if lib:
        env["UNIDOM_HIP_SO"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        raise SystemExit(f"child {name} failed ({p.returncode}); nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    return {}


def fmt(t):
    return f"{t['median']:8.3f} ms ({t['lo']:.3f}..{t['hi']:.3f}, n={t['n']})"


KERNELS = ("pcl_fwd_kernel", "pcl_bwd_kernel")
FIELDS = (("vgpr_count", "VGPRs (arch + acc)"), ("agpr_count", "AGPRs"), ("vgpr_spill_count", "VGPR spills"), ("sgpr_spill_count", "SGPR spills"),
          ("private_segment_fixed_size", "scratch bytes / lane"))


def resources(src):
    """{kernel: {field: int}} from the metadata of csrc/plb_cluster.hip compiled as the Makefile compiles it, with -save-temps."""
    d = tempfile.mkdtemp(prefix="plb_two_hand_asm_")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-save-temps", "-c",
           os.path.abspath(src), "-o", "tmp.o"]
    subprocess.run(cmd, cwd=d, check=True, capture_output=True)
    text = open(os.path.join(d, "plb_cluster-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n  - ", meta):
        m = re.search(r"\.name:\s+(\S+)", block)
        for k in KERNELS:
            if m and k in m.group(1):
                out[k] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1)) for f, _ in FIELDS}
    import shutil
    shutil.rmtree(d, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--parent-src", default="", help="the parent commit's tree (for --resources)")
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_two_hand_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20 and args.rounds >= 2
    if args.child:
        return child(args)
    L = []
    if args.resources:
        before = resources(os.path.join(args.parent_src, "unidom_amd", "csrc", "plb_cluster.hip"))
        after = resources(os.path.join(ROOT, "unidom_amd", "csrc", "plb_cluster.hip"))
        L += ["(c) persistent kernels, code-object metadata (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -save-temps), parent tree -> this tree", ""]
        for k in KERNELS:
            L.append(f"  {k}")
            for f, label in FIELDS:
                note = "" if after[k][f] == before[k][f] else ("   (lower)" if after[k][f] < before[k][f] else "   (HIGHER)")
                L.append(f"    {label:22s} {before[k][f]:6d} -> {after[k][f]:6d}{note}")
        L.append("")
        text = "\n".join(L) + "\n"
        open(args.out, "a").write(text)
        print(text)
        return
    L += ["PLB f64 path with both primitives actuated (ud_plb_conf.action_dim1), one MI355X",
          f"median (min..max) of {args.repeats} calls after {args.warmup} warm-up calls, device events; tools/plb_two_hand_cost.py", ""]
    if args.parent_lib:
        series = {"parent": [], "this": []}
        for _ in range(args.rounds):
            series["parent"].append(run_child("legacy", args, lib=args.parent_lib))
            series["this"].append(run_child("legacy", args))
        L.append(f"(a) legacy handle (action_dim1 = 0), the benched Torus shape (8 envs x 1000 particles, n_grid 64, 19 substeps): {args.rounds} processes per "
                 "library, the parent commit's and this one alternating")
        ok = True
        for path in (2, 1):
            for kind in ("fwd", "fwd_loss_bwd"):
                key = f"path{path}_{kind}"
                for who in ("parent", "this"):
                    L.append(f"  path {path} {kind:13s} {who:6s} per process [ms]: " + "  ".join(f"{r[key]['median']:.3f} ({r[key]['lo']:.3f}..{r[key]['hi']:.3f})"
                                                                                                  for r in series[who]))
                pm, tm = [r[key]["median"] for r in series["parent"]], [r[key]["median"] for r in series["this"]]
                mid = statistics.median(tm)
                where = "within" if min(pm) <= mid <= max(pm) else ("BELOW (faster than)" if mid < min(pm) else "ABOVE (slower than)")
                ok = ok and where != "ABOVE (slower than)"
                L.append(f"  path {path} {kind:13s} parent against itself {min(pm):.3f}..{max(pm):.3f}; this library's median of medians {mid:.3f}: {where} that spread")
        L.append("  verdict: " + ("legacy handles do not pay: no median above the parent's own run-to-run spread" if ok
                                  else "NOT inside the parent's own run-to-run spread: see the ABOVE lines"))
        L.append("")
    w = run_child("bimanual", args)
    L.append("(b) BimanualConf (two actuated Spheres, action [B,6]) beside MoveConf (the same rod, one Sphere, action [B,3]); persistent path, 1000 particles, "
             "n_grid 64, 19 substeps")
    L.append("  task       B  call            time per step call                          substeps/s")
    for B in (1, 8):
        for name in ("move", "bimanual"):
            for kind in ("fwd", "fwd_loss_bwd"):
                t = w[f"B{B}_{name}_{kind}"]
                L.append(f"  {name:9s} {B:2d}  {kind:14s}  {fmt(t)}   {t['substeps_per_s']:12.0f}")
    L.append("")
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
