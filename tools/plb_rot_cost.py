#!/usr/bin/env python
"""What rotating primitives cost on the PLB f64 path, and whether the handles that existed before them still run at their speed.

    python tools/plb_rot_cost.py --parent-tree PATH [--repeats 25] [--warmup 5] [--rounds 2] [--out profiles/plb_rot_cost.txt]

PATH is a checkout of the parent commit with its library built: its own tools/plb_writer_cost.py children are run from it (the parent's
Python over the parent's library), alternating with this tree's, `--rounds` processes each.

  existing    tools/plb_writer_cost.py's `writer` child (WriterConf, 10 000 particles, n_grid 64, 19 substeps, B = 1 and 8, constant-
              orientation Capsule and the Sphere in its place, forward and forward + loss + adjoint) and its `sphere` child (Sphere-only
              Torus handle, path = 1, B = 8) on both trees.  The verdict per line: this tree's medians within the spread of the parent's.
  rotating    the Writer shape on a rot_state handle with six action dimensions against the constant-orientation Capsule of the same
              process: forward and forward + loss + adjoint, substeps/s and the ratio.
  kernels     rocprofv3 kernel trace (a run of its own per handle) of forward + loss + adjoint step calls at B = 8: per-kernel time of the
              rotating handle beside the constant-orientation one.
Every timing is the median (min..max) of `--repeats` calls after `--warmup` untimed ones, device events (plb_writer_cost.timed).
"""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rot_cfg(rot):
    from unidom_amd.engine.plb_simulator import WriterConf
    cfg = WriterConf()
    if rot:
        cfg.rot_state, cfg.action_dim, cfg.action_scale_w = True, 6, (0.05, 0.05, 0.05)
    return cfg


def make(rot, B):
    import torch
    from unidom_amd.engine.plb_simulator import PlbSimulator
    sim = PlbSimulator(rot_cfg(rot), batch_size=B)
    st = sim.reset()
    a = [0.3, -0.5, 0.2] + ([0.3, -0.2, 0.25] if rot else [])
    act = torch.tensor([a] * B, dtype=torch.float64, device=sim.device)
    G = sim.n_grid ** 3
    td, ts = torch.zeros(G, dtype=torch.float64, device=sim.device), torch.rand(G, dtype=torch.float64, device=sim.device)

    def fwd():
        with torch.no_grad():
            sim.step(st, act)

    def fwd_bwd():
        s = st._replace(x=st.x.detach().requires_grad_(True), E=st.E.detach().requires_grad_(True))
        s1 = sim.step(s, act.detach().requires_grad_(True))
        loss, _ = sim.compute_loss(s1, td, ts, (1.0, 1.0, 1.0), True)
        loss.sum().backward()

    return sim, fwd, fwd_bwd


def child(args):
    import torch
    from tools.plb_writer_cost import timed
    out = {}
    if args.child == "rot":
        for B in (1, 8):
            for name, rot in (("const", False), ("rot", True)):
                sim, fwd, fwd_bwd = make(rot, B)
                assert sim.launch_plan() == 1
                for kind, fn in (("fwd", fwd), ("fwd_loss_bwd", fwd_bwd)):
                    t = timed(fn, torch.cuda.synchronize, args.warmup, args.repeats)
                    t["substeps_per_s"] = sim.substeps * B / (t["median"] * 1e-3)
                    out[f"B{B}_{name}_{kind}"] = t
                sim.check_status()
    else:                                   # trace_const / trace_rot: five forward + loss + adjoint calls at B = 8
        sim, _, fwd_bwd = make(args.child == "trace_rot", 8)
        for _ in range(5):
            fwd_bwd()
        torch.cuda.synchronize()
    print("RESULT " + json.dumps(out))


def run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} in {cwd} failed ({p.returncode}); nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    return {}


def trace(name, args, outdir):
    d = tempfile.mkdtemp(prefix="plb_rot_trace_", dir=outdir)
    run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "-f", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", name,
         "--repeats", str(args.repeats), "--warmup", str(args.warmup)], ROOT)
    stats = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
    rows = list(csv.DictReader(open(stats[0])))
    shutil.rmtree(d, ignore_errors=True)
    per = {}
    for r in rows:
        if "plb_" in r["Name"]:
            key = r["Name"].split("(")[0].replace("void ud::", "").replace("ud::", "")
            per[key] = per.get(key, 0.0) + float(r["TotalDurationNs"])
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_rot_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20
    if args.child:
        return child(args)
    tail = ["--repeats", str(args.repeats), "--warmup", str(args.warmup)]
    L = ["PLB f64 path, rotating primitives (rot_state): cost on one MI355X; tools/plb_rot_cost.py",
         f"median of {args.repeats} calls after {args.warmup} warm-up calls, device events; one process per block, parent and this tree alternating", ""]
    if args.parent_tree:
        trees = (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT))
        series = {(who, c): [] for who, _ in trees for c in ("writer", "sphere")}
        for _ in range(args.rounds):
            for c in ("writer", "sphere"):
                for who, tree in trees:
                    series[(who, c)].append(run([sys.executable, os.path.join(tree, "tools", "plb_writer_cost.py"), "--child", c] + tail, tree))
        L.append(f"existing handles, {args.rounds} processes per tree: median per process [ms per step call]")
        ok = True
        for c in ("writer", "sphere"):
            for key in series[("parent", c)][0]:
                pm, tm = [r[key]["median"] for r in series[("parent", c)]], [r[key]["median"] for r in series[("this", c)]]
                lo, hi = min(pm), max(pm)
                inside = all(lo <= t <= hi for t in tm)
                worst = max(max(t / hi - 1, 1 - t / lo) for t in tm)
                ok = ok and inside
                L.append(f"  {c:6s} {key:24s} parent " + " ".join(f"{v:8.3f}" for v in pm) + "   this " + " ".join(f"{v:8.3f}" for v in tm) +
                         ("   within the parent's spread" if inside else f"   OUTSIDE the parent's spread by {100 * worst:.2f} %"))
        L.append("  verdict: " + ("every line within the parent's own run-to-run spread" if ok else "NOT every line within the parent's own run-to-run spread"))
        L.append("")
    w = run([sys.executable, os.path.abspath(__file__), "--child", "rot"] + tail, ROOT)
    L.append("Writer shape (10 000 particles, n_grid 64, 19 substeps): rot_state handle with action_dim 6 against the constant-orientation Capsule, one process")
    L.append("  B  call            constant orientation                      rotating                                  substeps/s const / rot     rot / const time")
    for B in (1, 8):
        for kind in ("fwd", "fwd_loss_bwd"):
            a, b = w[f"B{B}_const_{kind}"], w[f"B{B}_rot_{kind}"]
            f = lambda t: f"{t['median']:8.3f} ms ({t['lo']:.3f}..{t['hi']:.3f})"
            L.append(f"  {B:1d}  {kind:14s}  {f(a):40s}  {f(b):40s}  {a['substeps_per_s']:9.0f} / {b['substeps_per_s']:9.0f}   {b['median'] / a['median']:6.3f}")
    L.append("")
    outdir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(outdir, exist_ok=True)
    tc, tr = trace("trace_const", args, outdir), trace("trace_rot", args, outdir)
    L.append("kernel time of five forward + loss + adjoint step calls at B = 8 (rocprofv3 kernel trace, one run per handle) [us per step call]")
    import re
    pair = lambda k: re.sub(r"<(true|false|1|2)>$", "", k.replace("_rot", "")) if not re.search(r"p2g|g2p", k) else k
    names = sorted(set(pair(k) for k in list(tc) + list(tr)))
    for n in names:
        c = sum(v for k, v in tc.items() if pair(k) == n) / 5e3
        r = sum(v for k, v in tr.items() if pair(k) == n) / 5e3
        L.append(f"  {n:28s} constant {c:10.1f}   rotating {r:10.1f}   {r - c:+9.1f}")
    L.append(f"  {'sum':28s} constant {sum(tc.values()) / 5e3:10.1f}   rotating {sum(tr.values()) / 5e3:10.1f}   {(sum(tr.values()) - sum(tc.values())) / 5e3:+9.1f}")
    text = "\n".join(L) + "\n"
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
