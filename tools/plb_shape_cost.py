#!/usr/bin/env python
"""What the Box, Cylinder and Torus primitives cost on the PLB f64 path, and whether the handles that existed before them still run at
their speed.

    python tools/plb_shape_cost.py [--parent-tree PATH] [--repeats 25] [--warmup 5] [--rounds 2] [--out profiles/plb_shape_cost.txt]

  shapes      the Writer shape (WriterConf: 10 000 particles, n_grid 64, 19 substeps) with a Box / Cylinder / Torus in the Capsule's place,
              B = 1 and 8, constant orientation and rot_state with six action dimensions, forward and forward + loss + adjoint.  The four
              handles of a block live in one process and are timed in turn, call by call (Capsule, Box, Cylinder, Torus, Capsule, ...), so
              that drift hits them alike; median (min..max) of `--repeats` calls per handle after `--warmup` untimed ones, device events,
              and the ratio to the Capsule.
  existing    with --parent-tree (a checkout of the parent commit with its library built): tools/plb_writer_cost.py's `writer` and
              `sphere` children on both trees, alternating processes, `--rounds` each -- the existing Capsule / Sphere handles run the
              instruction streams they ran before, so this tree's medians must lie within the spread of the parent's.  Per line: every
              process median of both trees, how many of this tree's lie between the least and the largest of the parent's, and the verdict
              on this tree's median over its processes (of a handful of processes with the same distribution some always fall outside the
              other handful's range, so the count alone says little; give --rounds 5 or more).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("capsule", 1, (0.0, 0.0, 0.0)), ("box", 3, (0.03, 0.06, 0.03)), ("cylinder", 4, (0.03, 0.06, 0.0)), ("torus", 5, (0.045, 0.02, 0.0)))


def shape_cfg(kind, shape, rot):
    """WriterConf with the primitive swapped: sizes close to the Capsule's (radius 0.03, segment 0.06), so the contact reaches about as many cells."""
    from unidom_amd.engine.plb_simulator import WriterConf
    cfg = WriterConf()
    cfg.prim_kind, cfg.prim_shape = (kind,), (shape,)
    if rot:
        cfg.rot_state, cfg.action_dim, cfg.action_scale_w = True, 6, (0.05, 0.05, 0.05)
    return cfg


def make(kind, shape, rot, B):
    import torch
    from unidom_amd.engine.plb_simulator import PlbSimulator
    sim = PlbSimulator(shape_cfg(kind, shape, rot), batch_size=B)
    assert sim.launch_plan() == 1
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

    return sim, {"fwd": fwd, "fwd_loss_bwd": fwd_bwd}


def child(args):
    import torch
    out = {}
    for B in (1, 8):
        for rot in (False, True):
            handles = [(name,) + make(kind, shape, rot, B) for name, kind, shape in SHAPES]
            for call in ("fwd", "fwd_loss_bwd"):
                ms = {name: [] for name, _, _ in handles}
                for it in range(args.warmup + args.repeats):
                    for name, _, fns in handles:                       # in turn, call by call
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fns[call]()
                        b.record()
                        torch.cuda.synchronize()
                        if it >= args.warmup:
                            ms[name].append(a.elapsed_time(b))
                for name, sim, _ in handles:
                    out[f"B{B}_{'rot' if rot else 'const'}_{call}_{name}"] = dict(median=statistics.median(ms[name]), lo=min(ms[name]), hi=max(ms[name]),
                                                                                    substeps=sim.substeps)
            for _, sim, _ in handles:
                sim.check_status()
            del handles
    print("RESULT " + json.dumps(out))


def main():
    from tools.plb_rot_cost import run
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_shape_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20
    if args.child:
        return child(args)
    tail = ["--repeats", str(args.repeats), "--warmup", str(args.warmup)]
    L = ["PLB f64 path, Box / Cylinder / Torus primitives: cost on one MI355X; tools/plb_shape_cost.py",
         f"median (min..max) of {args.repeats} calls after {args.warmup} warm-up calls, device events", ""]
    if args.parent_tree:
        trees = (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT))
        series = {(who, c): [] for who, _ in trees for c in ("writer", "sphere")}
        for _ in range(args.rounds):
            for c in ("writer", "sphere"):
                for who, tree in trees:
                    series[(who, c)].append(run([sys.executable, os.path.join(tree, "tools", "plb_writer_cost.py"), "--child", c] + tail, tree))
                    print(f"existing: {c} of {who} done", flush=True)
        L.append(f"existing handles, {args.rounds} processes per tree, parent and this tree alternating: median per process [ms per step call]")
        ok = True
        for c in ("writer", "sphere"):
            for key in series[("parent", c)][0]:
                pm, tm = [r[key]["median"] for r in series[("parent", c)]], [r[key]["median"] for r in series[("this", c)]]
                lo, hi = min(pm), max(pm)
                n_in = sum(lo <= t <= hi for t in tm)
                mid = statistics.median(tm)
                inside = lo <= mid <= hi
                ok = ok and inside
                L.append(f"  {c:6s} {key:24s} parent " + " ".join(f"{v:8.3f}" for v in pm) + "   this " + " ".join(f"{v:8.3f}" for v in tm) +
                         f"   {n_in} of {len(tm)} inside {lo:.3f}..{hi:.3f}; median of this tree's {mid:.3f} " +
                         ("within the parent's spread" if inside else f"OUTSIDE the parent's spread by {100 * max(mid / hi - 1, 1 - mid / lo):.2f} %") +
                         f" ({100 * (mid / statistics.median(pm) - 1):+.2f} % of the parent's median)")
        L.append("  verdict (this tree's median over its processes against the least and largest of the parent's process medians): " +
                 ("every line within the parent's own run-to-run spread" if ok else "NOT every line within the parent's own run-to-run spread"))
    else:
        L.append("existing handles against the parent: not measured in this run (no --parent-tree)")
    L.append("")
    w = run([sys.executable, os.path.abspath(__file__), "--child", "shapes"] + tail, ROOT)
    L.append("Writer shape (10 000 particles, n_grid 64, 19 substeps), the primitive swapped; the four handles of a block timed in turn in one process [ms per step call]")
    L.append("  B  orientation  call            " + "".join(f"{name:34s}" for name, _, _ in SHAPES) + "ratio to the Capsule (box, cylinder, torus)")
    for B in (1, 8):
        for mode in ("const", "rot"):
            for call in ("fwd", "fwd_loss_bwd"):
                t = [w[f"B{B}_{mode}_{call}_{name}"] for name, _, _ in SHAPES]
                f = lambda r: f"{r['median']:8.3f} ({r['lo']:.3f}..{r['hi']:.3f})"
                L.append(f"  {B:1d}  {mode:11s}  {call:14s}  " + "".join(f"{f(r):34s}" for r in t) + "  ".join(f"{r['median'] / t[0]['median']:6.3f}" for r in t[1:]))
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
