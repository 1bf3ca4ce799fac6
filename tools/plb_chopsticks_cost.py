#!/usr/bin/env python
"""What the Chopsticks primitive costs on the PLB f64 path, and whether the handles that existed before it still run at their speed.

    python tools/plb_chopsticks_cost.py [--parent-tree PATH] [--repeats 25] [--warmup 5] [--rounds 3] [--out profiles/plb_chopsticks_cost.txt]

  chopsticks  the Writer shape (WriterConf: 10 000 particles, n_grid 64, 19 substeps) on rot_state with a Chopsticks in the Capsule's place,
              B = 1 and 8, forward and forward + loss + adjoint: the rotating Capsule with six action dimensions against the Chopsticks
              with seven.  The two handles of a block live in one process and are timed in turn, call by call, so that drift hits them alike;
              median (min..max) of `--repeats` calls per handle after `--warmup` untimed ones, device events, and the ratio to the Capsule.
              No bar is set for it: nobody has measured a Chopsticks before.
  existing    with --parent-tree (a checkout of the parent commit with its library built): tools/plb_shape_cost.py's `shapes` child on both
              trees, alternating processes, `--rounds` each; of its lines the Writer's Capsule and the Torus with a constant orientation and
              the rotating Box are reported.  Those handles run the instruction streams they ran before, so the condition is: this tree's
              median over its processes lies within the spread (least .. largest process median) the parent shows in the same session.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXISTING = (("const", "capsule"), ("const", "torus"), ("rot", "box"))


def make(chop, B):
    import torch
    from unidom_amd.engine.plb_simulator import PlbSimulator, WriterConf
    cfg = WriterConf()
    cfg.rot_state, cfg.action_scale_w = True, (0.05, 0.05, 0.05)
    if chop:          # the reference's primitive defaults: two sticks of the Capsule's size, opened to 0.1, closing
        cfg.prim_kind, cfg.action_dim, cfg.prim_min_gap, cfg.prim_init_gap, cfg.action_scale_gap = (6,), 7, (0.06,), (0.1,), 0.01
    else:
        cfg.action_dim = 6
    sim = PlbSimulator(cfg, batch_size=B)
    assert sim.launch_plan() == 1 and sim.chopsticks == chop
    st = sim.reset()
    a = [0.3, -0.5, 0.2, 0.3, -0.2, 0.25] + ([0.5] if chop else [])
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
        handles = [(name,) + make(chop, B) for name, chop in (("capsule6", False), ("chopsticks7", True))]
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
            for name, _, _ in handles:
                out[f"B{B}_{call}_{name}"] = dict(median=statistics.median(ms[name]), lo=min(ms[name]), hi=max(ms[name]))
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plb_chopsticks_cost.txt"))
    args = ap.parse_args()
    assert args.repeats >= 20
    if args.child:
        return child(args)
    tail = ["--repeats", str(args.repeats), "--warmup", str(args.warmup)]
    L = ["PLB f64 path, Chopsticks primitive: cost on one MI355X; tools/plb_chopsticks_cost.py",
         f"median (min..max) of {args.repeats} calls after {args.warmup} warm-up calls, device events", ""]
    if args.parent_tree:
        trees = (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT))
        series = {who: [] for who, _ in trees}
        for i in range(args.rounds):
            for who, tree in trees:
                series[who].append(run([sys.executable, os.path.join(tree, "tools", "plb_shape_cost.py"), "--child", "shapes"] + tail, tree))
                print(f"existing: round {i} of {who} done", flush=True)
        L.append(f"existing handles (Writer shape), {args.rounds} processes per tree, parent and this tree alternating: median per process [ms per step call];")
        L.append("spread = least .. largest process median of the parent in this session")
        ok = True
        for B in (1, 8):
            for mode, name in EXISTING:
                for call in ("fwd", "fwd_loss_bwd"):
                    key = f"B{B}_{mode}_{call}_{name}"
                    pm, tm = [r[key]["median"] for r in series["parent"]], [r[key]["median"] for r in series["this"]]
                    lo, hi, mid = min(pm), max(pm), statistics.median(tm)
                    inside = lo <= mid <= hi
                    ok = ok and inside
                    L.append(f"  {key:30s} parent " + " ".join(f"{v:8.3f}" for v in pm) + "   this " + " ".join(f"{v:8.3f}" for v in tm) +
                             f"   spread {lo:.3f}..{hi:.3f} ({100 * (hi / lo - 1):.2f} %); median of this tree's {mid:.3f} " +
                             ("within it" if inside else f"OUTSIDE it by {100 * max(mid / hi - 1, 1 - mid / lo):.2f} %") +
                             f" ({100 * (mid / statistics.median(pm) - 1):+.2f} % of the parent's median)")
        L.append("  verdict: " + ("every line within the parent's own run-to-run spread" if ok else "NOT every line within the parent's own run-to-run spread"))
    else:
        L.append("existing handles against the parent: not measured in this run (no --parent-tree)")
    L.append("")
    w = run([sys.executable, os.path.abspath(__file__), "--child", "chopsticks"] + tail, ROOT)
    L.append("Writer shape (10 000 particles, n_grid 64, 19 substeps) on rot_state: the rotating Capsule (six action dimensions) and a Chopsticks in its")
    L.append("place (seven), the two handles of a block timed in turn in one process [ms per step call]")
    L.append("  B  call            capsule, 6 dims                   chopsticks, 7 dims                ratio")
    for B in (1, 8):
        for call in ("fwd", "fwd_loss_bwd"):
            t = [w[f"B{B}_{call}_{name}"] for name in ("capsule6", "chopsticks7")]
            f = lambda r: f"{r['median']:8.3f} ({r['lo']:.3f}..{r['hi']:.3f})"
            L.append(f"  {B:1d}  {call:14s}  " + "".join(f"{f(r):34s}" for r in t) + f"{t[1]['median'] / t[0]['median']:6.3f}")
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
