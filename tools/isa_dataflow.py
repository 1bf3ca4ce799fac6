"""Dataflow of one pass through a loop of a hipcc -save-temps .s file, freed of registers and schedule: every value the pass leaves
behind (LDS / global stores, registers that are live around the loop) as an expression DAG over the values it found on entry,
printed in a canonical SSA form.  Floating-point structure is kept exactly (which products are fused into an fma, which are
rounded first, the association of every sum; operands of commutative ops are sorted), so two builds of one source round alike
iff their listings agree up to the names of the entry values -- the check behind the explicit roundings of cloth_fast_bwd.hip.

Branches are not followed: the blocks of the loop are walked in file order, --skip drops blocks (the side of a branch that is not
wanted), exec masks are ignored (a value written under a mask is the value of the lanes that run the block).
usage: python tools/isa_dataflow.py file.s kernel_substring [--header BB1_47] [--skip BB1_54,BB1_62] [--shape]
  --shape   print one line per sink with a hash of its expression in which entry values count only by kind (for diffing builds)"""
import argparse
import hashlib
import re
import sys

ap = argparse.ArgumentParser()
ap.add_argument("path"); ap.add_argument("kernel")
ap.add_argument("--header", default=None); ap.add_argument("--skip", default="")
ap.add_argument("--shape", action="store_true")
args = ap.parse_args()

lines = open(args.path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and args.kernel in l and ":" in l)
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
blocks, cur = [], None
for l in lines[start:end]:
    t = l.strip()
    m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)", t)
    if m:
        cur = {"label": m.group(1) or "bb." + m.group(2), "hdr": None, "ins": []}
        h = re.search(r"Header=(BB\d+_\d+)", t)
        if h:
            cur["hdr"] = h.group(1)
        blocks.append(cur)
        continue
    if cur is None or not t or t.startswith("."):
        continue
    if t.startswith(";"):
        h = re.search(r"Header=(BB\d+_\d+)", t)
        if h and not cur["ins"]:
            cur["hdr"] = h.group(1)
        if "Loop Header" in t and not cur["ins"]:
            cur["hdr"] = cur["label"]
        continue
    cur["ins"].append(t.split(";")[0].strip())
if args.header is None:
    from collections import Counter
    c = Counter()
    for b in blocks:
        if b["hdr"]:
            c[b["hdr"]] += len(b["ins"])
    args.header = c.most_common(1)[0][0]
# the loop = from its header to the last block that names it (blocks in between without the comment, e.g. %Flow, belong to it too)
idx = [i for i, b in enumerate(blocks) if b["hdr"] == args.header]
skip = set(filter(None, args.skip.split(",")))
loop = [b for b in blocks[idx[0]:idx[-1] + 1] if b["label"] not in skip]

# ---- expressions (hash-consed tuples) ----
COMM = {"add", "mul"}


def mk(op, *a):
    if op in COMM:
        a = tuple(sorted(a, key=repr))
    if op == "fma":
        a = tuple(sorted(a[:2], key=repr)) + (a[2],)
    if op == "neg" and isinstance(a[0], tuple) and a[0][0] == "neg":
        return a[0][1]
    return (op,) + tuple(a)


reg = {}
read_first, written = set(), set()


def rd(r):
    if r not in reg:
        if r not in written:
            read_first.add(r)
        reg[r] = ("in", r)
    return reg[r]


def wr(r, e):
    written.add(r)
    reg[r] = e


def split_ops(s):
    out, depth, cur_ = [], 0, ""
    for ch in s:
        if ch in "[(":
            depth += 1
        if ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur_.strip()); cur_ = ""
        else:
            cur_ += ch
    if cur_.strip():
        out.append(cur_.strip())
    mods = {}
    if out:
        toks, depth, cur_ = [], 0, ""
        for ch in out[-1]:
            if ch in "[(":
                depth += 1
            if ch in "])":
                depth -= 1
            if ch == " " and depth == 0:
                if cur_:
                    toks.append(cur_)
                cur_ = ""
            else:
                cur_ += ch
        if cur_:
            toks.append(cur_)
        out[-1] = toks[0]
        for m_ in toks[1:]:
            k, _, v = m_.partition(":")
            mods[k] = v if v else True
    return out, mods


def regs_of(o):
    """register names an operand covers, [] for literals"""
    o = o.lstrip("-").strip("|")
    m = re.match(r"^([vsa])\[(\d+):(\d+)\]$", o)
    if m:
        return [f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    if re.match(r"^[vsa]\d+$", o):
        return [o]
    if o in ("vcc", "exec", "scc", "m0", "vcc_lo", "vcc_hi"):
        return [o]
    return []


def val(o, half=None):
    """expression of a 32-bit source operand (half: element of a register pair)"""
    neg = o.startswith("-")
    if neg:
        o = o[1:]
    ab = o.startswith("|")
    o = o.strip("|")
    rs = regs_of(o)
    if rs:
        e = rd(rs[half if (half is not None and len(rs) > 1) else 0]) if not (len(rs) > 1 and half is None) else tuple(["cat"] + [rd(r) for r in rs])
    else:
        e = ("c", o)
    if ab:
        e = mk("abs", e)
    if neg:
        e = mk("neg", e)
    return e


def bits(s, n, default):
    if s is None:
        return [default] * n
    v = [int(x) for x in s.strip("[]").split(",")]
    return v + [default] * (n - len(v))


sinks = []
nload = [0]


def run(ins):
    mn, _, rest = ins.partition(" ")
    ops, mods = split_ops(rest.strip())
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", mn)
    if base in ("s_nop", "s_waitcnt", "s_barrier", "s_branch") or base.startswith("s_cbranch"):
        return
    if base in ("s_and_saveexec_b64", "s_or_saveexec_b64"):
        for r in regs_of(ops[0]):
            wr(r, ("exec_save",))
        return
    if ops and regs_of(ops[0]) == ["exec"]:
        return
    f2 = {"v_add_f32": "add", "v_mul_f32": "mul", "v_max_f32": "max", "v_min_f32": "min"}
    if base in f2 or base in ("v_sub_f32", "v_subrev_f32"):
        a, b = val(ops[1]), val(ops[2])
        if "quad_perm" in mods or any(k.startswith("row_") and k not in ("row_mask",) for k in mods):
            ctrl = ",".join(f"{k}:{v}" for k, v in sorted(mods.items()) if k not in ("row_mask", "bank_mask", "bound_ctrl"))
            a = ("dpp", ctrl, a)
        if base == "v_sub_f32":
            e = mk("add", a, mk("neg", b))
        elif base == "v_subrev_f32":
            e = mk("add", b, mk("neg", a))
        else:
            e = mk(f2[base], a, b)
        wr(regs_of(ops[0])[0], e)
        return
    if base == "v_fmac_f32":
        d = regs_of(ops[0])[0]
        wr(d, mk("fma", val(ops[1]), val(ops[2]), rd(d)))
        return
    if base == "v_fma_f32":
        wr(regs_of(ops[0])[0], mk("fma", val(ops[1]), val(ops[2]), val(ops[3])))
        return
    if base in ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32"):
        n = 3 if base == "v_pk_fma_f32" else 2
        sel, selh = bits(mods.get("op_sel"), 3, 0), bits(mods.get("op_sel_hi"), 3, 1)
        nl, nh = bits(mods.get("neg_lo"), 3, 0), bits(mods.get("neg_hi"), 3, 0)
        res = []
        for h, (s_, ng) in enumerate(((sel, nl), (selh, nh))):
            src = []
            for q in range(n):
                e = val(ops[1 + q], s_[q])
                src.append(mk("neg", e) if ng[q] else e)
            res.append(mk("mul", *src) if base == "v_pk_mul_f32" else mk("add", *src) if base == "v_pk_add_f32" else mk("fma", *src))
        d = regs_of(ops[0])
        wr(d[0], res[0]); wr(d[1], res[1])
        return
    if base in ("v_mov_b32", "s_mov_b32") and not any(k in mods for k in ("quad_perm", "row_bcast", "row_shr", "row_ror", "row_mirror", "row_half_mirror")):
        wr(regs_of(ops[0])[0], val(ops[1]))
        return
    if base == "s_mov_b64":
        d, s_ = regs_of(ops[0]), regs_of(ops[1])
        for q, r in enumerate(d):
            wr(r, rd(s_[q]) if len(s_) > q else ("c", ops[1]))
        return
    if base == "v_cndmask_b32":
        cond = val(ops[3]) if len(ops) > 3 else rd("vcc")
        wr(regs_of(ops[0])[0], ("sel", cond, val(ops[2]), val(ops[1])))   # cond ? src1 : src0
        return
    if base.startswith("v_cmp_"):
        if mn.endswith("_e64"):
            d, a = regs_of(ops[0]), ops[1:]
        else:
            d, a = ["vcc"], ops[1:] if regs_of(ops[0]) == ["vcc"] else ops
        e = (base,) + tuple(val(o) for o in a)
        for r in d:
            wr(r, e)
        return
    if base.startswith("v_permlane") and base.endswith("swap_b32"):
        a, b = regs_of(ops[0])[0], regs_of(ops[1])[0]
        ea, eb = rd(a), rd(b)
        wr(a, (base + ".0", ea, eb)); wr(b, (base + ".1", ea, eb))
        return
    if base.startswith("ds_write") or base.startswith("global_store"):
        sinks.append((base + " " + " ".join(f"{k}:{v}" for k, v in sorted(mods.items())), tuple(val(o) for o in ops)))
        return
    # generic: first operand is the destination, the rest are sources; loads get a serial number (memory is not modelled)
    d = regs_of(ops[0]) if ops else []
    srcs = tuple(val(o) for o in ops[1:] if o != "off")
    tag = base + "".join(f" {k}:{v}" for k, v in sorted(mods.items()) if k not in ("row_mask", "bank_mask"))
    if base in ("v_mov_b32",):   # dpp move: the old value of the destination is an input
        srcs = (rd(d[0]),) + srcs
    if base.startswith(("global_load", "s_load", "ds_read")):
        nload[0] += 1
    if base.startswith("s_") and not base.startswith("s_load"):
        for r in ("scc",):
            wr(r, (tag + ".scc",) + srcs)
    for q, r in enumerate(d):
        wr(r, (tag + (f".{q}" if len(d) > 1 else ""),) + srcs)


for b in loop:
    for ins in b["ins"]:
        run(ins)

carried = sorted(read_first & written, key=lambda r: (r[0], int(r[1:]) if r[1:].isdigit() else -1))
names, order = {}, []


def ssa(e):
    if not isinstance(e, tuple):
        return str(e)
    if e[0] == "in":
        return e[1]
    if e[0] == "c":
        return "#" + e[1]
    if e in names:
        return names[e]
    a = [ssa(x) for x in e[1:]]
    names[e] = f"t{len(names)}"
    order.append(f"{names[e]} = {e[0]}({', '.join(a)})")
    return names[e]


FLOAT_OPS = {"add", "mul", "fma", "neg", "abs", "max", "min", "sel", "dpp", "v_rsq_f32", "v_readlane_b32"}


def shape(e, memo={}):
    """hash of the floating-point structure: entry values, constants, loads and integer arithmetic are all one kind of leaf, a
    select counts by its two values (not by its condition, which the builds may express differently)"""
    if not isinstance(e, tuple) or not (e[0] in FLOAT_OPS or e[0].startswith(("v_permlane", "v_mov_b32"))):
        return "L"
    if e not in memo:
        kids = [shape(x) for x in (e[2:] if e[0] in ("sel", "dpp") else e[1:])]
        if e[0] in COMM or e[0] == "sel":
            kids.sort()
        if e[0] == "fma":
            kids = sorted(kids[:2]) + kids[2:]
        memo[e] = hashlib.md5((e[0] + "(" + ",".join(kids) + ")").encode()).hexdigest()[:10]
    return memo[e]


sys.setrecursionlimit(100000)
print(f"# loop {args.header}: blocks {[b['label'] for b in loop]}")
print(f"# carried registers: {carried}")
out = []
for what, a in sinks:
    out.append((what, a))
for r in carried:
    out.append((f"carry {r}", (reg[r],)))
for what, a in out:
    if args.shape:
        print(what.split()[0], shape(a[-1]))
    else:
        n0 = len(order)
        refs = [ssa(x) for x in a]
        for l in order[n0:]:
            print("    " + l)
        print(f"{what} <- {', '.join(refs)}")
