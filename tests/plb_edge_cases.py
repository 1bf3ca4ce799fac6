"""Shared by tests/test_plb_edge_cases.py (CPU, the twin alone) and tests/test_plb_edges_gpu.py (a plain module, no fixtures): the inputs that
put the PLB persistent kernels (csrc/plb_cluster.hip), the multi-kernel adjoint (csrc/plb_adj.hip) and the loss kernels at the shapes and
branches the rest of the suite never reaches, and their reference, torch.autograd through oracle/twin/plb_twin_torch.py (f64, dense grid).

A step case is the tuple of tests/test_plb.py::_small_case (x, v, C, F, prim, soft, act, E, nu, ys) plus seeded cotangents of the five step
outputs (an entry may be None: that output takes no part in the loss) and the conf fields that differ from the Torus conf: n_particles,
substeps, upper_bound, lower_bound.  Every step case runs at quality 0.5: n_grid 32, dt 2e-4.

    body        a box on the floor whose size follows N (the density of _small_case's 300 particles), falling at 0.8: the lowest cells take the
                ground-friction branch
    sphere 0    within 0.004 of a particle of the body: sticky contact, so the action carries a cotangent (the cells take (pos1 - pos) / dt:
                the +-1 / dt of the two positions cancel along a free axis, and the start position keeps the cotangent of prim_pos alone)
    envs        E, nu drawn per env; yield stress cycles (1762.2, 30, 200), +-10 % beyond three envs: env 1 yields almost everywhere, env 0 hardly
    actions     _small_case's range times S / 9 (the same travel per substep); above 9 substeps the clip at +-1 caps it, there 0.3 of the range
                keeps the sphere inside the cube over the whole step

Step cases, by tag:
    n{N}_b{B}_s{S}   plain: part sizes (one part, a last part of one particle, full last parts), ring residues (S = 1, 2: the ring of three
                     exchange grids has not wrapped), the PCL_SMAX = 128 boundary on both sides, 19 envs (a call cut into launches; the twin
                     follows PICK_LAUNCHES), the largest persistent body and the first one past it
    clip             N = 37, B = 3, S = 3; raw action 1.7 in env 0's x and -1.3 in env 1's z (strictly beyond the clip: its cotangent is exactly
                     0), bounds widened to +-3 so that the primitive is free to travel the clipped distance; in these two envs sphere 0 holds
                     one node at the body's fringe (`_fringe_node`)
    bound            primitive 0 starts ON its upper bound in x (upper_bound[0] inside the body) and its x action pushes outward: pos + pv > hi
                     strictly in every substep, the trajectory stays on the bound and passes nothing on, nothing to action x; the cells take
                     (hi - pos) / dt, which substep 0 books to the start position
    xclamp           particle XCLAMP_P of every env starts within 1e-5 of 1 - 3 dx with velocity 8 outward: its new x is the bound in every
                     substep, and the cotangent of its x reaches the inputs through g2p alone
    only_prim, only_F   the plain N = 37 inputs with a loss on prim_pos alone / on F alone: the other output cotangents are absent.  only_prim
                     reaches no leaf but prim_pos and the action (structural zeros: `zero`); only_F leaves prim_pos a zero by cancellation (`cancel`)
No input sits on an exact tie of a clamp (torch.minimum / maximum split the cotangent there, the kernels pass it): asserted by
tests/test_plb_edge_cases.py on `trajectory`.

Loss cases (ud_plb_loss_fwd / bwd on the sphere handle, n_grid 32, B = 3, g_loss = LOSS_GL with one exact 0): see `loss_case`."""
import zlib
from typing import NamedTuple, Optional

import numpy as np

from oracle.twin.plb_twin import PlbConf

QUALITY = 0.5
N_GRID, DT = 32, 2e-4
X_MAX = 1.0 - 3.0 / N_GRID                  # the upper position clamp, 0.90625: exact in binary
LEAVES = ("x", "v", "C", "F", "prim", "act", "E", "nu", "ys", "fric")
PICK_LAUNCHES = (0, 7, 8, 15, 16, 18)       # first and last env of a launch of 8, of a launch of 16, and of the rest
XCLAMP_P = 5
LOSS_GL = (1.0, 0.0, -2.5)

PART_SIZES = (1, 5, 32, 33, 37, 64)
PART_TAGS = tuple(f"n{N}_b3_s3" for N in PART_SIZES)
RING_TAGS = tuple(f"n37_b3_s{S}" for S in (1, 2, 3, 4))
SMAX_TAGS = ("n33_b2_s128", "n33_b2_s129")
LAUNCH_TAG = "n1000_b19_s2"
LARGEST_TAGS = ("n1024_b2_s2", "n1025_b2_s2")
CLAMP_TAGS = ("clip", "bound", "xclamp", "only_prim", "only_F")
STEP_TAGS = tuple(dict.fromkeys(PART_TAGS + RING_TAGS + SMAX_TAGS + (LAUNCH_TAG,) + LARGEST_TAGS + CLAMP_TAGS))


class StepCase(NamedTuple):
    tag: str
    N: int
    B: int
    S: int
    conf_kw: dict                 # upper_bound / lower_bound where they differ
    inputs: tuple                 # x, v, C, F, prim, soft, act, E, nu, ys
    w: tuple                      # cotangents of (x, v, C, F, prim_pos) out; None = absent
    zero: tuple                   # leaves whose gradient is structurally zero: both sides must give exactly 0
    cancel: tuple                 # leaves whose gradient is zero by cancellation (see CANCEL_BAR): exactly 0 in the twin, round-off in the kernels
    pick: Optional[tuple]         # the envs the twin follows (None = all)


_CASES, _TWIN, _LOSS = {}, {}, {}


def CANCEL_BAR(case, grads):
    """A sticky sphere hands its cells (pos[s + 1] - pos[s]) / dt, so substep s books a sum G_s to pos[s + 1] and -G_s to pos[s]; along a free axis
    pos[s + 1] = pos[s] + pv passes G_s on and the two cancel: with no cotangent on prim_pos itself the start position receives exactly 0 from
    autograd, which adds and subtracts the same number.  The kernels collect +G_s and -G_s with atomics from several waves, in an order of their
    own for each: what is left is the round-off of sums of size |G_s|, and sum_s G_s / S is the action's gradient.  The bar is the adjoint
    tolerance, 1e-6, of S max |g_action|."""
    return 1e-6 * case.S * np.abs(grads["act"]).max()


def _rng(tag):
    return np.random.default_rng(zlib.crc32(f"plb_edges/{tag}".encode()))


def _plain(tag, N, B, S):
    rng = _rng(tag)
    k = min(1.0, (N / 300.0) ** (1.0 / 3.0))
    side, height = max(0.25 * k, 0.04), max(0.12 * k, 0.03)
    x = rng.uniform(size=(B, N, 3)) * np.array([side, height, side]) + np.array([0.5 - side / 2, 0.035, 0.5 - side / 2])
    v = rng.normal(size=(B, N, 3)) * 0.3 + np.array([0.0, -0.8, 0.0])
    Cm = rng.normal(size=(B, N, 3, 3)) * 2.0
    F = np.eye(3)[None, None] + rng.normal(size=(B, N, 3, 3)) * 0.12
    prim = np.stack([x[:, N // 2] + rng.normal(size=(B, 3)) * 0.004, np.array([0.2, 0.7, 0.2]) + rng.normal(size=(B, 3)) * 0.01], 1)
    soft = np.full((B, 2), 666.0)
    act = rng.uniform(-0.9, 0.9, size=(B, 3)) * np.array([1.0, 0.3, 1.0]) * (S / 9.0 if S <= 9 else 0.3)
    E = rng.uniform(3e3, 6e3, size=B)
    nu = rng.uniform(0.25, 0.4, size=B)
    ys = np.array([1762.2, 30.0, 200.0])[np.arange(B) % 3]
    if B > 3:
        ys = ys * rng.uniform(0.9, 1.1, size=B)                # every env its own
    w = tuple(rng.normal(size=s) for s in ((B, N, 3), (B, N, 3), (B, N, 3, 3), (B, N, 3, 3), (B, 2, 3)))
    return [x, v, Cm, F, prim, soft, act, E, nu, ys], w


def _fringe_node(x):
    """The clipped sphere crosses 1 / S of the cube per substep: the cells it holds take 1 / (3 dt) = 1667.  Held at the body's heart that tears
    the body apart within the step (velocities of 1e7, cotangents of 1e14 -- the twin's own prim_pos gradient, (w + G) - G, is then w rounded to
    an ulp of G: percents).  So the sphere sits ON a grid node (its reach, 0.0285, is below dx: it holds that node alone) at the body's fringe:
    an occupied node on which no particle puts more than 0.4 % of its mass -- the largest such share >= 0.05 %.  -> the node's index [3]"""
    base = (x * N_GRID - 0.5).astype(np.int64)
    fx = x * N_GRID - base
    w = np.stack([0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1) ** 2, 0.5 * (fx - 0.5) ** 2])            # [3 offsets, N, 3 axes]
    top = {}
    for i in range(3):
        for j in range(3):
            for k in range(3):
                share = w[i, :, 0] * w[j, :, 1] * w[k, :, 2]
                for p, node in enumerate(map(tuple, base + np.array([i, j, k]))):
                    top[node] = max(top.get(node, 0.0), share[p])
    ok = {node: t for node, t in top.items() if 5e-4 <= t <= 4e-3}
    return np.array(max(ok, key=ok.get), np.float64)


def step_case(tag) -> StepCase:
    """the same arrays whenever it is asked again"""
    if tag in _CASES:
        return _CASES[tag]
    kw, zero, cancel, pick = {}, (), (), None
    if tag.startswith("n"):
        N, B, S = (int(t[1:]) for t in tag.split("_"))
        ins, w = _plain(tag, N, B, S)
        if tag == LAUNCH_TAG:
            pick = PICK_LAUNCHES
    else:
        N, B, S = 37, 3, 3
        ins, w = _plain("n37_b3_s3" if tag.startswith("only_") else tag, N, B, S)
        x, v, Cm, F, prim, soft, act, E, nu, ys = ins
        if tag == "clip":
            act[0, 0], act[1, 2] = 1.7, -1.3
            kw = dict(upper_bound=(3.0, 3.0, 3.0), lower_bound=(-3.0, -3.0, -3.0))
            for b in (0, 1):
                prim[b, 0] = _fringe_node(x[b]) / N_GRID + np.array([0.001, 0.0007, -0.0005])
        elif tag == "bound":
            hi = 0.47
            prim[:, 0, 0] = hi
            x[:, N // 2, 0] = hi - 0.003                       # the body's particle stays beside the sphere
            act[:, 0] = np.array([0.25, 0.12, 0.2])            # outward, inside the clip
            kw = dict(upper_bound=(hi, 1.0, 1.0))
        elif tag == "xclamp":
            x[:, XCLAMP_P, 0] = X_MAX - 1e-5 * np.array([0.9, 0.5, 0.2])
            v[:, XCLAMP_P, 0] = 8.0
            Cm[:, XCLAMP_P] = 0.0
            # alone out there, its own stress is all that acts on it: a mild strain with well separated singular values
            F[:, XCLAMP_P] = np.diag([1.03, 0.98, 1.01]) + (F[:, XCLAMP_P] - np.eye(3)) * 0.04
        elif tag == "only_prim":
            w = (None, None, None, None, w[4])
            zero = ("x", "v", "C", "F", "E", "nu", "ys", "fric")   # the trajectory depends on prim_pos and the action alone
        elif tag == "only_F":
            w = (None, None, None, w[3], None)
            cancel = ("prim",)
        else:
            raise KeyError(tag)
    _CASES[tag] = StepCase(tag, N, B, S, kw, tuple(ins), tuple(w), zero, cancel, pick)
    return _CASES[tag]


def twin_conf(case):
    class Short(PlbConf):
        substeps = case.S
    conf = Short(quality=QUALITY, n_particles=case.N, **case.conf_kw)
    assert (conf.n_grid, conf.substeps) == (N_GRID, case.S) and abs(conf.dt - DT) < 1e-18
    return conf


def trajectory(case):
    """-> (pos [B, S + 1, 2, 3], un [B, S, 2, 3]): the primitive trajectory and pos + pv before the bound clamp, as PlbTorchTwin.step forms them"""
    prim, act = case.inputs[4], case.inputs[6]
    conf = twin_conf(case)
    lo, hi = np.array(conf.lower_bound), np.array(conf.upper_bound)
    pv = np.zeros_like(prim)
    pv[:, 0] = np.clip(act, -1, 1) / case.S
    pos, un = [prim.copy()], []
    for _ in range(case.S):
        un.append(pos[-1] + pv)
        pos.append(np.maximum(np.minimum(un[-1], hi), lo))
    return np.stack(pos, 1), np.stack(un, 1)


def twin_step(case, perm=None, w=None):
    """The twin's step and its autograd for `case` (its picked envs) -> (outputs [5], {leaf: gradient}); a leaf the loss does not reach gives zeros.
    perm: the particles enter in that order (another summation order on the grid) and every per-particle result comes back un-permuted.
    Without perm / w the result is computed once and kept: nobody may write into it."""
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    keep = perm is None and w is None
    if keep and case.tag in _TWIN:
        return _TWIN[case.tag]
    torch.set_num_threads(8)
    w = case.w if w is None else w
    ins = list(case.inputs)
    if case.pick is not None:
        sel = list(case.pick)
        ins = [np.ascontiguousarray(a[sel]) for a in ins]
        w = [None if wi is None else np.ascontiguousarray(wi[sel]) for wi in w]
    if perm is not None:
        ins[:4] = [np.ascontiguousarray(a[:, perm]) for a in ins[:4]]
        w = [wi if (wi is None or i == 4) else np.ascontiguousarray(wi[:, perm]) for i, wi in enumerate(w)]
    x, v, Cm, F, prim, soft, act, E, nu, ys = ins
    conf = twin_conf(case)
    T = lambda a, r=True: torch.tensor(np.asarray(a, np.float64), requires_grad=r)
    L = dict(x=T(x), v=T(v), C=T(Cm), F=T(F), prim=T(prim), act=T(act), E=T(E), nu=T(nu), ys=T(ys), fric=T(np.full(len(E), conf.ground_friction)))
    out = PlbTorchTwin(conf).step(L["x"], L["v"], L["C"], L["F"], L["prim"], L["act"], T(soft, False), L["E"], L["nu"], L["ys"], L["fric"])
    sum((o * torch.tensor(wi)).sum() for o, wi in zip(out, w) if wi is not None).backward()
    outs = [o.detach().numpy().copy() for o in out]
    grads = {k: (np.zeros(t.shape) if t.grad is None else t.grad.numpy().copy()) for k, t in L.items()}
    if perm is not None:
        inv = np.argsort(perm)
        outs[:4] = [o[:, inv] for o in outs[:4]]
        for k in ("x", "v", "C", "F"):
            grads[k] = grads[k][:, inv]
    if keep:
        for a in outs + list(grads.values()):
            a.setflags(write=False)
        _TWIN[case.tag] = (outs, grads)
    return outs, grads


# -- losses ----------------------------------------------------------------------------------------------------------------------------
class LossCase(NamedTuple):
    tag: str
    N: int
    soft: bool
    x: np.ndarray                 # [3, N, 3]
    prim: np.ndarray              # [3, 2, 3]
    target_density: np.ndarray    # [n_grid^3]: the twin's grid mass of another cloud
    target_sdf: np.ndarray        # [n_grid^3]: random
    weights: tuple                # (contact, density, sdf)
    zero: tuple                   # "prim" where the contact gradient is structurally zero
    inside: tuple                 # (env, particle, sphere) of the particles put inside a sphere


LOSS_TAGS = tuple(f"n{N}_{c}" for N in (1, 255, 256, 257) for c in ("soft", "hard")) + \
    ("inside0_soft", "inside0_hard", "insideboth_hard", "sdfonly_soft", "sdfonly_hard")


def loss_case(tag) -> LossCase:
    """n{N}_{soft|hard}    N = 1 (the soft normaliser is one term), 255 / 256 / 257 (a ragged last block, a full one, a block of one thread);
                           every particle outside both spheres, the hard minimum unique and positive
    inside0_*              N = 257, one particle of every env inside sphere 0: raw <= 0 passes no gradient; hard: sphere 0's minimum is 0
    insideboth_hard        a particle inside each sphere: the contact is 0 and its gradient exactly 0
    sdfonly_*              weights (0, 0, 1.3): neither contact nor density reach the gradient"""
    if tag in _LOSS:
        return _LOSS[tag]
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    kind, contact = tag.split("_")
    N = int(kind[1:]) if kind[0] == "n" else 257
    B = 3
    rng = _rng("loss/" + kind)
    x = rng.uniform(0.35, 0.65, size=(B, N, 3))
    prim = np.stack([np.array([0.5, 0.74, 0.5]) + rng.normal(size=(B, 3)) * 0.01, np.array([0.26, 0.5, 0.5]) + rng.normal(size=(B, 3)) * 0.01], 1)
    weights, zero, inside = (3.0, 0.7, 1.3), (), ()
    if kind in ("inside0", "insideboth"):
        inside = tuple((b, 100 + b, 0) for b in range(B))
        if kind == "insideboth":
            inside += tuple((b, 30 + b, 1) for b in range(B))
            zero = ("prim",)
        for b, p, pi in inside:
            u = rng.normal(size=3)
            x[b, p] = prim[b, pi] + 0.012 * u / np.linalg.norm(u)          # radius 0.025
    elif kind == "sdfonly":
        weights, zero = (0.0, 0.0, 1.3), ("prim",)
    conf = PlbConf(quality=QUALITY, n_particles=N)
    other = rng.uniform(0.36, 0.66, size=(1, max(N, 64), 3))
    td = PlbTorchTwin(conf).grid_mass(torch.tensor(other))[0].numpy().copy()
    ts = rng.normal(size=conf.n_grid ** 3)
    _LOSS[tag] = LossCase(tag, N, contact == "soft", x, prim, td, ts, weights, zero, inside)
    return _LOSS[tag]


def twin_loss(case, perm=None):
    """-> (loss [3], parts [3, 3], g_x, g_prim) of the twin with g_loss = LOSS_GL"""
    import torch
    from oracle.twin.plb_twin_torch import PlbTorchTwin
    x = case.x if perm is None else np.ascontiguousarray(case.x[:, perm])
    tx, tp = torch.tensor(x, requires_grad=True), torch.tensor(case.prim, requires_grad=True)
    tw = PlbTorchTwin(PlbConf(quality=QUALITY, n_particles=case.N))
    total, parts = tw.loss(tx, tp, torch.tensor(case.target_density), torch.tensor(case.target_sdf), case.weights, soft_contact=case.soft)
    (total * torch.tensor(LOSS_GL, dtype=torch.float64)).sum().backward()
    gx = tx.grad.numpy().copy()
    if perm is not None:
        gx = gx[:, np.argsort(perm)]
    return total.detach().numpy().copy(), parts.detach().numpy().copy(), gx, tp.grad.numpy().copy()


def contact_distances(case):
    """max(|x - prim| - r, 0) per env, sphere, particle [3, 2, N] (with the twin's 1e-14 under the root)"""
    d = case.x[:, None] - case.prim[:, :, None]
    return np.maximum(np.sqrt((d * d).sum(-1) + 1e-14) - 0.025, 0.0)
