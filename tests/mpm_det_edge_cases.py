"""Shared by tests/test_mpm_det_edge_cases.py (CPU) and tests/test_mpm_det_edges_gpu.py (a plain module, no fixtures): the inputs that put the
deterministic MPM mode (ud_mpm_conf.deterministic: csrc/mpm_det.hip, mpm_det.h, the deterministic branches of mpm_large.hip) at the shapes and
branches tests/test_mpm_det.py never reaches, and their references, each computed once per process and left unchanged:
    checker(tag)       oracle.pyoracle.mpm_det_forward: the mode's own source built for the CPU, f32 -- the forward is compared bit for bit
    oracle_fwd(tag)    MpmOracle.step_fwd, f32: the independent restatement (dense grid)
    oracle_bwd(tag)    MpmOracle.step_bwd in f64 (the adjoint reference) or f32 (what f32 alone costs at these shapes)

Geometry: LegacyConf (n_grid 64, res 32^3, dt 1e-4), B = 2, S = 4 unless stated; cells_* and n8192 n_grid 128, res 64^3, B = 1, S = 1.
States and cotangents are scaled as in tests/test_mpm_gpu.py::test_mpm_step_edge_cases (v 0.3, C 2, F = I + 0.03, gx 1, gv 1e-2, gC 1e-4,
gF 1e-2, gppos = gprot = 1), one fixed seed per case, friction 0.3, clip = True.  Material is drawn from {1, 2} and hardness from U[0.5, 2]
per particle -- from N alone, so that cases of one N can share a handle (material and hardness are fixed when a handle is created).

An IRREGULAR particle is what the kernels call one (mpm_det.h det_regular): base = trunc(x inv_dx - 0.5) has base + 2 >= res on some axis (or
base < 0: x < -dx / 2, which no state of a step reaches) -- its stencil is cut by the scatter and clamped by the gather, it gets bucket key -1
and is merged into every offset's walk by index.  A particle with x inv_dx < 0.5 is NOT one: the truncation gives base 0 with fx < 0.5
(negative quadratic weights, cells with m < 0), its stencil is whole and it is bucketed like any other.  So only the upper edge of `res`
produces irregular particles; the *_upper cases exist for that reason.

  tag                          N    what it reaches
  corner                       160  x = 0.004 + U(0, 0.06)^3: base 0 with fx < 0.5 (34 / 28 particles per env), the friction and boundary bands
                                    of all three axes.  No irregular particle.
  upper_edge                   160  the plain cloud (0.15 + U(0, 0.06)^3) with x0 += 0.30: regular and irregular particles mixed -- the merge in
                                    det_cells_kernel MODE 0 and MODE 1, key -1 and nirr in det_sort_kernel; x0 >= 0.5078 lies past res
                                    (det_pre_kernel's t == 1 pass with gl != sl), but every cell those gathers clamp to is scattered to
  all_irregular                160  the corner cloud with y = 0.0002 + U(0, 0.004): every weight w[1] of the y axis negative.  (All regular.)
  all_irregular_upper          160  x0 in [0.48, 0.51): EVERY particle irregular, no bucket exists; some past res on x
  upper_corner                 160  x0, x1, x2 all += 0.30: clamped gathers on three axes -- several offsets of one particle land in the same
                                    cell (MODE 1 selects by cell_gather)
  past_upper                   160  x0 in [0.49, 0.53), x1 and x2 spread over 0.2: a thin sheet half of which lies past res -- its scatter is dropped
                                    whole, its gathers clamp to cells (31, j, k) that NOBODY scatters to: det_pre_kernel's t == 1 pass with
                                    gl != sl appends them, the cell sums give m = 0 there
  crowded                      96   a cube of 1.5 cells at 0.2: buckets far longer than DET_K = 8 (the tail loop), no irregular particle.  In this and
                                    the next three cases and the small bodies the box stands BESIDE the body (see BESIDE)
  crowded_corner               96   the same cube at 0.002
  crowded_upper                96   the same cube at x0 = 0.4609 (29.5 cells): long buckets merged with irregular particles in one walk
  bucket_boundary              24   three neighbouring base cells with exactly 7, 8 and 9 particles in shuffled index order
  n1_s1, n1, n2, n3, n64, n65       small bodies (plain cloud): det_trq_kernel with N < 3 (the trace over particles 0..N-1), one particle,
                                    both sides of the sort's npow2 = 64; n1_s1: one substep
  four_boxes_corner,           160  soft contact, P = 4 boxes, zero rotation: det_reduce_cells_kernel with K = 1 + 18 * 4
  four_boxes_upper_edge, four_boxes_corner_one_substep (S = 1)
  turning_boxes_corner (P = 4), turning_boxes_crowded_corner (P = 2, N = 96): rotation actions 20 x the translation scale -- the rotation goes
                                    through the platform's sinf / cosf, so these are never compared bit for bit: adjoint and tolerance forward
  cells_32751, cells_32778     1213 / 1214 isolated particles on a pitch-4 lattice of base cells (arange(2, 60, 4)^3, shuffled),
                                    x n_grid - base in [0.6, 1.4): disjoint stencils, exactly 27 N touched cells -- the backward's limit of
                                    32768 listed cells from both sides
  n8192                        8192 a uniform cloud in [0.1, 0.4]^3: the largest body the mode accepts; forward only
"""
from typing import NamedTuple

import numpy as np

MU0, LA0 = 100 / (2 * 1.1), 100 * 0.1 / (1.1 * 0.8)
LEGACY = dict(n_grid=64, res=(32, 32, 32), dt=1e-4)
SCALED = dict(n_grid=128, res=(64, 64, 64), dt=1e-4)
DET_K = 8                      # csrc/mpm_det.hip
DET_SORT_CELLS = 32768         # csrc/mpm_det.hip, include/unidom_hip.h
DET_MAX_PARTICLES = 8192       # include/unidom_hip.h

# tag: (seed, N, S, P (0 = position control), geometry)
_SPEC = {
    "corner": (11, 160, 4, 0, LEGACY),
    "upper_edge": (11, 160, 4, 0, LEGACY),
    "all_irregular": (11, 160, 4, 0, LEGACY),
    "all_irregular_upper": (12, 160, 4, 0, LEGACY),
    "upper_corner": (13, 160, 4, 0, LEGACY),
    "past_upper": (28, 160, 4, 0, LEGACY),
    "crowded": (14, 96, 4, 0, LEGACY),
    "crowded_corner": (15, 96, 4, 0, LEGACY),
    "crowded_upper": (16, 96, 4, 0, LEGACY),
    "bucket_boundary": (17, 24, 4, 0, LEGACY),
    "n1_s1": (18, 1, 1, 0, LEGACY),
    "n1": (19, 1, 4, 0, LEGACY),
    "n2": (20, 2, 4, 0, LEGACY),
    "n3": (21, 3, 4, 0, LEGACY),
    "n64": (22, 64, 4, 0, LEGACY),
    "n65": (23, 65, 4, 0, LEGACY),
    "four_boxes_corner": (11, 160, 4, 4, LEGACY),
    "four_boxes_upper_edge": (11, 160, 4, 4, LEGACY),
    "four_boxes_corner_one_substep": (11, 160, 1, 4, LEGACY),
    "turning_boxes_corner": (24, 160, 4, 4, LEGACY),
    "turning_boxes_crowded_corner": (25, 96, 4, 2, LEGACY),
    "cells_32751": (26, 1213, 1, 0, SCALED),
    "cells_32778": (26, 1214, 1, 0, SCALED),
    "n8192": (27, 8192, 1, 0, SCALED),
}
TURNING = ("turning_boxes_corner", "turning_boxes_crowded_corner")
SMALL = ("n1_s1", "n1", "n2", "n3", "n64", "n65")
# Position control writes the box's velocity into every cell the box holds, whatever was summed there.  A box of half-size 0.02 at the centre of
# a body 1.5 cells wide holds ALL its cells: the step's outputs then do not depend on the cell sums at all (the reference's gv is identically
# zero) and a wrong sum would pass.  In these cases the box stands beside the body, 0.035 along x, and holds its outermost layer of cells only.
BESIDE = ("crowded", "crowded_corner", "crowded_upper", "bucket_boundary") + SMALL
REUSE = ("corner", "all_irregular", "upper_edge")          # N = 160, position control: one handle serves them all
ALL_TAGS = tuple(_SPEC)
BITWISE_TAGS = tuple(t for t in ALL_TAGS if t not in TURNING)              # zero rotation: the forward equals the checker bit for bit
BACKWARD_TAGS = tuple(t for t in ALL_TAGS if t not in ("n8192", "cells_32778"))

FWD_BARS = dict(x=5e-6, v=1e-4, C=1e-3, F=5e-5)            # the project's forward bars against the independent oracle
ADJ_BAR = 5e-3                                              # test_mpm_step_edge_cases' bar for the default kernels at these shapes
F32_BAR = 5e-4                                              # the oracle's own f32 adjoint against its f64 one: keeps 10 x under ADJ_BAR
MAIN_KEYS = ("gx", "gv", "gC", "gF", "gppos", "gaction")    # + gprot under soft contact: held at ADJ_BAR
SCALAR_KEYS = ("gfriction", "gmu", "glamda")                # held at 5 x ADJ_BAR (the ratio of test_collide_matches_oracle)


class Case(NamedTuple):
    tag: str
    N: int
    B: int
    S: int
    P: int                # primitives
    pc: bool              # position control (P = 1) or soft contact
    geom: dict            # n_grid, res, dt
    material: np.ndarray  # [N] int32
    hard: np.ndarray      # [N] float32
    st: dict              # the step's inputs, f32
    g: dict               # cotangents of the outputs, f32 (gprot under soft contact only)


_CASES, _CHK, _FWD, _BWD = {}, {}, {}, {}


def rel(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def particle_tables(N):
    """material in {1, 2} and hardness in [0.5, 2] per particle, from N alone"""
    rng = np.random.default_rng(7000 + N)
    return rng.integers(1, 3, size=N).astype(np.int32), rng.uniform(0.5, 2.0, size=N).astype(np.float32)


def _positions(tag, rng, B, N, n_grid):
    u = lambda *s: rng.uniform(size=s)
    if tag in ("cells_32751", "cells_32778"):
        ax = np.arange(2, 60, 4)
        sites = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
        sites = sites[np.random.default_rng(2600).permutation(len(sites))]          # the same lattice order for both sizes
        return ((sites[None, :N] + 0.6 + 0.8 * u(B, N, 3)) / n_grid).astype(np.float32)
    if tag == "n8192":
        return (0.1 + 0.3 * u(B, N, 3)).astype(np.float32)
    if tag == "bucket_boundary":
        cells = np.repeat(np.array([[10, 10, 10], [11, 10, 10], [10, 11, 10]]), [7, 8, 9], axis=0)
        cells = cells[rng.permutation(N)]                     # the buckets' members in interleaved index order
        return ((cells[None] + 0.6 + 0.8 * u(B, N, 3)) / n_grid).astype(np.float32)   # x inv_dx - 0.5 in base + [0.1, 0.9)
    if tag in ("crowded", "crowded_corner", "crowded_upper", "turning_boxes_crowded_corner"):
        lo = np.array({"crowded": [0.2] * 3, "crowded_upper": [29.5 / 64, 0.2, 0.2]}.get(tag, [0.002] * 3))
        return (lo + u(B, N, 3) * (1.5 / 64)).astype(np.float32)
    lo = 0.004 if tag in ("corner", "all_irregular", "four_boxes_corner", "four_boxes_corner_one_substep", "turning_boxes_corner") else 0.15
    x = (lo + rng.uniform(0, 0.06, size=(B, N, 3))).astype(np.float32)
    if tag in ("upper_edge", "four_boxes_upper_edge"):
        x[..., 0] += np.float32(0.30)                         # res = 32 cells of dx = 1 / 64 end at 0.5; x0 in [0.45, 0.51)
    if tag == "upper_corner":
        x += np.float32(0.30)
    if tag == "all_irregular":
        x[..., 1] = (0.0002 + rng.uniform(0, 0.004, size=(B, N))).astype(np.float32)
    if tag == "past_upper":
        x[..., 0] = (0.49 + rng.uniform(0, 0.04, size=(B, N))).astype(np.float32)     # base0 >= 32 = res from 0.5078 on: nothing scattered
        x[..., 1:] = (0.15 + rng.uniform(0, 0.2, size=(B, N, 2))).astype(np.float32)  # thin: cells (31, j, k) that only gathers reach
    if tag == "all_irregular_upper":
        x[..., 0] = (0.48 + rng.uniform(0, 0.03, size=(B, N))).astype(np.float32)     # base0 >= 30 = res - 2 from 0.4766 on
    return x


def case(tag) -> Case:
    """the same arrays whenever it is asked again; nobody may write into them"""
    if tag in _CASES:
        return _CASES[tag]
    seed, N, S, P, geom = _SPEC[tag]
    pc, P = P == 0, max(P, 1)
    B = 1 if geom is SCALED else 2
    rng = np.random.default_rng(seed)
    x = _positions(tag, rng, B, N, geom["n_grid"])
    pa = (P,) if P > 1 else ()
    ppos = np.zeros((B,) + pa + (S, 3), np.float32)
    ppos[..., 0, :] = (x.mean(1)[:, None] if P > 1 else x.mean(1)) + rng.normal(size=(B,) + pa + (3,)).astype(np.float32) * 0.01
    if tag in BESIDE:
        ppos[..., 0, 0] += np.float32(-0.035 if tag == "crowded_upper" else 0.035)
    prot = np.zeros((B,) + pa + (S, 4), np.float32)
    prot[..., 0] = 1
    action = (rng.normal(size=(B, P, 6)) * 0.01).astype(np.float32)
    action[..., 3:] = action[..., 3:] * 20 if tag in TURNING else 0.0
    st = dict(x=x, v=(rng.normal(size=(B, N, 3)) * 0.3).astype(np.float32), C=(rng.normal(size=(B, N, 3, 3)) * 2).astype(np.float32),
              F=(np.eye(3) + rng.normal(size=(B, N, 3, 3)) * 0.03).astype(np.float32), J=np.ones((B, N), np.float32), ppos=ppos, prot=prot,
              psize=np.tile(np.float32([0.02, 0.02, 0.02]), (B,) + pa + (1,)), friction=np.full(B, 0.3, np.float32),
              mu=np.full(B, MU0, np.float32), lamda=np.full(B, LA0, np.float32), action=action.reshape(B, 6 * P))
    g = dict(gx=rng.normal(size=(B, N, 3)), gv=rng.normal(size=(B, N, 3)) * 0.01, gC=rng.normal(size=(B, N, 3, 3)) * 1e-4,
             gF=rng.normal(size=(B, N, 3, 3)) * 0.01, gppos=rng.normal(size=(B,) + pa + (S, 3)), gprot=rng.normal(size=(B,) + pa + (S, 4)))
    g = {k: v.astype(np.float32) for k, v in g.items()}
    if pc:
        del g["gprot"]         # position control: no rotation cotangent crosses the boundary
    mat, hard = particle_tables(N)
    for a in list(st.values()) + list(g.values()) + [mat, hard]:
        a.setflags(write=False)
    _CASES[tag] = Case(tag, N, B, S, P, pc, geom, mat, hard, st, g)
    return _CASES[tag]


def envs(c: Case, sel):
    """the inputs and cotangents of the envs `sel` of a case"""
    return {k: np.ascontiguousarray(v[sel]) for k, v in c.st.items()}, {k: np.ascontiguousarray(v[sel]) for k, v in c.g.items()}


def stencil_stats(c: Case, st=None):
    """What the first substep of each env meets, in the kernels' integer arithmetic (particle_pre's truncation, det_regular, cell_scatter,
    cell_gather): n_irr, the longest bucket, the touched cells (scatter or gather), the gather cells nobody scatters to, and the largest
    number of offsets of one particle that gather from one cell."""
    x = (c.st if st is None else st)["x"]
    res = np.array(c.geom["res"])
    inv_dx = np.float32(c.geom["n_grid"])
    out = []
    off = np.stack(np.meshgrid(range(3), range(3), range(3), indexing="ij"), -1).reshape(27, 3)
    for b in range(x.shape[0]):
        base = (x[b] * inv_dx - np.float32(0.5)).astype(np.int32)                  # f32 product and difference, truncated
        regular = ((base >= 0) & (base + 2 < res)).all(1)
        lin = lambda ijk: (ijk[..., 0] * res[1] + ijk[..., 1]) * res[2] + ijk[..., 2]
        _, counts = np.unique(lin(base[regular]), return_counts=True) if regular.any() else (None, np.zeros(1, int))
        cells = base[:, None, :] + off[None]                                      # [N, 27, 3]
        cells = np.where(cells < 0, cells + res, cells)                           # negative indices wrap
        inside = ((cells >= 0) & (cells < res)).all(-1)
        scatter = set(lin(cells[inside]).tolist())
        gl = lin(np.clip(cells, 0, res - 1))
        gather = set(gl.reshape(-1).tolist())
        same = max(int(np.unique(row, return_counts=True)[1].max()) for row in gl)
        out.append(dict(n_irr=int((~regular).sum()), max_bucket=int(counts.max()), buckets=sorted(counts.tolist()),
                        touched=len(scatter | gather), gather_only=len(gather - scatter), offsets_per_cell=same,
                        low=int((x[b] * inv_dx < 0.5).any(1).sum())))
    return out


def _oracle(c: Case):
    from oracle.pyoracle import MpmOracle
    return MpmOracle(c.N, n_grid=c.geom["n_grid"], res=c.geom["res"], steps=c.S, dt=c.geom["dt"], position_control=c.pc,
                     material=c.material, hardness=c.hard, n_prim=c.P)


def _freeze(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def checker(tag, st=None):
    """mpm_det_forward of the case (kept) or of other inputs of its shape (`st`: not kept)"""
    from oracle.pyoracle import mpm_det_forward
    c = case(tag)
    if st is None and tag in _CHK:
        return _CHK[tag]
    out = mpm_det_forward(c.st if st is None else st, c.N, n_grid=c.geom["n_grid"], res=c.geom["res"], steps=c.S, dt=c.geom["dt"],
                          material=c.material, hardness=c.hard, position_control=c.pc, n_prim=c.P, sdf_kind=0,
                          prim_friction=[0.1] * c.P, prim_softness=[666.0] * c.P)
    if st is None:
        _CHK[tag] = _freeze(out)
    return out


def oracle_fwd(tag):
    if tag not in _FWD:
        c = case(tag)
        _FWD[tag] = _freeze(_oracle(c).step_fwd(dict(c.st), nthreads=4))
    return _FWD[tag]


def oracle_bwd(tag, dtype=np.float64):
    """the oracle's adjoint with clip = True, forward and adjoint in `dtype`"""
    key = (tag, np.dtype(dtype).name)
    if key not in _BWD:
        c = case(tag)
        st = {k: v.astype(dtype) for k, v in c.st.items()}
        g = {k: v.astype(dtype) for k, v in c.g.items()}
        _BWD[key] = _freeze(_oracle(c).step_bwd(st, g, clip=True, nthreads=4))
    return _BWD[key]


def compared_keys(c: Case):
    return MAIN_KEYS + (() if c.pc else ("gprot",)) + SCALAR_KEYS


# Leaves whose f64 reference is identically zero -- asserted by tests/test_mpm_det_edge_cases.py, which also asserts that every other compared
# leaf is not: the GPU test asks for an exact zero there, not a vacuous ratio.
#   gaction_rot  gaction[:, 6 p + 3 : 6 p + 6] of every primitive p: zero rotation with clip (the reference's NaN of d|w| / dw at w = 0, laundered
#                to 0; position control reports 0 there by contract)
#   gaction      all of it: with one substep the action moves no row that the step reads
#   gfriction    no cell of the case lies in the ground-friction band
_ROT, _OFF_GROUND = ("gaction_rot",), ("gaction_rot", "gfriction")
ZEROS = {
    "corner": _ROT, "upper_edge": _OFF_GROUND, "all_irregular": _ROT, "all_irregular_upper": _OFF_GROUND, "upper_corner": _OFF_GROUND,
    "past_upper": _OFF_GROUND, "crowded": _OFF_GROUND, "crowded_corner": _ROT, "crowded_upper": _OFF_GROUND, "bucket_boundary": _OFF_GROUND,
    "n1_s1": _OFF_GROUND, "n1": _OFF_GROUND, "n2": _OFF_GROUND, "n3": _OFF_GROUND, "n64": _OFF_GROUND, "n65": _OFF_GROUND,
    "four_boxes_corner": _ROT, "four_boxes_upper_edge": _OFF_GROUND, "four_boxes_corner_one_substep": ("gaction",),
    "turning_boxes_corner": (), "turning_boxes_crowded_corner": (), "cells_32751": _ROT,
}
# (gmu and glamda are not among them even at N = 1: with the box beside the body the particle's own stress reaches its own new state.)


def split_zero(c: Case, key, a):
    """-> (the part of gradient `key` that is compared by ratio, the part the reference has identically zero); either may be None"""
    z = ZEROS[c.tag]
    if key == "gaction" and "gaction_rot" in z:
        a6 = a.reshape(a.shape[0], c.P, 6)
        return a6[..., :3], a6[..., 3:]
    return (None, a) if key in z else (a, None)


def make_sim(c: Case, deterministic=1, max_envs=None):
    """a handle for the case's shape, built as tests/test_mpm_det.py::_det_sim and tests/test_mpm_gpu.py::make_collide_sim build theirs"""
    from unidom_amd.engine.mpm_simulator import SimpleMPMSimulator

    class Conf:
        n_grid, res, dt = c.geom["n_grid"], c.geom["res"], c.geom["dt"]
        steps = c.S
        E, nu = 100, 0.2
        ground_friction = 0.1
        dx, inv_dx = 1 / c.geom["n_grid"], float(c.geom["n_grid"])
        p_vol = (dx * 0.5) ** 2
        p_mass = p_vol * 1
        gravity = (0, -9.8, 0)
        n_primitive = 1
    conf = Conf()
    conf.deterministic = deterministic
    sim = SimpleMPMSimulator(conf, max_envs or c.B, use_position_control=c.pc)
    sim.n_particles, sim.material, sim.h = c.N, np.array(c.material), np.array(c.hard)
    sim.n_primitive = c.P
    sim._make_handle()
    return sim
