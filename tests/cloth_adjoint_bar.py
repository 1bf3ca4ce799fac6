"""Shared by tests/test_cloth_adjoint_f64_gpu.py and tests/test_cloth_adjoint_bar.py (a plain module, no fixtures): the bodies the
cloth dispatch of csrc/cloth.hip tells apart, the CPU oracle's forward with the f64 (R64) and f32 (R32) adjoints of one f32
trajectory, and the bar a kernel's adjoint has to meet against them.

The bar is oracle/ref_chain.py's:   |HIP - R64|max <= KAPPA |R32 - R64|max + REL_FLOOR |R64|max   (KAPPA, REL_FLOOR from there).
gx and gv meet it once per env, with all three maxima taken over that env's slice, so that a wrong first or last env of a launch
cannot hide behind the others; gprim, gactions, gk and gmu meet it over the whole tensor, because a per-env slice of them has too
few elements (8, 8 T, 1, 1) for |R32 - R64|max to be a stable yardstick -- which is also why every case has B >= 3.
"""
import numpy as np

from conftest import cloth_reset_x, make_cloth_case
from oracle import ref_chain as rc

KEYS = ("gx", "gv", "gprim", "gactions", "gk", "gmu")
FWD_KEYS = ("x", "v", "prim", "x_list", "v_list", "prim_list")
PER_ENV = ("gx", "gv")
CONSTS = ("gravity", "damping", "dt", "max_v", "small_num")
NTHREADS = 8


class Conf:  # fold_cloth1_env.py:15-33
    N = 80
    gravity = 0.5
    stiffness = 900
    damping = 2
    dt = 2e-3
    max_v = 2.0
    small_num = 1e-8
    mu = 0.5
    seed = 1
    substeps = 7


def make_conf(**kw):
    c = Conf()
    for q, val in kw.items():
        setattr(c, q, val)
    return c


# -- mask builders -----------------------------------------------------------------------------------------------------------
def rect_mask(N, rows, cols, i0=8, j0=8):
    """rows x cols particles with the corner at (i0, j0); particle order is row-major, so a spring spans cols + 1 indices"""
    m = np.zeros((N, N), np.float32)
    m[i0:i0 + rows, j0:j0 + cols] = 1
    assert 0 < i0 and i0 + rows < N and 0 < j0 and j0 + cols < N
    return m


def disk_mask(N, ci, cj, r):
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return (((ii - ci) ** 2 + (jj - cj) ** 2) <= r ** 2).astype(np.float32)


def slice_mask(N, i0, i1, j0, j1):
    m = np.zeros((N, N), np.float32)
    m[i0:i1, j0:j1] = 1
    return m


def spring_span(mask):
    """the widest index distance of a spring (what ud_cloth_create derives the halo of the several-workgroup kernels from)"""
    m = np.asarray(mask) != 0
    N = m.shape[0]
    pid = -np.ones((N + 2, N + 2), np.int64)
    pid[1:-1, 1:-1][m] = np.arange(int(m.sum()))
    c = pid[1:-1, 1:-1]
    far = 0
    for di, dj in ((0, 1), (1, -1), (1, 0), (1, 1)):
        nb = pid[1 + di:N + 1 + di, 1 + dj:N + 1 + dj]
        both = (c >= 0) & (nb >= 0)
        if both.any():
            far = max(far, int((nb[both] - c[both]).max()))
    return far


# -- inputs --------------------------------------------------------------------------------------------------------------------
def make_case(rng, conf, mask, B, T, big=None):
    """make_cloth_case on the body; lattices finer than 80 (`big`, default N > 80) take the T-shirt tests' gentler deformation and
    stiffness range"""
    big = conf.N > 80 if big is None else big
    P_x = cloth_reset_x(conf.N, mask)
    if not big:
        return list(make_cloth_case(rng, B, T, P_x=P_x))
    x, v, prim, k, mu, actions = make_cloth_case(rng, B, T, P_x=P_x, deform=0.0003, v_scale=0.01)
    k = rng.uniform(3000, 6000, size=B).astype(np.float32)
    return [x, v, prim, k, mu, actions]


def cotangents(rng, B, T, P, lists=True):
    n = lambda *s: rng.normal(size=s).astype(np.float32)
    g = dict(gx=n(B, P, 3), gv=n(B, P, 3), gprim=n(B, 2, 4))
    if lists:
        g.update(gx_list=n(T, B, P, 3), gv_list=n(T, B, P, 3), gprim_list=n(T, B, 2, 4))
    return g


def make_oracle(conf, mask, order):
    from oracle.pyoracle import ClothOracle
    return ClothOracle(np.asarray(mask), N=conf.N, order=order, substeps=int(conf.substeps), **{q: getattr(conf, q) for q in CONSTS})


def reference(orc, case, g, normalize=True, nthreads=NTHREADS, need_contact=True, small_num=Conf.small_num):
    """One oracle, one f32 trajectory: its forward (lists and grasp sets), the f64 adjoint along it (R64) and the f32 adjoint (R32).
    The f64 sweep must have followed every grasp decision of the f32 forward (flips == 0); the case must grasp, and (need_contact)
    put a particle on the ground (y <= small_num at a substep's input: the friction block, without which gmu is 0 against 0)."""
    fwd = orc.rollout_fwd(*case, want_lists=True, want_grasp=True, want_ckpt=need_contact, nthreads=nthreads)
    for q in FWD_KEYS:
        assert np.isfinite(fwd[q]).all(), q
    assert fwd["grasp"].sum() > 0, "the case must exercise the grasp"
    if need_contact:
        P = orc.P
        y = fwd.pop("ckpt")[..., :P * 3].reshape(-1, P, 3)[..., 1]
        assert (y <= np.float32(small_num)).any(), "the case must put a particle on the ground"
    gl = tuple(g.get(q) for q in ("gx_list", "gv_list", "gprim_list"))
    r64 = orc.rollout_bwd(*case, g["gx"], g["gv"], g["gprim"], *gl, normalize=normalize, nthreads=nthreads, adjoint_dtype=np.float64)
    r32 = orc.rollout_bwd(*case, g["gx"], g["gv"], g["gprim"], *gl, normalize=normalize, nthreads=nthreads, adjoint_dtype=np.float32)
    assert r64.pop("flips") == 0, "the f64 sweep decided a grasp test otherwise than the f32 forward"
    return fwd, r64, r32


# -- the checks ----------------------------------------------------------------------------------------------------------------
def assert_forward_bit_exact(h, o, keys=FWD_KEYS):
    np.testing.assert_array_equal(h["grasp"], o["grasp"])
    for q in keys:
        np.testing.assert_array_equal(h[q], o[q], err_msg=q)


def _one(tag, hip, r64, r32):
    e, e32, n = np.abs(hip - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    ratio = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
    return e, e32, n, ratio, rc.bar(r64, r32)


def adjoint_bar_report(tag, hip, r64, r32, zero=()):
    """-> {tensor: (worst |HIP - R64| / bar, worst |HIP - R64| / |R32 - R64|, env of the worst or None)}; prints one ADJBAR line per
    tensor.  Asserts what does not depend on the bar: finite values, |R64|max > 0 (`zero`: tensors that are identically 0 for the
    body -- the stiffness gradient of a body without springs -- where HIP must be exactly 0 too)."""
    out = {}
    for q in KEYS:
        h, a, b = (np.asarray(t[q], np.float64) for t in (hip, r64, r32))
        assert h.shape == a.shape == b.shape, (tag, q, h.shape, a.shape)
        assert np.isfinite(h).all() and np.isfinite(a).all() and np.isfinite(b).all(), (tag, q)
        if q in zero:
            assert not a.any() and not b.any() and not h.any(), (tag, q, "expected identically zero")
            print(f"ADJBAR {tag}/{q}: identically zero (no springs)")
            out[q] = (0.0, 0.0, None)
            continue
        if q in PER_ENV:
            rows = [_one(tag, h[e], a[e], b[e]) + (e,) for e in range(h.shape[0])]
        else:
            rows = [_one(tag, h, a, b) + (None,)]
        for e, e32, n, ratio, bar, env in rows:
            assert n > 0, (tag, q, env, "|R64|max is 0: nothing is compared")
        w = max(rows, key=lambda r: r[0] / r[4])
        worst_ratio = max(r[3] for r in rows)
        print(f"ADJBAR {tag}/{q}: |HIP-R64| {w[0]:.3e}  |R32-R64| {w[1]:.3e}  |R64| {w[2]:.3e}  bar {w[4]:.3e}  "
              f"ratio {worst_ratio:.3f}  err/bar {w[0] / w[4]:.3f}" + ("" if w[5] is None else f"  (worst env {w[5]} of {len(rows)})"))
        out[q] = (w[0] / w[4], worst_ratio, w[5])
    return out


def assert_adjoint_within_bar(tag, hip, r64, r32, zero=()):
    """every tensor of KEYS within the bar (see the module docstring); -> adjoint_bar_report's figures"""
    rep = adjoint_bar_report(tag, hip, r64, r32, zero=zero)
    over = {q: v for q, v in rep.items() if v[0] > 1.0}
    assert not over, (tag, "over the bar: {tensor: (err / bar, err / |R32 - R64|, env)}", over)
    return rep
