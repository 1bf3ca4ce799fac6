"""Inputs and assertions shared by tests/test_devfn_cpu.py (host builds of the product's device functions) and tests/test_devfn_gpu.py
(the same functions on the MI355X through tests/devfn/libdevfn.so).  Not a test module.

SVD inputs (all seeded, N = 4096 per family; Q, Q1, Q2 random proper rotations from a QR):
  * near-rotation  Q (I + eps E), E standard normal -- a cluster of three singular values at 1, where one Jacobi sweep squares nothing;
  * two-cluster and in-clamp spectra  Q1 diag(s) Q2, s in {(1, 1+d, 0.5), (2, 1, 1+d), (1+d, 1, 1-d), (1.45, 0.75+d, 0.75)} -- the last
    spans the plastic clamp's range;
  * exact cases (identity, 2 I, diagonal, permutation, rotation, reflection, diag(1e3, 1, 1e-3) between rotations) and rank 2 / 1 / 0.
Residuals are evaluated one precision up (f64 for f32, np.longdouble for f64) and counted in eps of the type under test.

The bar, 16 eps for max|UtU - I|, max|Vh Vht - I|, max|U S Vh - A| / S0 (and, f32 only, |S - S_lapack| / S0 and |U Vh - polar(A)| against
LAPACK in f64): the host builds with the early exit at round-off level measure at most 8.3 eps on exactly these families (see the tables in
the two test modules), the smallest signature of the too-early exit was 120 eps (UtU - I = 1.4e-5 at eps = 1e-5 in f32); 16 is about twice
the former and far below the latter.  The fast f32 build takes its cosine from a 1-ulp v_rsq, which scales both columns of a rotation by
(1 +- 1 ulp), at most 8 rotations per column in 4 sweeps: its bar for Vh Vht - I, S and the reconstruction is 32 eps (16 + 8 * 2)."""
import functools

import numpy as np

N = 4096
LADDER32 = (0.3, 1e-2, 1e-3, 3e-4, 1e-4, 5e-5, 1e-5, 1e-6, 1e-7, 0.0)
LADDER64 = LADDER32 + (1e-8, 3e-9, 1e-9, 1e-10, 1e-12, 1e-15)
SPECTRA = {"s(1,1+d,.5)": lambda d: (1.0, 1.0 + d, 0.5), "s(2,1,1+d)": lambda d: (2.0, 1.0, 1.0 + d),
           "s(1+d,1,1-d)": lambda d: (1.0 + d, 1.0, 1.0 - d), "clamp(1.45,.75+d,.75)": lambda d: (1.45, 0.75 + d, 0.75)}
BAR = 16.0          # eps
BAR_FAST = 32.0     # eps: Vh Vht - I, S and the reconstruction of the fast f32 build (1-ulp v_rsq cosine)


def rotations(rng, n):
    Q, R = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    Q = Q * np.sign(np.einsum("nii->ni", R))[:, None, :]
    return Q * np.linalg.det(Q)[:, None, None]          # det +1


@functools.lru_cache(maxsize=None)
def families(dtype):
    """-> tuple of (name, A [N, 3, 3] of dtype, polar): polar marks the families whose U Vh is compared with LAPACK's polar factor."""
    dtype = np.dtype(dtype)
    ladder = LADDER32 if dtype == np.float32 else LADDER64
    rng = np.random.default_rng(20240607)
    out = []
    for eps in ladder:
        A = rotations(rng, N) @ (np.eye(3) + eps * rng.normal(size=(N, 3, 3)))
        out.append((f"nearrot eps={eps:g}", A.astype(dtype), True))
    for name, spec in SPECTRA.items():
        for d in ladder:
            A = (rotations(rng, N) * np.asarray(spec(d))[None, None, :]) @ rotations(rng, N)
            out.append((f"{name} d={d:g}", A.astype(dtype), name.startswith("clamp")))
    for _, A, _ in out:
        A.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exact_cases(dtype):
    """-> (full-rank [n, 3, 3], rank-deficient [m, 3, 3]) of dtype"""
    rng = np.random.default_rng(7)
    Q = rotations(rng, 40)
    full = [np.eye(3), 2 * np.eye(3), np.diag([3.0, 0.5, 1.25]), np.diag([0.25, 4.0, 1.0]), np.eye(3)[[2, 0, 1]], np.eye(3)[[1, 0, 2]]]
    full += list(Q[:8])                                                        # pure rotations
    full += [np.diag([1.0, 1.0, -1.0]) @ q for q in Q[8:12]] + [-np.eye(3)]    # reflections, det < 0
    full += [(Q[12 + i] * np.asarray([1e3, 1.0, 1e-3])) @ Q[20 + i] for i in range(8)]
    full += [np.diag([1e3, 1.0, 1e-3]) @ Q[28], Q[29] @ np.diag([1e-3, 1e3, 1.0])]
    u, v, w, z = rng.normal(size=(4, 3))
    defi = [np.zeros((3, 3)), np.outer(u, v), np.outer(u, v) + np.outer(w, z), np.diag([1.0, 0.0, 2.0]), np.diag([0.0, 0.0, 5.0]),
            (Q[30] * np.asarray([2.0, 1.0, 0.0])) @ Q[31], (Q[32] * np.asarray([2.0, 0.0, 0.0])) @ Q[33]]
    # rows / columns of zeros: products with al * be == 0 exactly
    defi += [np.asarray([[1.0, 2.0, 0.0], [3.0, 4.0, 0.0], [5.0, 6.0, 0.0]]), np.asarray([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])]
    return np.asarray(full).astype(dtype), np.asarray(defi).astype(dtype)


def scaling_cases(dtype):
    """a few hundred full-rank matrices over the ladder for the A * 2^k test"""
    fam = families(dtype)
    return np.concatenate([A[:64] for _, A, _ in fam[:10]])


def _wide(dtype):
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def residuals(A, U, S, Vh):
    """per-matrix residuals in eps of A's type, evaluated one precision up: dict of [n] arrays (rec is absolute / eps; divide by S0 yourself)"""
    w, eps = _wide(A.dtype), float(np.finfo(A.dtype).eps)
    Aw, Uw, Sw, Vw = (np.asarray(a).astype(w) for a in (A, U, S, Vh))
    I = np.eye(3, dtype=w)
    mx = lambda M: np.abs(M).max(axis=(1, 2)).astype(np.float64) / eps
    return dict(uu=mx(np.swapaxes(Uw, 1, 2) @ Uw - I), vv=mx(Vw @ np.swapaxes(Vw, 1, 2) - I), rec=mx((Uw * Sw[:, None, :]) @ Vw - Aw),
                s0=np.asarray(S[:, 0], np.float64))


def check_full_rank(tag, A, U, S, Vh, polar=False, fast=False):
    """The issue's assertions for matrices of full rank; returns the worst residuals (eps) for the DEVFN line."""
    eps = float(np.finfo(A.dtype).eps)
    for name, a in (("U", U), ("S", S), ("Vh", Vh)):
        assert np.isfinite(a).all(), f"{tag}: {name} not finite"
    assert (S[:, 0] >= S[:, 1]).all() and (S[:, 1] >= S[:, 2]).all() and (S[:, 2] >= 0).all(), f"{tag}: S not sorted / negative"
    r = residuals(A, U, S, Vh)
    worst = dict(uu=r["uu"].max(), vv=r["vv"].max(), rec=(r["rec"] / r["s0"]).max())
    loose = BAR_FAST if fast else BAR
    assert worst["uu"] <= BAR, f"{tag}: max|UtU - I| = {worst['uu']:.1f} eps > {BAR}"
    assert worst["vv"] <= loose, f"{tag}: max|Vh Vht - I| = {worst['vv']:.1f} eps > {loose}"
    assert worst["rec"] <= loose, f"{tag}: max|U S Vh - A| / S0 = {worst['rec']:.1f} eps > {loose}"
    if A.dtype == np.float32:          # LAPACK in f64 is an honest reference for f32 only
        A64 = A.astype(np.float64)
        Ul, Sl, Vl = np.linalg.svd(A64)
        worst["s"] = (np.abs(S.astype(np.float64) - Sl).max(axis=1) / Sl[:, 0]).max() / eps
        assert worst["s"] <= loose, f"{tag}: max|S - S_lapack| / S0 = {worst['s']:.1f} eps > {loose}"
        if polar:
            worst["polar"] = np.abs(U.astype(np.float64) @ Vh.astype(np.float64) - Ul @ Vl).max() / eps
            assert worst["polar"] <= BAR, f"{tag}: max|U Vh - polar(A)| = {worst['polar']:.1f} eps > {BAR}"
    return worst


def check_rank_deficient(tag, A, U, S, Vh, fast=False):
    """rank 2 / 1 / 0: finite, S sorted and >= 0, Vh orthogonal, reconstruction.  Nothing is asserted on U: the product zeroes the U column
    of a vanishing singular value (so UtU != I there, and U Vh is not a polar factor) -- kept as it is, callers only use U S Vh."""
    for name, a in (("U", U), ("S", S), ("Vh", Vh)):
        assert np.isfinite(a).all(), f"{tag}: {name} not finite"
    assert (S[:, 0] >= S[:, 1]).all() and (S[:, 1] >= S[:, 2]).all() and (S[:, 2] >= 0).all(), f"{tag}: S not sorted / negative"
    r = residuals(A, U, S, Vh)
    loose = BAR_FAST if fast else BAR
    assert r["vv"].max() <= loose, f"{tag}: max|Vh Vht - I| = {r['vv'].max():.1f} eps"
    assert (r["rec"] <= loose * r["s0"]).all(), f"{tag}: reconstruction {np.max(r['rec'] / np.maximum(r['s0'], 1e-300)):.1f} eps of S0"
    zero = (A == 0).all(axis=(1, 2))
    assert (S[zero] == 0).all() and (U[zero] == 0).all(), f"{tag}: the zero matrix must give S = 0 and the zeroed U"


def check_all_families(tag, svd, dtype, fast=False):
    """svd(A [n, 3, 3]) -> U, S, Vh.  Every family, the exact cases and the power-of-two scaling; returns {quantity: worst eps}."""
    worst = {}
    for name, A, polar in families(dtype):
        U, S, Vh = svd(A)
        w = check_full_rank(f"{tag} / {name}", A, U, S, Vh, polar=polar, fast=fast)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    full, defi = exact_cases(dtype)
    w = check_full_rank(f"{tag} / exact cases", full, *svd(full), fast=fast)
    for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), float(v))
    check_rank_deficient(f"{tag} / rank-deficient", defi, *svd(defi), fast=fast)
    A = scaling_cases(dtype)
    U, S, Vh = svd(A)
    for k in (8, -8):
        Uk, Sk, Vk = svd((A * dtype(2.0) ** k).astype(dtype))
        assert np.array_equal(Sk, S * dtype(2.0) ** k), f"{tag}: S does not scale exactly with A * 2^{k}"
        assert np.array_equal(Uk, U) and np.array_equal(Vk, Vh), f"{tag}: U / Vh change under A * 2^{k}"
    return worst


def devfn_line(tag, worst):
    return "DEVFN " + tag + ": " + "  ".join(f"{k} {v:.1f}" for k, v in worst.items()) + "  (worst, in eps)"


# ---- scalar sets ---------------------------------------------------------------------------------------------------------------------

def _mantissas(bits, n):
    """n mantissa patterns of `bits` bits: all zeros, all ones, the neighbours of both, near-halfway patterns (low bits 0111.. / 1000..,
    and the top half-way points), the rest seeded random"""
    rng = np.random.default_rng(bits)
    top = (1 << bits) - 1
    fixed = [0, 1, 2, 3, top, top - 1, top - 2, 1 << (bits - 1), (1 << (bits - 1)) - 1, (1 << (bits - 1)) + 1,
             0x555555 & top if bits == 23 else 0x5555555555555 & top, 0x2AAAAA & top if bits == 23 else 0xAAAAAAAAAAAAA & top]
    for k in range(1, 12):              # trailing 0111..1 / 1000..0 of every short length: quotients and roots of these sit next to ties
        fixed += [(1 << k) - 1, 1 << k, top ^ ((1 << k) - 1), top ^ (1 << k)]
    m = np.concatenate([np.asarray(fixed, np.uint64), rng.integers(0, top + 1, size=n - len(fixed), dtype=np.uint64)])
    return m


def f32_set(e_lo, e_hi, n_mant=4096, negative=False):
    """every exponent e_lo..e_hi (value in [2^e, 2^(e+1))) times n_mant mantissas -> f32 [(e_hi - e_lo + 1) * n_mant]"""
    m = _mantissas(23, n_mant).astype(np.uint32)
    e = (np.arange(e_lo, e_hi + 1) + 127).astype(np.uint32)
    bits = (e[:, None] << np.uint32(23)) | m[None, :]
    if negative:
        bits = bits | np.uint32(0x80000000)
    return bits.reshape(-1).view(np.float32)


def f64_set(e_lo, e_hi, n_mant=4096):
    m = _mantissas(52, n_mant)
    e = (np.arange(e_lo, e_hi + 1) + 1023).astype(np.uint64)
    return ((e[:, None] << np.uint64(52)) | m[None, :]).reshape(-1).view(np.float64)


F32_SPECIALS = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-30, -3e38, 1e-45, -1e-45, 1e-40, 5.877e-39, 1.1754942e-38,
                           1.17549435e-38, 3.4028235e38, -3.4028235e38, 2.0 ** -96, 2.0 ** -97, 2.0 ** -126], np.float32)


def assert_bits_equal(tag, got, want, args=()):
    """f32 arrays equal bit for bit (any NaN equals any NaN)"""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {g.size} differ; first at {i}: args {[float(a[i]) for a in args]} "
                             f"got {float(g[i])!r} ({g.view(np.uint32)[i]:#x}) want {float(w[i])!r} ({w.view(np.uint32)[i]:#x})")


def ulp_err_f64(got, exact_wide):
    """|got - exact| in ulps of the f64 result, exact given in np.longdouble"""
    e = exact_wide.astype(np.float64)
    return np.abs((got.astype(np.longdouble) - exact_wide) / np.spacing(np.abs(e)).astype(np.longdouble)).astype(np.float64)


def expf_points():
    """[-87, 88.7] densely plus the branch edges and NaN"""
    rng = np.random.default_rng(3)
    x = np.concatenate([np.linspace(-87.0, 88.7, 200001), rng.uniform(-87.0, 88.7, 200000), rng.uniform(-1.0, 1.0, 50000),
                        (np.arange(-126, 129)[:, None] * np.log(2.0) * 0.5 + np.asarray([-1e-5, 0.0, 1e-5])[None, :]).reshape(-1)]).astype(np.float32)
    x = x[(x >= np.float32(-87.0)) & (x < np.float32(88.7))]
    edge = np.asarray([-87.0, 88.7, 0.0, -0.0, np.nan, np.inf, -np.inf, 100.0, -100.0, -88.0, 1e-10, -1e-10], np.float32)
    edge = np.concatenate([edge, np.nextafter(np.float32([-87.0, -87.0, 88.7, 88.7]), np.float32([-1e9, 1e9, -1e9, 1e9]))])
    return np.concatenate([x, edge])
