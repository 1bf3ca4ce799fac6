"""CPU: the cloth DEPTH observation's ABI names, the NumPy twin the GPU tests compare with, and the opt-in default."""
import ctypes

import numpy as np

from test_cloth_depth_gpu import depth_twin, twin_bwd


def test_depth_symbols_are_listed_and_exported():
    from unidom_amd import _lib
    L = ctypes.CDLL(_lib.build())
    for name in ("ud_cloth_depth_fwd", "ud_cloth_depth_bwd"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name), f"{name} is not exported by the cross-compiled library"


def _after(h, p, hq, q):
    """True when particle p comes after q in ascending (height, index) order, NaN above +inf."""
    if np.isnan(h) or np.isnan(hq):
        if np.isnan(h) and np.isnan(hq):
            return p > q
        return bool(np.isnan(h))
    return h > hq or (h == hq and p > q)


def test_twin_agrees_with_a_literal_per_pixel_loop():
    rng = np.random.default_rng(11)
    H, W, ps, zo = 24, 40, np.float32(1 / 32), np.float32(0.01)
    x = rng.uniform(-0.1, 1.35, size=(2, 200, 3)).astype(np.float32)
    x[..., 1] = rng.integers(-2, 6, size=(2, 200)).astype(np.float32) * np.float32(0.01)   # many ties, negative heights
    x[0, 17, 1] = x[1, 3, 0] = x[1, 5, 2] = np.nan
    x[0, 40, 0], x[0, 41, 2], x[1, 9, 1], x[1, 10, 1] = np.inf, -np.inf, np.inf, -np.inf
    img, owner = depth_twin(x, H, W, ps, zo)
    g_img = rng.normal(size=img.shape).astype(np.float32)
    gx = twin_bwd(owner, g_img)

    def pixel(c, n):   # clip(floor(c / ps), 0, n - 1) spelled out
        f = np.floor(np.float32(c) / ps)
        if np.isnan(f):
            return 0
        return int(min(max(f, 0), n - 1))

    for m in range(2):
        cols = [pixel(c, W) for c in x[m, :, 0]]
        rows = [pixel(c, H) for c in x[m, :, 2]]
        hs = x[m, :, 1] + zo
        seen_owner = np.full(200, -1)
        for r in range(H):
            for c in range(W):
                best = None
                for p in range(200):
                    if rows[p] == r and cols[p] == c and (best is None or _after(hs[p], p, hs[best], best)):
                        best = p
                want = np.float32(0) if best is None else hs[best]
                np.testing.assert_array_equal(img[m, r, c], want)
                if best is not None:
                    seen_owner[best] = r * W + c
        np.testing.assert_array_equal(owner[m], seen_owner)
        for p in range(200):
            want = g_img[m].ravel()[seen_owner[p]] if seen_owner[p] >= 0 else 0
            np.testing.assert_array_equal(gx[m, p], np.float32([0, want, 0]))


def test_default_conf_still_reports_particles():
    from unidom_amd.envs.basic.cloth_env import ClothEnv
    from unidom_amd.envs.fold_cloth1_env import DefaultConf
    from unidom_amd.envs.fold_cloth_tshirt_env import DefaultConf as TshirtConf
    for conf in (DefaultConf(), TshirtConf()):
        assert getattr(conf, "obs_type", ClothEnv.PARTICLE) == ClothEnv.PARTICLE
    assert ClothEnv.DEPTH == "DEPTH"
    import inspect
    assert inspect.signature(ClothEnv.get_obs).parameters["obs_type"].default == ClothEnv.PARTICLE
