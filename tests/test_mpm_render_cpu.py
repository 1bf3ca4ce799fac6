"""CPU: tests/mpm_render_twin.py, the MPM renderer's specification, held to something other than itself -- f64 geometry through the
pixel centres (ray-sphere, slab test, the cut hollow sphere's outer shell), the point-mode coverage and blend evaluated by hand, the
unmirrored RGB orientation, and the scene of the kernel-level GPU test.

The depth bound 2e-6 (relative) is the one tests/test_cloth_render_cpu.py holds the cloth twin to: the worst case of a chain of about
twenty f32 roundings.  The container bound adds 2 eps: the march stops within eps of the surface along the normal, hence within
eps / cos <= 2 eps along a ray whose incidence cosine is >= 0.5."""
import functools

import numpy as np
import pytest

import cloth_render_twin as ct
import mpm_render_twin as twin
from mpm_render_cases import (BOWL_SIZES, EDGE, KERNEL_SIZES, SIZES, bowl_outer_f64, bowl_sdf_f64, box_depth_f64, kernel_scene,
                              local_rays_f64, plane_depth_f64, quat, single_particle, sphere_depth_f64, unproject)

BOUND = 2e-6
EPS = float(twin.MARCH_EPS)


@pytest.mark.parametrize("size,centre,radius", [((640, 480), (0.5, 0.1, 0.5), 0.008)] + [(s, (0.45, 0.1, 0.55), 0.05) for s in SIZES])
def test_sphere_depth_is_the_f64_closed_form(size, centre, radius):
    conf = twin.Conf(width=size[0], height=size[1], radius=radius)
    x = np.float32([centre])
    _, depth, idimg = twin.render(conf, x)
    s = idimg == 0
    ws = sphere_depth_f64(conf, x[0].astype(np.float64), float(np.float32(radius)))
    hit64 = np.isfinite(ws)
    print(f"{size}: {s.sum()} sphere pixels (f64: {hit64.sum()})")
    assert s.sum() > 0 and (s ^ hit64).sum() <= 2                   # the sets may differ in a pixel whose ray grazes the limb
    both = s & hit64
    rel = np.abs(depth[both].astype(np.float64) - ws[both]) / ws[both]
    print(f"{size}: max rel sphere depth error {rel.max():.3e}")
    assert rel.max() <= BOUND


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("q", [(1.0, 0.0, 0.0, 0.0), tuple(quat((1, 2, 3), 0.7))], ids=["aligned", "rotated"])
def test_box_depth_is_the_f64_slab_test(size, q):
    conf = twin.Conf(width=size[0], height=size[1], mode=1)
    pos, q32, sz = np.float32([0.45, 0.12, 0.5]), np.float32(q), np.float32([0.08, 0.05, 0.06])
    far = np.float32([[5.0, 5.0, 5.0]])                            # the one particle: out of view
    _, depth, idimg = twin.render(conf, far, pos[None], q32[None], sz[None])
    b = idimg == -4
    wb = box_depth_f64(conf, pos.astype(np.float64), q32.astype(np.float64), sz.astype(np.float64))
    hit64 = np.isfinite(wb)
    print(f"{size}: {b.sum()} box pixels (f64: {hit64.sum()})")
    assert b.sum() > 0 and (b ^ hit64).sum() <= 2
    both = b & hit64
    rel = np.abs(depth[both].astype(np.float64) - wb[both]) / wb[both]
    print(f"{size}: max rel box depth error {rel.max():.3e}")
    assert rel.max() <= BOUND


@pytest.mark.parametrize("size", SIZES)
def test_container_depth_on_the_outer_shell(size):
    """the bowl turned bottom-up towards the camera: rays that meet its outer lower hemisphere from outside at cosine >= 0.5"""
    conf = twin.Conf(width=size[0], height=size[1], mode=1, prim_kind=1)
    pos, q32, sz = np.float32([0.5, 0.15, 0.5]), np.float32(quat((0, 0, 1), 2.6)), BOWL_SIZES[0]
    far = np.float32([[5.0, 5.0, 5.0]])
    _, depth, idimg = twin.render(conf, far, pos[None], q32[None], sz[None])
    dep64, ok = bowl_outer_f64(conf, pos.astype(np.float64), q32.astype(np.float64), sz)
    print(f"{size}: {ok.sum()} rays on the outer shell at cosine >= 0.5, {(idimg == -4).sum()} container pixels")
    assert ok.sum() > 0 and (idimg[ok] == -4).all()
    err = np.abs(depth[ok].astype(np.float64) - dep64[ok])
    print(f"{size}: max container depth error {err.max():.3e} (bound {2 * EPS + 2e-6:.3e})")
    assert err.max() <= 2 * EPS + 2e-6
    # every hit, inside and rim included, lies within eps of the f64 SDF's zero set (1e-6: the 1e-12 terms and f32 rounding)
    hit = idimg == -4
    o, dl = local_rays_f64(conf, pos.astype(np.float64), q32.astype(np.float64))
    sdf = bowl_sdf_f64(sz, o[:, None, None] + depth.astype(np.float64) * dl)
    assert np.abs(sdf[hit]).max() <= EPS + 1e-6


@pytest.mark.parametrize("point_size", [1, 2, 3, 5])
def test_point_covers_point_size_squared_pixels(point_size):
    conf = twin.Conf(width=50, height=38, mode=1, point_size=point_size, particle_color=(0.2, 0.4, 0.6, 0.5))
    x = np.float32([unproject(conf, 0.413, 0.467, 0.6)])
    _, depth, idimg = twin.render(conf, x)
    assert (idimg == 0).sum() == point_size ** 2
    v, u = np.nonzero(idimg == 0)
    assert u.max() - u.min() == point_size - 1 and v.max() - v.min() == point_size - 1
    assert abs(0.5 * (u.min() + u.max() + 1) - 0.413 * 50) <= 0.5 + 1e-4 and abs(0.5 * (v.min() + v.max() + 1) - 0.467 * 38) <= 0.5 + 1e-4
    assert np.all(np.abs(depth[idimg == 0] - 0.6) <= 0.6 * BOUND)


def test_point_blend_over_the_ground_is_the_formula():
    W, H = 50, 38
    rgba = (100 / 255, 100 / 255, 249 / 255, 125 / 255)
    u, v = 20, 25
    opaque = twin.Conf(width=W, height=H, mode=1)
    far = np.float32([[5.0, 5.0, 5.0]])
    ground_rgb, gdepth, gid = twin.render(opaque, far)
    assert gid[v, u] == -3
    gd = float(plane_depth_f64(opaque, opaque.ground_z)[v, u])
    conf = twin.Conf(width=W, height=H, mode=1, particle_color=rgba)
    x = np.float32([unproject(conf, (u + 0.5) / W, (v + 0.5) / H, 0.5 * gd)])
    rgb, depth, idimg = twin.render(conf, x)
    assert (idimg == 0).sum() == 1 and idimg[v, u] == 0 and abs(depth[v, u] - 0.5 * gd) <= gd * BOUND
    # by hand, in f32: the ground's shaded colour under the cloth twin's lit, then the blend and the u8 rounding
    f32 = np.float32
    k = ct._K(conf)
    rx, ry = (f32(u + 0.5) - k.cx) / k.fx, (k.cy - f32(v + 0.5)) / k.fy
    t = gdepth[v, u]
    lit = ct._lit(k, [k.R[0, 2], k.R[1, 2], k.R[2, 2]], [t * rx, t * ry, -t])
    for c in range(3):
        behind = min(max(f32(conf.ground_color[c]) * lit, f32(0)), f32(1))
        assert int(behind * f32(255) + f32(0.5)) == ground_rgb[v, u, c]
        a = f32(rgba[3])
        want = a * f32(rgba[c]) + (f32(1) - a) * behind
        assert rgb[v, u, c] == int(min(max(want, f32(0)), f32(1)) * f32(255) + f32(0.5))
    other = np.ones((H, W), bool)
    other[v, u] = False
    assert np.array_equal(rgb[other], ground_rgb[other])
    # a point behind the ground is not taken
    xb = np.float32([unproject(conf, (u + 0.5) / W, (v + 0.5) / H, 1.5 * gd)])
    rgb_b, depth_b, id_b = twin.render(conf, xb)
    assert id_b[v, u] == -3 and np.array_equal(rgb_b, ground_rgb)


@functools.lru_cache(maxsize=None)
def _scene_render(size, kind, mode, point_size):
    conf, x, pp, pr, sz = kernel_scene(size[0], size[1], kind, mode, point_size)
    return [twin.render(conf, x[m], pp[m], pr[m], sz) for m in range(3)]


@pytest.mark.parametrize("size", KERNEL_SIZES)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("mode,point_size", [(0, 1), (1, 1), (1, 3), (1, 4), (1, 5)])
def test_kernel_scene_holds_every_kind(size, kind, mode, point_size):
    """the scene the kernels are compared on must exercise what it claims to (tests/test_mpm_render_gpu.py asserts equality only)"""
    frames = _scene_render(size, kind, mode, point_size)
    for m, (_, depth, idimg) in enumerate(frames):
        kinds = set(np.unique(idimg).tolist())
        # (points 4 and 5 pixels wide are there for the kernel's path threshold; at 37 x 29 they may bury a whole primitive)
        assert ({-1, -3, -4, -5} <= kinds if point_size <= 3 else {-1, -3} <= kinds and kinds & {-4, -5}) and (idimg >= 0).sum() > 100, (m, kinds)
        assert (idimg[idimg >= 0] < 1020).any() and (idimg >= 1020).any()
        # dropped or hidden particles appear nowhere
        for name in ("nan", "outside", "behind", "tie_hi") + (("near",) if mode == 0 else ()):
            assert not (idimg == EDGE[name]).any(), (m, name)
        assert (idimg == EDGE["tie_lo"]).any() and (idimg == EDGE["front"]).any()
        if mode == 1:
            assert (idimg == EDGE["near"]).sum() == point_size ** 2      # znear <= d < znear + r: a point, not a sphere
        if mode == 0 or point_size >= 3:
            assert (idimg == EDGE["reach_in"]).any() and (idimg == EDGE["reach_in"])[:, 0].any()     # centred left of column 0
        if mode == 0:
            assert (idimg == EDGE["sunk"]).any()
        if size == (50, 38) and (mode == 0 or point_size >= 3):
            v, u = np.nonzero(idimg == EDGE["corner"])
            assert u.min() < 32 <= u.max() and v.min() < 32 <= v.max()   # in all four tiles
        assert np.all(depth[idimg == -1] == 0) and np.all(depth[idimg != -1] >= np.float32(0.05))
    assert not np.array_equal(frames[0][2], frames[1][2]) and not np.array_equal(frames[1][2], frames[2][2])


def test_orientation_is_unmirrored_rgb():
    """a particle left of the image centre appears in the left half, coloured (R, G, B) as given -- the cloth renderer's
    [:, ::-1, ::-1] (py_render.py:110-111) is not applied by ParticlePyRenderer / WaterPyRenderer (:140-145, :169-174)"""
    conf = twin.Conf(width=80, height=60, mode=1, point_size=3, particle_color=(1.0, 0.5, 0.0, 1.0))
    x = np.float32([unproject(conf, 0.2, 0.3, 0.6)])
    rgb, depth, idimg = twin.render(conf, x)
    v, u = np.nonzero(idimg == 0)
    assert len(u) == 9 and u.max() < 40 and v.max() < 30 and abs(u.mean() + 0.5 - 0.2 * 80) < 1 and abs(v.mean() + 0.5 - 0.3 * 60) < 1
    assert np.all(rgb[idimg == 0] == np.uint8([255, 128, 0]))
    # sphere mode: the same place
    conf0 = twin.Conf(width=80, height=60, mode=0, radius=0.02)
    _, _, id0 = twin.render(conf0, x)
    v0, u0 = np.nonzero(id0 == 0)
    assert len(u0) > 4 and abs(u0.mean() + 0.5 - 0.2 * 80) < 1 and abs(v0.mean() + 0.5 - 0.3 * 60) < 1


def test_single_particle_without_primitives():
    for mode in (0, 1):
        conf, x = single_particle(37, 29, mode)
        rgb, depth, idimg = twin.render(conf, x[0])
        assert set(np.unique(idimg).tolist()) == {-3, -1, 0}
