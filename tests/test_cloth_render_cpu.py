"""CPU: tests/cloth_render_twin.py, the cloth renderer's specification, held to something other than itself -- f64 geometry through
the pixel centres, watertight coverage, the orientation py_render.py:110-111 returns, and the scene of the kernel-level GPU test.

The depth bound 2e-6 (relative) is the worst case of a chain of about twenty f32 roundings (20 * 2^-24 = 1.2e-6, the constants'
own rounding on top); it was fixed before the twin's operation order was."""
import functools

import numpy as np
import pytest
from scipy.ndimage import binary_fill_holes

import cloth_render_twin as twin
from cloth_render_cases import SIZES, flat_patch, kernel_scene, plane_depth_f64, sphere_depth_f64

BOUND = 2e-6


@functools.lru_cache(maxsize=None)
def _patch_render(size, height):
    conf = twin.Conf(width=size[0], height=size[1])
    xg, faces = flat_patch(height)
    assert len(faces) == 840
    return conf, twin.render(conf, faces, xg, None, unmirrored=True)


@pytest.mark.parametrize("height", [0.0, 0.02, 0.05])
@pytest.mark.parametrize("size", SIZES)
def test_mesh_depth_is_the_f64_ray_plane_depth(size, height):
    conf, (_, depth, tri) = _patch_render(size, height)
    cov = tri >= 0
    assert cov.sum() > 0
    want = plane_depth_f64(conf, height)
    rel = np.abs(depth[cov].astype(np.float64) - want[cov]) / want[cov]
    print(f"{size} h={height}: {cov.sum()} covered pixels, max rel depth error {rel.max():.3e}")
    assert rel.max() <= BOUND


@pytest.mark.parametrize("height", [0.0, 0.02, 0.05])
@pytest.mark.parametrize("size", SIZES)
def test_shared_edges_leave_no_hole(size, height):
    _, (_, _, tri) = _patch_render(size, height)
    cov = tri >= 0
    holes = binary_fill_holes(cov) & ~cov
    print(f"{size} h={height}: {cov.sum()} covered pixels, {holes.sum()} holes")
    assert cov.sum() > 0 and holes.sum() == 0


def test_returned_orientation_background_and_channel_order():
    conf = twin.Conf()
    # a small patch at world y = 0.7 (sim z = 0.7), just above the ground
    verts = np.float32([[0.45, 0.05, 0.68], [0.55, 0.05, 0.68], [0.45, 0.05, 0.72], [0.55, 0.05, 0.72]])
    faces = np.int32([[0, 1, 2], [3, 2, 1]])
    color, depth, tri = twin.render(conf, faces, verts, None)
    raw_c, raw_d, raw_t = twin.render(conf, faces, verts, None, unmirrored=True)
    assert color.shape == (480, 640, 3) and color.dtype == np.uint8 and depth.shape == (480, 640) and depth.dtype == np.float32
    cols = np.nonzero(tri >= 0)[1]
    assert len(cols) > 0 and cols.max() < 320                       # world y > 0.5 ends up left of the centre ...
    assert np.nonzero(raw_t >= 0)[1].min() >= 320                   # ... and was right of it before the mirror
    np.testing.assert_array_equal(color, raw_c[:, ::-1, ::-1])      # mirrored, channels reversed (BGR)
    np.testing.assert_array_equal(depth, raw_d[:, ::-1])
    mesh = tri >= 0
    assert (color[mesh][:, 0] > color[mesh][:, 2]).all()            # the default cloth colour is blue: channel 0 of a BGR image
    assert (depth[mesh] > 0).all()
    bg = tri == -1
    assert bg.any() and (tri == -3).any()
    assert (depth[bg] == 0).all() and (color[bg] == 255).all()
    assert (depth[~bg] >= np.float32(conf.znear)).all()


@pytest.mark.parametrize("size", SIZES)
def test_ground_depth_is_the_f64_closed_form(size):
    conf = twin.Conf(width=size[0], height=size[1])
    _, depth, tri = twin.render(conf, np.zeros((0, 3), np.int32), np.zeros((1, 3), np.float32), None, unmirrored=True)
    g = tri == -3
    want = plane_depth_f64(conf, conf.ground_z)
    rel = np.abs(depth[g].astype(np.float64) - want[g]) / want[g]
    print(f"{size}: {g.sum()} ground pixels, max rel depth error {rel.max():.3e}")
    assert g.sum() > 0.3 * g.size and (tri == -1).any() and rel.max() <= BOUND


# the gripper at reset (primitive0, radius 0.01: seven pixels across at full size, below one at the small sizes) and a larger sphere
# that every size sees
@pytest.mark.parametrize("size,sphere", [((640, 480), (0.5, 0.5, 0.5, 0.01))] + [(s, (0.45, 0.1, 0.55, 0.05)) for s in SIZES])
def test_sphere_depth_is_the_f64_closed_form(size, sphere):
    conf = twin.Conf(width=size[0], height=size[1])
    sphere = np.float32(sphere)
    _, depth, tri = twin.render(conf, np.zeros((0, 3), np.int32), np.zeros((1, 3), np.float32), sphere[None], unmirrored=True)
    s = tri == -2
    ws = sphere_depth_f64(conf, sphere[:3].astype(np.float64), float(sphere[3]))
    hit64 = np.isfinite(ws)
    print(f"{size}: {s.sum()} sphere pixels (f64: {hit64.sum()})")
    assert s.sum() > 0 and (s ^ hit64).sum() <= 2                   # the sets may differ in a pixel whose ray grazes the limb
    both = s & hit64
    rel = np.abs(depth[both].astype(np.float64) - ws[both]) / ws[both]
    print(f"{size}: max rel sphere depth error {rel.max():.3e}")
    assert rel.max() <= BOUND


@pytest.mark.parametrize("size", [(50, 38), (37, 29)])
def test_kernel_scene_holds_every_kind(size):
    """the scene the kernels are compared on must exercise what it claims to (tests/test_cloth_render_gpu.py asserts equality only)"""
    conf, faces, verts, spheres = kernel_scene(*size)
    assert verts.shape[1] <= 64
    tris = [twin.render(conf, faces, verts[m], spheres[m], unmirrored=True)[2] for m in range(3)]
    t0 = tris[0]
    ids = set(np.unique(t0[t0 >= 0]).tolist())
    assert {-1, -2, -3} <= set(np.unique(t0).tolist()) and len(ids) >= 3
    assert 0 in ids and 7 in ids and 11 in ids and (13 in ids or 14 in ids)
    assert ids & set(range(1, 7))                                   # some sub-pixel triangle of the fan takes a pixel
    assert not ids & {8, 9, 10, 12}                                 # off-screen, near-dropped, zero area, the duplicate's higher index
    ys, xs = np.nonzero(t0 == 0)
    assert len({(y // 32, x // 32) for y, x in zip(ys, xs)}) >= 2   # the big triangle spans several tiles
    assert (tris[1] == -2).sum() > (tris[0] == -2).sum()            # frame 1 shows both spheres, frame 0 hides one behind the mesh
    assert set(np.unique(tris[2]).tolist()) == {-1, -3}
