"""Scenes for the cloth renderer's tests: the flat patch of the CPU tests, the f64 closed forms the twin is held to, and the hand-made
scene of the kernel-level GPU test (every path of csrc/cloth_render.hip in three frames of at most 64 vertices)."""
import numpy as np

from cloth_render_twin import Conf, camera_f64

SIZES = [(640, 480), (80, 60), (50, 38), (37, 29)]   # full size; most triangles below a pixel; neither a multiple of a tile nor a wave


def mask_faces(mask):
    """ClothSimulator.set_indices (cloth_simulator.py:72-103 of the reference): a square is kept iff its 3 x 3 neighbourhood is cloth."""
    N = mask.shape[0]
    sq = []
    for i in range(N - 1):
        for j in range(N - 1):
            if np.all(mask[[i - 1, i - 1, i - 1, i, i, i, i + 1, i + 1, i + 1], [j - 1, j, j + 1, j - 1, j, j + 1, j - 1, j, j + 1]] != 0):
                a, b, c, d = i * N + j, (i + 1) * N + j, i * N + j + 1, (i + 1) * N + j + 1
                sq += [(a, b, c), (d, c, b)]
    return np.asarray(sq, np.int32).reshape(-1, 3)


def flat_patch(height, N=80, size=16):
    """fold_cloth1's 16 x 32 patch at rest (conftest.fold_cloth1_mask / cloth_reset_x), lifted to sim y = height: (x_grid [N*N,3], faces)."""
    m = np.zeros((N, N), np.float32)
    m[size * 2:size * 3, size * 2:size * 4] = 1
    ii, jj = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    xg = np.stack([ii / N, np.full_like(ii, height, dtype=np.float64), (N - jj) / N], -1).astype(np.float32)
    return xg.reshape(-1, 3), mask_faces(m)


def rays_f64(conf):
    """(rx, ry) [H,W] of the unmirrored pixel centres and the f64 camera"""
    cam = camera_f64(conf)
    u = np.arange(conf.width, dtype=np.float64) + 0.5
    v = np.arange(conf.height, dtype=np.float64) + 0.5
    rx, ry = np.meshgrid((u - cam["cx"]) / cam["fx"], (cam["cy"] - v) / cam["fy"])
    return rx, ry, cam


def plane_depth_f64(conf, z):
    """depth [H,W] at which the ray through each pixel centre meets the render-frame plane of height z (inf where it does not)"""
    rx, ry, cam = rays_f64(conf)
    R, P = cam["R"], cam["P"]
    D2 = R[0, 2] * rx + R[1, 2] * ry - R[2, 2]
    with np.errstate(divide="ignore"):
        return np.where(D2 < 0, (z - P[2]) / D2, np.inf)


def sphere_depth_f64(conf, centre_sim, r):
    """near-root depth [H,W] of the sphere (centre in sim order), nan where the ray misses"""
    rx, ry, cam = rays_f64(conf)
    c = cam["R"] @ (np.asarray(centre_sim, np.float64)[[0, 2, 1]] - cam["P"])
    a = rx * rx + ry * ry + 1.0
    b = rx * c[0] + ry * c[1] - c[2]
    disc = b * b - a * (c @ c - r * r)
    with np.errstate(invalid="ignore"):
        return (b - np.sqrt(disc)) / a


def unproject(conf, a, b, depth):
    """the sim-order point seen at the fraction (a, b) of the unmirrored image (a: left to right, b: top to bottom) at `depth`"""
    cam = camera_f64(conf)
    rx, ry = (a * conf.width - cam["cx"]) / cam["fx"], (cam["cy"] - b * conf.height) / cam["fy"]
    w = cam["P"] + cam["R"].T @ (depth * np.array([rx, ry, -1.0]))
    return [w[0], w[2], w[1]]


def kernel_scene(W, H):
    """(conf, faces [F,3] i32, vertices [3,V,3] f32, spheres [3,2,4] f32).  Frame 0 holds, by face index:
      0       a triangle spanning several 32 x 32 tiles (at 50 x 38: four)
      1..6    a fan of six sub-pixel triangles in front of it
      7       a triangle partly off-screen          8   one fully off-screen
      9       one with a vertex nearer than znear (dropped whole)
      10      one of zero area (a repeated vertex)
      11, 12  coplanar duplicates (the same three indices twice): the lower index wins every pixel
      13, 14  a patch above the ground, given in world coordinates
    sphere 0 in front of the mesh, sphere 1 behind it.  Frame 1: the same, moved and rescaled in depth, sphere 1 brought in front.
    Frame 2: the whole mesh off-screen and no sphere (radius 0): ground and background only."""
    conf = Conf(width=W, height=H)
    P = lambda a, b, d: unproject(conf, a, b, d)
    pw = 1.0 / W                                    # one pixel as a fraction of the width

    def frame(dx, dy, ds):
        v = [P(0.05 + dx, 0.10 + dy, 1.0 * ds), P(0.95 + dx, 0.20 + dy, 1.2 * ds), P(0.40 + dx, 0.95 + dy, 0.9 * ds)]           # 0-2
        fa, fb = (int(0.30 * W) + 0.6) / W + dx, (int(0.31 * H) + 0.55) / H + dy      # fan centre: a tenth of a pixel off a pixel centre
        v += [P(fa, fb, 0.7 * ds)]                                                                                                   # 3
        v += [P(fa + 0.45 * pw * np.cos(i * np.pi / 3), fb + 0.45 * pw * np.sin(i * np.pi / 3) * W / H, 0.7 * ds) for i in range(6)]  # 4-9
        v += [P(-0.3 + dx, 0.5 + dy, 0.8 * ds), P(0.2 + dx, 0.6 + dy, 0.8 * ds), P(-0.1 + dx, 0.9 + dy, 0.8 * ds)]                 # 10-12
        v += [P(1.5 + dx, 1.5 + dy, 1.0), P(1.8 + dx, 1.5 + dy, 1.0), P(1.6 + dx, 1.9 + dy, 1.0)]                                  # 13-15
        v += [P(0.5 + dx, 0.5 + dy, 0.03), P(0.6 + dx, 0.5 + dy, 0.5), P(0.55 + dx, 0.6 + dy, 0.5)]                                # 16-18
        v += [P(0.2 + dx, 0.2 + dy, 0.5), P(0.3 + dx, 0.25 + dy, 0.5)]                                                              # 19-20
        v += [P(0.6 + dx, 0.1 + dy, 0.6 * ds), P(0.9 + dx, 0.15 + dy, 0.6 * ds), P(0.7 + dx, 0.4 + dy, 0.6 * ds)]                  # 21-23
        v += [[0.1 + 3 * dx, 0.1, 0.75], [0.25 + 3 * dx, 0.1, 0.75], [0.1 + 3 * dx, 0.1, 0.9], [0.25 + 3 * dx, 0.1, 0.9]]           # 24-27
        return v

    faces = [(0, 1, 2)] + [(3, 4 + i, 4 + (i + 1) % 6) for i in range(6)] + [(10, 11, 12), (13, 14, 15), (16, 17, 18), (19, 20, 19),
                                                                             (21, 22, 23), (21, 22, 23), (24, 25, 26), (27, 26, 25)]
    verts = np.asarray([frame(0.0, 0.0, 1.0), frame(0.04, -0.03, 0.9), frame(3.0, 0.0, 1.0)], np.float32)
    spheres = np.zeros((3, 2, 4), np.float32)
    spheres[0, 0] = P(0.45, 0.45, 0.6) + [0.05]
    spheres[0, 1] = P(0.5, 0.5, 1.5) + [0.05]
    spheres[1, 0] = P(0.2, 0.7, 0.5) + [0.03]
    spheres[1, 1] = P(0.75, 0.3, 0.4) + [0.04]
    return conf, np.asarray(faces, np.int32), verts, spheres
